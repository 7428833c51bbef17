"""Build and load tests/native/warp_tail_harness.hip: the WARP instances of the sampler tail (tail_warp_kernel<NV, SESSION> through tail_launch,
the function the engine calls) with the per-utterance warper records and the per-slot sampler records, and the product's kernels that write
both (see the .hip file). A null ``warp`` pointer launches the instance without the feature on the same operands."""
import ctypes as C
import os
import subprocess

from gemm_harness import CSRC, HIPCC_FLAGS, ROOT
from slot_gen_harness import SlotGen
from tail_harness import DevDims, DevGen

SRC = os.path.join(ROOT, "tests", "native", "warp_tail_harness.hip")
PTTS_OK = 0


def build(out_dir):
    """One translation unit with build()'s hipcc flags, linked against torch's HIP runtime as __graft_entry__.build() links the product."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    obj, lib = os.path.join(out_dir, "warp_tail_harness.o"), os.path.join(out_dir, "libwarp_tail_harness.so")
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC, "-c", SRC, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    subprocess.check_call(["g++", "-shared", "-o", lib, obj, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class WhArgs(C.Structure):
    """struct WhArgs of warp_tail_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("logits", "ids", "cur_len", "unfinished", "has_eos", "first_unf", "gen", "dims", "row_maxlen", "slot_gen",
                                          "warp")] + \
               [(n, C.c_int) for n in ("ids_ld", "B", "K", "V", "eos", "pad", "session", "row0", "grid")]


class DevWarp(C.Structure):
    """struct DevWarp of ptts_lm_kernels.h."""
    _fields_ = [(n, C.c_float) for n in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")]


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.wh_last_error.restype = C.c_char_p
        L.wh_args_size.argtypes = [C.c_int]
        for which, st in enumerate((WhArgs, DevGen, DevDims, SlotGen, DevWarp)):
            assert L.wh_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between the harness and tests/warp_tail_harness.py"
        L.wh_tail.argtypes = [C.POINTER(WhArgs), C.c_void_p]
        L.wh_set_warp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
        L.wh_set_slot_gen.argtypes = [C.c_void_p, C.c_int, C.POINTER(DevGen), C.c_int, C.c_void_p]

    def error(self):
        return self.lib.wh_last_error().decode()

    # each launcher returns the PTTS_* status
    def tail(self, a, stream):
        return self.lib.wh_tail(C.byref(a), stream)

    def set_warp(self, recs, row0, nrows, wp, stream):
        return self.lib.wh_set_warp(recs, row0, nrows, *wp, stream)

    def set_slot_gen(self, recs, row, gen, stream, row_base=0):
        """gen: a tail_harness.DevGen (own = 1) or None (the cleared record)."""
        return self.lib.wh_set_slot_gen(recs, row, None if gen is None else C.byref(gen), row_base, stream)
