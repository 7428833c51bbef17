"""Build and load tests/native/record_tail_harness.hip: the RECORD instances of the sampler tail (tail_record_kernel / tail_warp_record_kernel<NV,
SESSION> through tail_launch) and the raw-logits record node (step_logits_record_kernel through step_logits_record_launch), the two functions
the engine calls, with the product's kernels that write the records (see the .hip file). A null ``rec`` launches the instance without the
feature on the same operands."""
import ctypes as C
import os
import subprocess

from gemm_harness import CSRC, HIPCC_FLAGS, ROOT
from slot_gen_harness import SlotGen
from tail_harness import DevDims, DevGen
from warp_tail_harness import DevWarp

SRC = os.path.join(ROOT, "tests", "native", "record_tail_harness.hip")
PTTS_OK = 0
ENTRY_POINTS = ("rh_last_error", "rh_args_size", "rh_tail", "rh_logits_record", "rh_set_step_record", "rh_set_warp", "rh_set_slot_gen")


def build(out_dir):
    """One translation unit with build()'s hipcc flags, linked against torch's HIP runtime as __graft_entry__.build() links the product."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    obj, lib = os.path.join(out_dir, "record_tail_harness.o"), os.path.join(out_dir, "librecord_tail_harness.so")
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC, "-c", SRC, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    subprocess.check_call(["g++", "-shared", "-o", lib, obj, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class RhArgs(C.Structure):
    """struct RhArgs of record_tail_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("logits", "ids", "cur_len", "unfinished", "has_eos", "first_unf", "gen", "dims", "row_maxlen", "slot_gen",
                                          "slot_tprefix", "warp", "rec", "tables", "pos_table", "h")] + \
               [(n, C.c_int) for n in ("ids_ld", "B", "K", "V", "eos", "pad", "H", "bos", "session", "row0", "grid")]


class StepRecord(C.Structure):
    """struct StepRecord of ptts_step_record_kernels.h."""
    _fields_ = [("scores", C.c_void_p), ("logits", C.c_void_p), ("cap_steps", C.c_int), ("reserved", C.c_int), ("step_stride", C.c_longlong)]


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.rh_last_error.restype = C.c_char_p
        L.rh_args_size.argtypes = [C.c_int]
        for which, st in enumerate((RhArgs, DevGen, DevDims, SlotGen, DevWarp, StepRecord)):
            assert L.rh_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between the harness and tests/record_tail_harness.py"
        L.rh_tail.argtypes = [C.POINTER(RhArgs), C.c_void_p]
        L.rh_logits_record.argtypes = [C.POINTER(RhArgs), C.c_void_p]
        L.rh_set_step_record.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p]
        L.rh_set_warp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
        L.rh_set_slot_gen.argtypes = [C.c_void_p, C.c_int, C.POINTER(DevGen), C.c_int, C.c_void_p]

    def error(self):
        return self.lib.rh_last_error().decode()

    # each launcher returns the PTTS_* status
    def tail(self, a, stream):
        return self.lib.rh_tail(C.byref(a), stream)

    def logits_record(self, a, stream):
        return self.lib.rh_logits_record(C.byref(a), stream)

    def set_step_record(self, recs, row0, nrows, scores, logits, cap_steps, step_stride, per_row, stream):
        return self.lib.rh_set_step_record(recs, row0, nrows, scores, logits, cap_steps, step_stride, per_row, stream)

    def set_warp(self, recs, row0, nrows, wp, stream):
        return self.lib.rh_set_warp(recs, row0, nrows, *wp, stream)

    def set_slot_gen(self, recs, row, gen, stream, row_base=0):
        return self.lib.rh_set_slot_gen(recs, row, None if gen is None else C.byref(gen), row_base, stream)
