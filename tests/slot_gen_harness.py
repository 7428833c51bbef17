"""Build and load tests/native/slot_gen_harness.hip: tail_launch with the per-slot sampler records of a continuous session and the
product's record-writing kernel (set_slot_gen_kernel) behind thin C entry points that take device pointers (see the .hip file). The
operands of a launch are tail_harness.ThArgs."""
import ctypes as C
import os
import subprocess

import tail_harness as TH
from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "slot_gen_harness.hip")
ENTRY_POINTS = ("sg_last_error", "sg_args_size", "sg_tail", "sg_set_slots")
PAD_WORD = 7  # 32-bit word of a record that is padding (between DevGen::top_p and the 8-aligned seed): its content is not part of the contract


class SlotGen(C.Structure):
    """struct SlotGen of ptts_lm_kernels.h: the sampler record of one slot."""
    _fields_ = [("g", TH.DevGen), ("own", C.c_int), ("row_base", C.c_int)]


WORDS = C.sizeof(SlotGen) // 4


def build(out_dir):
    """One translation unit with build()'s hipcc flags, linked as tail_harness.build() links its own."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    obj, lib = os.path.join(out_dir, "slot_gen_harness.o"), os.path.join(out_dir, "libslot_gen_harness.so")
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC, "-c", SRC, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    subprocess.check_call(["g++", "-shared", "-o", lib, obj, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.sg_last_error.restype = C.c_char_p
        L.sg_args_size.argtypes = [C.c_int]
        for which, st in enumerate((TH.ThArgs, TH.DevGen, SlotGen)):
            assert L.sg_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between the harness and its Python description"
        L.sg_tail.argtypes = [C.POINTER(TH.ThArgs), C.c_void_p, C.c_void_p]
        L.sg_set_slots.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def error(self):
        return self.lib.sg_last_error().decode()

    # each launcher returns the PTTS_* status
    def tail(self, a, slot_gen, stream):
        return self.lib.sg_tail(C.byref(a), slot_gen, stream)

    def set_slots(self, slot_gen, B, row0, nrows, gen, stream):
        """gen: a tail_harness.DevGen (own = 1, row_base 0) or None (the cleared record)."""
        return self.lib.sg_set_slots(slot_gen, B, row0, nrows, None if gen is None else C.byref(gen), stream)
