"""Build and load tests/native/penalty_harness.hip: the product's history_penalty_kernel through penalty_launch (the function the engine calls)
and set_penalty_kernel behind thin C entry points that take device pointers (see the .hip file)."""
import ctypes as C
import os
import subprocess

from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "penalty_harness.hip")
PTTS_OK, PTTS_E_INVALID, PTTS_E_UNSUPPORTED = 0, -1, -5
ENTRY_POINTS = ("ph_last_error", "ph_args_size", "ph_set_records", "ph_penalty")


def build(out_dir):
    """One translation unit with build()'s hipcc flags, linked against torch's HIP runtime as __graft_entry__.build() links the product."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    obj, lib = os.path.join(out_dir, "penalty_harness.o"), os.path.join(out_dir, "libpenalty_harness.so")
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC, "-c", SRC, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    subprocess.check_call(["g++", "-shared", "-o", lib, obj, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class PhArgs(C.Structure):
    """struct PhArgs of penalty_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("logits", "ids", "cur_len", "pen")] + [(n, C.c_int) for n in ("ids_ld", "B", "K", "V", "row0", "nb")]


class HistoryPenalty(C.Structure):
    """struct HistoryPenalty of ptts_penalty_kernels.h."""
    _fields_ = [("repetition_penalty", C.c_float), ("no_repeat_ngram", C.c_int)]


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.ph_last_error.restype = C.c_char_p
        L.ph_args_size.argtypes = [C.c_int]
        for which, st in enumerate((PhArgs, HistoryPenalty)):
            assert L.ph_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between the harness and tests/penalty_harness.py"
        self.max_vocab = L.ph_args_size(2)
        L.ph_set_records.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
        L.ph_penalty.argtypes = [C.POINTER(PhArgs), C.c_void_p]

    def error(self):
        return self.lib.ph_last_error().decode()

    # each launcher returns the PTTS_* status
    def set_records(self, pen_ptr, row0, nrows, repetition_penalty, no_repeat_ngram, stream):
        return self.lib.ph_set_records(pen_ptr, row0, nrows, repetition_penalty, no_repeat_ngram, stream)

    def penalty(self, a, stream):
        return self.lib.ph_penalty(C.byref(a), stream)
