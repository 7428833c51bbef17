"""Build and load tests/native/logit_edit_harness.hip: the product's logit_edit_kernel through logit_edit_launch (the function the engine calls)
and copy_logit_edit_kernel behind thin C entry points that take device pointers (see the .hip file)."""
import ctypes as C
import os
import subprocess

from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "logit_edit_harness.hip")
PTTS_OK, PTTS_E_INVALID, PTTS_E_UNSUPPORTED = 0, -1, -5
ENTRY_POINTS = ("lh_last_error", "lh_args_size", "lh_copy_records", "lh_logit_edit")


def build(out_dir):
    """One translation unit with build()'s hipcc flags, linked against torch's HIP runtime as __graft_entry__.build() links the product."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    obj, lib = os.path.join(out_dir, "logit_edit_harness.o"), os.path.join(out_dir, "liblogit_edit_harness.so")
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC, "-c", SRC, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    subprocess.check_call(["g++", "-shared", "-o", lib, obj, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class LhArgs(C.Structure):
    """struct LhArgs of logit_edit_harness.hip."""
    _fields_ = ([(n, C.c_void_p) for n in ("logits", "cur_len", "t_prefix", "hdr", "bias", "decay", "flags")]
                + [(n, C.c_int) for n in ("ld_v", "ld_t", "t_prefix_stride", "B", "K", "V", "eos", "row0", "nb")])


class LogitEditHeader(C.Structure):
    """struct LogitEditHeader of ptts_logit_edit_kernels.h."""
    _fields_ = [(n, C.c_int) for n in ("mask", "decay_start", "table_len", "reserved")]


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.lh_last_error.restype = C.c_char_p
        L.lh_args_size.argtypes = [C.c_int]
        for which, st in enumerate((LhArgs, LogitEditHeader)):
            assert L.lh_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between the harness and tests/logit_edit_harness.py"
        self.max_vocab = L.lh_args_size(2)
        L.lh_copy_records.argtypes = [C.POINTER(LhArgs), C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.lh_logit_edit.argtypes = [C.POINTER(LhArgs), C.c_void_p]

    def error(self):
        return self.lib.lh_last_error().decode()

    # each launcher returns the PTTS_* status
    def copy_records(self, a, src, dst0, n, stream):
        return self.lib.lh_copy_records(C.byref(a), src, dst0, n, stream)

    def logit_edit(self, a, stream):
        return self.lib.lh_logit_edit(C.byref(a), stream)
