"""Build and load tests/native/tail_harness.hip: the product's sampler tail (tail_kernel<NV, SESSION> through tail_launch, the function the
engine calls), session_reset_rows_kernel and embed_kernel<WT, SESSION> behind thin C entry points that take device pointers (see the .hip file)."""
import ctypes as C
import os
import subprocess

from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "tail_harness.hip")
PTTS_OK, PTTS_E_INVALID = 0, -1
ENTRY_POINTS = ("th_last_error", "th_args_size", "th_tail_instances", "th_tail", "th_reset_rows", "th_embed")


def build(out_dir):
    """One translation unit with build()'s hipcc flags, linked against torch's HIP runtime as __graft_entry__.build() links the product."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    obj, lib = os.path.join(out_dir, "tail_harness.o"), os.path.join(out_dir, "libtail_harness.so")
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC, "-c", SRC, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    subprocess.check_call(["g++", "-shared", "-o", lib, obj, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class ThArgs(C.Structure):
    """struct ThArgs of tail_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("logits", "ids", "cur_len", "unfinished", "has_eos", "first_unf", "gen", "dims", "tables", "pos_table",
                                          "h", "row_maxlen")] + \
               [(n, C.c_int) for n in ("ids_ld", "B", "K", "V", "eos", "pad", "H", "bos", "bf16_tables", "session", "row0", "grid")]


class DevGen(C.Structure):
    """struct DevGen of ptts_lm_kernels.h (written into a device buffer as raw bytes)."""
    _fields_ = [(n, C.c_int) for n in ("max_length", "min_new_tokens", "do_sample", "top_k", "use_eos_gate")] + \
               [("temperature", C.c_float), ("top_p", C.c_float), ("seed", C.c_ulonglong)]


class DevDims(C.Structure):
    """struct DevDims of ptts_lm_kernels.h."""
    _fields_ = [("P", C.c_int), ("N", C.c_int), ("max_length", C.c_int), ("T_prefix", C.c_int), ("prefix", C.c_void_p), ("prefix_ld", C.c_int)]


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.th_last_error.restype = C.c_char_p
        L.th_args_size.argtypes = [C.c_int]
        for which, st in enumerate((ThArgs, DevGen, DevDims)):
            assert L.th_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between the harness and tests/tail_harness.py"
        L.th_tail.argtypes = [C.POINTER(ThArgs), C.c_void_p]
        L.th_embed.argtypes = [C.POINTER(ThArgs), C.c_void_p]
        L.th_reset_rows.argtypes = [C.POINTER(ThArgs), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.th_tail_instances.argtypes = [C.POINTER(C.c_int), C.c_int]

    def error(self):
        return self.lib.th_last_error().decode()

    def tail_instances(self):
        """(NV, SESSION) of every tail_kernel instance the harness reaches."""
        n = self.lib.th_tail_instances(None, 0)
        buf = (C.c_int * (2 * n))()
        self.lib.th_tail_instances(buf, n)
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]

    # each launcher returns the PTTS_* status
    def tail(self, a, stream):
        return self.lib.th_tail(C.byref(a), stream)

    def embed(self, a, stream):
        return self.lib.th_embed(C.byref(a), stream)

    def reset_rows(self, a, row_maxlen, row0, nrows, live, max_length, stream):
        return self.lib.th_reset_rows(C.byref(a), row_maxlen, row0, nrows, live, max_length, stream)
