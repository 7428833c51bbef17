"""Build and load tests/native/score_harness.hip: the product's score_launch (final LayerNorm + LM heads + cross-entropy kernel), the weight packing
and the existing PRO_LN / EPI_STORE heads projection behind thin C entry points that take device pointers (see the .hip file)."""
import ctypes as C
import os
import subprocess

from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "score_harness.hip")
PTTS_OK = 0
ENTRY_POINTS = ("sh_last_error", "sh_args_size", "sh_pack", "sh_score", "sh_project")


def build(out_dir):
    """One translation unit with build()'s hipcc flags, linked against torch's HIP runtime as __graft_entry__.build() links the product. A library
    in `out_dir` that is newer than the harness source and every product header is kept."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    obj, lib = os.path.join(out_dir, "score_harness.o"), os.path.join(out_dir, "libscore_harness.so")
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    if os.path.exists(lib) and all(os.path.getmtime(d) <= os.path.getmtime(lib) for d in deps):
        return lib
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC, "-c", SRC, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    subprocess.check_call(["g++", "-shared", "-o", lib, obj, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


def default_dir():
    return os.path.join(ROOT, "build", "score_harness")


class ShArgs(C.Structure):
    """struct ShArgs of score_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("x", "gamma", "beta", "W", "ids", "labels", "nll", "counted", "logits", "xw", "out")] + \
               [(n, C.c_int) for n in ("x_ld", "H", "K", "V", "B", "Q", "Qs", "T", "bos", "eos", "M")]


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.sh_last_error.restype = C.c_char_p
        assert L.sh_args_size() == C.sizeof(ShArgs), "ShArgs layout differs between the harness and tests/score_harness.py"
        L.sh_pack.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.sh_score.argtypes = [C.c_int, C.POINTER(ShArgs), C.c_void_p]
        L.sh_project.argtypes = [C.c_int, C.POINTER(ShArgs), C.c_void_p]

    def error(self):
        return self.lib.sh_last_error().decode()

    def check(self, rc):
        assert rc == PTTS_OK, self.error()

    def pack(self, bf16, w):
        """w fp32 [N, K] on the device -> the packed strips in the engine dtype (a uint8 tensor)."""
        import torch

        N, K = w.shape
        out = torch.empty(N * K * (2 if bf16 else 4), dtype=torch.uint8, device=w.device)
        self.check(self.lib.sh_pack(int(bf16), w.data_ptr(), out.data_ptr(), N, K, None))
        return out

    def score(self, bf16, a):
        return self.lib.sh_score(int(bf16), C.byref(a), None)

    def project(self, bf16, a):
        return self.lib.sh_project(int(bf16), C.byref(a), None)
