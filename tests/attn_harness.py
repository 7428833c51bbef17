"""Build and load tests/native/attn_harness.hip: the product's attention kernels (attn_kernel through launch_attn, the two prefill kernels through
launch_prefill_attn, kv_append_kernel, the two T5 attention kernels) behind thin C entry points that take device pointers (see the .hip file)."""
import ctypes as C
import os
import subprocess

from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "attn_harness.hip")
PTTS_OK, PTTS_E_INVALID, PTTS_E_UNSUPPORTED = 0, -1, -5
ENTRY_POINTS = ("ah_last_error", "ah_args_size", "ah_instances", "ah_attn", "ah_prefill_attn", "ah_kv_append", "ah_t5_attn")
# ah_instances kinds, with the mangled-name pattern of each kernel: the captures are the template arguments (engine dtype t = bf16_t / f = float)
KINDS = ("attn_kernel", "prefill_attn_kernel", "prefill_attn_mfma_kernel", "kv_append_kernel", "t5_attn_kernel", "t5_attn_mfma_kernel")


def build(out_dir):
    """One translation unit with build()'s hipcc flags, linked against torch's HIP runtime as __graft_entry__.build() links the product."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    obj, lib = os.path.join(out_dir, "attn_harness.o"), os.path.join(out_dir, "libattn_harness.so")
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC, "-c", SRC, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    subprocess.check_call(["g++", "-shared", "-o", lib, obj, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class AhArgs(C.Structure):
    """struct AhArgs of attn_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("q", "knew", "vnew", "kcache", "vcache", "cur_len", "dims", "mask", "cos", "sin", "part", "direct_out", "stats",
                                          "kscale", "vscale")] + \
               [(n, C.c_int) for n in ("q_ld", "kv_ld", "cap", "kv_bound", "mask_ld", "S", "Q", "nheads", "H", "kv_heads", "n_rep", "cross", "fused_append",
                                       "out_fo", "hostP", "hostN", "B", "bf16", "waves", "mode")] + [("scale", C.c_float)]


class AhT5Args(C.Structure):
    """struct AhT5Args of attn_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("qkv", "bias", "mask", "out")] + \
               [(n, C.c_int) for n in ("ld", "inner", "bias_ld", "bias_zero", "N", "out_fo", "B", "nheads", "bf16", "mfma")]


class DevDims(C.Structure):
    """struct DevDims of ptts_lm_kernels.h (written into a device buffer as raw bytes)."""
    _fields_ = [("P", C.c_int), ("N", C.c_int), ("max_length", C.c_int), ("T_prefix", C.c_int), ("prefix", C.c_void_p), ("prefix_ld", C.c_int)]


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.ah_last_error.restype = C.c_char_p
        L.ah_args_size.argtypes = [C.c_int]
        for which, st in enumerate((AhArgs, AhT5Args, DevDims)):
            assert L.ah_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between the harness and tests/attn_harness.py"
        for n in ("ah_attn", "ah_prefill_attn", "ah_kv_append"):
            getattr(L, n).argtypes = [C.POINTER(AhArgs), C.c_void_p]
        L.ah_t5_attn.argtypes = [C.POINTER(AhT5Args), C.c_void_p]
        L.ah_instances.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]

    def error(self):
        return self.lib.ah_last_error().decode()

    def instances(self):
        """{kernel name: [template arguments as the harness lists them]}: attn_kernel (bf16, NW, KV8), prefill_attn_kernel (bf16, KV8),
        prefill_attn_mfma_kernel (bf16, NW), kv_append_kernel (bf16, KV8), the T5 kernels (bf16,)."""
        width = (3, 2, 2, 2, 1, 1)
        out = {}
        for kind, name in enumerate(KINDS):
            n = self.lib.ah_instances(kind, None, 0)
            buf = (C.c_int * (3 * n))()
            self.lib.ah_instances(kind, buf, n)
            out[name] = [tuple(buf[3 * i:3 * i + width[kind]]) for i in range(n)]
        return out

    # each launcher returns the PTTS_* status
    def attn(self, a, stream):
        return self.lib.ah_attn(C.byref(a), stream)

    def prefill_attn(self, a, stream):
        return self.lib.ah_prefill_attn(C.byref(a), stream)

    def kv_append(self, a, stream):
        return self.lib.ah_kv_append(C.byref(a), stream)

    def t5_attn(self, a, stream):
        return self.lib.ah_t5_attn(C.byref(a), stream)
