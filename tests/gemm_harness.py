"""Build and load tests/native/gemm_harness.hip: the product's prefill-sized GEMM kernels (gemm_glds_kernel instances, gemm_tile_kernel,
gemm_block_kernel, the 128-row PRO_COPY strips, launch_gemm) behind thin C entry points that take device pointers (see the .hip file)."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parler_tts_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "gemm_harness.hip")

PTTS_OK, PTTS_E_INVALID, PTTS_E_UNSUPPORTED = 0, -1, -5
EPI_STORE, EPI_RESID, EPI_KV, EPI_GELU_WT, EPI_GATE_WT = 0, 2, 3, 4, 5
EPIS = (EPI_STORE, EPI_RESID, EPI_KV, EPI_GELU_WT, EPI_GATE_WT)
EPI_NAMES = {EPI_STORE: "STORE", EPI_RESID: "RESID", EPI_KV: "KV", EPI_GELU_WT: "GELU_WT", EPI_GATE_WT: "GATE_WT"}
# build()'s hipcc flags (kernel-argument preload included: the preloaded entry points are what the product runs)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-mllvm", "-amdgpu-kernarg-preload-count=14"]


def parts():
    """(tag, defines) of the translation units: one common part, one per (engine dtype, epilogue); tag t = bf16, f = fp32."""
    out = [("common", ["-DGH_COMMON"])]
    for d, wt in (("t", "bf16_t"), ("f", "float")):
        for e in EPIS:
            out.append((f"{d}{e}", [f"-DGH_WT={wt}", f"-DGH_EPI={e}", f"-DGH_TAG={d}{e}"] + (["-DGH_BF16"] if d == "t" else [])))
    return out


def build(out_dir):
    """Compile every part in parallel and link them against torch's HIP runtime, as __graft_entry__.build() links the product library."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)

    def compile_part(p):
        tag, defs = p
        obj = os.path.join(out_dir, f"gemm_harness_{tag}.o")
        cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC] + defs + ["-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
        return obj

    with ThreadPoolExecutor(max_workers=min(16, len(parts()), os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_part, parts()))
    lib = os.path.join(out_dir, "libgemm_harness.so")
    subprocess.check_call(["g++", "-shared", "-o", lib] + objs + ["-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class GhArgs(C.Structure):
    """struct GhArgs of gemm_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("W", "x", "out", "kcache", "vcache", "kv_layers", "rs_part", "nx_out", "nx_gamma", "ss_out")] + \
               [(n, C.c_int) for n in ("M", "N", "K", "x_ld", "out_ld", "nheads", "kv_rows_per_b", "kv_cap", "kv_col0", "kv_nlayers", "rs_n")] + \
               [("rs_invD", C.c_float), ("rms_eps", C.c_float), ("xcd_swz", C.c_int)]


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.gh_last_error.restype = C.c_char_p
        assert L.gh_args_size() == C.sizeof(GhArgs), "GhArgs layout differs between gemm_harness.hip and tests/gemm_harness.py"
        L.gh_pack.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        for d in "tf":
            for e in EPIS:
                getattr(L, f"gh_gemm_{d}{e}").argtypes = [C.POINTER(GhArgs), C.c_void_p]
                getattr(L, f"gh_tile_{d}{e}").argtypes = [C.POINTER(GhArgs), C.c_void_p]
                getattr(L, f"gh_block_{d}{e}").argtypes = [C.c_int, C.POINTER(GhArgs), C.c_void_p]
                getattr(L, f"gh_strip_{d}{e}").argtypes = [C.c_int, C.POINTER(GhArgs), C.c_void_p]
        for e in EPIS:
            getattr(L, f"gh_glds_dispatch_t{e}").argtypes = [C.POINTER(GhArgs), C.c_void_p]
            getattr(L, f"gh_glds_t{e}").argtypes = [C.POINTER(C.c_int), C.POINTER(GhArgs), C.c_void_p]

    def error(self):
        return self.lib.gh_last_error().decode()

    def glds_instances(self):
        """(EPI, BNS, BMT, WN, WM, NST, RP) of every gemm_glds_kernel instance the harness launches directly."""
        n = self.lib.gh_glds_instances(None, 0)
        buf = (C.c_int * (7 * n))()
        self.lib.gh_glds_instances(buf, n)
        return [tuple(buf[7 * i:7 * i + 7]) for i in range(n)]

    # each launcher returns the PTTS_* status; `bf16` selects the engine dtype (glds: bf16 only)
    def pack(self, bf16, src, dst, N, K, stream):
        return self.lib.gh_pack(int(bf16), src, dst, N, K, stream)

    def gemm(self, bf16, epi, a, stream):
        return getattr(self.lib, f"gh_gemm_{'t' if bf16 else 'f'}{epi}")(C.byref(a), stream)

    def tile(self, bf16, epi, a, stream):
        return getattr(self.lib, f"gh_tile_{'t' if bf16 else 'f'}{epi}")(C.byref(a), stream)

    def block(self, bf16, epi, ns, a, stream):
        return getattr(self.lib, f"gh_block_{'t' if bf16 else 'f'}{epi}")(ns, C.byref(a), stream)

    def strip(self, bf16, epi, by_value, a, stream):
        return getattr(self.lib, f"gh_strip_{'t' if bf16 else 'f'}{epi}")(int(by_value), C.byref(a), stream)

    def glds_dispatch(self, epi, a, stream):
        return getattr(self.lib, f"gh_glds_dispatch_t{epi}")(C.byref(a), stream)

    def glds(self, inst, a, stream):
        t = (C.c_int * 7)(*inst)
        return getattr(self.lib, f"gh_glds_t{inst[0]}")(t, C.byref(a), stream)
