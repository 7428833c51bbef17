"""Build and load tests/native/step_harness.hip: the product's batched decode-step kernels (the strip GEMMs with every prologue / epilogue pair
of strip_path, rows_prep_kernel, lnproj_fused_kernel, xattn_fused_kernel, the e4m3 strips of ptts_lm_w8.hip) behind thin C entry points that take
device pointers (see the .hip file), and the product's plan of a strip-path forward (ptts_step_plan.h) behind host-only ones. The plan asks the
product's GEMV translation units which widths they serve (ptts_gemv_k_ok), so their objects are linked in as tests/gemv_harness.py links them: the ones
build() left beside the sources where they are fresh, else compiled here as further parts."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import step_plan as SP
from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "step_harness.hip")
W8_SRC = os.path.join(CSRC, "ptts_lm_w8.hip")  # the product's own translation unit of the e4m3 strips: ptts_strip_w8_launch is the product's

PTTS_OK, PTTS_E_INVALID, PTTS_E_UNSUPPORTED = 0, -1, -5
PRO_PLAIN, PRO_LN, PRO_ATTN, PRO_COPY, PRO_LNS, PRO_RMS = 0, 1, 2, 3, 4, 5
EPI_STORE, EPI_GELU, EPI_RESID, EPI_GELU_WT = 0, 1, 2, 4
PRO_NAMES = {PRO_PLAIN: "PLAIN", PRO_LN: "LN", PRO_ATTN: "ATTN", PRO_COPY: "COPY", PRO_LNS: "LNS"}
EPI_NAMES = {EPI_STORE: "STORE", EPI_GELU: "GELU", EPI_RESID: "RESID", EPI_GELU_WT: "GELU_WT"}
# the (prologue, epilogue) pairs that strip_path and its ln_gemm / prep_copy_gemm instantiate (ptts_lm.hip)
GEMM_PAIRS = ((PRO_COPY, EPI_STORE), (PRO_COPY, EPI_RESID), (PRO_COPY, EPI_GELU_WT), (PRO_LNS, EPI_STORE), (PRO_LNS, EPI_GELU_WT),
              (PRO_LN, EPI_STORE), (PRO_LN, EPI_GELU), (PRO_LN, EPI_GELU_WT), (PRO_ATTN, EPI_RESID), (PRO_PLAIN, EPI_RESID))
KINDS = ("lnproj_fused_kernel", "xattn_fused_kernel", "rows_prep_kernel", "gemm_strip_kernel_w8")  # sh_instances kinds
KIND_WIDTH = (5, 4, 2, 3)


def entry_points():
    names = {"sh_last_error", "sh_args_size", "sh_instances", "sh_pack", "sh_pack_w8", "sh_plan_size", "sh_lns_fits", "sh_strip_plan"}
    for d in "tf":
        names |= {f"sh_gemm_{d}{p}{e}" for p, e in GEMM_PAIRS} | {f"sh_rows_prep_{d}", f"sh_lnproj_{d}", f"sh_xattn_{d}"}
    return names


def parts():
    """(tag, source, defines) of the translation units; tag t = bf16, f = fp32."""
    out = [("common", SRC, ["-DSH_COMMON"]), ("w8", W8_SRC, [])]
    for d, wt in (("t", "bf16_t"), ("f", "float")):
        for p, e in GEMM_PAIRS:
            out.append((f"gemm_{d}{p}{e}", SRC, ["-DSH_GEMM", f"-DSH_WT={wt}", f"-DSH_PRO={p}", f"-DSH_EPI={e}", f"-DSH_TAG={d}{p}{e}"]))
        for kind in ("PREP", "LNPROJ", "XATTN"):
            out.append((f"{kind.lower()}_{d}", SRC, [f"-DSH_{kind}", f"-DSH_WT={wt}", f"-DSH_TAG={d}"]))
    return out


def build(out_dir):
    """Compile every part in parallel (at most 16 at a time) and link them against torch's HIP runtime, as __graft_entry__.build() links the
    product library."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)

    def compile_part(p):
        tag, src, defs = p
        obj = os.path.join(out_dir, f"step_harness_{tag}.o")
        cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-I", CSRC] + defs + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
        return obj

    from gemv_harness import UNITS, product_object

    def compile_unit(u):  # the product's own object, or the unit compiled with build()'s flags
        obj = product_object(u)
        if obj is None:
            obj = os.path.join(out_dir, u + ".o")
            cmd = ["hipcc"] + HIPCC_FLAGS + ["-I", CSRC, "-c", os.path.join(CSRC, u + ".hip"), "-o", obj]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
        return obj

    with ThreadPoolExecutor(max_workers=min(16, len(parts()) + len(UNITS), os.cpu_count() or 1)) as ex:
        units = [ex.submit(compile_unit, u) for u in UNITS]
        objs = list(ex.map(compile_part, parts())) + [u.result() for u in units]
    # the product's units are compiled with default visibility: the version script keeps their symbols local (as tests/gemv_harness.py does)
    vs = os.path.join(out_dir, "step_harness.map")
    with open(vs, "w") as f:
        f.write("{ global: " + " ".join(n + ";" for n in sorted(entry_points())) + " local: *; };\n")
    lib = os.path.join(out_dir, "libstep_harness.so")
    subprocess.check_call(["g++", "-shared", "-o", lib] + objs + ["-Wl,--version-script=" + vs, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class ShGemm(C.Structure):
    """struct ShGemm of step_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("W", "W8", "wscale", "x", "out", "dst", "gamma", "beta", "part", "stats", "stats_out", "lnstat")] + \
               [(n, C.c_int) for n in ("M", "N", "K", "x_ld", "out_ld", "x_row_mul", "x_row_off", "x_fo", "out_fo", "decode", "S", "nheads")]


class ShLnProj(C.Structure):
    """struct ShLnProj of step_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("W", "x", "gamma", "beta", "out", "kcache", "vcache")] + \
               [(n, C.c_int) for n in ("M", "N", "K", "x_ld", "out_ld", "out_fo", "kv_Q", "kv_cap", "kv_heads", "kv_H")]


class ShXAttn(C.Structure):
    """struct ShXAttn of step_harness.hip."""
    _fields_ = [(n, C.c_void_p) for n in ("W", "x", "gamma", "beta", "kcache", "vcache", "cur_len", "dims", "mask", "cos", "sin", "out")] + \
               [(n, C.c_int) for n in ("B", "K", "x_ld", "x_row_mul", "x_row_off", "cap", "mask_ld", "nheads", "kv_heads", "n_rep", "out_fo")] + \
               [("scale", C.c_float)]


class DevDims(C.Structure):
    """struct DevDims of ptts_lm_kernels.h (written into a device buffer as raw bytes)."""
    _fields_ = [("P", C.c_int), ("N", C.c_int), ("max_length", C.c_int), ("T_prefix", C.c_int), ("prefix", C.c_void_p), ("prefix_ld", C.c_int)]


STRUCTS = (ShGemm, ShLnProj, ShXAttn, DevDims)


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.sh_last_error.restype = C.c_char_p
        L.sh_args_size.argtypes = [C.c_int]
        for which, st in enumerate(STRUCTS):
            assert L.sh_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between step_harness.hip and tests/step_harness.py"
        L.sh_instances.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
        L.sh_pack.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.sh_pack_w8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        for which, st in enumerate((SP.StepSwitches, SP.StepConfig, SP.StripPlan)):
            assert L.sh_plan_size(which) == C.sizeof(st), f"{st.__name__} layout differs between ptts_step_plan.h and tests/step_plan.py"
        L.sh_strip_plan.argtypes = [C.c_void_p, C.POINTER(SP.StepSwitches), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SP.StripPlan), C.POINTER(C.c_int)]
        for d in "tf":
            for p, e in GEMM_PAIRS:
                getattr(L, f"sh_gemm_{d}{p}{e}").argtypes = [C.POINTER(ShGemm), C.c_void_p]
            getattr(L, f"sh_rows_prep_{d}").argtypes = [C.c_int, C.POINTER(ShGemm), C.c_void_p]
            getattr(L, f"sh_lnproj_{d}").argtypes = [C.c_int, C.c_int, C.POINTER(ShLnProj), C.c_void_p]
            getattr(L, f"sh_xattn_{d}").argtypes = [C.c_int, C.POINTER(ShXAttn), C.c_void_p]

    def error(self):
        return self.lib.sh_last_error().decode()

    def instances(self):
        """{kind: [template arguments as the harness lists them]}: lnproj_fused_kernel (bf16, UW, NF4, G, EPI), xattn_fused_kernel (bf16, UW, NF4, G),
        rows_prep_kernel (bf16, PRO), the e4m3 gemm_strip_kernel instances (PRO, EPI, MTP)."""
        out = {}
        for kind, name in enumerate(KINDS):
            n = self.lib.sh_instances(kind, None, 0)
            buf = (C.c_int * (5 * n))()
            self.lib.sh_instances(kind, buf, n)
            out[name] = [tuple(buf[5 * i:5 * i + KIND_WIDTH[kind]]) for i in range(n)]
        return out

    # each launcher returns the PTTS_* status; `bf16` selects the engine dtype
    def pack(self, bf16, src, dst, N, K, stream):
        return self.lib.sh_pack(int(bf16), src, dst, N, K, stream)

    def pack_w8(self, src, dst, N, K, stream):
        return self.lib.sh_pack_w8(src, dst, N, K, stream)

    def gemm(self, bf16, pro, epi, a, stream):
        return getattr(self.lib, f"sh_gemm_{'t' if bf16 else 'f'}{pro}{epi}")(C.byref(a), stream)

    def rows_prep(self, bf16, pro, a, stream):
        return getattr(self.lib, f"sh_rows_prep_{'t' if bf16 else 'f'}")(pro, C.byref(a), stream)

    def lnproj(self, bf16, epi, g, a, stream):
        return getattr(self.lib, f"sh_lnproj_{'t' if bf16 else 'f'}")(epi, g, C.byref(a), stream)

    def xattn(self, bf16, gsz, a, stream):
        return getattr(self.lib, f"sh_xattn_{'t' if bf16 else 'f'}")(gsz, C.byref(a), stream)

    # ---- the product's plan (ptts_step_plan.h), host only ----
    def lns_fits(self, M, K, bf16):
        return bool(self.lib.sh_lns_fits(M, K, int(bf16)))

    def strip_plan(self, cfg, sw, prefill, B, Q=1, prefill_attn_mode=3):
        """(StripPlan, kernel launches of one layer, of the head projection) of a prefill over Q positions per utterance or of a decode step, or None
        where the call is no strip-path forward of an engine of this config."""
        plan, counts = SP.StripPlan(), (C.c_int * 2)()
        if self.lib.sh_strip_plan(C.addressof(cfg), C.byref(sw), int(prefill), B, Q, prefill_attn_mode, C.byref(plan), counts) != PTTS_OK:
            return None
        return plan, counts[0], counts[1]
