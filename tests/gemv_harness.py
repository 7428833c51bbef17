"""Build and load tests/native/gemv_harness.hip: the product's row-per-wave GEMV decode step (gemv_kernel with every prologue / epilogue pair of
gemv_step, qkv_attn_kernel, xfold_attn_kernel, xq_attn_kernel) behind thin C entry points that take device pointers and buffer extents (see the
.hip file). The kernels are the product's three translation units ptts_gemv_{bf16,f32,w8}.hip: the objects build() left beside the sources where
they are newer than every source and header, else compiled here as further parts with build()'s flags."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import step_plan as SP
from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "gemv_harness.hip")
UNITS = ("ptts_gemv_bf16", "ptts_gemv_f32", "ptts_gemv_w8")  # the product's GEMV translation units

PTTS_OK, PTTS_E_INVALID, PTTS_E_HIP, PTTS_E_UNSUPPORTED = 0, -1, -2, -5
GV_LN, GV_ATTN, GV_COPY, GV_SOFTMAX, GV_ATTN2, GV_LNP = 0, 1, 2, 3, 4, 5
GV_STORE, GV_RESID, GV_GELU_WT = 0, 1, 2
GV_F32, GV_BF16, GV_BF16_W8 = 0, 1, 2
MODES = (GV_F32, GV_BF16, GV_BF16_W8)
PRO_NAMES = {GV_LN: "LN", GV_ATTN: "ATTN", GV_COPY: "COPY", GV_SOFTMAX: "SOFTMAX", GV_ATTN2: "ATTN2", GV_LNP: "LNP"}
EPI_NAMES = {GV_STORE: "STORE", GV_RESID: "RESID", GV_GELU_WT: "GELU_WT"}
MODE_NAMES = {GV_F32: "fp32", GV_BF16: "bf16", GV_BF16_W8: "w8"}
ENTRY_POINTS = ("gvh_last_error", "gvh_args_size", "gvh_const", "gvh_gemv_k_ok", "gvh_qkvattn_ok", "gvh_xfoldattn_ok", "gvh_xqattn_ok",
                "gvh_qkvattn_rows_per_split", "gvh_gemv", "gvh_qkvattn", "gvh_xfoldattn", "gvh_xqattn",
                "gvh_step_config", "gvh_default_switches", "gvh_step_config_size", "gvh_gemv_plan")  # the last four: host only, the product's plan


def _headers():
    inc = os.path.join(ROOT, "include")
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))] + [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")]


def product_object(unit):
    """The object build() left beside the sources, if it is newer than its source and every header (build()'s own rule); else None."""
    obj, src = os.path.join(CSRC, unit + ".o"), os.path.join(CSRC, unit + ".hip")
    if not os.path.exists(obj):
        return None
    t = os.path.getmtime(obj)
    return obj if all(os.path.getmtime(f) <= t for f in [src] + _headers()) else None


def build(out_dir):
    """Compile the harness part, and the product's GEMV units that have no fresh object, in parallel; link them against torch's HIP runtime, as
    __graft_entry__.build() links the product library. Returns the library path; build.reused holds the product objects linked as they were."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    jobs = [(SRC, os.path.join(out_dir, "gemv_harness.o"), ["-fvisibility=hidden"])]
    objs, build.reused = [jobs[0][1]], []
    for u in UNITS:
        o = product_object(u)
        if o is None:  # as a part, with build()'s flags
            o = os.path.join(out_dir, u + ".o")
            jobs.append((os.path.join(CSRC, u + ".hip"), o, []))
        else:
            build.reused.append(u)
        objs.append(o)

    def compile_part(j):
        src, obj, extra = j
        cmd = ["hipcc"] + HIPCC_FLAGS + extra + ["-I", CSRC, "-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
        return obj

    with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        list(ex.map(compile_part, jobs))
    # the product's units are compiled with default visibility: the version script keeps their symbols (ptts_gemv_launch, ...) local, so the harness's
    # copies cannot interpose on the product library's in a process that loads both
    vs = os.path.join(out_dir, "gemv_harness.map")
    with open(vs, "w") as f:
        f.write("{ global: " + " ".join(n + ";" for n in ENTRY_POINTS) + " local: *; };\n")
    lib = os.path.join(out_dir, "libgemv_harness.so")
    subprocess.check_call(["g++", "-shared", "-o", lib] + objs + ["-Wl,--version-script=" + vs, "-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


def _struct(ptrs, sizes, ints, floats=(), tail=()):
    return [(n, C.c_void_p) for n in ptrs] + [(n, C.c_longlong) for n in sizes] + [(n, C.c_int) for n in ints] + [(n, C.c_float) for n in floats] + [(n, C.c_int) for n in tail]


class GvhGemv(C.Structure):
    """struct GvhGemv of gemv_harness.hip."""
    _fields_ = _struct(("W", "wscale", "x", "xw", "resid", "part", "stats", "gamma", "beta", "mask", "n_valid", "out", "hsum"),
                       ("n_W", "n_wscale", "n_x", "n_xw", "n_resid", "n_part", "n_stats", "n_gamma", "n_mask", "n_out", "n_hsum"),
                       ("mode", "pro", "epi", "S", "M", "N", "K", "npart", "nheads", "ne", "x_ld", "xw_ld", "out_ld", "pad_"))


class GvhQkvAttn(C.Structure):
    """struct GvhQkvAttn of gemv_harness.hip."""
    _fields_ = _struct(("W", "wscale", "x", "gamma", "beta", "kcache", "vcache", "cur_len", "P", "mask", "part", "stats"),
                       ("n_W", "n_wscale", "n_x", "n_gamma", "n_cache", "n_cur_len", "n_mask", "n_part", "n_stats"),
                       ("mode", "S", "M", "H", "nheads", "kv_heads", "x_ld", "cap", "kv_bound", "mask_ld"), ("scale",), ("pad_",))


class GvhXfold(C.Structure):
    """struct GvhXfold of gemv_harness.hip."""
    _fields_ = _struct(("Mw", "Uw", "x", "gamma", "beta", "n_valid", "mask", "xpart"), ("n_Mw", "n_Uw", "n_x", "n_gamma", "n_mask", "n_xpart"),
                       ("mode", "H", "nheads", "nur"))


class GvhXq(C.Structure):
    """struct GvhXq of gemv_harness.hip."""
    _fields_ = _struct(("W", "wscale", "x", "gamma", "beta", "kcache", "vcache", "mask", "n_valid", "out"),
                       ("n_W", "n_wscale", "n_x", "n_gamma", "n_cache", "n_mask", "n_out"),
                       ("mode", "M", "H", "nheads", "kv_heads", "x_ld", "out_ld", "mask_ld", "cap"), ("scale",))


STRUCTS = (GvhGemv, GvhQkvAttn, GvhXfold, GvhXq)


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.gvh_last_error.restype = C.c_char_p
        L.gvh_args_size.argtypes = [C.c_int]
        for which, st in enumerate(STRUCTS):
            assert L.gvh_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between gemv_harness.hip and tests/gemv_harness.py"
        for n in ("gvh_const", "gvh_qkvattn_rows_per_split"):
            getattr(L, n).argtypes = [C.c_int]
        for n in ("gvh_gemv_k_ok", "gvh_qkvattn_ok", "gvh_xqattn_ok"):
            getattr(L, n).argtypes = [C.c_int, C.c_int]
        L.gvh_xfoldattn_ok.argtypes = [C.c_int, C.c_int, C.c_int]
        for n, st in (("gvh_gemv", GvhGemv), ("gvh_qkvattn", GvhQkvAttn), ("gvh_xfoldattn", GvhXfold), ("gvh_xqattn", GvhXq)):
            getattr(L, n).argtypes = [C.POINTER(st), C.c_void_p]
        self.PMAX, self.MAX_ROWS = L.gvh_const(0), L.gvh_const(1)
        L.gvh_default_switches.argtypes = [C.POINTER(SP.StepSwitches)]
        sw = SP.StepSwitches(**{n: -99 for n in SP.StepSwitches.DEFAULTS})
        assert L.gvh_default_switches(C.byref(sw)) == C.sizeof(SP.StepSwitches) and L.gvh_step_config_size() == C.sizeof(SP.StepConfig), "ptts_step_plan.h / tests/step_plan.py"
        assert {n: getattr(sw, n) for n in SP.StepSwitches.DEFAULTS} == SP.StepSwitches.DEFAULTS, "StepSwitches defaults differ between ptts_step_plan.h and tests/step_plan.py"
        L.gvh_step_config.argtypes = [C.c_void_p, C.POINTER(SP.StepConfig)]
        L.gvh_gemv_plan.argtypes = [C.c_void_p, C.POINTER(SP.StepSwitches), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]

    def error(self):
        return self.lib.gvh_last_error().decode()

    # each launcher returns a PTTS_* status
    def gemv(self, a, stream):
        return self.lib.gvh_gemv(C.byref(a), stream)

    def qkvattn(self, a, stream):
        return self.lib.gvh_qkvattn(C.byref(a), stream)

    def xfoldattn(self, a, stream):
        return self.lib.gvh_xfoldattn(C.byref(a), stream)

    def xqattn(self, a, stream):
        return self.lib.gvh_xqattn(C.byref(a), stream)

    def gemv_k_ok(self, K, mode):
        return bool(self.lib.gvh_gemv_k_ok(K, mode))

    def qkvattn_ok(self, H, mode):
        return bool(self.lib.gvh_qkvattn_ok(H, mode))

    def xfoldattn_ok(self, H, nheads, mode):
        return bool(self.lib.gvh_xfoldattn_ok(H, nheads, mode))

    def xqattn_ok(self, H, mode):
        return bool(self.lib.gvh_xqattn_ok(H, mode))

    def rows_per_split(self, mode):
        return self.lib.gvh_qkvattn_rows_per_split(mode)

    # ---- the product's plan (ptts_step_plan.h), host only ----
    def step_config(self, cfg):
        """StepConfig of a ptts_config (step_plan.config), or None where the harness declines the config."""
        out = SP.StepConfig()
        return out if self.lib.gvh_step_config(C.addressof(cfg), C.byref(out)) == PTTS_OK else None

    def gemv_plan(self, cfg, sw, M, kv_bound, xfold_valid):
        """(launches, per_layer, head, cross, fuse_qa, S_f) of one gemv_step: launches = [(pro, epi, S, M, N, K, mode)] in launch order, per_layer / head =
        kernel launches of one layer / of the head projection. None where M utterances of this engine do not run the GEMV step."""
        cap = 8 * cfg.num_layers + 1
        buf, counts = (C.c_int * (7 * cap))(), (C.c_int * 5)()
        n = self.lib.gvh_gemv_plan(C.addressof(cfg), C.byref(sw), M, kv_bound, int(xfold_valid), buf, cap, counts)
        if n < 0:
            return None
        assert n <= cap
        return ([tuple(buf[7 * i:7 * i + 7]) for i in range(n)],) + tuple(counts)
