"""Build and load tests/native/dac_harness.hip: the DAC codec's kernels (conv_mfma_kernel, conv_lds_kernel, resunit_lds_kernel, the final convolution,
conv_in_kernel, the RVQ kernels, the pack kernels) and their dispatch (ptts_dac_launch.h) behind thin C entry points that take device pointers."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "dac_harness.hip")
PTTS_OK, PTTS_E_INVALID, PTTS_E_UNSUPPORTED = 0, -1, -5
CONV_MFMA, CONV_LDS = 0, 1
ENTRY_POINTS = ("dh_last_error", "dh_sizes", "dh_conv_plan", "dh_resunit_plan", "dh_conv_out_plan", "dh_pack_plan", "dh_instances", "dh_conv", "dh_resunit",
                "dh_conv_out", "dh_conv_in", "dh_rvq_table", "dh_rvq_gather", "dh_cb_normalize", "dh_rvq_encode", "dh_snake")
# dh_instances kinds and how many template arguments each lists
KINDS = ("conv_mfma_kernel", "conv_lds_kernel", "resunit_lds_kernel", "conv_out_tanh_kernel", "conv_out_tanh_lds_kernel", "rvq_gather_kernel")
WIDTH = (2, 5, 6, 1, 1, 1)
PARTS = ("CONV", "RES", "MISC")
MAXTAPS = 8


def build(out_dir):
    """Three translation units compiled in parallel with build()'s hipcc flags, linked against torch's HIP runtime as the product library is."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)

    def compile_part(part):
        obj = os.path.join(out_dir, f"dac_harness_{part.lower()}.o")
        cmd = ["hipcc"] + HIPCC_FLAGS + ["-fvisibility=hidden", "-Wno-unused-function", "-I", CSRC, f"-DDH_PART_{part}", "-c", SRC, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
        return obj

    with ThreadPoolExecutor(max_workers=min(16, len(PARTS))) as ex:
        objs = list(ex.map(compile_part, PARTS))
    lib = os.path.join(out_dir, "libdac_harness.so")
    subprocess.check_call(["g++", "-shared", "-o", lib] + objs + ["-L" + torch_lib, "-l:libamdhip64.so", "-Wl,-rpath," + torch_lib])
    return lib


class ConvShape(C.Structure):
    """struct DacConvShape of ptts_dac_launch.h."""
    _fields_ = [(n, C.c_int) for n in ("Cin", "Cout", "ksize", "dil", "stride", "transposed", "bf16", "pad")]


class ConvPlan(C.Structure):
    """struct DacConvPlan."""
    _fields_ = [("kernel", C.c_int), ("p", C.c_int * 5)] + [(n, C.c_uint) for n in ("grid_x", "grid_y", "block", "lds")]

    def instance(self):
        return (self.kernel,) + tuple(self.p)


class ResPlan(C.Structure):
    """struct DacResPlan."""
    _fields_ = [(n, C.c_int) for n in ("NW", "WD", "RAW", "F32", "XIN", "ACT")] + [(n, C.c_uint) for n in ("grid_x", "block", "lds")]

    def instance(self):
        return (self.NW, self.WD, self.RAW, self.F32, self.XIN, self.ACT)


class OutPlan(C.Structure):
    """struct DacOutPlan."""
    _fields_ = [("lds_kernel", C.c_int)] + [(n, C.c_uint) for n in ("grid_x", "grid_y", "block", "lds")]


class PackPlan(C.Structure):
    """struct DacPackPlan."""
    _fields_ = [("ktap", C.c_int * (MAXTAPS * 8)), ("s_co", C.c_longlong), ("s_ci", C.c_longlong), ("s_k", C.c_longlong), ("ntaps", C.c_int), ("nphase", C.c_int)]


class DhConv(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x", "w", "bias", "skip", "out_raw", "out_act", "alpha", "lens", "Wp", "ktap")] + [("shape", ConvShape)] + \
               [(n, C.c_int) for n in ("B", "Tin", "len_mul", "act_f32", "forced")] + [("plan", ConvPlan)]


class DhRes(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x", "w7", "b7", "alpha7", "w1", "b1", "alpha1", "skip", "out_raw", "out_act", "alpha_in", "lens", "Wp7", "Wp1", "ktap")] + \
               [(n, C.c_int) for n in ("C", "dil", "B", "T", "len_mul", "act_f32")] + [("plan", ResPlan)]


class DhOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x", "w", "bias", "wt", "out", "skip_of", "t_end_of", "lens")] + [("out_ld", C.c_longlong)] + \
               [(n, C.c_int) for n in ("B", "T", "C", "skip", "t_end", "len_mul", "rows", "force_direct")]


class DhGather(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("codes", "tab", "p_lens", "start", "slot", "table", "z", "lens")] + [("ld", C.c_longlong)] + \
               [(n, C.c_int) for n in ("cap", "K", "T", "B", "ncodes", "latent", "z_bf16", "t0", "stream")]


class DhEncode(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("z", "in_w", "in_b", "cb", "cbn", "cbn_sq", "out_w", "out_b", "codes")] + \
               [(n, C.c_int) for n in ("B", "T", "latent", "cdim", "ncodes", "nq")]


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        L = self.lib
        L.dh_last_error.restype = C.c_char_p
        L.dh_sizes.argtypes = [C.c_int]
        for which, st in enumerate((DhConv, DhRes, DhOut, DhGather, DhEncode, ConvShape, ConvPlan, ResPlan, OutPlan, PackPlan)):
            assert L.dh_sizes(which) == C.sizeof(st), f"{st.__name__} layout differs between the harness and tests/dac_harness.py"
        L.dh_conv_plan.argtypes = [C.POINTER(ConvShape), C.c_int, C.c_int, C.POINTER(ConvPlan)]
        L.dh_conv_plan.restype = None
        L.dh_resunit_plan.argtypes = [C.POINTER(ConvShape), C.POINTER(ConvShape), C.c_int, C.c_int, C.c_longlong] + [C.c_int] * 6 + [C.POINTER(ResPlan)]
        L.dh_conv_out_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OutPlan)]
        L.dh_conv_out_plan.restype = None
        L.dh_pack_plan.argtypes = [C.POINTER(ConvShape), C.POINTER(PackPlan)]
        L.dh_pack_plan.restype = None
        L.dh_instances.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
        L.dh_conv.argtypes = [C.POINTER(DhConv), C.c_void_p]
        L.dh_resunit.argtypes = [C.POINTER(DhRes), C.c_void_p]
        L.dh_conv_out.argtypes = [C.POINTER(DhOut), C.c_void_p]
        L.dh_conv_in.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]
        L.dh_rvq_table.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p]
        L.dh_rvq_gather.argtypes = [C.POINTER(DhGather), C.c_void_p]
        L.dh_cb_normalize.argtypes = [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p]
        L.dh_rvq_encode.argtypes = [C.POINTER(DhEncode), C.c_void_p]
        L.dh_snake.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]

    def error(self):
        return self.lib.dh_last_error().decode()

    def instances(self):
        """{kernel name: [template arguments as the harness lists them]}."""
        out = {}
        for kind, name in enumerate(KINDS):
            n = self.lib.dh_instances(kind, None, 0)
            buf = (C.c_int * (6 * n))()
            self.lib.dh_instances(kind, buf, n)
            out[name] = [tuple(buf[6 * i:6 * i + WIDTH[kind]]) for i in range(n)]
        return out

    # ---- pure host
    def conv_plan(self, shape, B, Tin):
        p = ConvPlan()
        self.lib.dh_conv_plan(C.byref(shape), B, Tin, C.byref(p))
        return p

    def resunit_plan(self, c7, c1, no_fuse=0, xin_mask=-1, frames=0, B=1, T=1, raw=1, act_f32=0, xin=0, act=1):
        """(fusable, xin at this width and size, the plan or None where the outputs are refused)."""
        p = ResPlan()
        rc = self.lib.dh_resunit_plan(C.byref(c7), C.byref(c1), no_fuse, xin_mask, frames, B, T, raw, act_f32, xin, act, C.byref(p))
        return bool(rc & 1), bool(rc & 2), None if rc & 4 else p

    def conv_out_plan(self, Cw, B, T, force_direct=False):
        p = OutPlan()
        self.lib.dh_conv_out_plan(Cw, B, T, int(force_direct), C.byref(p))
        return p

    def pack_plan(self, shape):
        p = PackPlan()
        self.lib.dh_pack_plan(C.byref(shape), C.byref(p))
        return p

    # ---- launchers: each returns the PTTS_* status
    def conv(self, a, stream):
        return self.lib.dh_conv(C.byref(a), stream)

    def resunit(self, a, stream):
        return self.lib.dh_resunit(C.byref(a), stream)

    def conv_out(self, a, stream):
        return self.lib.dh_conv_out(C.byref(a), stream)

    def rvq_gather(self, a, stream):
        return self.lib.dh_rvq_gather(C.byref(a), stream)

    def rvq_encode(self, a, stream):
        return self.lib.dh_rvq_encode(C.byref(a), stream)
