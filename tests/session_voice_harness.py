"""Build and load tests/native/session_voice_harness.hip: tail_launch with the per-slot voice-prompt lengths of a continuous session,
embed_kernel<float, true> with them, and the product's kernels a voice admission runs on the sampler state, behind thin C entry points that
take device pointers (see the .hip file). The operands of a launch are tail_harness.ThArgs."""
import ctypes as C
import os
import subprocess

import slot_gen_harness as SG
import tail_harness as TH
from gemm_harness import CSRC, HIPCC_FLAGS, ROOT

SRC = os.path.join(ROOT, "tests", "native", "session_voice_harness.hip")
ENTRY_POINTS = ("sv_last_error", "sv_args_size", "sv_tail", "sv_embed", "sv_set_prefix")


def build(out_dir):
    """One translation unit with build()'s hipcc flags, linked as tail_harness.build() links its own."""
    import torch

    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    os.makedirs(out_dir, exist_ok=True)
    obj, lib = os.path.join(out_dir, "session_voice_harness.o"), os.path.join(out_dir, "libsession_voice_harness.so")
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
        L.sv_last_error.restype = C.c_char_p
        L.sv_args_size.argtypes = [C.c_int]
        for which, st in enumerate((TH.ThArgs, TH.DevGen, TH.DevDims, SG.SlotGen)):
            assert L.sv_args_size(which) == C.sizeof(st), f"{st.__name__} layout differs between the harness and its Python description"
        assert L.sv_args_size(3) == 48  # SlotGen keeps its layout
        L.sv_tail.argtypes = [C.POINTER(TH.ThArgs), C.c_void_p, C.c_void_p, C.c_void_p]
        L.sv_embed.argtypes = [C.POINTER(TH.ThArgs), C.c_void_p, C.c_void_p]
        L.sv_set_prefix.argtypes = [C.POINTER(TH.ThArgs), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]

    def error(self):
        return self.lib.sv_last_error().decode()

    # each launcher returns the PTTS_* status
    def tail(self, a, slot_gen, slot_tprefix, stream):
        return self.lib.sv_tail(C.byref(a), slot_gen, slot_tprefix, stream)

    def embed(self, a, slot_tprefix, stream):
        return self.lib.sv_embed(C.byref(a), slot_tprefix, stream)

    def set_prefix(self, a, prefix, prefix_ld, slot_tprefix, row, T, max_length, stream):
        return self.lib.sv_set_prefix(C.byref(a), prefix, prefix_ld, slot_tprefix, row, T, max_length, stream)
