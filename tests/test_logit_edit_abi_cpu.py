"""CPU: include/ptts_logit_edit.h against its ctypes binding (declarations, struct layout) and a torch-free C client; the kernel's harness
(tests/native/logit_edit_harness.hip) cross-compiles for gfx950 without a GPU, exports exactly its entry points and holds the product's kernel,
whose decay is a separately rounded product and sum."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from parler_tts_amd import _native
from parler_tts_amd.engine import DecoderEngine
from parler_tts_amd.generation_extras import LogitEdits

import logit_edit_harness as LH
import test_device_penalties_cpu as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptts_logit_edit.h")
SYMBOLS = ("ptts_set_logit_edits", "ptts_set_slot_logit_edits")
FIELDS = [("const int32_t*", "bias_tokens"), ("const float*", "bias_values"), ("const int32_t*", "bad_tokens"), ("const int32_t*", "suppress_tokens"),
          ("const int32_t*", "begin_suppress_tokens"), ("int32_t", "n_bias"), ("int32_t", "n_bad"), ("int32_t", "n_suppress"), ("int32_t", "n_begin_suppress"),
          ("int32_t", "decay_on"), ("int32_t", "decay_start"), ("double", "decay_factor")]
LLVM = "/opt/rocm/lib/llvm/bin"


def test_header_declarations_and_ctypes_prototypes_agree_and_ptts_h_keeps_its_46():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r'^#include "ptts.h"', hdr, flags=re.M)
    assert sorted(set(re.findall(r"\b(ptts_\w+)\s*\(", code))) == sorted(SYMBOLS) == sorted(_native.LOGIT_EDIT_SYMBOLS)
    others = (set(_native.SYMBOLS) | set(_native.SESSION_SYMBOLS) | set(_native.SESSION_KV8_SYMBOLS) | set(_native.SESSION_VOICE_SYMBOLS)
              | set(_native.SESSION_VOICE_ROWS_SYMBOLS) | set(_native.DAC_STREAM_VOICE_SYMBOLS) | set(_native.PENALTY_SYMBOLS) | set(_native.WARP_SYMBOLS)
              | set(_native.SCORE_SYMBOLS))
    assert not set(_native.LOGIT_EDIT_SYMBOLS) & others
    C = _native.C
    ctype_of = {"ptts_engine*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "const ptts_logit_edits*": C.POINTER(_native.PttsLogitEdits)}
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/ptts_logit_edit.h"
        res, args = _native.LOGIT_EDIT_SYMBOLS[name]
        params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
        assert res is C.c_int and [ctype_of[p] for p in params] == list(args), (name, params)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ptts_logit_edits\s*;", code)
    fields = [(" ".join(f.split()[:-1]), f.split()[-1]) for f in m.group(1).split(";") if f.strip()]
    assert fields == FIELDS
    field_type = {"const int32_t*": C.POINTER(C.c_int32), "const float*": C.POINTER(C.c_float), "int32_t": C.c_int32, "double": C.c_double}
    assert [(n, t) for n, t in _native.PttsLogitEdits._fields_] == [(n, field_type[t]) for t, n in FIELDS]
    # ptts.h: the 46 declarations of ABI v8, untouched, and no other header knows this one
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptts.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(ptts_\w+)\s*\(", base))) == 46 == len(_native.SYMBOLS) and _native.ABI_VERSION == 8
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "ptts_logit_edit.h":
            assert "ptts_logit_edit" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert '"ptts_logit_edit.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()  # a change to it rebuilds the library
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read()
    for name in SYMBOLS:
        assert re.search(r'extern "C" int ' + name + r"\(", src), f"{name} is not defined in ptts_lm.hip"


def test_library_exports_the_entry_points_and_a_null_engine_is_a_value_error():
    lib = TP._built_library()
    for name in SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native.LOGIT_EDIT_SYMBOLS[name][1]
    rec, keep = DecoderEngine._logit_edits(LogitEdits(bias=((3, 1.5),), decay=(4, 1.1)))
    with pytest.raises(ValueError, match="null engine"):
        _native.check(lib.ptts_set_logit_edits(None, ctypes.byref(rec), None), "ptts_set_logit_edits")
    with pytest.raises(ValueError, match="null engine"):
        _native.check(lib.ptts_set_slot_logit_edits(None, 0, ctypes.byref(rec), None), "ptts_set_slot_logit_edits")
    del keep


def test_the_wrapper_lays_the_record_out_as_the_header_does():
    ed = LogitEdits(bias=((3, 1.5), (7, -2.0)), bad=(5,), suppress=(1, 2, 9), begin_suppress=(), decay=(4, 1.25), suppress_on=True, begin_suppress_on=True)
    rec, keep = DecoderEngine._logit_edits(ed)
    assert (rec.n_bias, rec.n_bad, rec.n_suppress, rec.n_begin_suppress, rec.decay_on, rec.decay_start, rec.decay_factor) == (2, 1, 3, 1, 1, 4, 1.25)
    assert [rec.bias_tokens[i] for i in range(2)] == [3, 7] and [rec.bias_values[i] for i in range(2)] == [1.5, -2.0]
    assert rec.bad_tokens[0] == 5 and [rec.suppress_tokens[i] for i in range(3)] == [1, 2, 9]
    assert rec.begin_suppress_tokens[0] == -1  # a list with nothing inside the vocabulary is still a stage: one token the library ignores
    rec, keep = DecoderEngine._logit_edits(None)
    assert (rec.n_bias, rec.n_bad, rec.n_suppress, rec.n_begin_suppress, rec.decay_on) == (0, 0, 0, 0, 0) and LogitEdits().neutral and not ed.neutral


def test_torch_free_c_client_of_the_header_builds_links_and_is_refused_with_a_message(tmp_path):
    """The header is plain C99 beside ptts.h (and C++); a client that knows nothing of torch links against the library and gets the refusals."""
    gcc, gxx = shutil.which("gcc"), shutil.which("g++")
    assert gcc is not None and gxx is not None, "no host compiler: the library itself is linked with g++"
    TP._built_library()
    inc = os.path.join(ROOT, "include")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", HEADER])
    src = tmp_path / "client.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\n#include "ptts_penalty.h"\n#include "ptts_warp.h"\n#include "ptts_logit_edit.h"\n'
                   "int main(void) {\n"
                   "  int32_t toks[2] = {3, 7};\n  float vals[2] = {1.5f, -2.0f};\n"
                   "  ptts_logit_edits le = {toks, vals, toks, toks, NULL, 2, 1, 2, 0, 1, 4, 1.25};\n"
                   "  int a = ptts_set_logit_edits(NULL, &le, NULL);\n"
                   "  int b = ptts_set_slot_logit_edits(NULL, 0, NULL, NULL);\n"
                   '  printf("%d %d %d %d %d %s\\n", a != PTTS_OK, b != PTTS_OK, (int)sizeof(le), (int)offsetof(ptts_logit_edits, n_bias),\n'
                   "         (int)offsetof(ptts_logit_edits, decay_factor), ptts_last_error());\n"
                   "  return 0;\n}\n")
    exe = str(tmp_path / "client")
    libdir = os.path.dirname(_native.LIB_PATH)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", exe, "-L" + libdir, "-lptts_hip", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath-link," + torch_lib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    P = _native.PttsLogitEdits
    want = f"1 1 {ctypes.sizeof(P)} {P.n_bias.offset} {P.decay_factor.offset} "
    assert ctypes.sizeof(P) == 72 and out.returncode == 0 and out.stdout.startswith(want) and "null engine" in out.stdout, (out.returncode, out.stdout, out.stderr[-500:])


# ---- the kernel's harness -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return LH.Harness(LH.build(str(tmp_path_factory.mktemp("logit_edit_harness"))))


def _code_objects(lib, tmp_path):
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copy(lib, str(tmp_path / "lib.so"))  # the code objects are written next to the file they come from
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(tmp_path / "lib.so")], capture_output=True, cwd=str(tmp_path), check=True)
    objs = [str(tmp_path / f) for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert objs, "no embedded gfx950 code objects found"
    return objs


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == set(LH.ENTRY_POINTS), exported ^ set(LH.ENTRY_POINTS)
    assert harness.max_vocab == 2048


def test_product_and_harness_hold_the_kernel_and_its_decay_is_not_fused(harness, tmp_path):
    TP._built_library()
    for which, lib in (("product", _native.LIB_PATH), ("harness", harness.lib._name)):
        names = set()
        for obj in _code_objects(lib, tmp_path / which):
            syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", obj], capture_output=True, text=True, check=True).stdout
            names |= set(re.findall(r"\b(_ZL?\d+(?:logit_edit_kernel|copy_logit_edit_kernel)\w*)", syms))
        assert any("17logit_edit_kernel" in n for n in names) and any("22copy_logit_edit_kernel" in n for n in names), (which, names)
    # the harness is one small translation unit: its disassembly is the kernel's. A product and a sum, never a fused multiply-add
    asm = ""
    for obj in _code_objects(harness.lib._name, tmp_path / "asm"):
        asm += subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", obj], capture_output=True, text=True, check=True).stdout
    body = asm.split("logit_edit_kernel", 1)[1]
    assert "v_mul_f32" in body and "v_add_f32" in body
    assert not re.search(r"\bv_(fma|fmac|mac|mad)_f32", asm)
