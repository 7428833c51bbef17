"""CPU: include/ptts_step_record.h against its ctypes binding (declarations, struct layout) and a torch-free C client; the library exports both
entry points; the harness of the step records (tests/native/record_tail_harness.hip) cross-compiles for gfx950 without a GPU, exports exactly its
entry points and holds exactly the RECORD instances and the logits node the product holds - while tail_kernel / tail_warp_kernel keep their six
instances each under their names."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from parler_tts_amd import _native

import record_tail_harness as RH
import test_device_penalties_cpu as TP
import test_tail_harness_cpu as TT
import test_warp_tail_harness_cpu as TWH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptts_step_record.h")
SYMBOLS = ("ptts_set_step_records", "ptts_set_slot_step_records")
FIELDS = [("float*", "scores_dev"), ("float*", "logits_dev"), ("int32_t", "cap_steps")]


def test_header_declarations_and_ctypes_prototypes_agree_and_ptts_h_keeps_its_46():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r'^#include "ptts.h"', hdr, flags=re.M)
    assert sorted(set(re.findall(r"\b(ptts_\w+)\s*\(", code))) == sorted(SYMBOLS) == sorted(_native.STEP_RECORD_SYMBOLS)
    others = (set(_native.SYMBOLS) | set(_native.SESSION_SYMBOLS) | set(_native.SESSION_KV8_SYMBOLS) | set(_native.SESSION_VOICE_SYMBOLS)
              | set(_native.SESSION_VOICE_ROWS_SYMBOLS) | set(_native.DAC_STREAM_VOICE_SYMBOLS) | set(_native.PENALTY_SYMBOLS) | set(_native.WARP_SYMBOLS)
              | set(_native.SCORE_SYMBOLS) | set(_native.LOGIT_EDIT_SYMBOLS))
    assert not set(_native.STEP_RECORD_SYMBOLS) & others
    C = _native.C
    ctype_of = {"ptts_engine*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "const ptts_step_records*": C.POINTER(_native.PttsStepRecords)}
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/ptts_step_record.h"
        res, args = _native.STEP_RECORD_SYMBOLS[name]
        params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
        assert res is C.c_int and [ctype_of[p] for p in params] == list(args), (name, params)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ptts_step_records\s*;", code)
    fields = [(" ".join(f.split()[:-1]), f.split()[-1]) for f in m.group(1).split(";") if f.strip()]
    assert fields == FIELDS
    field_type = {"float*": C.c_void_p, "int32_t": C.c_int32}
    assert [(n, t) for n, t in _native.PttsStepRecords._fields_] == [(n, field_type[t]) for t, n in FIELDS]
    # ptts.h: the 46 declarations of ABI v8, untouched, and no other header knows this one
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptts.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(ptts_\w+)\s*\(", base))) == 46 == len(_native.SYMBOLS) and _native.ABI_VERSION == 8
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "ptts_step_record.h":
            assert "ptts_step_record" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert '"ptts_step_record.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()  # a change to it rebuilds the library
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read()
    for name in SYMBOLS:
        assert re.search(r'extern "C" int ' + name + r"\(", src), f"{name} is not defined in ptts_lm.hip"
    # the header states the contract and names the reference lines it restates
    for phrase in ("generation/utils.py", "modeling_parler_tts.py:3540", "logits_processors.py:44-53", "cap_steps", "threshold"):
        assert phrase in hdr, phrase


def test_library_exports_the_entry_points_and_a_null_engine_is_a_value_error():
    lib = TP._built_library()
    for name in SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native.STEP_RECORD_SYMBOLS[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(SYMBOLS) <= exported
    rec = _native.PttsStepRecords(None, None, 0)
    with pytest.raises(ValueError, match="null engine"):
        _native.check(lib.ptts_set_step_records(None, ctypes.byref(rec), None), "ptts_set_step_records")
    with pytest.raises(ValueError, match="null engine"):
        _native.check(lib.ptts_set_slot_step_records(None, 0, ctypes.byref(rec), None), "ptts_set_slot_step_records")


def test_torch_free_c_client_of_the_header_builds_links_and_is_refused_with_a_message(tmp_path):
    """The header is plain C99 beside ptts.h (and C++); a client that knows nothing of torch links against the library and gets the refusals."""
    gcc, gxx = shutil.which("gcc"), shutil.which("g++")
    assert gcc is not None and gxx is not None, "no host compiler: the library itself is linked with g++"
    TP._built_library()
    inc = os.path.join(ROOT, "include")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", HEADER])
    src = tmp_path / "client.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\n#include "ptts_logit_edit.h"\n#include "ptts_step_record.h"\n'
                   "int main(void) {\n"
                   "  float buf[8];\n"
                   "  ptts_step_records r = {buf, NULL, 2};\n"
                   "  int a = ptts_set_step_records(NULL, &r, NULL);\n"
                   "  int b = ptts_set_slot_step_records(NULL, 0, NULL, NULL);\n"
                   '  printf("%d %d %d %d %d %s\\n", a != PTTS_OK, b != PTTS_OK, (int)sizeof(r), (int)offsetof(ptts_step_records, logits_dev),\n'
                   "         (int)offsetof(ptts_step_records, cap_steps), ptts_last_error());\n"
                   "  return 0;\n}\n")
    exe = str(tmp_path / "client")
    libdir = os.path.dirname(_native.LIB_PATH)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", exe, "-L" + libdir, "-lptts_hip", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath-link," + torch_lib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    S = _native.PttsStepRecords
    want = f"1 1 {ctypes.sizeof(S)} {S.logits_dev.offset} {S.cap_steps.offset} "
    assert ctypes.sizeof(S) == 24 and out.returncode == 0 and out.stdout.startswith(want) and "null engine" in out.stdout, (out.returncode, out.stdout, out.stderr[-500:])


# ---- the harness ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return RH.Harness(RH.build(str(tmp_path_factory.mktemp("record_tail_harness"))))


def test_harness_cross_compiles_and_exports_its_entry_points(harness):
    out = subprocess.run(["nm", "-D", "--defined-only", harness.lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == set(RH.ENTRY_POINTS), exported ^ set(RH.ENTRY_POINTS)


def test_harness_holds_the_record_instances_of_the_product_and_the_existing_twelve_keep_their_names(harness, tmp_path):
    TP._built_library()
    want = {(nv, s) for nv in (8, 18, 32) for s in (0, 1)}
    for i, pattern in enumerate((r"_Z18tail_record_kernelILi(\d+)ELb([01])EE", r"_Z23tail_warp_record_kernelILi(\d+)ELb([01])EE")):
        product = TWH._kernels_in(_native.LIB_PATH, tmp_path / f"product{i}", pattern)
        assert product == want == TWH._kernels_in(harness.lib._name, tmp_path / f"harness{i}", pattern), (pattern, product)
    node = r"(step_logits_record_kerne)(l)"
    for which, lib in (("product", _native.LIB_PATH), ("harness", harness.lib._name)):
        os.makedirs(str(tmp_path / which), exist_ok=True)
        shutil.copy(lib, str(tmp_path / which / "lib.so"))
        subprocess.run([os.path.join(TT.LLVM, "llvm-objdump"), "--offloading", str(tmp_path / which / "lib.so")], capture_output=True, cwd=str(tmp_path / which), check=True)
        syms = ""
        for f in os.listdir(tmp_path / which):
            if "amdgcn" in f:
                syms += subprocess.run([os.path.join(TT.LLVM, "llvm-readelf"), "--symbols", str(tmp_path / which / f)], capture_output=True, text=True, check=True).stdout
        assert re.search(node, syms) and "set_step_record_kernel" in syms, which
    # the twelve instances of the parent commit, under their names
    assert TT._tail_instances_in(_native.LIB_PATH, tmp_path / "tail") == want
    assert TWH._kernels_in(_native.LIB_PATH, tmp_path / "warp", r"_Z16tail_warp_kernelILi(\d+)ELb([01])EE") == want
