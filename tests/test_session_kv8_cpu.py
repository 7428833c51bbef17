"""CPU: the additive C ABI of include/ptts_session_kv8.h (continuous sessions on the e4m3 self-attention cache: ptts_session_begin_kv8,
ptts_debug_self_kv), its binding table, and the one line of ``ContinuousBatcher`` that chooses the entry point - driven by the oracle
stand-in of tests/test_continuous_scheduler_cpu.py. What the HIP session computes is covered by tests/test_session_kv8_gpu.py."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

import parler_tts_amd as P
from parler_tts_amd import _native
import test_continuous_scheduler_cpu as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptts_session_kv8.h")
KV8_SYMBOLS = ("ptts_session_begin_kv8", "ptts_debug_self_kv")


def test_header_declares_exactly_the_two_symbols_and_the_tables_are_disjoint():
    hdr = open(HEADER).read()
    assert re.search(r'^#include "ptts.h"', hdr, flags=re.M)
    assert sorted(set(re.findall(r"\b(ptts_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))) == sorted(KV8_SYMBOLS)
    assert sorted(_native.SESSION_KV8_SYMBOLS) == sorted(KV8_SYMBOLS)
    assert not set(_native.SESSION_KV8_SYMBOLS) & (set(_native.SYMBOLS) | set(_native.SESSION_SYMBOLS))
    assert _native.ABI_VERSION == 8
    # the headers it extends do not know it: it is included beside ptts.h
    for name in ("ptts.h", "ptts_session.h"):
        assert "ptts_session_kv8" not in open(os.path.join(ROOT, "include", name)).read()
    # a change to it rebuilds the library
    assert '"ptts_session_kv8.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++17", "-x", "c++"])])
def test_header_compiles_as_c99_and_cxx17(tmp_path, compiler, flags):
    compiler = shutil.which(compiler) or shutil.which({"gcc": "cc", "g++": "c++"}[compiler])
    src = tmp_path / "use.c"
    src.write_text('#include "ptts_session_kv8.h"\n'
                   "int (*begin)(ptts_engine*, int32_t, int32_t, int32_t, void*) = ptts_session_begin_kv8;\n"
                   "int (*kv)(ptts_engine*, int32_t, void**, void**, float**, float**, int32_t*, int32_t*, int32_t*) = ptts_debug_self_kv;\n"
                   "int main(void) { return begin == 0 || kv == 0; }\n")
    subprocess.run([compiler, *flags, "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")],
                   check=True)


def _lib():
    import __graft_entry__

    __graft_entry__.build()  # incremental; cross-compiles without a GPU
    return _native.load_library()


def test_library_exports_both_and_a_null_engine_is_a_value_error():
    lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(KV8_SYMBOLS) <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in KV8_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native.SESSION_KV8_SYMBOLS[name][1]
    with pytest.raises(ValueError, match="null engine"):
        _native.check(lib.ptts_session_begin_kv8(None, 12, 9, 4, None), "ptts_session_begin_kv8")
    out = [ctypes.c_void_p() for _ in range(4)]
    n = [ctypes.c_int32() for _ in range(3)]
    with pytest.raises(ValueError, match="null argument"):
        _native.check(lib.ptts_debug_self_kv(None, 0, *[ctypes.byref(x) for x in out + n]), "ptts_debug_self_kv")


class Kv8SessionEngine(TS.OracleSessionEngine):
    """The stand-in with the e4m3 cache: the scheduler must open its session with ``kv_fp8=True``."""
    kv_fp8 = True

    def begin_session(self, slots, enc_width, prompt_width, kv_fp8=False):
        self.begin_calls = getattr(self, "begin_calls", []) + [kv_fp8]
        super().begin_session(slots, enc_width, prompt_width)


def test_the_batcher_passes_kv_fp8_only_to_an_engine_that_has_the_cache():
    kw = dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, do_sample=False, max_new_tokens=30, min_new_tokens=30)
    reqs = TS._requests(4, seed=5)
    # an engine without the attribute gets the three-argument call: its begin_session has no such keyword
    m, spec, sd, dac, eng, _ = TS._model()
    assert "kv_fp8" not in inspect.signature(eng.begin_session).parameters and not hasattr(eng, "kv_fp8")
    plain = P.ContinuousBatcher(m, **kw).run(reqs)
    # the same model on an engine with the e4m3 cache: one begin_session, with the keyword; the schedule and the results are the same
    m8, _, _, _, _, _ = TS._model()
    eng8 = Kv8SessionEngine(spec, sd)
    m8._get_engine = lambda B, N, Pp, L, T=0: eng8
    cb = P.ContinuousBatcher(m8, **kw)
    assert eng8.begin_calls == [True]
    out = cb.run(reqs)
    assert eng8.begin_calls == [True]
    assert [n for _, n in out] == [n for _, n in plain]
    assert eng8.log == eng.log
    # kv_fp8 = False on the engine (8 rows or fewer keep the bf16 cache): the old call
    eng8.kv_fp8, eng8.begin_calls = False, []
    P.ContinuousBatcher(m8, **kw)
    assert eng8.begin_calls == [False]
