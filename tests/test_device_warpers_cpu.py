"""CPU: the layers above the WARP instances of the sampler tail (include/ptts_warp.h) - the header against its ctypes binding and a torch-free C
client, the routing of ``generate()`` with and without ``model.enable_device_warpers()`` on the engine stand-in of
tests/test_generate_glue_cpu.py, and ``ContinuousBatcher`` on the oracle-backed session stand-ins: refusals, validation, and the order of calls
around an admission."""
import ctypes
import os
import re
import shutil
import subprocess
import threading

import pytest
import torch

import parler_tts_amd as P
from parler_tts_amd import _native
from parler_tts_amd.engine import DecoderEngine

import test_batched_admission_cpu as TB
import test_device_penalties_cpu as TP
import test_generate_glue_cpu as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptts_warp.h")
WARP_SYMBOLS = ("ptts_set_sample_warp", "ptts_set_slot_sample_warp")
FIELDS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


# ---- the header and the binding -----------------------------------------------------------------------------------------------------------
def test_header_declarations_and_ctypes_prototypes_agree_and_ptts_h_keeps_its_46():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r'^#include "ptts.h"', hdr, flags=re.M)
    assert sorted(set(re.findall(r"\b(ptts_\w+)\s*\(", code))) == sorted(WARP_SYMBOLS) == sorted(_native.WARP_SYMBOLS)
    others = (set(_native.SYMBOLS) | set(_native.SESSION_SYMBOLS) | set(_native.SESSION_KV8_SYMBOLS) | set(_native.SESSION_VOICE_SYMBOLS)
              | set(_native.DAC_STREAM_VOICE_SYMBOLS) | set(_native.PENALTY_SYMBOLS))
    assert not set(_native.WARP_SYMBOLS) & others
    C = _native.C
    ctype_of = {"ptts_engine*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "const ptts_sample_warp*": C.POINTER(_native.PttsSampleWarp)}
    for name in WARP_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/ptts_warp.h"
        res, args = _native.WARP_SYMBOLS[name]
        params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
        assert res is C.c_int and [ctype_of[p] for p in params] == list(args), (name, params)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ptts_sample_warp\s*;", code)
    fields = [tuple(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == [("float", n) for n in FIELDS]
    assert [(n, t) for n, t in _native.PttsSampleWarp._fields_] == [(n, C.c_float) for n in FIELDS]
    # ptts.h: the 46 declarations of ABI v8, untouched, and no other header knows this one
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptts.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(ptts_\w+)\s*\(", base))) == 46 == len(_native.SYMBOLS) and _native.ABI_VERSION == 8
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "ptts_warp.h":
            assert "ptts_warp" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert '"ptts_warp.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()  # a change to it rebuilds the library
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read()
    for name in WARP_SYMBOLS:
        assert re.search(r'extern "C" int ' + name + r"\(", src), f"{name} is not defined in ptts_lm.hip"


def test_library_exports_the_entry_points_and_a_null_engine_is_a_value_error():
    lib = TP._built_library()
    for name in WARP_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native.WARP_SYMBOLS[name][1]
    w = _native.PttsSampleWarp(0.05, 0.9, 3e-4, 2e-3)
    with pytest.raises(ValueError, match="null engine"):
        _native.check(lib.ptts_set_sample_warp(None, ctypes.byref(w), None), "ptts_set_sample_warp")
    with pytest.raises(ValueError, match="null engine"):
        _native.check(lib.ptts_set_slot_sample_warp(None, 0, ctypes.byref(w), None), "ptts_set_slot_sample_warp")


def test_torch_free_c_client_of_the_header_builds_links_and_is_refused_with_a_message(tmp_path):
    """The header is plain C99 beside ptts.h (and C++); a client that knows nothing of torch links against the library and gets the refusals."""
    gcc, gxx = shutil.which("gcc"), shutil.which("g++")
    if gcc is None or gxx is None:
        pytest.skip("no host compiler")
    TP._built_library()
    inc = os.path.join(ROOT, "include")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", HEADER])
    src = tmp_path / "client.c"
    src.write_text('#include <stdio.h>\n#include "ptts.h"\n#include "ptts_penalty.h"\n#include "ptts_warp.h"\n'
                   "int main(void) {\n"
                   "  ptts_sample_warp w = {0.05f, 0.9f, 3e-4f, 2e-3f};\n"
                   "  int a = ptts_set_sample_warp(NULL, &w, NULL);\n"
                   "  int b = ptts_set_slot_sample_warp(NULL, 0, &w, NULL);\n"
                   '  printf("%d %d %d %s\\n", a != PTTS_OK, b != PTTS_OK, (int)sizeof(w), ptts_last_error());\n'
                   "  return 0;\n}\n")
    exe = str(tmp_path / "client")
    libdir = os.path.dirname(_native.LIB_PATH)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", exe, "-L" + libdir, "-lptts_hip", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath-link," + torch_lib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("1 1 16 ") and "null engine" in out.stdout, (out.returncode, out.stdout, out.stderr[-500:])


BAD = [dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")), dict(typical_p=0.0), dict(typical_p=1.2), dict(typical_p=float("inf")),
       dict(epsilon_cutoff=-1e-3), dict(epsilon_cutoff=1.0), dict(eta_cutoff=1.0), dict(eta_cutoff=float("nan")), dict(eta_cutoff="much")]


@pytest.mark.parametrize("bad", BAD)
def test_the_engine_wrapper_checks_values_before_the_library_sees_them(bad):
    with pytest.raises(ValueError, match=next(iter(bad))):
        DecoderEngine._sample_warp(*(bad.get(n) for n in FIELDS))
    w = DecoderEngine._sample_warp(None, None, None, None)
    assert tuple(getattr(w, n) for n in FIELDS) == (0.0, 1.0, 0.0, 0.0)
    w = DecoderEngine._sample_warp(1.0, 1.0, 0.0, 0.0)  # the ends of the ranges are values
    assert (w.min_p, w.typical_p) == (1.0, 1.0)


# ---- generate(): which loop runs ----------------------------------------------------------------------------------------------------------
class RoutingEngine(TP.RoutingEngine):
    """The penalties' routing stand-in plus the warper setter."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.sample_warp, self.warp_calls = None, []

    def set_sample_warp(self, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, enabled=True):
        # an option the config leaves at None is that option's neutral value (releases of transformers differ in which defaults are None)
        vals = tuple(n if v is None else v for v, n in zip((min_p, typical_p, epsilon_cutoff, eta_cutoff), (0.0, 1.0, 0.0, 0.0)))
        self.warp_calls.append(vals + (True,) if enabled else (None, None, None, None, False))
        self.sample_warp = vals if enabled else None


def _routing_model():
    m, spec, sd, _ = TG._model()
    eng = RoutingEngine(spec, sd)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    return m, eng


def _call(m, **kw):
    return TP._call(m, **dict(dict(do_sample=True), **kw))


def test_generate_routing_with_the_switch_off_and_on():
    from transformers import LogitsProcessorList

    m, eng = _routing_model()
    assert not getattr(m, "device_warpers", False)
    for kw in (dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=2e-3)):
        _call(m, **kw)
        assert eng.prefills[-1] == "host" and eng.warp_calls == []  # off: the host loop, as ever, and the engine hears nothing
    _call(m)
    assert eng.prefills[-1] == "device" and eng.warp_calls == []
    assert m.enable_device_warpers() is m and m.device_warpers
    m._get_engine = lambda B, N, Pp, L, T=0: eng  # (the switch drops cached engines; the stand-in stays)
    _call(m, min_p=0.05)
    assert eng.prefills[-1] == "device" and eng.warp_calls == [(0.05, 1.0, 0.0, 0.0, True)]
    _call(m, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)
    assert eng.prefills[-1] == "device" and eng.warp_calls[-1] == (0.0, 0.9, 3e-4, 2e-3, True)
    streamer = P.ParlerTTSStreamer(m, device="cpu", play_steps=10, stride=8)  # the streamer path is the device loop too
    streamer.halo_frames = 64
    th = threading.Thread(target=lambda: _call(m, min_p=0.1, streamer=streamer))
    th.start()
    assert len([c for c in streamer]) >= 1
    th.join()
    assert eng.prefills[-1] == "device" and eng.warp_calls[-1][0] == 0.1 and eng.warp_calls[-1][-1] is True
    _call(m)  # a plain call after one with warpers: the instances go off again
    assert eng.prefills[-1] == "device" and eng.warp_calls[-1] == (None, None, None, None, False) and eng.sample_warp is None
    n = len(eng.warp_calls)
    _call(m)
    assert len(eng.warp_calls) == n  # and a plain call on a plain engine makes no call at all
    _call(m, do_sample=False, min_p=0.05)  # a greedy call builds no warper: plain, on the device
    assert eng.prefills[-1] == "device" and len(eng.warp_calls) == n
    # anything that needs the host's view of a step, or an option without a device implementation, keeps the host loop
    _call(m, min_p=0.05, logits_processor=LogitsProcessorList([P.ParlerTTSLogitsProcessor(1024, 9, 1, "cpu")]))
    assert eng.prefills[-1] == "host" and len(eng.warp_calls) == n
    _call(m, min_p=0.05, return_dict_in_generate=True, output_scores=True)
    assert eng.prefills[-1] == "host" and len(eng.warp_calls) == n
    _call(m, min_p=0.05, bad_words_ids=[[5]])
    assert eng.prefills[-1] == "host" and len(eng.warp_calls) == n
    _call(m, min_p=0.05, repetition_penalty=1.4)  # the penalties' switch is off: the pair runs on the host
    assert eng.prefills[-1] == "host" and len(eng.warp_calls) == n and eng.penalty_calls == []
    if hasattr(__import__("transformers").generation.logits_process, "TopHLogitsWarper"):
        _call(m, min_p=0.05, top_h=0.5)
        assert eng.prefills[-1] == "host" and len(eng.warp_calls) == n


def test_both_switches_keep_a_call_with_both_kinds_on_the_device_and_each_alone_does_not():
    m, eng = _routing_model()
    m.enable_device_penalties()
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m, min_p=0.05, repetition_penalty=1.4)
    assert eng.prefills[-1] == "host" and eng.warp_calls == [] and eng.penalty_calls == []
    m.enable_device_warpers()
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m, min_p=0.05, repetition_penalty=1.4, no_repeat_ngram_size=2)
    assert eng.prefills[-1] == "device" and eng.warp_calls == [(0.05, 1.0, 0.0, 0.0, True)] and eng.penalty_calls == [(1.4, 2, True)]
    _call(m, repetition_penalty=1.4)  # penalties alone: the warper instances go off, the node stays
    assert eng.prefills[-1] == "device" and eng.warp_calls[-1][-1] is False and eng.penalty_calls[-1] == (1.4, None, True)
    _call(m, eta_cutoff=2e-3)
    assert eng.prefills[-1] == "device" and eng.warp_calls[-1] == (0.0, 1.0, 0.0, 2e-3, True) and eng.penalty_calls[-1] == (None, None, False)
    m.enable_device_warpers(False)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m, eta_cutoff=2e-3)
    assert eng.prefills[-1] == "host"


def test_an_engine_without_the_attribute_receives_no_call():
    m, spec, sd, _ = TG._model()
    eng = TP.RoutingEngine(spec, sd)  # knows nothing of warpers
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m)
    _call(m, min_p=0.05)
    assert eng.prefills == ["device", "host"] and not hasattr(eng, "sample_warp")


# ---- ContinuousBatcher --------------------------------------------------------------------------------------------------------------------
class WarpSessionEngine(TP.PenaltySessionEngine):
    """The penalties' session stand-in plus the two warper setters, in the same ``calls`` list."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.sample_warp = None

    def set_sample_warp(self, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, enabled=True):
        self.calls.append(("warp", min_p, typical_p, epsilon_cutoff, eta_cutoff, enabled))
        self.sample_warp = (min_p, typical_p, epsilon_cutoff, eta_cutoff) if enabled else None

    def set_slot_sample_warp(self, slot, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, default=False):
        assert self.full[slot] is None, "the slot record is written while the slot is idle"
        self.calls.append(("slot_warp", slot, min_p, typical_p, epsilon_cutoff, eta_cutoff))


def _batcher(switch=True, penalties=False, **session):
    m, spec, sd, dac, _ = TB._model()
    eng = WarpSessionEngine(spec, sd)
    if switch:
        m.enable_device_warpers()
    if penalties:
        m.enable_device_penalties()
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    kw = dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, max_new_tokens=14, min_new_tokens=2, do_sample=True)
    kw.update(session)
    return P.ContinuousBatcher(m, **kw), eng


_req = TP._req


def test_without_the_switch_both_places_refuse_as_today():
    for kw in (dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=2e-3)):
        with pytest.raises(NotImplementedError, match="host loop"):
            _batcher(switch=False, **kw)
    cb, eng = _batcher(switch=False)
    assert eng.calls == [("begin",)]  # no setter call on an engine that never had the instances
    for kw in (dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=2e-3)):
        with pytest.raises(NotImplementedError, match="enable_device_warpers"):
            cb.submit(**_req(0, **kw))
    assert cb.pending() == 0 and cb.submit(**_req(0)) == 0


def test_other_extras_stay_refused_with_the_switch():
    with pytest.raises(NotImplementedError, match="bad_words_ids"):
        _batcher(min_p=0.05, bad_words_ids=[[5]])
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        _batcher(min_p=0.05, repetition_penalty=1.3)  # the penalties have their own switch
    if hasattr(__import__("transformers").generation.logits_process, "TopHLogitsWarper"):
        with pytest.raises(NotImplementedError, match="top_h"):
            _batcher(min_p=0.05, top_h=0.5)


def test_the_session_defaults_reach_the_engine_before_the_session_begins():
    cb, eng = _batcher(min_p=0.05, eta_cutoff=2e-3)
    assert eng.calls == [("warp", 0.05, 1.0, 0.0, 2e-3, True), ("begin",)]
    cb, eng = _batcher()
    assert eng.calls == [("warp", 0.0, 1.0, 0.0, 0.0, True), ("begin",)]  # neutral: the instances are there for the requests that bring warpers
    cb, eng = _batcher(penalties=True, typical_p=0.9, repetition_penalty=1.3)
    assert eng.calls == [("session", 1.3, 0, True), ("warp", 0.0, 0.9, 0.0, 0.0, True), ("begin",)]


@pytest.mark.parametrize("where", ["session", "submit"])
@pytest.mark.parametrize("bad", [b for b in BAD if not isinstance(next(iter(b.values())), str)])
def test_bad_values_are_value_errors_and_a_refused_submit_queues_nothing(where, bad):
    if where == "session":
        with pytest.raises(ValueError, match=next(iter(bad))):
            _batcher(**bad)
        return
    cb, eng = _batcher()
    cb.submit(**_req(0))
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError, match=next(iter(bad))):
        cb.submit(**_req(1, **bad))
    assert cb.pending() == 1 and len(cb._queue) == 1 and [c[0] for c in eng.calls] == ["warp", "begin"]
    assert torch.equal(state, torch.random.get_rng_state())  # no seed was drawn
    assert cb.submit(**_req(1)) == 1  # and it took no ticket


def test_single_admissions_write_the_slot_record_immediately_before_the_admission():
    cb, eng = _batcher(min_p=0.1)
    cb.run([_req(0, typical_p=0.5), _req(1), _req(2, min_p=0.0, eta_cutoff=2e-3), _req(3, epsilon_cutoff=3e-4)])
    calls = [c for c in eng.calls if c[0] in ("slot_warp", "admit_row", "admit_rows")]
    assert not any(c[0] == "admit_rows" for c in calls)
    admits = [i for i, c in enumerate(calls) if c[0] == "admit_row"]
    assert len(admits) == 4
    before = [calls[i - 1] if i > 0 and calls[i - 1][0] == "slot_warp" else None for i in admits]
    slot = [calls[i][1] for i in admits]
    assert before[0] == ("slot_warp", slot[0], 0.1, 0.5, 0.0, 0.0)  # the session's min_p fills the option left out
    assert before[1] is None                                       # no options: no call, the slot runs on the session's record
    assert before[2] == ("slot_warp", slot[2], 0.0, 1.0, 0.0, 2e-3)  # a request may switch the session's min_p off for itself
    assert before[3] == ("slot_warp", slot[3], 0.1, 1.0, 3e-4, 0.0)
    assert sum(c[0] == "slot_warp" for c in calls) == 3
    assert sum(c[0] == "retire" for c in eng.calls) == 4           # retire_row puts the session's record back: nothing else to undo


def test_group_admissions_write_every_record_before_the_one_engine_call():
    cb, eng = _batcher(slots=2, admit_batch=2, penalties=True, eta_cutoff=2e-3)
    cb.run([_req(0, min_p=0.3, repetition_penalty=1.5), _req(1, typical_p=0.4), _req(2), _req(3, epsilon_cutoff=1e-3)])
    calls = [c for c in eng.calls if c[0] in ("slot", "slot_warp", "admit_row", "admit_rows")]
    assert [c[0] for c in calls] == ["slot", "slot_warp", "slot_warp", "admit_rows", "slot_warp", "admit_rows"], calls
    s0, s1 = calls[3][1]
    assert calls[0] == ("slot", s0, 1.5, 0) and calls[1] == ("slot_warp", s0, 0.3, 1.0, 0.0, 2e-3) and calls[2] == ("slot_warp", s1, 0.0, 0.4, 0.0, 2e-3)
    assert calls[4] == ("slot_warp", calls[5][1][1], 0.0, 1.0, 1e-3, 2e-3)


def test_an_engine_left_with_the_instances_on_is_switched_off_by_a_batcher_without_the_switch():
    m, spec, sd, dac, _ = TB._model()
    eng = WarpSessionEngine(spec, sd)
    eng.sample_warp = (0.05, 1.0, 0.0, 0.0)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    P.ContinuousBatcher(m, slots=2, max_description_tokens=9, max_prompt_tokens=5, max_new_tokens=14)
    assert eng.calls == [("warp", None, None, None, None, False), ("begin",)]
