"""CPU: the layers above the history-penalty node (include/ptts_penalty.h) - the header against its ctypes binding and a torch-free C client,
the routing of ``generate()`` with and without ``model.enable_device_penalties()`` on the engine stand-in of tests/test_generate_glue_cpu.py,
and ``ContinuousBatcher`` on the oracle-backed session stand-ins: refusals, validation, and the order of calls around an admission."""
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
import test_generate_glue_cpu as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptts_penalty.h")
PENALTY_SYMBOLS = ("ptts_set_history_penalty", "ptts_set_slot_history_penalty")


# ---- the header and the binding -----------------------------------------------------------------------------------------------------------
def test_header_declarations_and_ctypes_prototypes_agree_and_ptts_h_keeps_its_46():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r'^#include "ptts.h"', hdr, flags=re.M)
    assert sorted(set(re.findall(r"\b(ptts_\w+)\s*\(", code))) == sorted(PENALTY_SYMBOLS) == sorted(_native.PENALTY_SYMBOLS)
    others = set(_native.SYMBOLS) | set(_native.SESSION_SYMBOLS) | set(_native.SESSION_KV8_SYMBOLS) | set(_native.SESSION_VOICE_SYMBOLS) | set(_native.DAC_STREAM_VOICE_SYMBOLS)
    assert not set(_native.PENALTY_SYMBOLS) & others
    C = _native.C
    ctype_of = {"ptts_engine*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "const ptts_history_penalty*": C.POINTER(_native.PttsHistoryPenalty)}
    for name in PENALTY_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/ptts_penalty.h"
        res, args = _native.PENALTY_SYMBOLS[name]
        params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
        assert res is C.c_int and [ctype_of[p] for p in params] == list(args), (name, params)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ptts_history_penalty\s*;", code)
    fields = [tuple(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == [("float", "repetition_penalty"), ("int32_t", "no_repeat_ngram_size")]
    assert [(n, t) for n, t in _native.PttsHistoryPenalty._fields_] == [("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32)]
    # ptts.h: the 46 declarations of ABI v8, untouched, and no other header knows this one
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptts.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(ptts_\w+)\s*\(", base))) == 46 == len(_native.SYMBOLS) and _native.ABI_VERSION == 8
    assert re.search(r"#define\s+PTTS_ABI_VERSION\s+8\b", base)
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "ptts_penalty.h":
            assert "ptts_penalty" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert '"ptts_penalty.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()  # a change to it rebuilds the library
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read()
    for name in PENALTY_SYMBOLS:
        assert re.search(r'extern "C" int ' + name + r"\(", src), f"{name} is not defined in ptts_lm.hip"


def _built_library():
    import __graft_entry__

    __graft_entry__.build()  # incremental; cross-compiles without a GPU
    return _native.load_library()


def test_library_exports_the_entry_points_and_a_null_engine_is_a_value_error():
    lib = _built_library()
    for name in PENALTY_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native.PENALTY_SYMBOLS[name][1]
    hp = _native.PttsHistoryPenalty(1.4, 2)
    with pytest.raises(ValueError, match="null engine"):
        _native.check(lib.ptts_set_history_penalty(None, ctypes.byref(hp), None), "ptts_set_history_penalty")
    with pytest.raises(ValueError, match="null engine"):
        _native.check(lib.ptts_set_slot_history_penalty(None, 0, ctypes.byref(hp), None), "ptts_set_slot_history_penalty")


def test_torch_free_c_client_of_the_header_builds_links_and_is_refused_with_a_message(tmp_path):
    """The header is plain C99 beside ptts.h (and C++); a client that knows nothing of torch links against the library and gets the refusals."""
    gcc, gxx = shutil.which("gcc"), shutil.which("g++")
    if gcc is None or gxx is None:
        pytest.skip("no host compiler")
    _built_library()
    inc = os.path.join(ROOT, "include")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", HEADER])
    src = tmp_path / "client.c"
    src.write_text('#include <stdio.h>\n#include "ptts.h"\n#include "ptts_penalty.h"\n'
                   "int main(void) {\n"
                   "  ptts_history_penalty hp = {1.4f, 2};\n"
                   "  int a = ptts_set_history_penalty(NULL, &hp, NULL);\n"
                   "  int b = ptts_set_slot_history_penalty(NULL, 0, &hp, NULL);\n"
                   '  printf("%d %d %d %s\\n", a != PTTS_OK, b != PTTS_OK, (int)sizeof(hp), ptts_last_error());\n'
                   "  return 0;\n}\n")
    exe = str(tmp_path / "client")
    libdir = os.path.dirname(_native.LIB_PATH)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", exe, "-L" + libdir, "-lptts_hip", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath-link," + torch_lib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("1 1 8 ") and "null engine" in out.stdout, (out.returncode, out.stdout, out.stderr[-500:])


@pytest.mark.parametrize("bad", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
                                 dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5)])
def test_the_engine_wrapper_checks_values_before_the_library_sees_them(bad):
    with pytest.raises(ValueError, match=next(iter(bad))):
        DecoderEngine._history_penalty(bad.get("repetition_penalty"), bad.get("no_repeat_ngram_size"))
    hp = DecoderEngine._history_penalty(None, None)
    assert (hp.repetition_penalty, hp.no_repeat_ngram_size) == (1.0, 0)


# ---- generate(): which loop runs ----------------------------------------------------------------------------------------------------------
class RoutingEngine(TG.OracleEngine):
    """The stand-in of test_generate_glue_cpu.py plus the penalty setter: records its calls and which loop prefilled (sample = the device loop)."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.history_penalty, self.penalty_calls, self.prefills = None, [], []

    def set_history_penalty(self, repetition_penalty=None, no_repeat_ngram_size=None, enabled=True):
        self.penalty_calls.append((repetition_penalty, no_repeat_ngram_size, enabled))
        self.history_penalty = (repetition_penalty, no_repeat_ngram_size) if enabled else None

    def prefill(self, enc, enc_mask, prompt, prompt_mask, sample=True):
        self.prefills.append("device" if sample else "host")
        super().prefill(enc, enc_mask, prompt, prompt_mask, sample=sample)


def _routing_model():
    m, spec, sd, _ = TG._model()
    eng = RoutingEngine(spec, sd)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    return m, eng


def _call(m, **kw):
    g = torch.Generator().manual_seed(3)
    kw = dict(dict(do_sample=False, max_new_tokens=12, min_new_tokens=12), **kw)
    return m.generate(input_ids=torch.randint(3, 128, (1, 6), generator=g), prompt_input_ids=torch.randint(3, 128, (1, 3), generator=g), **kw)


def test_generate_routing_with_the_switch_off_and_on():
    from transformers import LogitsProcessorList

    m, eng = _routing_model()
    assert not getattr(m, "device_penalties", False)
    _call(m, repetition_penalty=1.4, no_repeat_ngram_size=2)
    assert eng.prefills == ["host"] and eng.penalty_calls == []  # off: the host loop, as ever, and the engine hears nothing
    _call(m)
    assert eng.prefills == ["host", "device"] and eng.penalty_calls == []
    assert m.enable_device_penalties() is m and m.device_penalties
    m._get_engine = lambda B, N, Pp, L, T=0: eng  # (the switch drops cached engines; the stand-in stays)
    _call(m, repetition_penalty=1.4, no_repeat_ngram_size=2)
    assert eng.prefills[-1] == "device" and eng.penalty_calls == [(1.4, 2, True)]
    _call(m, no_repeat_ngram_size=3)
    assert eng.prefills[-1] == "device" and eng.penalty_calls[-1] == (None, 3, True)  # an option left at the config's None is the neutral value
    streamer = P.ParlerTTSStreamer(m, device="cpu", play_steps=10, stride=8)  # the streamer path is the device loop too
    streamer.halo_frames = 64
    th = threading.Thread(target=lambda: _call(m, repetition_penalty=1.4, streamer=streamer))
    th.start()
    assert len([c for c in streamer]) >= 1
    th.join()
    assert eng.prefills[-1] == "device" and eng.penalty_calls[-1] == (1.4, None, True)
    _call(m)  # a plain call after one with penalties: the node goes off again
    assert eng.prefills[-1] == "device" and eng.penalty_calls[-1] == (None, None, False) and eng.history_penalty is None
    n = len(eng.penalty_calls)
    _call(m)
    assert len(eng.penalty_calls) == n  # and a plain call on a plain engine makes no call at all
    # anything that needs the host's view of a step keeps the host loop, with the penalties as transformers' processors
    _call(m, repetition_penalty=1.4, logits_processor=LogitsProcessorList([P.ParlerTTSLogitsProcessor(1024, 9, 1, "cpu")]))
    assert eng.prefills[-1] == "host" and len(eng.penalty_calls) == n
    _call(m, repetition_penalty=1.4, do_sample=True, min_p=0.05)
    assert eng.prefills[-1] == "host" and len(eng.penalty_calls) == n
    _call(m, repetition_penalty=1.4, return_dict_in_generate=True, output_scores=True)
    assert eng.prefills[-1] == "host" and len(eng.penalty_calls) == n
    m.enable_device_penalties(False)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m, repetition_penalty=1.4)
    assert eng.prefills[-1] == "host" and len(eng.penalty_calls) == n


# ---- ContinuousBatcher --------------------------------------------------------------------------------------------------------------------
class PenaltySessionEngine(TB.GroupSessionEngine):
    """The group stand-in plus the two setters: ``calls`` is the order in which setters, admissions and retirements reach the engine."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.history_penalty, self.calls = None, []

    def set_history_penalty(self, repetition_penalty=None, no_repeat_ngram_size=None, enabled=True):
        self.calls.append(("session", repetition_penalty, no_repeat_ngram_size, enabled))
        self.history_penalty = (repetition_penalty, no_repeat_ngram_size) if enabled else None

    def set_slot_history_penalty(self, slot, repetition_penalty=None, no_repeat_ngram_size=None, default=False):
        assert self.full[slot] is None, "the slot record is written while the slot is idle"
        self.calls.append(("slot", slot, repetition_penalty, no_repeat_ngram_size))

    def begin_session(self, *a, **k):
        self.calls.append(("begin",))
        super().begin_session(*a, **k)

    def admit_row(self, row, *a, **k):
        if not getattr(self, "_in_group", False):
            self.calls.append(("admit_row", row))
        super().admit_row(row, *a, **k)

    def admit_rows(self, rows, *a, **k):
        self.calls.append(("admit_rows", tuple(rows)))
        super().admit_rows(rows, *a, **k)

    def retire_row(self, row):
        self.calls.append(("retire", row))
        super().retire_row(row)


def _batcher(switch=True, **session):
    m, spec, sd, dac, _ = TB._model()
    eng = PenaltySessionEngine(spec, sd)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    if switch:
        m.enable_device_penalties()
        m._get_engine = lambda B, N, Pp, L, T=0: eng
    kw = dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, max_new_tokens=14, min_new_tokens=2)
    kw.update(session)
    return P.ContinuousBatcher(m, **kw), eng


def _req(i=0, **kw):
    g = torch.Generator().manual_seed(40 + i)
    return dict(input_ids=torch.randint(3, 128, (9,), generator=g), prompt_input_ids=torch.randint(3, 128, (5,), generator=g), max_new_tokens=12, **kw)


def test_without_the_switch_both_places_refuse_as_today():
    with pytest.raises(NotImplementedError, match="host loop"):
        _batcher(switch=False, repetition_penalty=1.3)
    with pytest.raises(NotImplementedError, match="host loop"):
        _batcher(switch=False, no_repeat_ngram_size=2)
    cb, eng = _batcher(switch=False)
    assert eng.calls == [("begin",)]  # no setter call on an engine that never had the node
    for bad in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2)):
        with pytest.raises(NotImplementedError, match="enable_device_penalties"):
            cb.submit(**_req(0, **bad))
    assert cb.pending() == 0 and cb.submit(**_req(0)) == 0


def test_other_extras_stay_refused_with_the_switch():
    with pytest.raises(NotImplementedError, match="bad_words_ids"):
        _batcher(repetition_penalty=1.3, bad_words_ids=[[5]])


def test_the_session_defaults_reach_the_engine_before_the_session_begins():
    cb, eng = _batcher(repetition_penalty=1.3, no_repeat_ngram_size=4)
    assert eng.calls == [("session", 1.3, 4, True), ("begin",)]
    cb, eng = _batcher()
    assert eng.calls == [("session", 1.0, 0, True), ("begin",)]  # neutral: the node is there for the requests that bring penalties


@pytest.mark.parametrize("where", ["session", "submit"])
@pytest.mark.parametrize("bad", [dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0), dict(repetition_penalty=float("inf")),
                                 dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.5)])
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
    assert cb.pending() == 1 and len(cb._queue) == 1 and [c[0] for c in eng.calls] == ["session", "begin"]
    assert torch.equal(state, torch.random.get_rng_state())
    assert cb.submit(**_req(1)) == 1  # and takes no ticket


def test_single_admissions_write_the_slot_record_immediately_before_the_admission():
    cb, eng = _batcher(repetition_penalty=1.2)
    cb.run([_req(0, repetition_penalty=1.5), _req(1), _req(2, no_repeat_ngram_size=3), _req(3, repetition_penalty=1.0, no_repeat_ngram_size=0)])
    calls = [c for c in eng.calls if c[0] in ("slot", "admit_row", "admit_rows")]
    assert not any(c[0] == "admit_rows" for c in calls)
    admits = [i for i, c in enumerate(calls) if c[0] == "admit_row"]
    assert len(admits) == 4
    before = [calls[i - 1] if i > 0 and calls[i - 1][0] == "slot" else None for i in admits]
    slot = [calls[i][1] for i in admits]
    assert before[0] == ("slot", slot[0], 1.5, 0)          # the request's value over the session's n
    assert before[1] is None                               # no options: no call, the slot runs on the session's record
    assert before[2] == ("slot", slot[2], 1.2, 3)          # the session's p fills the option left out
    assert before[3] == ("slot", slot[3], 1.0, 0)          # a request may switch the session's penalties off for itself
    assert sum(c[0] == "slot" for c in calls) == 3
    assert sum(c[0] == "retire" for c in eng.calls) == 4   # retire_row puts the session's record back: nothing else to undo


def test_group_admissions_write_every_record_before_the_one_engine_call():
    cb, eng = _batcher(slots=2, admit_batch=2, no_repeat_ngram_size=2)
    cb.run([_req(0, repetition_penalty=1.5), _req(1), _req(2), _req(3, no_repeat_ngram_size=5)])
    calls = [c for c in eng.calls if c[0] in ("slot", "admit_row", "admit_rows")]
    assert [c[0] for c in calls] == ["slot", "admit_rows", "slot", "admit_rows"], calls
    assert calls[0] == ("slot", calls[1][1][0], 1.5, 2) and calls[2] == ("slot", calls[3][1][1], 1.0, 5)


def test_an_engine_left_with_the_node_on_is_switched_off_by_a_batcher_without_the_switch():
    m, spec, sd, dac, _ = TB._model()
    eng = PenaltySessionEngine(spec, sd)
    eng.history_penalty = (1.3, 0)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    P.ContinuousBatcher(m, slots=2, max_description_tokens=9, max_prompt_tokens=5, max_new_tokens=14)
    assert eng.calls == [("session", None, None, False), ("begin",)]
