"""CPU: group admissions of ``parler_tts_amd.ContinuousBatcher(admit_batch=N)`` (``ptts_admit_rows``), driven without a GPU by the oracle
stand-in of tests/test_continuous_scheduler_cpu.py extended with ``admit_rows``: the size of the groups, FIFO pairing with ascending idle
slots, the clamp of the spare rows at the batch-size class boundaries, the fall-back to single admissions, results against the per-request
pipeline, and the declaration of the new symbol. What the HIP engine computes is covered by tests/test_batched_admission_gpu.py."""
import os
import re

import pytest
import torch

import parler_tts_amd as P
from parler_tts_amd import _native

import test_continuous_scheduler_cpu as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class GroupSessionEngine(TS.OracleSessionEngine):
    """The stand-in with ``admit_rows``: every request of a group is computed as ``admit_row`` computes it (the oracle on the request alone),
    after the checks of the whole list; ``groups`` records (slots, step count) per call and ``singles`` the slots of ``admit_row`` calls."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.groups, self.singles, self.max_batches = [], [], []

    def admit_row(self, row, *a, **k):
        super().admit_row(row, *a, **k)
        if not getattr(self, "_in_group", False):
            self.singles.append(row)

    def admit_rows(self, rows, enc, enc_mask, prompt, prompt_mask, max_lengths=None, sample=True, gens=None):
        rows = list(rows)
        n = len(rows)
        assert n >= 1 and len(set(rows)) == n and gens is None
        assert tuple(enc.shape) == (n, self.N, self.spec.hidden_size) and tuple(enc_mask.shape) == (n, self.N)
        for r in rows:
            if not 0 <= r < self.B or self.full[r] is not None:
                raise ValueError(f"slot {r} is not an idle slot of the session")
        self._in_group = True
        try:
            for j, r in enumerate(rows):
                self.admit_row(r, enc[j], enc_mask[j], None if prompt is None else prompt[j], None if prompt_mask is None else prompt_mask[j],
                               max_length=max_lengths[j], sample=sample)
        finally:
            self._in_group = False
        self.groups.append((rows, self.steps))


def _model():
    m, spec, sd, dac, _, codec_groups = TS._model()
    eng = GroupSessionEngine(spec, sd)

    def get_engine(B, N, Pp, L, T=0):
        eng.max_batches.append(B)
        return eng

    m._get_engine = get_engine
    return m, spec, sd, dac, eng


KW = dict(max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_new_tokens=30, min_new_tokens=30)


@pytest.mark.parametrize("slots,spare", [(3, 0), (4, 0), (7, 0), (8, 0), (9, 4), (2, 2), (5, 3), (6, 2), (1, 3), (12, 4), (32, 4)])
def test_spare_rows_are_clamped_to_the_batch_size_class_of_the_slots(slots, spare):
    """admit_batch 4: the engine of `slots + spare` rows stays in the class of `slots` (<= 4, <= 8, wider), and a clamp that leaves fewer than 2
    spare rows means single admissions on an engine of exactly `slots` rows."""
    assert P.ContinuousBatcher.spare_rows(slots, 4) == spare
    assert P.ContinuousBatcher.spare_rows(slots, 1) == 0
    cls = lambda b: 0 if b <= 4 else (1 if b <= 8 else 2)
    assert cls(slots + spare) == cls(slots)
    m, spec, sd, dac, eng = _model()
    cb = P.ContinuousBatcher(m, slots=slots, admit_batch=4, **KW)
    assert cb.spare == spare and eng.max_batches == [slots + spare] and eng.B == slots


def test_admit_batch_must_be_positive():
    m, *_ = _model()
    with pytest.raises(ValueError, match="admit_batch"):
        P.ContinuousBatcher(m, slots=2, admit_batch=0, **KW)


def test_groups_pair_ascending_idle_slots_with_the_queue_in_fifo_order_and_never_exceed_the_spare_rows():
    m, spec, sd, dac, eng = _model()
    reqs = TS._requests(30, seed=2)
    cb = P.ContinuousBatcher(m, slots=10, admit_batch=4, poll_steps=16, **KW)
    assert cb.spare == 4
    tickets = [cb.submit(**r) for r in reqs]
    finished = [t for t, w, n in cb]
    assert sorted(finished) == tickets
    # the first poll: 10 idle slots, 30 queued -> groups of 4, 4, 2 over slots 0..9 in order, before any step
    assert eng.groups[:3] == [([0, 1, 2, 3], 0), ([4, 5, 6, 7], 0), ([8, 9], 0)]
    assert all(2 <= len(rows) <= 4 for rows, _ in eng.groups) and all(rows == sorted(rows) for rows, _ in eng.groups)
    assert cb.admission_groups == [len(rows) for rows, _ in eng.groups] and cb.admissions == 30
    # FIFO over single and group admissions alike: the i-th admission is the i-th submission (its length identifies it, EOS is blocked)
    admits = [(slot, step) for kind, slot, step in eng.log if kind == "admit"]
    assert len(admits) == 30 and len(eng.singles) + sum(len(rows) for rows, _ in eng.groups) == 30
    L = [r["max_new_tokens"] + 1 for r in reqs]
    open_, order = {}, 0
    for kind, slot, step in eng.log:
        if kind == "admit":
            open_[slot] = (order, step)
            order += 1
        else:
            i, s0 = open_.pop(slot)
            assert step - s0 == L[i] - 2, (i, slot, step, s0)
    # several slots free at one poll at least once after the start (requests of equal length admitted together end together)
    assert any(step > 0 for _, step in eng.groups)


def test_results_equal_the_per_request_pipeline_in_submission_order():
    m, spec, sd, dac, eng = _model()
    reqs = TS._requests(8, seed=1)
    out = P.ContinuousBatcher(m, slots=2, admit_batch=4, poll_steps=4, **{**KW, "min_new_tokens": 0}).run(reqs)
    assert eng.max_batches == [4] and eng.groups[0] == ([0, 1], 0)
    for r, (wav, n) in zip(reqs, out):
        ref = TS._reference(m, spec, sd, dac, r, 9, 5, 0)
        assert wav.dim() == 1 and n == wav.shape[0] == ref.shape[0]
        assert torch.allclose(wav, ref, atol=1e-6)


@pytest.mark.parametrize("slots,admit_batch", [(4, 1), (10, 1), (3, 4), (8, 4)])
def test_without_spare_rows_every_admission_is_one_admit_row(slots, admit_batch):
    """admit_batch = 1 (the default), and a clamp that leaves no group: admit_rows is never called, the engine has exactly `slots` rows."""
    m, spec, sd, dac, eng = _model()
    eng.admit_rows = None  # calling it would raise
    reqs = TS._requests(2 * slots + 1, seed=3)
    cb = P.ContinuousBatcher(m, slots=slots, admit_batch=admit_batch, **KW)
    out = cb.run(reqs)
    assert len(out) == len(reqs) and eng.singles == [s for kind, s, _ in eng.log if kind == "admit"] and len(eng.singles) == len(reqs)
    assert eng.singles[:slots] == list(range(slots)) and eng.max_batches == [slots] and cb.admission_groups == []


def test_a_group_of_one_goes_through_admit_row():
    m, spec, sd, dac, eng = _model()
    cb = P.ContinuousBatcher(m, slots=10, admit_batch=4, **KW)
    out = cb.run(TS._requests(5, seed=4))
    assert len(out) == 5 and eng.groups == [([0, 1, 2, 3], 0)] and eng.singles == [4]


class RefusingEngine(GroupSessionEngine):
    """Raises ``ValueError`` from the call that is handed the request whose encoded description is ``refuse``, before changing any state."""

    refuse = None

    def admit_row(self, row, enc, *a, **k):
        if self.refuse is not None and not getattr(self, "_in_group", False) and torch.equal(enc, self.refuse):
            raise ValueError("refused by the engine")
        super().admit_row(row, enc, *a, **k)

    def admit_rows(self, rows, enc, *a, **k):
        if self.refuse is not None and any(torch.equal(e, self.refuse) for e in enc):
            raise ValueError("refused by the engine")
        super().admit_rows(rows, enc, *a, **k)


@pytest.mark.parametrize("slots,admit_batch,bad,lost,queued", [(3, 1, 1, [1], [2, 3, 4, 5]), (9, 4, 2, [0, 1, 2, 3], [4, 5]), (9, 4, 5, [4, 5], [])])
def test_an_admission_that_raises_loses_only_what_was_handed_to_the_failing_call(slots, admit_batch, bad, lost, queued):
    """Six requests meet idle slots at the first poll and the engine refuses the call that carries ticket `bad`. A request leaves the queue
    immediately before the call that admits it (alone, or with its group of up to 4): the request or group of the failing call is lost, the
    admissions before it stand, the requests behind it are still queued, and iterating on finishes all of those as a clean run does."""
    reqs = [dict(r, max_new_tokens=12) for r in TS._requests(6, seed=5)]

    def batcher():
        m, spec, sd, dac, _ = _model()
        eng = RefusingEngine(spec, sd)
        m._get_engine = lambda *a: eng
        return P.ContinuousBatcher(m, slots=slots, admit_batch=admit_batch, **KW), eng

    clean = batcher()[0].run(reqs)
    cb, eng = batcher()
    tickets = [cb.submit(**r) for r in reqs]
    eng.refuse = cb._queue[bad].enc
    with pytest.raises(ValueError, match="refused by the engine"):
        next(iter(cb))
    stand = [t for t in tickets if t not in lost + queued]
    assert [r.ticket for r in cb._queue] == queued
    assert [r.ticket for r in cb._slot if r is not None] == stand and [f is not None for f in eng.full] == [s < len(stand) for s in range(slots)]
    assert cb.admissions == len(stand) and cb.pending() == 6 - len(lost) and eng.steps == 0
    got = {t: (w, n) for t, w, n in cb}
    assert sorted(got) == sorted(stand + queued) and cb.pending() == 0
    for t, (w, n) in got.items():
        assert n == clean[t][1] == w.shape[0] and torch.equal(w, clean[t][0]), t


def test_header_and_ctypes_prototypes_of_ptts_admit_rows_agree(tmp_path):
    """The new entry point is additive: include/ptts.h keeps its declarations and ABI version 8 and includes include/ptts_session.h, which
    declares ptts_admit_rows; _native.SESSION_SYMBOLS binds it beside the SYMBOLS of ptts.h."""
    import shutil
    import subprocess

    C = _native.C
    inc = os.path.join(ROOT, "include")
    hdr = open(os.path.join(inc, "ptts.h")).read()
    assert re.search(r"#define\s+PTTS_ABI_VERSION\s+8\b", hdr) and _native.ABI_VERSION == 8  # additive: the version does not move
    assert re.search(r'^#include "ptts_session.h"', hdr, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "ptts_session.h")).read(), flags=re.S)
    decls = re.findall(r"^\s*(?:const\s+char\s*\*|int32_t|int|void)\s+(ptts_\w+)\s*\(", code, flags=re.M)
    assert decls == ["ptts_admit_rows"] == list(_native.SESSION_SYMBOLS) and not set(decls) & set(_native.SYMBOLS)
    m = re.search(r"\bint\s+ptts_admit_rows\s*\(([^)]*)\)\s*;", code)
    assert m, "ptts_admit_rows is not declared in include/ptts_session.h"
    params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
    assert params == ["ptts_engine*", "int32_t", "const int32_t*", "const float*", "const int32_t*", "const float*", "const int32_t*", "const int32_t*",
                      "int32_t", "const ptts_gen_params* const*", "void*"]
    res, args = _native.SESSION_SYMBOLS["ptts_admit_rows"]
    host_i32 = C.POINTER(C.c_int32)  # rows and max_lengths are host arrays, the masks device pointers
    assert res is C.c_int and args == [C.c_void_p, C.c_int32, host_i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, host_i32, C.c_int32,
                                       C.POINTER(C.POINTER(_native.PttsGenParams)), C.c_void_p]
    # a C caller that includes ptts.h alone sees the declaration; either header compiles on its own as C99 and as C++
    gcc, gxx = shutil.which("gcc") or shutil.which("cc"), shutil.which("g++") or shutil.which("c++")
    src = tmp_path / "caller.c"
    src.write_text('#include "ptts.h"\nint (*fp)(ptts_engine*, int32_t, const int32_t*, const float*, const int32_t*, const float*, const int32_t*, '
                   'const int32_t*, int32_t, const ptts_gen_params* const*, void*) = ptts_admit_rows;\n')
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)])
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "ptts_session.h")])
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", os.path.join(inc, "ptts_session.h")])
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read()
    assert re.search(r'extern "C" int ptts_admit_rows\(', src)
    import __graft_entry__

    __graft_entry__.build()  # incremental; cross-compiles without a GPU
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "ptts_admit_rows" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert hasattr(_native.load_library(), "ptts_admit_rows")
    from parler_tts_amd.engine import DecoderEngine

    assert hasattr(DecoderEngine, "admit_rows")
