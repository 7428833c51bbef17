"""CPU: per-request sampler options of ``ContinuousBatcher.submit`` on the oracle stand-in of tests/test_continuous_scheduler_cpu.py - what
reaches ``admit_row`` (nothing new for a request without options, the merged record otherwise), seeds, refusals, and the streaming batcher."""
import pytest
import torch

import parler_tts_amd as P
import test_continuous_scheduler_cpu as TS
import test_continuous_streaming_cpu as TST

KEYS = {"min_new_tokens", "do_sample", "temperature", "top_k", "top_p", "use_eos_gate", "seed"}


class RecordingEngine(TS.OracleSessionEngine):
    """The stand-in with today's ``admit_row`` signature plus ``gen=``: records the keywords of every admission."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.calls = []

    def admit_row(self, row, enc, enc_mask, prompt, prompt_mask, max_length=0, sample=True, **kw):
        assert set(kw) <= {"gen"}, kw
        self.calls.append(dict(kw))
        super().admit_row(row, enc, enc_mask, prompt, prompt_mask, max_length=max_length, sample=sample)


def _batcher(**session):
    m, spec, sd, dac, _, _ = TS._model()
    eng = RecordingEngine(spec, sd)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    kw = dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, max_new_tokens=14, min_new_tokens=2)
    kw.update(session)
    return P.ContinuousBatcher(m, **kw), eng


def _req(i=0):
    g = torch.Generator().manual_seed(40 + i)
    return dict(input_ids=torch.randint(3, 128, (9,), generator=g), prompt_input_ids=torch.randint(3, 128, (5,), generator=g), max_new_tokens=12)


def test_a_request_without_options_is_admitted_by_the_same_call_as_ever():
    cb, eng = _batcher(do_sample=True, temperature=0.8, top_k=30, top_p=0.9)
    cb.run([_req(0), _req(1)])
    assert eng.calls == [{}, {}]  # no `gen` keyword at all: an engine with the old signature keeps working


def test_the_record_is_the_requests_options_over_the_sessions_values():
    cb, eng = _batcher(do_sample=True, temperature=0.8, top_k=30, top_p=0.9)
    cb.run([dict(_req(0), temperature=0.7, seed=5), _req(1), dict(_req(2), do_sample=False), dict(_req(3), top_k=0, top_p=1.0, min_new_tokens=4, seed=2 ** 64 - 1),
            dict(_req(4), do_sample=False, seed=9), dict(_req(5), seed=11)])
    g = [c.get("gen") for c in eng.calls]
    assert g[0] == dict(min_new_tokens=2, do_sample=True, temperature=0.7, top_k=30, top_p=0.9, use_eos_gate=True, seed=5)
    assert g[1] is None and "gen" not in eng.calls[1]
    assert g[2] == dict(min_new_tokens=2, do_sample=False, temperature=0.8, top_k=30, top_p=0.9, use_eos_gate=True, seed=0)
    assert g[3] == dict(min_new_tokens=4, do_sample=True, temperature=0.8, top_k=0, top_p=1.0, use_eos_gate=True, seed=2 ** 64 - 1)
    assert g[4]["seed"] == 9 and g[4]["do_sample"] is False  # a seed with greedy decoding is accepted (and has no effect)
    assert g[5] == dict(min_new_tokens=2, do_sample=True, temperature=0.8, top_k=30, top_p=0.9, use_eos_gate=True, seed=11)  # a seed alone: own stream
    for x in g:
        assert x is None or (set(x) == KEYS and type(x["temperature"]) is float and type(x["top_k"]) is int)
    # a greedy session: a request may still sample, with the session's warpers as the caller gave them
    cb, eng = _batcher(do_sample=False, top_k=40, top_p=0.95)
    cb.run([dict(_req(0), do_sample=True, seed=3)])
    assert eng.calls[0]["gen"] == dict(min_new_tokens=2, do_sample=True, temperature=1.0, top_k=40, top_p=0.95, use_eos_gate=True, seed=3)


def test_seed_none_is_drawn_from_torchs_rng_at_submit():
    seeds = []
    for _ in range(2):
        torch.manual_seed(1234)
        cb, eng = _batcher(do_sample=True)
        cb.submit(**_req(0), temperature=0.7)
        cb.submit(**_req(1), top_k=10)
        assert [r.gen["seed"] for r in cb._queue] and all(0 <= r.gen["seed"] < 2 ** 62 for r in cb._queue)  # drawn at submit, not at admission
        for _ in cb:
            pass
        seeds.append([c["gen"]["seed"] for c in eng.calls])
    assert seeds[0] == seeds[1] and seeds[0][0] != seeds[0][1]


@pytest.mark.parametrize("bad", [dict(temperature=0), dict(temperature=0.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                                 dict(top_p=0), dict(top_p=1.5), dict(top_k=-1), dict(min_new_tokens=-1)])
def test_bad_values_raise_at_submit_and_leave_the_queue_unchanged(bad):
    cb, eng = _batcher(do_sample=True)
    cb.submit(**_req(0))
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError, match=next(iter(bad))):
        cb.submit(**_req(1), **bad)
    assert cb.pending() == 1 and len(cb._queue) == 1 and eng.calls == []
    assert torch.equal(state, torch.random.get_rng_state())  # a refused submit draws no seed
    assert cb.submit(**_req(1)) == 1  # and takes no ticket


class RecordingStreamEngine(TST.StreamSessionEngine):
    def __init__(self, spec, sd, kind):
        super().__init__(spec, sd, kind)
        self.calls = []

    def admit_row(self, row, enc, enc_mask, prompt, prompt_mask, max_length=0, sample=True, **kw):
        assert set(kw) <= {"gen"}, kw
        self.calls.append(dict(kw))
        super().admit_row(row, enc, enc_mask, prompt, prompt_mask, max_length=max_length, sample=sample)


def test_the_streaming_batcher_forwards_the_same_record():
    """_poll and _admit go through one admission helper: the same requests reach admit_row with the same keywords in both modes."""
    reqs = [dict(_req(0), temperature=0.7, seed=5), _req(1), dict(_req(2), do_sample=False), dict(_req(3), top_p=0.5)]
    calls = []
    for stream in ({}, dict(stream_chunk_frames=4)):
        m, eng0, codec, _ = TST._model()
        eng = RecordingStreamEngine(eng0.spec, eng0.sd, "clean")
        m._get_engine = lambda B, N, Pp, L, T=0: eng
        torch.manual_seed(77)
        cb = P.ContinuousBatcher(m, slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, max_new_tokens=14, min_new_tokens=14, do_sample=True,
                                 temperature=0.8, **stream)
        tickets = [cb.submit(**r) for r in reqs]
        if stream:
            assert sorted(t for t, c, last in cb.chunks() if last) == tickets
            assert sorted(codec.resets) == [0, 0, 1, 1]  # stream_reset still follows every admission
        else:
            assert sorted(t for t, w, n in cb) == tickets
        calls.append(eng.calls)
    assert calls[0] == calls[1] and len(calls[0]) == 4
    g0 = calls[0][0]["gen"]
    assert set(g0) == KEYS and (g0["min_new_tokens"], g0["do_sample"], g0["temperature"], g0["seed"]) == (14, True, 0.7, 5)
    assert "gen" not in calls[0][1] and calls[0][2]["gen"]["do_sample"] is False and calls[0][3]["gen"]["top_p"] == 0.5
