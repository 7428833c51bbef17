"""CPU: the layers above the step records (include/ptts_step_record.h) on the oracle-backed engine stand-ins - the routing of ``generate()`` with
and without ``model.enable_device_step_records()`` (which loop runs, the tuples' lengths and shapes against the host loop's, the interplay with
the other three switches, the engine's record switched off again) and ``ContinuousBatcher``: validation and refusals, the order of the slot
record against the admission (single, group), the lifecycle of ``step_records(ticket)`` and ``cancel()``."""
import threading

import pytest
import torch

import parler_tts_amd as P

import test_batched_admission_cpu as TB
import test_device_logit_edits_cpu as TE
import test_device_penalties_cpu as TP
import test_generate_glue_cpu as TG

V, K = 1088, 9


class RoutingEngine(TE.RoutingEngine):
    """The logit edits' routing stand-in plus the step-record setter. It records nothing into the arenas: what is checked here is which loop
    runs, what the engine is handed and what generate() makes of the arenas."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.step_records, self.record_calls, self.host_loops = None, [], 0

    def set_step_records(self, scores=None, logits=None, cap_steps=0, enabled=True):
        self.record_calls.append((scores, logits, cap_steps) if enabled else False)
        self.step_records = (scores, logits, cap_steps) if enabled else None


def _routing_model():
    m, spec, sd, _ = TG._model()
    eng = RoutingEngine(spec, sd)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    host = m._run_host_loop

    def counted(*a, **k):
        eng.host_loops += 1
        return host(*a, **k)

    m._run_host_loop = counted
    return m, eng


def _call(m, **kw):
    return TP._call(m, **dict(dict(min_new_tokens=2, return_dict_in_generate=True), **kw))


def _shapes(out, name):
    return [tuple(t.shape) for t in out[name]]


def test_generate_routing_with_the_switch_off_and_on():
    from transformers import LogitsProcessorList

    m, eng = _routing_model()
    assert not getattr(m, "device_step_records", False)
    ref = {}
    for kw in (dict(output_scores=True), dict(output_logits=True), dict(output_scores=True, output_logits=True)):
        out = _call(m, **kw)
        assert eng.prefills[-1] == "host" and eng.record_calls == []  # off: the host loop, as ever, and the engine hears nothing
        ref[tuple(sorted(kw))] = out
    assert eng.host_loops == 3
    assert m.enable_device_step_records() is m and m.device_step_records
    m._get_engine = lambda B, N, Pp, L, T=0: eng  # (the switch drops cached engines; the stand-in stays)
    for kw in (dict(output_scores=True), dict(output_logits=True), dict(output_scores=True, output_logits=True)):
        n = len(eng.record_calls)
        out = _call(m, **kw)
        assert eng.prefills[-1] == "device" and eng.host_loops == 3, kw  # _run_host_loop is not entered
        scores, logits, cap = eng.record_calls[n]
        assert cap == 12 and (scores is not None) == ("output_scores" in kw) and (logits is not None) == ("output_logits" in kw)
        for t in (scores, logits):
            assert t is None or (tuple(t.shape) == (12, K, V) and t.dtype == torch.float32 and t.is_contiguous())
        assert eng.record_calls[n + 1] is False and eng.step_records is None  # the engine lets go of the arenas when the call ends
        host = ref[tuple(sorted(kw))]
        assert torch.equal(out.sequences, host.sequences)
        for name in ("scores", "logits"):
            assert (name in out) == ("output_" + name in kw) == (name in host)
            if name in out:  # the host loop's tuple: one [B*K, V] matrix per step made
                assert isinstance(out[name], tuple) and len(out[name]) == len(host[name]) and _shapes(out, name) == _shapes(host, name)
                arena = scores if name == "scores" else logits
                assert all(t.data_ptr() == arena[i].data_ptr() for i, t in enumerate(out[name]))  # views of the arena the engine wrote
    # score outputs without return_dict_in_generate are no outputs: the plain device loop, no record
    n = len(eng.record_calls)
    TP._call(m, min_new_tokens=2, output_scores=True)
    assert eng.prefills[-1] == "device" and len(eng.record_calls) == n
    # the streamer path is the device loop too
    streamer = P.ParlerTTSStreamer(m, device="cpu", play_steps=10, stride=8)
    streamer.halo_frames = 64
    got = {}
    th = threading.Thread(target=lambda: got.update(out=_call(m, output_scores=True, streamer=streamer)))
    th.start()
    assert len([c for c in streamer]) >= 1
    th.join()
    assert eng.prefills[-1] == "device" and eng.host_loops == 3 and len(got["out"]["scores"]) == len(ref[("output_scores",)]["scores"])
    # a user processor or stopping criterion keeps the host loop, with the host loop's tuples
    n = len(eng.record_calls)
    out = _call(m, output_scores=True, logits_processor=LogitsProcessorList([P.ParlerTTSLogitsProcessor(1024, 9, 1, "cpu")]))
    assert eng.prefills[-1] == "host" and eng.host_loops == 4 and len(eng.record_calls) == n and len(out["scores"]) == 12
    # an option whose own switch is off keeps it too
    _call(m, output_scores=True, repetition_penalty=1.4)
    assert eng.prefills[-1] == "host" and len(eng.record_calls) == n and eng.penalty_calls == []
    _call(m, output_logits=True, forced_eos_token_id=1024)
    assert eng.prefills[-1] == "host" and len(eng.record_calls) == n
    m.enable_device_step_records(False)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m, output_scores=True)
    assert eng.prefills[-1] == "host" and len(eng.record_calls) == n


def test_a_record_left_on_the_engine_is_switched_off_by_a_following_plain_call():
    m, eng = _routing_model()
    m.enable_device_step_records()
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    eng.step_records = (torch.empty(1), None, 1)  # what a call that raised half-way would leave behind
    TP._call(m, min_new_tokens=2)
    assert eng.prefills[-1] == "device" and eng.record_calls == [False] and eng.step_records is None
    TP._call(m, min_new_tokens=2)
    assert eng.record_calls == [False]  # and a plain call on a plain engine makes no call at all


def test_interplay_with_each_of_the_other_three_switches():
    m, eng = _routing_model()
    m.enable_device_step_records()
    cases = [("enable_device_penalties", dict(repetition_penalty=1.4, no_repeat_ngram_size=2), lambda: eng.penalty_calls[-1] == (1.4, 2, True)),
             ("enable_device_warpers", dict(do_sample=True, min_p=0.05), lambda: eng.warp_calls[-1] == (0.05, 1.0, 0.0, 0.0, True)),
             ("enable_device_logit_edits", dict(suppress_tokens=[3, 4]), lambda: eng.edit_calls[-1].suppress == (3, 4))]
    for switch, kw, reached in cases:
        m._get_engine = lambda B, N, Pp, L, T=0: eng
        n = len(eng.record_calls)
        _call(m, output_scores=True, **kw)  # the option's own switch is off: the host loop
        assert eng.prefills[-1] == "host" and len(eng.record_calls) == n, switch
        getattr(m, switch)()
        m._get_engine = lambda B, N, Pp, L, T=0: eng
        out = _call(m, output_scores=True, output_logits=True, **kw)
        assert eng.prefills[-1] == "device" and reached(), switch
        assert eng.record_calls[n][2] == 12 and eng.record_calls[n + 1] is False and len(out["scores"]) == len(out["logits"]) >= 1
        getattr(m, switch)(False)
    # the two excluded logit-edit combinations keep the host loop with the record switch on as well
    m.enable_device_logit_edits(), m.enable_device_penalties()
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    n = len(eng.record_calls)
    _call(m, output_scores=True, sequence_bias={(7,): 2.0}, repetition_penalty=1.4)
    assert eng.prefills[-1] == "host" and len(eng.record_calls) == n
    _call(m, output_scores=True, exponential_decay_length_penalty=(3, 1.2), min_new_tokens=5)
    assert eng.prefills[-1] == "host" and len(eng.record_calls) == n


def test_an_engine_without_the_attribute_receives_no_call():
    m, spec, sd, _ = TG._model()
    eng = TP.RoutingEngine(spec, sd)  # knows nothing of step records
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    TP._call(m)
    _call(m, output_scores=True)
    assert eng.prefills == ["device", "host"] and not hasattr(eng, "step_records")


# ---- ContinuousBatcher --------------------------------------------------------------------------------------------------------------------
class RecordSessionEngine(TE.EditSessionEngine):
    """The logit edits' session stand-in plus the two step-record setters, in the same ``calls`` list. A slot's admission fills step 0 of its
    buffers with the slot's number, every decode step the next record with the step's index: enough to see which buffer belongs to whom."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.step_records, self.slot_bufs = None, {}

    def set_step_records(self, scores=None, logits=None, cap_steps=0, enabled=True):
        self.calls.append(("records", scores, logits, cap_steps, enabled))
        self.step_records = (scores, logits, cap_steps) if enabled else None

    def set_slot_step_records(self, slot, scores=None, logits=None, cap_steps=0, default=False):
        assert self.full[slot] is None, "the slot record is written while the slot is idle"
        for t in (scores, logits):
            assert t is None or (tuple(t.shape) == (cap_steps, K, V) and t.dtype == torch.float32)
        self.calls.append(("slot_records", slot, scores is not None, logits is not None, cap_steps))
        self.slot_bufs[slot] = [t for t in (scores, logits) if t is not None]

    def admit_row(self, row, *a, **k):
        super().admit_row(row, *a, **k)
        for t in self.slot_bufs.get(row, []):
            t[0] = float(row)

    def decode_steps(self, n):
        before = list(self.cur)
        super().decode_steps(n)
        for s, bufs in self.slot_bufs.items():
            if self.full[s] is not None:
                for t in bufs:
                    for i in range(before[s] - 1, min(self.cur[s] - 1, t.shape[0])):
                        t[i] = float(i)

    def retire_row(self, row):
        self.slot_bufs.pop(row, None)  # ptts_retire_row clears the slot's record
        super().retire_row(row)


def _batcher(switch=True, **session):
    m, spec, sd, dac, _ = TB._model()
    eng = RecordSessionEngine(spec, sd)
    if switch:
        m.enable_device_step_records()
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    kw = dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, max_new_tokens=14, min_new_tokens=2)
    kw.update(session)
    return P.ContinuousBatcher(m, **kw), eng


def _req(i=0, **kw):
    return dict(TP._req(i), **kw)


def test_without_the_switch_submit_refuses_and_the_engine_hears_nothing():
    cb, eng = _batcher(switch=False)
    assert [c[0] for c in eng.calls] == ["begin"]
    for kw in (dict(output_scores=True), dict(output_logits=True)):
        with pytest.raises(ValueError, match="enable_device_step_records"):
            cb.submit(**_req(0, **kw))
    assert cb.pending() == 0 and cb.submit(**_req(0)) == 0  # a refused submit queues nothing and takes no ticket
    for name in ("output_scores", "output_logits"):  # for a whole session they stay refused: they belong to a request
        with pytest.raises(NotImplementedError, match=name):
            _batcher(**{name: True})


def test_the_session_is_opened_with_records_on_and_an_engine_left_with_them_is_switched_off():
    cb, eng = _batcher()
    assert eng.calls == [("records", None, None, 0, True), ("begin",)]  # "on, no slot records yet", before the session begins
    m, spec, sd, dac, _ = TB._model()
    eng = RecordSessionEngine(spec, sd)
    eng.step_records = (None, None, 0)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    P.ContinuousBatcher(m, slots=2, max_description_tokens=9, max_prompt_tokens=5, max_new_tokens=14)
    assert eng.calls == [("records", None, None, 0, False), ("begin",)]


def test_single_admissions_set_the_slot_record_immediately_before_the_admission_and_the_lifecycle():
    cb, eng = _batcher()
    t0 = cb.submit(**_req(0, output_scores=True))
    t1 = cb.submit(**_req(1))
    t2 = cb.submit(**_req(2, output_scores=True, output_logits=True, max_new_tokens=7))
    t3 = cb.submit(**_req(3, output_logits=True))
    with pytest.raises(KeyError):
        cb.step_records(t0)  # not before the request has finished
    got = {}
    for t, w, n in cb:
        if t != t1:
            rec = cb.step_records(t)  # available once the waveform has been yielded
            got[t] = rec
            with pytest.raises(KeyError):
                cb.step_records(t)  # handed out once
    with pytest.raises(KeyError):
        cb.step_records(t1)  # asked for none
    calls = [c for c in eng.calls if c[0] in ("slot_records", "admit_row", "admit_rows")]
    admits = [i for i, c in enumerate(calls) if c[0] == "admit_row"]
    assert len(admits) == 4 and not any(c[0] == "admit_rows" for c in calls)
    before = [calls[i - 1] if i > 0 and calls[i - 1][0] == "slot_records" else None for i in admits]
    slot = [calls[i][1] for i in admits]
    assert before[0] == ("slot_records", slot[0], True, False, 12) and before[1] is None
    assert before[2] == ("slot_records", slot[2], True, True, 7) and before[3] == ("slot_records", slot[3], False, True, 12)
    assert sorted(got[t0]) == ["scores"] and sorted(got[t2]) == ["logits", "scores"] and sorted(got[t3]) == ["logits"]
    # trimmed to the request's steps (min_new_tokens = max_new_tokens here: every request runs to its limit), K x V each
    assert tuple(got[t0]["scores"].shape) == (12, K, V) and tuple(got[t2]["scores"].shape) == (7, K, V) == tuple(got[t2]["logits"].shape)
    assert float(got[t0]["scores"][0, 0, 0]) == float(slot[0]) and [float(x) for x in got[t0]["scores"][1:, 0, 0]] == list(range(1, 12))
    assert cb._records == {} and all(r is None for r in cb._slot)


def test_group_admissions_set_every_record_before_the_one_engine_call():
    cb, eng = _batcher(slots=2, admit_batch=2)
    cb.run([_req(0, output_scores=True), _req(1, output_logits=True), _req(2), _req(3, output_scores=True)])
    calls = [c for c in eng.calls if c[0] in ("slot_records", "admit_row", "admit_rows")]
    assert [c[0] for c in calls] == ["slot_records", "slot_records", "admit_rows", "slot_records", "admit_rows"], calls
    s0, s1 = calls[2][1]
    assert calls[0] == ("slot_records", s0, True, False, 12) and calls[1] == ("slot_records", s1, False, True, 12)
    assert calls[3] == ("slot_records", calls[4][1][1], True, False, 12)
    assert sorted(cb._records) == [0, 1, 3]  # run() read none of them: still there for step_records()
    assert tuple(cb.step_records(3)["scores"].shape) == (12, K, V)


def test_close_drops_the_records_nobody_read():
    cb, eng = _batcher()
    cb.run([_req(0, output_scores=True), _req(1, output_logits=True)])
    assert sorted(cb._records) == [0, 1]  # run() reads none: the batcher holds them until step_records() or close()
    cb.close()
    assert cb._records == {}
    with pytest.raises(KeyError):
        cb.step_records(0)


def test_cancel_frees_the_buffers_of_a_running_and_of_a_queued_request():
    cb, eng = _batcher(slots=1)
    t0 = cb.submit(**_req(0, output_scores=True))
    t1 = cb.submit(**_req(1, output_logits=True))
    it = iter(cb.chunks()) if cb.chunk is not None else None
    assert it is None
    cb._poll()  # admits t0, runs a few steps
    assert cb._slot[0].ticket == t0 and cb._slot[0].records is not None and 0 in eng.slot_bufs
    assert cb.cancel(t0) and cb._slot[0] is None and 0 not in eng.slot_bufs
    assert cb.cancel(t1) and cb.pending() == 0
    for t in (t0, t1):
        with pytest.raises(KeyError):
            cb.step_records(t)
    t2 = cb.submit(**_req(2))  # the slot is reused by a request without a record: no setter call for it
    n = sum(c[0] == "slot_records" for c in eng.calls)
    assert [t for t, _, _ in cb] == [t2] and sum(c[0] == "slot_records" for c in eng.calls) == n == 1
