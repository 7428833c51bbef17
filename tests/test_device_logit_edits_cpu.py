"""CPU: the layers above the logit-edit node (include/ptts_logit_edit.h) - the record ``generation_extras.logit_edits_of`` builds and the two
rules of the node's place in the chain, the routing of ``generate()`` with and without ``model.enable_device_logit_edits()`` on the engine
stand-in of tests/test_generate_glue_cpu.py, and ``ContinuousBatcher`` on the oracle-backed session stand-ins: refusals, validation, and the
order of the slot record against the admission for single, group and voice admissions."""
import threading

import pytest
import torch

import parler_tts_amd as P
from parler_tts_amd.generation_extras import LOGIT_EDIT_OPTIONS, LogitEdits, logit_edit_rule_broken, logit_edits_of

import test_batched_admission_cpu as TB
import test_device_penalties_cpu as TP
import test_device_warpers_cpu as TW
import test_generate_glue_cpu as TG
import test_session_voice_groups_cpu as TVG

V, EOS = 1088, 1024  # the decoder of the stand-in models


# ---- the record and the rules -------------------------------------------------------------------------------------------------------------
def test_the_record_of_the_five_options():
    ed = logit_edits_of(V, EOS, 40, sequence_bias={(EOS,): 2.0, (5,): -1.5}, bad_words_ids=[[7], [EOS]], suppress_tokens=[3, V, V + 9],
                        begin_suppress_tokens=[EOS], exponential_decay_length_penalty=(6, 1.1))
    assert ed == LogitEdits(((EOS, 2.0), (5, -1.5)), (7, EOS), (3,), (EOS,), (6, 1.1), True, True) and not ed.neutral
    assert logit_edits_of(V, EOS, 40, sequence_bias=[[[5], 1.5]]).bias == ((5, 1.5),)  # transformers' list form
    assert logit_edits_of(V, EOS) == LogitEdits() and LogitEdits().neutral
    ed = logit_edits_of(V, EOS, suppress_tokens=[V + 1])  # nothing inside the vocabulary: still the stage, which changes nothing
    assert ed.suppress == () and ed.suppress_on and not ed.neutral
    assert set(LOGIT_EDIT_OPTIONS) == {"sequence_bias", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "exponential_decay_length_penalty"}


@pytest.mark.parametrize("bad, match", [
    (dict(sequence_bias={(5, 6): 1.0}), "single-token"), (dict(bad_words_ids=[[5, 6]]), "single-token"),
    (dict(sequence_bias={(V,): 1.0}), "outside the vocabulary"), (dict(bad_words_ids=[[V + 3]]), "outside the vocabulary"),
    (dict(sequence_bias={(5,): float("-inf")}), "finite"), (dict(sequence_bias={(5,): 1}), "sequence_bias"), (dict(sequence_bias={}), "sequence_bias"),
    (dict(bad_words_ids=[5]), "bad_words_ids"), (dict(suppress_tokens=[1.5]), "suppress_tokens"), (dict(suppress_tokens=[None]), "suppress_tokens"), (dict(begin_suppress_tokens=["a"]), "begin_suppress_tokens"), (dict(begin_suppress_tokens=7), "begin_suppress_tokens"),
    (dict(exponential_decay_length_penalty=(-1, 1.1)), "exponential_decay_length_penalty"), (dict(exponential_decay_length_penalty=(3, 0.0)), "exponential_decay_length_penalty"),
    (dict(exponential_decay_length_penalty=(3, float("nan"))), "exponential_decay_length_penalty"), (dict(exponential_decay_length_penalty=(3,)), "exponential_decay_length_penalty"),
    (dict(exponential_decay_length_penalty=(3, 1e30)), "overflows"),
])
def test_what_the_node_does_not_compute_is_a_value_error(bad, match):
    with pytest.raises(ValueError, match=match):
        logit_edits_of(V, EOS, 40, **bad)


def test_the_two_rules():
    bias, decay = LogitEdits(bias=((5, 1.0),)), LogitEdits(decay=(6, 1.1))
    assert logit_edit_rule_broken(bias, None, None, 0) is None and logit_edit_rule_broken(bias, 1.0, 0, 30) is None  # a neutral penalty beside it is fine
    assert "sequence_bias" in logit_edit_rule_broken(bias, 1.3, 0, 0) and "sequence_bias" in logit_edit_rule_broken(bias, 1.0, 2, 0)
    assert logit_edit_rule_broken(LogitEdits(bad=(5,), suppress=(3,), suppress_on=True), 1.3, 2, 50) is None  # the sets commute with everything
    assert logit_edit_rule_broken(decay, 1.3, 2, 7) is None  # min_new_tokens <= start + 1
    assert "min_new_tokens" in logit_edit_rule_broken(decay, None, None, 8)


# ---- generate(): which loop runs ----------------------------------------------------------------------------------------------------------
class RoutingEngine(TW.RoutingEngine):
    """The warpers' routing stand-in plus the logit-edit setter."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.logit_edits, self.edit_calls = None, []

    def set_logit_edits(self, edits=None, enabled=True):
        self.edit_calls.append(edits if enabled else False)
        self.logit_edits = (edits if edits is not None else LogitEdits()) if enabled else None


def _routing_model():
    m, spec, sd, _ = TG._model()
    assert (m.config.decoder.vocab_size, m.config.decoder.eos_token_id) == (V, EOS)
    eng = RoutingEngine(spec, sd)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    return m, eng


def _call(m, **kw):
    return TP._call(m, **dict(dict(min_new_tokens=2), **kw))


EACH = [dict(sequence_bias={(EOS,): -2.0}), dict(bad_words_ids=[[5], [EOS]]), dict(suppress_tokens=[3, 4]), dict(begin_suppress_tokens=[EOS]),
        dict(exponential_decay_length_penalty=(3, 1.2))]


def test_generate_routing_with_the_switch_off_and_on():
    from transformers import LogitsProcessorList

    m, eng = _routing_model()
    assert not getattr(m, "device_logit_edits", False)
    for kw in EACH:
        _call(m, **kw)
        assert eng.prefills[-1] == "host" and eng.edit_calls == []  # off: the host loop, as ever, and the engine hears nothing
    _call(m)
    assert eng.prefills[-1] == "device" and eng.edit_calls == []
    assert m.enable_device_logit_edits() is m and m.device_logit_edits
    m._get_engine = lambda B, N, Pp, L, T=0: eng  # (the switch drops cached engines; the stand-in stays)
    for kw in EACH:
        _call(m, **kw)
        assert eng.prefills[-1] == "device" and eng.edit_calls[-1] == logit_edits_of(V, EOS, 13, **kw), kw
    _call(m, **{k: v for kw in EACH for k, v in kw.items()})  # all five in one call
    assert eng.prefills[-1] == "device" and eng.edit_calls[-1] == LogitEdits(((EOS, -2.0),), (5, EOS), (3, 4), (EOS,), (3, 1.2), True, True)
    streamer = P.ParlerTTSStreamer(m, device="cpu", play_steps=10, stride=8)  # the streamer path is the device loop too
    streamer.halo_frames = 64
    th = threading.Thread(target=lambda: _call(m, suppress_tokens=[9], streamer=streamer))
    th.start()
    assert len([c for c in streamer]) >= 1
    th.join()
    assert eng.prefills[-1] == "device" and eng.edit_calls[-1].suppress == (9,)
    _call(m)  # a plain call after one with edits: the node goes off again
    assert eng.prefills[-1] == "device" and eng.edit_calls[-1] is False and eng.logit_edits is None
    n = len(eng.edit_calls)
    _call(m)
    assert len(eng.edit_calls) == n  # and a plain call on a plain engine makes no call at all
    # anything that needs the host's view of a step, or an option without a device implementation, keeps the host loop
    _call(m, suppress_tokens=[9], logits_processor=LogitsProcessorList([P.ParlerTTSLogitsProcessor(1024, 9, 1, "cpu")]))
    assert eng.prefills[-1] == "host" and len(eng.edit_calls) == n
    _call(m, suppress_tokens=[9], return_dict_in_generate=True, output_scores=True)
    assert eng.prefills[-1] == "host" and len(eng.edit_calls) == n
    _call(m, suppress_tokens=[9], forced_eos_token_id=EOS)
    assert eng.prefills[-1] == "host" and len(eng.edit_calls) == n
    _call(m, suppress_tokens=[9], renormalize_logits=True)
    assert eng.prefills[-1] == "host" and len(eng.edit_calls) == n
    _call(m, suppress_tokens=[9], repetition_penalty=1.4)  # the penalties' switch is off: the pair runs on the host
    assert eng.prefills[-1] == "host" and len(eng.edit_calls) == n and eng.penalty_calls == []
    m.enable_device_logit_edits(False)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m, suppress_tokens=[9])
    assert eng.prefills[-1] == "host" and len(eng.edit_calls) == n


def test_each_eligibility_rule_sends_the_call_to_the_host_loop():
    m, eng = _routing_model()
    m.enable_device_logit_edits()
    m.enable_device_penalties()
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m, bad_words_ids=[[5, 6]])  # a multi-token entry depends on the history
    assert eng.prefills[-1] == "host" and eng.edit_calls == []
    _call(m, sequence_bias={(5, 6): 1.0, (7,): 2.0})
    assert eng.prefills[-1] == "host" and eng.edit_calls == []
    _call(m, sequence_bias={(7,): float("-inf")})
    assert eng.prefills[-1] == "host" and eng.edit_calls == []
    _call(m, exponential_decay_length_penalty=(3, 1.2), min_new_tokens=5)  # 5 > start + 1: transformers' chain would meet the blocked EOS
    assert eng.prefills[-1] == "host" and eng.edit_calls == []
    _call(m, exponential_decay_length_penalty=(3, 1.2), min_new_tokens=4)
    assert eng.prefills[-1] == "device" and eng.edit_calls[-1].decay == (3, 1.2)
    _call(m, exponential_decay_length_penalty=(3, 1.2), min_new_tokens=0, min_length=7)  # min_length counts the BOS column: 6 new tokens
    assert eng.prefills[-1] == "host"
    n = len(eng.edit_calls)
    _call(m, sequence_bias={(7,): 2.0}, repetition_penalty=1.4)  # the bias does not commute with the penalty: the host loop, both as processors
    assert eng.prefills[-1] == "host" and len(eng.edit_calls) == n and eng.penalty_calls == []
    _call(m, sequence_bias={(7,): 2.0}, no_repeat_ngram_size=2)
    assert eng.prefills[-1] == "host" and len(eng.edit_calls) == n and eng.penalty_calls == []
    _call(m, sequence_bias={(7,): 2.0}, repetition_penalty=1.0)  # a neutral penalty beside it is fine
    assert eng.prefills[-1] == "device" and eng.edit_calls[-1].bias == ((7, 2.0),)
    _call(m, bad_words_ids=[[5]], suppress_tokens=[3], repetition_penalty=1.4, no_repeat_ngram_size=2)  # the sets commute with the penalties
    assert eng.prefills[-1] == "device" and eng.edit_calls[-1].bad == (5,) and eng.penalty_calls[-1] == (1.4, 2, True)


def test_the_three_switches_together_and_each_missing_one():
    m, eng = _routing_model()
    kw = dict(do_sample=True, min_p=0.05, repetition_penalty=1.4, suppress_tokens=[3], begin_suppress_tokens=[EOS])
    for on in ((True, True, False), (True, False, True), (False, True, True)):
        m.enable_device_penalties(on[0]), m.enable_device_warpers(on[1]), m.enable_device_logit_edits(on[2])
        m._get_engine = lambda B, N, Pp, L, T=0: eng
        _call(m, **kw)
        assert eng.prefills[-1] == "host" and eng.edit_calls == [] and eng.warp_calls == [] and eng.penalty_calls == []
    m.enable_device_penalties(), m.enable_device_warpers(), m.enable_device_logit_edits()
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m, **kw)
    assert eng.prefills[-1] == "device" and eng.penalty_calls == [(1.4, None, True)] and eng.warp_calls == [(0.05, 1.0, 0.0, 0.0, True)]
    assert eng.edit_calls == [LogitEdits(suppress=(3,), begin_suppress=(EOS,), suppress_on=True, begin_suppress_on=True)]
    _call(m, do_sample=True, min_p=0.05)  # warpers alone: the other two nodes go off
    assert eng.prefills[-1] == "device" and eng.edit_calls[-1] is False and eng.penalty_calls[-1] == (None, None, False)


def test_an_engine_without_the_attribute_receives_no_call():
    m, spec, sd, _ = TG._model()
    eng = TP.RoutingEngine(spec, sd)  # knows nothing of logit edits
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    _call(m)
    _call(m, suppress_tokens=[3])
    assert eng.prefills == ["device", "host"] and not hasattr(eng, "logit_edits")


# ---- ContinuousBatcher --------------------------------------------------------------------------------------------------------------------
class EditSessionEngine(TW.WarpSessionEngine):
    """The warpers' session stand-in plus the two logit-edit setters, in the same ``calls`` list."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.logit_edits = None

    def set_logit_edits(self, edits=None, enabled=True):
        self.calls.append(("edits", edits, enabled))
        self.logit_edits = edits if enabled else None

    def set_slot_logit_edits(self, slot, edits=None, default=False):
        assert self.full[slot] is None, "the slot record is written while the slot is idle"
        self.calls.append(("slot_edits", slot, edits))


def _batcher(switch=True, penalties=False, **session):
    m, spec, sd, dac, _ = TB._model()
    eng = EditSessionEngine(spec, sd)
    if switch:
        m.enable_device_logit_edits()
    if penalties:
        m.enable_device_penalties()
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    kw = dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, max_new_tokens=14, min_new_tokens=2)
    kw.update(session)
    return P.ContinuousBatcher(m, **kw), eng


_req = TP._req


def test_without_the_switch_both_places_refuse_as_today():
    for kw in EACH:
        with pytest.raises(NotImplementedError, match="host loop"):
            _batcher(switch=False, **kw)
    cb, eng = _batcher(switch=False)
    assert eng.calls == [("begin",)]  # no setter call on an engine that never had the node
    for kw in EACH:
        with pytest.raises(NotImplementedError, match="enable_device_logit_edits"):
            cb.submit(**_req(0, **kw))
    assert cb.pending() == 0 and cb.submit(**_req(0)) == 0


def test_other_extras_stay_refused_with_the_switch():
    with pytest.raises(NotImplementedError, match="forced_eos_token_id"):
        _batcher(suppress_tokens=[3], forced_eos_token_id=EOS)
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        _batcher(suppress_tokens=[3], repetition_penalty=1.3)  # the penalties have their own switch
    with pytest.raises(NotImplementedError, match="renormalize_logits"):
        _batcher(renormalize_logits=True)


def test_the_session_defaults_reach_the_engine_before_the_session_begins():
    cb, eng = _batcher(suppress_tokens=[3], exponential_decay_length_penalty=(5, 1.1))
    assert eng.calls == [("edits", LogitEdits(suppress=(3,), decay=(5, 1.1), suppress_on=True), True), ("begin",)]
    cb, eng = _batcher()
    assert eng.calls == [("edits", LogitEdits(), True), ("begin",)]  # neutral: the node is there for the requests that bring edits
    cb, eng = _batcher(penalties=True, bad_words_ids=[[7]], repetition_penalty=1.3)
    assert eng.calls == [("session", 1.3, 0, True), ("edits", LogitEdits(bad=(7,)), True), ("begin",)]


@pytest.mark.parametrize("where", ["session", "submit"])
@pytest.mark.parametrize("bad, match", [(dict(bad_words_ids=[[5, 6]]), "single-token"), (dict(sequence_bias={(5, 6): 1.0}), "single-token"),
                                        (dict(sequence_bias={(V + 1,): 1.0}), "outside the vocabulary"), (dict(suppress_tokens=[0.5]), "suppress_tokens"),
                                        (dict(exponential_decay_length_penalty=(3, -1.0)), "exponential_decay_length_penalty"),
                                        (dict(exponential_decay_length_penalty=(0, 1.2)), "min_new_tokens")])  # the session's min_new_tokens is 2 > 0 + 1
def test_bad_values_and_broken_rules_are_value_errors_and_a_refused_submit_queues_nothing(where, bad, match):
    if where == "session":
        with pytest.raises(ValueError, match=match):
            _batcher(**bad)
        return
    cb, eng = _batcher()
    cb.submit(**_req(0))
    with pytest.raises(ValueError, match=match):
        cb.submit(**_req(1, **bad))
    assert cb.pending() == 1 and len(cb._queue) == 1 and [c[0] for c in eng.calls] == ["edits", "begin"]
    assert cb.submit(**_req(1)) == 1  # and it took no ticket


def test_the_rules_look_at_the_values_in_effect_for_the_request():
    cb, eng = _batcher(penalties=True, sequence_bias={(7,): 1.5})
    with pytest.raises(ValueError, match="sequence_bias"):
        cb.submit(**_req(0, repetition_penalty=1.3))  # the session's bias beside the request's penalty
    assert cb.submit(**_req(0, repetition_penalty=1.0)) == 0
    with pytest.raises(ValueError, match="sequence_bias"):
        _batcher(penalties=True, sequence_bias={(7,): 1.5}, no_repeat_ngram_size=2)
    cb, eng = _batcher(penalties=True, repetition_penalty=1.3)
    with pytest.raises(ValueError, match="sequence_bias"):
        cb.submit(**_req(0, sequence_bias={(7,): 1.5}))  # the request's bias beside the session's penalty
    assert cb.submit(**_req(0, sequence_bias={(7,): 1.5}, repetition_penalty=1.0)) == 0
    cb, eng = _batcher(exponential_decay_length_penalty=(1, 1.2))
    with pytest.raises(ValueError, match="min_new_tokens"):
        cb.submit(**_req(0, min_new_tokens=3))  # the session's decay beside the request's min_new_tokens
    assert cb.submit(**_req(0, min_new_tokens=1)) == 0 and cb.submit(**_req(1, min_new_tokens=9, exponential_decay_length_penalty=(8, 1.2))) == 1


def test_single_admissions_write_the_slot_record_immediately_before_the_admission():
    cb, eng = _batcher(suppress_tokens=[3])
    cb.run([_req(0, begin_suppress_tokens=[EOS]), _req(1), _req(2, suppress_tokens=[], exponential_decay_length_penalty=(4, 1.3)), _req(3, bad_words_ids=[[9]])])
    calls = [c for c in eng.calls if c[0] in ("slot_edits", "admit_row", "admit_rows")]
    assert not any(c[0] == "admit_rows" for c in calls)
    admits = [i for i, c in enumerate(calls) if c[0] == "admit_row"]
    assert len(admits) == 4
    before = [calls[i - 1] if i > 0 and calls[i - 1][0] == "slot_edits" else None for i in admits]
    slot = [calls[i][1] for i in admits]
    sup = dict(suppress=(3,), suppress_on=True)
    assert before[0] == ("slot_edits", slot[0], LogitEdits(begin_suppress=(EOS,), begin_suppress_on=True, **sup))  # the session's list fills the option left out
    assert before[1] is None                                                                                     # no options: no call, the slot runs on the session's record
    assert before[2] == ("slot_edits", slot[2], LogitEdits(decay=(4, 1.3), suppress_on=True))                    # a request may empty the session's list for itself
    assert before[3] == ("slot_edits", slot[3], LogitEdits(bad=(9,), **sup))
    assert sum(c[0] == "slot_edits" for c in calls) == 3
    assert sum(c[0] == "retire" for c in eng.calls) == 4  # retire_row puts the session's record back: nothing else to undo


def test_group_admissions_write_every_record_before_the_one_engine_call():
    cb, eng = _batcher(slots=2, admit_batch=2, penalties=True)
    cb.run([_req(0, suppress_tokens=[3], repetition_penalty=1.5), _req(1, bad_words_ids=[[4]]), _req(2), _req(3, begin_suppress_tokens=[5])])
    calls = [c for c in eng.calls if c[0] in ("slot", "slot_edits", "admit_row", "admit_rows")]
    assert [c[0] for c in calls] == ["slot", "slot_edits", "slot_edits", "admit_rows", "slot_edits", "admit_rows"], calls
    s0, s1 = calls[3][1]
    assert calls[0] == ("slot", s0, 1.5, 0) and calls[1] == ("slot_edits", s0, LogitEdits(suppress=(3,), suppress_on=True))
    assert calls[2] == ("slot_edits", s1, LogitEdits(bad=(4,)))
    assert calls[4] == ("slot_edits", calls[5][1][1], LogitEdits(begin_suppress=(5,), begin_suppress_on=True))


class VoiceEditEngine(TVG.VoiceGroupEngine):
    """The voice-group stand-in plus the logit-edit setters: ``events`` holds slot records and admissions in call order."""
    logit_edits = None

    def set_logit_edits(self, edits=None, enabled=True):
        self.logit_edits = edits if enabled else None

    def set_slot_logit_edits(self, slot, edits=None, default=False):
        assert self.full[slot] is None, "the slot record is written while the slot is idle"
        self.events.append(("edits", slot, edits))


def test_voice_admissions_alone_and_in_a_ragged_group_set_each_slots_record_before_the_pass():
    m, spec, sd, dac, _, enc_dac = TVG.TV._voice_model()
    eng = VoiceEditEngine(spec, sd)
    m.enable_device_logit_edits()
    m._get_engine = lambda *a: eng
    g = torch.Generator().manual_seed(9)
    voice = lambda T: torch.randint(0, 1024, (9, T), generator=g)  # noqa: E731
    kw = dict(slots=10, admit_batch=4, poll_steps=16, max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_new_tokens=12, min_new_tokens=2,
              max_voice_frames=8)
    dec = lambda s: LogitEdits(decay=(s, 1.2))  # noqa: E731
    # grouped: three prompts of ragged lengths in one pass, each slot's record in front of it
    cb = P.ContinuousBatcher(m, **kw, admit_voice_groups=True)
    reqs = [_req(0, decoder_input_ids=voice(3), exponential_decay_length_penalty=(3, 1.2)), _req(1, decoder_input_ids=voice(8)),
            _req(2, decoder_input_ids=voice(1), exponential_decay_length_penalty=(5, 1.2), begin_suppress_tokens=[EOS])]
    assert len(cb.run(reqs)) == 3
    assert eng.events[:3] == [("edits", 0, dec(3)), ("edits", 2, LogitEdits(begin_suppress=(EOS,), decay=(5, 1.2), begin_suppress_on=True)), ("admit_rows", (0, 1, 2))]
    assert eng.group_calls[0] == ([0, 1, 2], [3, 8, 1])
    # alone (the default): one admit_row(voice=) per request, its record immediately in front
    eng.events.clear()
    cb = P.ContinuousBatcher(m, **kw)
    assert len(cb.run([_req(0, decoder_input_ids=voice(4), exponential_decay_length_penalty=(3, 1.2)), _req(1, exponential_decay_length_penalty=(2, 1.2))])) == 2
    assert eng.events[:4] == [("edits", 0, dec(3)), ("admit_row", 0), ("edits", 1, dec(2)), ("admit_row", 1)]


def test_an_engine_left_with_the_node_on_is_switched_off_by_a_batcher_without_the_switch():
    m, spec, sd, dac, _ = TB._model()
    eng = EditSessionEngine(spec, sd)
    eng.logit_edits = LogitEdits(bad=(5,))
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    P.ContinuousBatcher(m, slots=2, max_description_tokens=9, max_prompt_tokens=5, max_new_tokens=14)
    assert eng.calls == [("edits", None, False), ("begin",)]
