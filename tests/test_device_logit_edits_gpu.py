"""GPU: sequence_bias / bad_words_ids / exponential_decay_length_penalty / suppress_tokens / begin_suppress_tokens as a device node
(include/ptts_logit_edit.h) through every layer above the kernel - ``generate()`` with ``model.enable_device_logit_edits()`` against the host
loop with transformers' processors, the step graph's node count, sessions at the engine level (a request with a record beside a plain one,
slot reuse, group and voice admissions, refusals) against the oracle loop under transformers' chain in transformers' order
(tests/logit_edit_model.py::greedy_reference) on requests whose top-2 margin is asserted, and ``ContinuousBatcher`` end to end with per-request
values. The kernel itself: tests/test_logit_edit_kernel_gpu.py."""
import ctypes

import pytest
import torch

import cases as C
import logit_edit_model as LM
from helpers import make_engine
from oracle import dac_oracle as DA
from parler_tts_amd.generation_extras import LogitEdits, logit_edits_of

pytestmark = pytest.mark.gpu

EOS = 1024
N_ENC, N_PROMPT, MAXLEN, MIN_NEW = 9, 4, 24, 2
# all five stages: EOS pushed down, then pulled up by a decay from column given + 6 on; half the codes banned, another quarter in the first column
EDIT = LM.Record(sequence_bias={(EOS,): -1.0, (7,): 3.0}, bad_words_ids=[[EOS], [700]], exponential_decay_length_penalty=(6, 3.0),
                 suppress_tokens=list(range(0, 512)), begin_suppress_tokens=list(range(512, 768)))
PLAIN = LM.Record()
# requests of cases.batch_case(20), scanned on the oracle (greedy_reference, MAXLEN 24, min_new_tokens 2): top-2 margin >= 3e-4 under the record
# they run with here - 9 / 7 under EDIT (1.7e-3 / 2.3e-3), 19 / 5 / 2 under the neutral record (5.0e-4 / 4.4e-4 / 3.9e-4), 3 under EDIT behind a
# voice prompt of 5 frames (3.0e-3), 13 behind one of 3 frames (1.6e-3)
BYSTANDER, EDITED, NEXT_PLAIN, GROUP, VOICE5, VOICE3 = 19, 9, 5, (7, 2), 3, 13


def _edits(rec, max_length=MAXLEN + 8):
    return logit_edits_of(1088, EOS, max_length, **rec._asdict())


def _voice_codes(T):
    return torch.randint(0, 1024, (9, T), generator=torch.Generator().manual_seed(77 if T == 5 else 78))


# ---- generate() on the tiny fp32 model ----------------------------------------------------------------------------------------------------
def _gen_inputs():
    g = torch.Generator().manual_seed(5)
    desc = torch.randint(3, 128, (2, 6), generator=g).cuda()
    prompt_ids = torch.randint(3, 128, (2, 3), generator=g).cuda()
    return dict(input_ids=desc, prompt_input_ids=prompt_ids, do_sample=False, max_new_tokens=36, min_new_tokens=4)


GENERATE = {
    "sequence_bias": dict(sequence_bias={(EOS,): -4.0, (5,): 6.0, (900,): 5.0}),
    "bad_words_ids": dict(bad_words_ids=[[v] for v in range(0, 1024, 2)] + [[EOS]]),
    "suppress_tokens": dict(suppress_tokens=list(range(1, 1024, 2)) + [5000]),
    "begin_suppress_tokens": dict(begin_suppress_tokens=list(range(0, 768))),
    "exponential_decay_length_penalty": dict(exponential_decay_length_penalty=(5, 2.0)),
}


def test_generate_with_the_switch_equals_the_host_loop_for_each_option_and_the_graph_has_one_node_more():
    import parler_tts_amd as P

    m, *_ = C.tiny_model(seed=6, eos_gain=6.0)
    m = m.to("cuda")
    kw = _gen_inputs()
    plain = m.generate(**kw)
    plain_ids, nodes_before = m._engine.ids().cpu(), m._engine.graph_nodes()
    m.enable_device_logit_edits()
    plain2 = m.generate(**kw)
    assert torch.equal(plain2, plain) and torch.equal(m._engine.ids().cpu(), plain_ids)
    assert m._engine.graph_nodes() == nodes_before and m._engine.logit_edits is None  # the switch alone changes nothing (a fresh engine: freshly captured)
    given = 1
    for name, opt in GENERATE.items():
        # the host loop (a caller's processor list, here the default one, keeps a call there): transformers' own chain, pinned by tests/test_generate_gpu.py
        host = m.generate(logits_processor=[P.ParlerTTSLogitsProcessor(EOS, 9, 2, "cuda")], **opt, **kw)
        host_ids = m._engine.ids().cpu()
        assert m._engine.logit_edits is None
        dev = m.generate(**opt, **kw)
        dev_ids = m._engine.ids().cpu()
        assert m._engine.logit_edits == logit_edits_of(1088, EOS, 37, **opt) and m._engine.graph_nodes() == nodes_before + 1, name
        assert torch.equal(dev_ids, host_ids) and dev.shape == host.shape and torch.equal(dev, host), name
        new = dev_ids[:, given:]
        live = new[new < 1024]  # the codes (the vocabulary's tail behind EOS is in no list here)
        if name == "bad_words_ids":
            assert bool((live % 2 == 1).all()) and bool((plain_ids[:, given:] % 2 == 0).any())
        if name == "suppress_tokens":
            assert bool((live % 2 == 0).all()) and bool((plain_ids[:, given:] % 2 == 1).any())
        if name == "begin_suppress_tokens":
            assert bool((dev_ids[:, given] >= 768).all()) and bool((plain_ids[:, given] < 768).any())
        if name == "exponential_decay_length_penalty":
            assert torch.equal(dev_ids[:, : given + 5 + 1], plain_ids[:, : given + 5 + 1])  # nothing changes up to the decay's start
    # a plain call afterwards runs the plain graphs again (cached under their own key: nothing is captured, the node is off)
    plain3 = m.generate(**kw)
    assert torch.equal(plain3, plain) and torch.equal(m._engine.ids().cpu(), plain_ids) and m._engine.logit_edits is None


def test_generate_with_a_voice_prompt_counts_begin_and_decay_from_the_given_columns():
    import parler_tts_amd as P

    m, *_ = C.tiny_model(seed=6, eos_gain=6.0)
    m = m.to("cuda").enable_device_logit_edits()
    kw = _gen_inputs()
    T = 5
    voice = torch.randint(0, 1024, (2 * 9, T), generator=torch.Generator().manual_seed(3)).cuda()
    opt = dict(begin_suppress_tokens=list(range(0, 768)), exponential_decay_length_penalty=(5, 2.0), decoder_input_ids=voice)
    host = m.generate(logits_processor=[P.ParlerTTSLogitsProcessor(EOS, 9, 2, "cuda")], **opt, **kw)
    host_ids = m._engine.ids().cpu()
    dev = m.generate(**opt, **kw)
    dev_ids = m._engine.ids().cpu()
    assert m._engine.logit_edits is not None and torch.equal(dev_ids, host_ids) and torch.equal(dev, host)
    assert bool((dev_ids[:, 1 + T] >= 768).all())


# ---- sessions at the engine level ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    return C.batch_case(20)


@pytest.fixture(scope="module")
def refs(pool):
    """Oracle loops under transformers' chain, computed once: {(request, record, voice frames)}: ids; the margin is asserted."""
    spec, sd, enc, em, pr, pm, _ = pool
    out = {}

    def ref(i, rec, T=0):
        key = (i, rec is EDIT, T)
        if key not in out:
            out[key] = LM.greedy_reference(spec, sd, enc[i:i + 1], em[i:i + 1], pr[i:i + 1], pm[i:i + 1], MAXLEN + T, MIN_NEW, rec,
                                           prefix=_voice_codes(T) if T else None)
            assert out[key][1] >= 3e-4, (key, out[key][1])
        return out[key][0]

    return ref


def _admit(eng, slot, pool, i, rec=None, **kw):
    _, _, enc, enc_mask, prompt, prompt_mask, _ = pool
    if rec is not None:
        eng.set_slot_logit_edits(slot, _edits(rec))
    eng.admit_row(slot, enc[i], enc_mask[i], prompt[i], prompt_mask[i], sample=True, **kw)


def _session(pool, slots, feature, max_batch=None, max_length=MAXLEN, default=None):
    spec, sd = pool[0], pool[1]
    eng = make_engine(spec, sd, torch.float32, max_batch=max_batch or slots, max_prompt=16)
    eng.set_gen_params(max_length=max_length, min_new_tokens=MIN_NEW, do_sample=False)
    if feature:
        eng.set_logit_edits(default)  # on, the neutral record unless the test gives one
    eng.begin_session(slots, N_ENC, N_PROMPT)
    return eng


def _row(eng, slot, ref):
    """The slot's ids up to where its reference ends (a request that ended keeps its columns until retire_row)."""
    return eng.row_ids(slot, ref.shape[1]).cpu()


def _slot_logits(eng, slot):
    return eng.logits().view(-1, eng.K, eng.V)[slot].cpu()


def test_a_request_with_a_record_beside_a_plain_one_then_the_slot_is_reused_on_the_default(pool, refs):
    def run(feature):
        eng = _session(pool, 4, feature)
        _admit(eng, 0, pool, BYSTANDER)
        eng.decode_steps(3)
        _admit(eng, 1, pool, EDITED, rec=EDIT if feature else None)
        eng.decode_steps(9)
        mid = (eng.row_ids(0, 14).cpu(), _slot_logits(eng, 0))
        eng.decode_steps(MAXLEN - 2 - 9)
        cur, live = eng.row_state()
        assert live[:2] == [False, False]
        return eng, mid, eng.row_ids(0, MAXLEN).cpu(), eng.row_ids(1, MAXLEN).cpu()

    eng_off, mid_off, by_off, ed_off = run(False)
    nodes_off = eng_off.graph_nodes()
    eng_off.close()
    eng, mid_on, by_on, ed_on = run(True)
    assert eng.graph_nodes() == nodes_off + 1
    # the bystander: ids and logits bit-identical to the session opened without the feature, and the oracle's tokens
    assert torch.equal(mid_on[0], mid_off[0]) and torch.equal(mid_on[1].view(torch.int32), mid_off[1].view(torch.int32))
    assert torch.equal(by_on, by_off) and torch.equal(by_on, refs(BYSTANDER, PLAIN))
    # the request with the record: the oracle loop under transformers' chain; without the feature, the plain loop
    want = refs(EDITED, EDIT)
    assert want.shape[1] < MAXLEN and torch.equal(ed_on[:, : want.shape[1]], want) and torch.equal(ed_off, refs(EDITED, PLAIN))
    new = want[:, 1:]
    assert bool(((new >= 512) & (new != 700)).all()) and bool((want[:, 1] >= 768).all())  # what the record bans never appears
    # the next request in the same slot, admitted without a record after retire_row: its plain tokens (the default was restored)
    eng.retire_row(1)
    _admit(eng, 1, pool, NEXT_PLAIN)
    eng.decode_steps(MAXLEN - 2)
    assert torch.equal(eng.row_ids(1, MAXLEN).cpu(), refs(NEXT_PLAIN, PLAIN))
    # ... a record set and taken back before the admission (NULL: the session's default) leaves the plain tokens too
    eng.retire_row(1)
    eng.set_slot_logit_edits(1, _edits(EDIT))
    eng.set_slot_logit_edits(1, default=True)
    _admit(eng, 1, pool, NEXT_PLAIN)
    eng.decode_steps(MAXLEN - 2)
    assert torch.equal(eng.row_ids(1, MAXLEN).cpu(), refs(NEXT_PLAIN, PLAIN))
    # ... and the same request alone through the static path (what generate() runs with the switch on) gives the record's tokens
    eng.retire_row(0)
    eng.retire_row(1)
    eng.set_logit_edits(_edits(EDIT))
    eng.set_gen_params(max_length=MAXLEN, min_new_tokens=MIN_NEW, do_sample=False)
    _, _, enc, em, pr, pm, _ = pool
    i = EDITED
    assert torch.equal(eng.generate_ids(enc[i:i + 1], em[i:i + 1], pr[i:i + 1], pm[i:i + 1]).cpu(), want)
    eng.close()


def test_a_session_default_record_serves_the_requests_that_bring_none(pool, refs):
    eng = _session(pool, 2, True, default=_edits(EDIT))
    _admit(eng, 0, pool, EDITED)            # no record of its own: the session's
    _admit(eng, 1, pool, BYSTANDER, rec=PLAIN)  # its own, neutral
    eng.decode_steps(MAXLEN - 2)
    want = refs(EDITED, EDIT)
    assert torch.equal(_row(eng, 0, want), want) and torch.equal(eng.row_ids(1, MAXLEN).cpu(), refs(BYSTANDER, PLAIN))
    eng.close()


def test_group_admission_with_one_record(pool, refs):
    _, _, enc, em, pr, pm, _ = pool
    eng = _session(pool, 2, True, max_batch=4)
    a, b = GROUP
    eng.set_slot_logit_edits(1, _edits(EDIT))
    eng.admit_rows([1, 0], enc[[a, b]], em[[a, b]], pr[[a, b]], pm[[a, b]], max_lengths=[MAXLEN, MAXLEN], sample=True)
    eng.decode_steps(MAXLEN - 2)
    want = refs(a, EDIT)
    assert torch.equal(_row(eng, 1, want), want)
    assert torch.equal(eng.row_ids(0, MAXLEN).cpu(), refs(b, PLAIN))
    eng.close()


def test_voice_admission_counts_begin_and_decay_from_the_slots_own_given_columns(pool, refs):
    total = MAXLEN + 5
    eng = _session(pool, 2, True, max_length=total)
    _admit(eng, 0, pool, BYSTANDER, max_length=MAXLEN)
    _admit(eng, 1, pool, VOICE5, rec=EDIT, voice=_voice_codes(5).cuda(), max_length=total)
    eng.decode_steps(MAXLEN - 2)
    want = refs(VOICE5, EDIT, 5)
    assert torch.equal(_row(eng, 1, want), want) and bool((want[:, 6] >= 768).all()) and want.shape[1] < total
    assert torch.equal(eng.row_ids(0, MAXLEN).cpu(), refs(BYSTANDER, PLAIN))
    eng.close()


def test_ragged_voice_group_every_slot_counts_from_its_own_prompt(pool, refs):
    _, _, enc, em, pr, pm, _ = pool
    eng = _session(pool, 2, True, max_batch=4, max_length=MAXLEN + 5)
    i, j = VOICE5, VOICE3
    eng.set_slot_logit_edits(0, _edits(EDIT))
    eng.set_slot_logit_edits(1, _edits(EDIT))
    eng.admit_rows([0, 1], enc[[i, j]], em[[i, j]], pr[[i, j]], pm[[i, j]], max_lengths=[MAXLEN + 5, MAXLEN + 3], sample=True,
                   voices=[_voice_codes(5).cuda(), _voice_codes(3).cuda()])
    eng.decode_steps(MAXLEN - 2)
    w5, w3 = refs(i, EDIT, 5), refs(j, EDIT, 3)
    assert torch.equal(_row(eng, 0, w5), w5) and torch.equal(_row(eng, 1, w3), w3)
    assert bool((w5[:, 6] >= 768).all()) and bool((w3[:, 4] >= 768).all())
    eng.close()


def test_refusals_are_values_and_change_nothing(pool, refs):
    from parler_tts_amd import _native as N
    from parler_tts_amd.engine import DecoderEngine

    spec, sd = pool[0], pool[1]
    eng = make_engine(spec, sd, torch.float32, max_batch=2, max_prompt=16)
    eng.set_gen_params(max_length=MAXLEN, min_new_tokens=MIN_NEW, do_sample=False)
    eng.set_logit_edits(_edits(EDIT))  # the feature on, and no session
    with pytest.raises(ValueError, match="no continuous session"):
        eng.set_slot_logit_edits(0, _edits(EDIT))
    with pytest.raises(ValueError, match="no continuous session"):
        eng.set_slot_logit_edits(0, default=True)
    eng.close()
    eng = _session(pool, 2, False)
    with pytest.raises(ValueError, match="without logit edits"):
        eng.set_slot_logit_edits(0, _edits(EDIT))  # a session begun with the feature off
    _admit(eng, 0, pool, BYSTANDER)
    with pytest.raises(ValueError, match="running session"):
        eng.set_logit_edits(_edits(EDIT))  # the setter inside a session that holds a request
    assert eng.logit_edits is None
    eng.close()
    eng = _session(pool, 2, True)
    _admit(eng, 0, pool, BYSTANDER)
    with pytest.raises(ValueError, match="still holds a request"):
        eng.set_slot_logit_edits(0, _edits(EDIT))  # a busy slot
    with pytest.raises(ValueError, match="outside the session"):
        eng.set_slot_logit_edits(2, _edits(EDIT))
    with pytest.raises(ValueError, match="running session"):
        eng.set_logit_edits(enabled=False)
    # the library's own checks, behind the wrapper's
    bad = [LogitEdits(bias=((1088, 1.0),)), LogitEdits(bias=((-1, 1.0),)), LogitEdits(bias=((5, float("inf")),)), LogitEdits(bias=((5, float("nan")),)),
           LogitEdits(bad=(1088,)), LogitEdits(bad=(-3,)), LogitEdits(decay=(-1, 1.5)), LogitEdits(decay=(3, 0.0)), LogitEdits(decay=(3, -2.0)),
           LogitEdits(decay=(3, float("inf"))), LogitEdits(decay=(3, float("nan")))]
    for ed in bad:
        rec, keep = DecoderEngine._logit_edits(ed)
        assert eng.lib.ptts_set_slot_logit_edits(eng._h, 1, ctypes.byref(rec), None) == N.PTTS_E_INVALID, ed
    rec, keep = DecoderEngine._logit_edits(LogitEdits(bias=((5, 1.0),)))
    rec.n_bias = -1
    assert eng.lib.ptts_set_slot_logit_edits(eng._h, 1, ctypes.byref(rec), None) == N.PTTS_E_INVALID
    rec.n_bias, rec.bias_values = 1, None
    assert eng.lib.ptts_set_slot_logit_edits(eng._h, 1, ctypes.byref(rec), None) == N.PTTS_E_INVALID
    eng.set_slot_logit_edits(1, default=True)
    _admit(eng, 1, pool, NEXT_PLAIN)  # the refused records left slot 1 on the default
    eng.decode_steps(MAXLEN - 2)
    assert torch.equal(eng.row_ids(0, MAXLEN).cpu(), refs(BYSTANDER, PLAIN))  # none of the refused calls touched the running request
    assert torch.equal(eng.row_ids(1, MAXLEN).cpu(), refs(NEXT_PLAIN, PLAIN))
    eng.close()


# ---- ContinuousBatcher end to end ---------------------------------------------------------------------------------------------------------
def test_continuous_batcher_end_to_end_with_per_request_records():
    """Requests through the scheduler: a suppress list's tokens never appear, a strong decay ends its request a few columns behind its start while
    its neighbours run to their length, and a request without options decodes as it does in a session without the feature."""
    import parler_tts_amd as P

    m, *_ = C.tiny_model(seed=2, eos_gain=6.0)  # (with the plain EOS row the EOS logit is 0.0 and |l| * m moves nothing)
    m = m.to("cuda")
    g = torch.Generator().manual_seed(313)
    base = [dict(input_ids=torch.randint(3, 128, (9 - i % 3,), generator=g), prompt_input_ids=torch.randint(3, 128, (5 - i % 2,), generator=g), max_new_tokens=30)
            for i in range(4)]
    kw = dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=5, do_sample=False, max_new_tokens=30, min_new_tokens=2)
    hop = DA.DAC_TINY.hop_length

    def run(reqs):
        cb = P.ContinuousBatcher(m, **kw)
        seen = {}
        orig = cb.eng.retire_row

        def retire(s):  # the raw ids of a request, read when the scheduler lets its slot go
            cur, _ = cb.eng.row_state()
            seen[cb._slot[s].ticket] = cb.eng.row_ids(s, cur[s]).cpu()
            orig(s)

        cb.eng.retire_row = retire
        out = cb.run(reqs)
        cb.close()
        return out, seen

    plain_out, plain_ids = run(base)
    m.enable_device_logit_edits()
    with pytest.raises(ValueError, match="single-token"):
        P.ContinuousBatcher(m, **kw).submit(**base[0], bad_words_ids=[[3, 4]])
    opts = [dict(suppress_tokens=list(range(0, 1024, 2))), dict(), dict(exponential_decay_length_penalty=(6, 8.0)), dict(begin_suppress_tokens=list(range(0, 900)))]
    out, ids = run([dict(r, **o) for r, o in zip(base, opts)])
    live = lambda t: t[:, 1:][t[:, 1:] < 1024]  # noqa: E731
    assert bool((live(ids[0]) % 2 == 1).all()) and bool((live(plain_ids[0]) % 2 == 0).any())
    assert torch.equal(ids[1], plain_ids[1]) and torch.equal(out[1][0], plain_out[1][0])  # the request without options: as in a session without the node
    assert plain_ids[2].shape[1] == 31 and 1 + 6 + 1 < ids[2].shape[1] <= 1 + 6 + 3 + 9  # the decay: EOS within a few columns of start, then codebook by codebook
    assert torch.equal(ids[2][:, :8], plain_ids[2][:, :8])  # ... and nothing before start
    assert bool((ids[3][:, 1] >= 900).all()) and bool((plain_ids[3][:, 1] < 900).any())
    assert out[2][1] < plain_out[2][1] and out[2][1] % hop == 0
