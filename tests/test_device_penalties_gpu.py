"""GPU: repetition_penalty / no_repeat_ngram_size as a device node (include/ptts_penalty.h) through every layer above the kernel -
``generate()`` with ``model.enable_device_penalties()`` against the host loop with transformers' processors, the step graph's node count,
sessions at the engine level (a penalised request beside a plain one, slot reuse, group and voice admissions, refusals) against the oracle
loop with transformers' processors (tests/penalty_model.py::greedy_reference) on requests whose top-2 margin is asserted, and
``ContinuousBatcher`` end to end with per-request values. The kernel itself: tests/test_history_penalty_kernel_gpu.py."""
import pytest
import torch

import cases as C
import penalty_model as PM
from helpers import make_engine
from oracle import dac_oracle as DA
from oracle import decoder_oracle as DO

pytestmark = pytest.mark.gpu

PEN = (1.4, 2)
NEUTRAL = (1.0, 0)
N_ENC, N_PROMPT, MAXLEN, MIN_NEW = 9, 4, 20, 19
# requests of cases.batch_case(20), scanned on the oracle (tests/penalty_model.py::greedy_reference): top-2 margin >= cases.MARGIN under the record
# they run with here - 13 / 0 / 3 under PEN (1.2e-3 / 8.4e-4 / 3.7e-4), 17 / 2 / 9 / 19 under the neutral record (1.6e-3 / 3.9e-4 / 6.5e-4 / 1.3e-3)
BYSTANDER, PENALISED, NEXT_PLAIN, GROUP, VOICE_REQ = 17, 13, 2, (0, 9), 3
VOICE_T = 5


# ---- generate() on the tiny fp32 model ----------------------------------------------------------------------------------------------------
def _gen_inputs():
    g = torch.Generator().manual_seed(5)
    desc = torch.randint(3, 128, (2, 6), generator=g).cuda()
    prompt_ids = torch.randint(3, 128, (2, 3), generator=g).cuda()
    return dict(input_ids=desc, prompt_input_ids=prompt_ids, do_sample=False, max_new_tokens=36, min_new_tokens=4)


def test_generate_with_the_switch_equals_the_host_loop_with_transformers_processors():
    import parler_tts_amd as P
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    m, *_ = C.tiny_model(seed=6, eos_gain=6.0)
    m = m.to("cuda")
    kw = _gen_inputs()
    plain = m.generate(**kw)
    plain_ids, nodes_before = m._engine.ids().cpu(), m._engine.graph_nodes()
    user = [RepetitionPenaltyLogitsProcessor(penalty=1.4), NoRepeatNGramLogitsProcessor(2), P.ParlerTTSLogitsProcessor(1024, 9, 2, "cuda")]
    host = m.generate(logits_processor=user, **kw)  # the host loop: pinned by tests/test_generate_gpu.py
    m.enable_device_penalties()
    plain2 = m.generate(**kw)
    assert torch.equal(plain2, plain) and torch.equal(m._engine.ids().cpu(), plain_ids)
    assert m._engine.graph_nodes() == nodes_before and m._engine.history_penalty is None  # the switch alone changes nothing (a fresh engine: freshly captured)
    dev = m.generate(repetition_penalty=1.4, no_repeat_ngram_size=2, **kw)
    dev_ids = m._engine.ids().cpu()
    assert m._engine.history_penalty == (pytest.approx(1.4), 2)
    assert m._engine.graph_nodes() == nodes_before + 1  # one node more per step
    assert dev.shape == host.shape and torch.equal(dev, host)
    assert dev.shape != plain.shape or not torch.equal(dev, plain)
    # no generated column closes a 2-gram its row has already seen (checked on the raw ids, BOS column included)
    for row in dev_ids.tolist():
        grams = [tuple(row[j:j + 2]) for j in range(len(row) - 1)]
        live = [g for g in grams if 1024 not in g]  # rows padded after their end repeat the pad id
        assert len(live) == len(set(live)), row
    # a plain call afterwards runs the plain graphs again (cached under their own key: nothing is captured, the node is off)
    plain3 = m.generate(**kw)
    assert torch.equal(plain3, plain) and torch.equal(m._engine.ids().cpu(), plain_ids) and m._engine.history_penalty is None


def test_sampled_call_with_a_voice_prompt_never_repeats_a_token_of_its_row():
    """no_repeat_ngram_size=1 over a seeded sampled call that continues 5 frames: the prompt columns count as history."""
    m, *_ = C.tiny_model(seed=4)
    m = m.to("cuda").enable_device_penalties()
    g = torch.Generator().manual_seed(11)
    desc, prompt_ids = torch.randint(3, 128, (2, 6), generator=g).cuda(), torch.randint(3, 128, (2, 3), generator=g).cuda()
    voice = torch.randint(0, 1024, (2 * 9, VOICE_T), generator=g).cuda()
    kw = dict(input_ids=desc, prompt_input_ids=prompt_ids, decoder_input_ids=voice, do_sample=True, temperature=0.9, top_k=40, max_new_tokens=24,
              min_new_tokens=24, no_repeat_ngram_size=1)
    torch.manual_seed(7)
    a = m.generate(**kw)
    ids = m._engine.ids().cpu()
    torch.manual_seed(7)
    b = m.generate(**kw)
    assert torch.equal(a, b) and torch.equal(ids, m._engine.ids().cpu())
    given = 1 + VOICE_T
    assert ids.shape == (18, given + 24)
    for r, row in enumerate(ids.tolist()):
        for j in range(given, len(row)):
            assert row[j] not in row[:j], (r, j, row)


# ---- sessions at the engine level ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    return C.batch_case(20)


@pytest.fixture(scope="module")
def refs(pool):
    """Oracle loops with transformers' processors, computed once: {(request, record, voice?): (ids, margin)}."""
    spec, sd, enc, em, pr, pm, _ = pool
    out = {}

    def ref(i, rec, prefix=None, max_length=MAXLEN):
        key = (i, rec, prefix is not None)
        if key not in out:
            out[key] = PM.greedy_reference(spec, sd, enc[i:i + 1], em[i:i + 1], pr[i:i + 1], pm[i:i + 1], max_length, MIN_NEW, [rec], prefix=prefix)
            assert out[key][1] >= C.MARGIN, (key, out[key][1])
        return out[key][0]

    return ref


def _voice_codes():
    return torch.randint(0, 1024, (9, VOICE_T), generator=torch.Generator().manual_seed(77))


def _admit(eng, slot, pool, i, pen=None, **kw):
    _, _, enc, enc_mask, prompt, prompt_mask, _ = pool
    if pen is not None:
        eng.set_slot_history_penalty(slot, *pen)
    eng.admit_row(slot, enc[i], enc_mask[i], prompt[i], prompt_mask[i], sample=True, **kw)


def _session(pool, slots, feature, max_batch=None, max_length=MAXLEN):
    spec, sd = pool[0], pool[1]
    eng = make_engine(spec, sd, torch.float32, max_batch=max_batch or slots, max_prompt=16)
    eng.set_gen_params(max_length=max_length, min_new_tokens=MIN_NEW, do_sample=False)
    if feature:
        eng.set_history_penalty()  # on, neutral defaults
    eng.begin_session(slots, N_ENC, N_PROMPT)
    return eng


def _slot_logits(eng, slot):
    K = eng.K
    return eng.logits().view(-1, K, eng.V)[slot].cpu()


def test_a_penalised_request_beside_a_plain_one_then_the_slot_is_reused_without_penalties(pool, refs):
    def run(feature):
        eng = _session(pool, 4, feature)
        _admit(eng, 0, pool, BYSTANDER)
        eng.decode_steps(3)
        _admit(eng, 1, pool, PENALISED, pen=PEN if feature else None)
        eng.decode_steps(9)
        mid = (eng.row_ids(0, 14).cpu(), _slot_logits(eng, 0))
        eng.decode_steps(9)  # the bystander ends 6 steps in, the penalised request with the last one (both by max_length)
        cur, live = eng.row_state()
        assert min(cur[:2]) >= MAXLEN and live[:2] == [False, False]
        return eng, mid, eng.row_ids(0, MAXLEN).cpu(), eng.row_ids(1, MAXLEN).cpu()

    eng_off, mid_off, by_off, pen_off = run(False)
    nodes_off = eng_off.graph_nodes()
    eng_off.close()
    eng, mid_on, by_on, pen_on = run(True)
    assert eng.graph_nodes() == nodes_off + 1
    # the bystander: ids and logits bit-identical to the session opened without the feature, and the oracle's tokens
    assert torch.equal(mid_on[0], mid_off[0]) and torch.equal(mid_on[1].view(torch.int32), mid_off[1].view(torch.int32))
    assert torch.equal(by_on, by_off) and torch.equal(by_on, refs(BYSTANDER, NEUTRAL))
    # the penalised request: the oracle loop with transformers' processors; without the feature, the plain loop
    assert torch.equal(pen_on, refs(PENALISED, PEN)) and torch.equal(pen_off, refs(PENALISED, NEUTRAL)) and not torch.equal(pen_on, pen_off)
    # the next request in the same slot, admitted without penalties after retire_row: its no-penalty tokens (the record was cleared)
    eng.retire_row(1)
    _admit(eng, 1, pool, NEXT_PLAIN)
    eng.decode_steps(MAXLEN - 2)
    assert torch.equal(eng.row_ids(1, MAXLEN).cpu(), refs(NEXT_PLAIN, NEUTRAL))
    # ... and the same request alone through the static path (what generate() runs with the switch on) gives the penalised tokens
    eng.retire_row(0)
    eng.retire_row(1)
    eng.set_history_penalty(*PEN)
    eng.set_gen_params(max_length=MAXLEN, min_new_tokens=MIN_NEW, do_sample=False)
    _, _, enc, em, pr, pm, _ = pool
    i = PENALISED
    assert torch.equal(eng.generate_ids(enc[i:i + 1], em[i:i + 1], pr[i:i + 1], pm[i:i + 1]).cpu(), refs(PENALISED, PEN))
    eng.close()


def test_group_admission_with_one_penalised_request(pool, refs):
    _, _, enc, em, pr, pm, _ = pool
    eng = _session(pool, 2, True, max_batch=4)
    a, b = GROUP
    eng.set_slot_history_penalty(1, *PEN)
    eng.admit_rows([1, 0], enc[[a, b]], em[[a, b]], pr[[a, b]], pm[[a, b]], max_lengths=[MAXLEN, MAXLEN], sample=True)
    eng.decode_steps(MAXLEN - 2)
    assert torch.equal(eng.row_ids(1, MAXLEN).cpu(), refs(a, PEN))
    assert torch.equal(eng.row_ids(0, MAXLEN).cpu(), refs(b, NEUTRAL))
    eng.close()


def test_voice_admission_counts_the_prompt_columns_as_history(pool, refs):
    total = MAXLEN + VOICE_T
    eng = _session(pool, 2, True, max_length=total)
    codes = _voice_codes()
    _admit(eng, 0, pool, BYSTANDER, max_length=MAXLEN)
    _admit(eng, 1, pool, VOICE_REQ, pen=PEN, voice=codes.cuda(), max_length=total)
    eng.decode_steps(MAXLEN - 2)
    want = refs(VOICE_REQ, PEN, prefix=codes, max_length=total)
    assert torch.equal(eng.row_ids(1, total).cpu(), want)
    assert torch.equal(eng.row_ids(0, MAXLEN).cpu(), refs(BYSTANDER, NEUTRAL))
    eng.close()


def test_refusals_are_values_and_change_nothing(pool):
    eng = _session(pool, 2, False)
    with pytest.raises(ValueError, match="without history penalties"):
        eng.set_slot_history_penalty(0, 1.4, 2)  # a session begun with the feature off
    _admit(eng, 0, pool, BYSTANDER)
    with pytest.raises(ValueError, match="running session"):
        eng.set_history_penalty(1.4, 2)  # the setter inside a session that holds a request
    assert eng.history_penalty is None
    eng.close()
    eng = _session(pool, 2, True)
    _admit(eng, 0, pool, BYSTANDER)
    with pytest.raises(ValueError, match="still holds a request"):
        eng.set_slot_history_penalty(0, 1.4, 2)  # a busy slot
    with pytest.raises(ValueError, match="outside the session"):
        eng.set_slot_history_penalty(2, 1.4, 2)
    with pytest.raises(ValueError, match="running session"):
        eng.set_history_penalty(enabled=False)
    from parler_tts_amd import _native as N
    import ctypes

    for bad in ((0.0, 0), (float("nan"), 0), (float("inf"), 0), (-1.0, 0), (1.2, -1)):  # the library's own checks, behind the wrapper's
        hp = N.PttsHistoryPenalty(*bad)
        assert eng.lib.ptts_set_slot_history_penalty(eng._h, 1, ctypes.byref(hp), None) == N.PTTS_E_INVALID
    eng.set_slot_history_penalty(1, default=True)
    eng.decode_steps(MAXLEN - 2)
    spec, sd, enc, em, pr, pm, _ = pool
    i = BYSTANDER
    base = DO.sample_loop(DO.DecoderOracle(spec, sd), enc[i:i + 1], em[i:i + 1], pr[i:i + 1], pm[i:i + 1], DO.GenParams(max_length=MAXLEN, min_new_tokens=MIN_NEW))
    assert torch.equal(eng.row_ids(0, MAXLEN).cpu(), base.sequences)  # none of the refused calls touched the running request
    eng.close()


# ---- ContinuousBatcher end to end ---------------------------------------------------------------------------------------------------------
E2E_SEEDS = (2, 313)  # tests/test_continuous_batching_gpu.py's model and inputs; margins under the records below asserted here
E2E_N, E2E_P = 9, 5
E2E = [(30, None), (12, dict(repetition_penalty=1.4, no_repeat_ngram_size=2)), (22, dict(no_repeat_ngram_size=3)), (17, None),
       (26, dict(repetition_penalty=1.0, no_repeat_ngram_size=0))]
E2E_SESSION = dict(repetition_penalty=1.2)


def _e2e_requests():
    g = torch.Generator().manual_seed(E2E_SEEDS[1])
    reqs = []
    for i, (n, pen) in enumerate(E2E):
        reqs.append(dict(input_ids=torch.randint(3, 128, (E2E_N - i % 3,), generator=g), prompt_input_ids=torch.randint(3, 128, (E2E_P - i % 2,), generator=g),
                         max_new_tokens=n, **(pen or {})))
    return reqs


def _e2e_reference(m, spec, sd, dsd, req, device):
    ids, mask = torch.zeros(1, E2E_N, dtype=torch.long), torch.zeros(1, E2E_N, dtype=torch.long)
    pids, pmask = torch.zeros(1, E2E_P, dtype=torch.long), torch.zeros(1, E2E_P, dtype=torch.long)
    d, p = req["input_ids"], req["prompt_input_ids"]
    ids[0, : d.shape[0]], mask[0, : d.shape[0]] = d, 1
    pids[0, : p.shape[0]], pmask[0, : p.shape[0]] = p, 1
    rec = (req.get("repetition_penalty", E2E_SESSION["repetition_penalty"]), req.get("no_repeat_ngram_size", 0))
    with torch.no_grad():
        enc = m._encode_description_eager(ids, mask).float() if device == "cpu" else m._encode_description(ids.to(device), mask.to(device)).float().cpu()
        prompt = m.embed_prompts(pids.to(device)).float().cpu()
        L = req["max_new_tokens"] + 1
        seq, margin = PM.greedy_reference(spec, sd, enc, mask, prompt, pmask, L, L - 1, [rec])
    c = DO.valid_frames(DO.undelay(seq, spec, L)[0])
    return margin, DA.DacOracle(DA.DAC_TINY, dsd).decode(c[None])[0, 0] if c.shape[1] else torch.zeros(1)


def test_continuous_batcher_end_to_end_with_per_request_penalties():
    import parler_tts_amd as P

    m, spec, sd, dsd = C.tiny_model(seed=E2E_SEEDS[0])
    m = m.to("cuda").enable_device_penalties()
    reqs = _e2e_requests()
    refs = [_e2e_reference(m, spec, sd, dsd, r, "cuda") for r in reqs]
    for i, (margin, _) in enumerate(refs):
        assert margin >= C.MARGIN, (i, margin)
    cb = P.ContinuousBatcher(m, slots=2, max_description_tokens=E2E_N, max_prompt_tokens=E2E_P, poll_steps=5, do_sample=False, max_new_tokens=30,
                             min_new_tokens=30, **E2E_SESSION)
    out = cb.run(reqs)
    hop = DA.DAC_TINY.hop_length
    for i, ((wav, n), (_, ref)) in enumerate(zip(out, refs)):
        cols = E2E[i][0] + 1
        assert n == wav.shape[0] == ref.shape[0] == hop * (cols - 9 if cols >= 17 else cols - 1), (i, n, ref.shape)
        err = float((wav.cpu() - ref).pow(2).mean().sqrt())
        assert err <= 1e-4, (i, err)
    cb.close()
    # without the switch the same constructor refuses, as ever
    m.enable_device_penalties(False)
    with pytest.raises(NotImplementedError, match="host loop"):
        P.ContinuousBatcher(m, slots=2, max_description_tokens=E2E_N, max_prompt_tokens=E2E_P, max_new_tokens=30, **E2E_SESSION)
