"""Per-request sampler parameters and seeds in a continuous session (ptts_admit_row_gen), on the GPU: the engine's tokens judged on the
engine's OWN logits against the host restatement (tests/slot_gen_cases.py::SlotSession over tests/sampler_model.py), bystanders, refusals,
graph reuse, and ContinuousBatcher end to end in both modes. Shapes: the tiny spec of tests/test_continuous_batching_gpu.py, fp32, engines
of 3 slots (GEMV step) and 12 slots (MFMA strips)."""
import ctypes

import numpy as np
import pytest
import torch

import cases as C
import sampler_cases as SC
import slot_gen_cases as GC
from helpers import log_parity, make_engine
from parler_tts_amd import _native as N

pytestmark = pytest.mark.gpu

LOG = "per_request_sampling.txt"
N_ENC, N_PROMPT, MAXLEN = 9, 4, 20
SESSION = dict(max_length=MAXLEN, min_new_tokens=19, do_sample=True, temperature=0.9, top_k=50, top_p=0.95, seed=7)
GREEDY = dict(min_new_tokens=0, do_sample=False)
REC_A = dict(min_new_tokens=2, do_sample=True, temperature=0.7, top_k=20, top_p=0.9, seed=0x5EEDA0000001)
REC_B = dict(min_new_tokens=19, do_sample=True, temperature=1.3, top_k=0, top_p=1.0, seed=0xB0B0000000000002)


def _pool():
    return C.batch_case(20)


def _admit(eng, slot, pool, i, max_length=MAXLEN, gen=None, sample=True):
    _, _, enc, enc_mask, prompt, prompt_mask, _ = pool
    kw = {} if gen is None else {"gen": gen}
    eng.admit_row(slot, enc[i], enc_mask[i], prompt[i], prompt_mask[i], max_length=max_length, sample=sample, **kw)


def _gen_of(d):
    """(sampler_cases.Gen, seed) of a record dict / of the session's parameters."""
    return SC.Gen(max_length=MAXLEN, min_new_tokens=d.get("min_new_tokens", 0), do_sample=d.get("do_sample", False), temperature=d.get("temperature", 1.0),
                  top_k=d.get("top_k", 0), top_p=d.get("top_p", 1.0), use_eos_gate=True), d.get("seed", 0)


@pytest.mark.parametrize("slots", [3, 12])
def test_tokens_follow_each_slots_own_parameters_on_the_engines_own_logits(slots):
    """A greedy request, two sampled requests with different records and a plain one, admitted at different steps (the second sampled record
    into the slot the greedy request has left). After the admission and after every decode step, every live slot's new column is what the
    restatement predicts from eng.logits(), that slot's record and draw_u(seed, t, k) - (7, t, b * K + k) for the plain slot."""
    pool = _pool()
    spec, sd = pool[0], pool[1]
    K, V = spec.num_codebooks, spec.vocab_size
    eng = make_engine(spec, sd, torch.float32, max_batch=slots)
    eng.set_gen_params(**SESSION)
    eng.begin_session(slots, N_ENC, N_PROMPT)
    ses_gp, ses_seed = _gen_of(SESSION)
    model = GC.SlotSession(slots, K, V, MAXLEN + 4, ses_gp, ses_seed, special_ids=(spec.eos_token_id, spec.pad_token_id, spec.bos_token_id), P=N_PROMPT)
    for b in range(slots):
        model.reset(b, 0, MAXLEN, None)
    last, plain = slots - 1, 1
    # step -> [(slot, request, max_length, record)]; slot 0's greedy request ends at 6 columns (after step 3) and is retired before step 6
    plan = {0: [(0, 3, 6, GREEDY), (plain, 5, MAXLEN, None)], 2: [(last, 7, MAXLEN, REC_A)], 6: [(0, 9, MAXLEN, REC_B)]}

    def check(slots_of_launch, what):
        cur, live = eng.row_state()
        lg = eng.logits().cpu().numpy().reshape(slots, K, V)
        cols = model.full.cur_len.copy()
        dev = {b: eng.row_ids(b, cur[b]).cpu().numpy() for b in range(slots)}

        def choose(row, accepted):
            tok = int(dev[row // K][row % K, int(cols[row // K])])
            assert tok in accepted, (what, row, tok, sorted(accepted))
            return tok

        model.step(lg, slots=slots_of_launch, choose=choose)
        f = model.full
        assert cur == [int(c) for c in f.cur_len], (what, cur, f.cur_len)
        assert live == [bool((f.unfinished[b * K:(b + 1) * K] > 0).any()) for b in range(slots)], what
        for b in range(slots):
            assert np.array_equal(dev[b], f.ids[b * K:(b + 1) * K, :cur[b]]), (what, b, np.argwhere(dev[b] != f.ids[b * K:(b + 1) * K, :cur[b]])[:6])

    for step in range(12):
        if step == 6:
            eng.retire_row(0)
            model.reset(0, 0, MAXLEN, None)
        for slot, req, L, rec in plan.get(step, []):
            _admit(eng, slot, pool, req, max_length=L, gen=rec)
            model.reset(slot, 1, L, None if rec is None else _gen_of(rec))
            check([slot], f"slots={slots} admission of slot {slot} at step {step}")  # the admission's own token, from its step-0 logits
        eng.decode_steps(1)
        check(None, f"slots={slots} step {step}")
    eng.close()
    f, st = model.full, model.stats
    assert [int(f.cur_len[b]) for b in (0, plain, last)] == [8, 14, 12] and sorted(model.own) == [0, last]
    share = st["ambiguous"] / st["draws"]
    log_parity(f"engine tokens on the engine's own logits, {slots} slots: greedy + 2 sampled records + 1 plain slot, 12 steps; {st['draws']} draws, "
               f"ambiguous {st['ambiguous']} ({100 * share:.2f} %)", LOG)
    assert st["draws"] >= 25 * K and share <= SC.AMBIGUOUS_CAP, st


@pytest.mark.parametrize("do_sample", [False, True])
@pytest.mark.parametrize("slots", [3, 12])
def test_bystanders_are_untouched_by_an_admission_with_a_record(slots, do_sample):
    """The schedule of tests/test_continuous_batching_gpu.py::test_bystanders_are_untouched_by_an_admission with the extra request admitted
    through ptts_admit_row_gen: ids and last logits of every other slot are identical with and without it."""
    pool = _pool()
    spec, sd = pool[0], pool[1]
    K, V = spec.num_codebooks, spec.vocab_size
    stay = [7, 9] if slots == 3 else [7, 9, 19, 18, 8, 17, 16, 6, 15, 14]

    def run(extra):
        eng = make_engine(spec, sd, torch.float32, max_batch=slots)
        eng.set_gen_params(max_length=20, min_new_tokens=19, do_sample=do_sample, temperature=0.9, top_k=50, top_p=0.95, seed=7)
        eng.begin_session(slots, N_ENC, N_PROMPT)
        for s, i in enumerate(stay):
            _admit(eng, s, pool, i)
        eng.decode_steps(4)
        if extra:
            _admit(eng, slots - 1, pool, 0, max_length=11, gen=REC_A if do_sample else REC_B)
        eng.decode_steps(3)
        eng.decode_steps(5)
        cur, live = eng.row_state()
        ids = [eng.row_ids(s, cur[s]).cpu() for s in range(len(stay))]
        lg = eng.logits().cpu().view(slots, K, V)[: len(stay)].clone()
        extra_cols = cur[slots - 1]
        eng.close()
        return cur[: len(stay)], live[: len(stay)], ids, lg, extra_cols

    cur_a, live_a, ids_a, lg_a, idle_cols = run(False)
    cur_b, live_b, ids_b, lg_b, extra_cols = run(True)
    assert cur_a == cur_b == [14] * len(stay) and all(live_a) and all(live_b)
    assert idle_cols == 1 and extra_cols == 10
    for a, b in zip(ids_a, ids_b):
        assert torch.equal(a, b)
    assert torch.equal(lg_a, lg_b)


def _raw_admit_gen(eng, slot, pool, i, max_length, gp):
    """ptts_admit_row_gen itself (DecoderEngine.admit_row always passes gp->max_length = 0)."""
    _, _, enc, enc_mask, prompt, prompt_mask, _ = pool
    t = [enc[i].to(eng.device, torch.float32).contiguous(), enc_mask[i].to(eng.device, torch.int32).contiguous(),
         prompt[i].to(eng.device, torch.float32).contiguous(), prompt_mask[i].to(eng.device, torch.int32).contiguous()]
    rc = eng.lib.ptts_admit_row_gen(eng._h, slot, *(ctypes.c_void_p(x.data_ptr()) for x in t), max_length, 1, ctypes.byref(gp),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    N.check(rc, "ptts_admit_row_gen")


def test_refusals_are_values():
    pool = _pool()
    spec, sd = pool[0], pool[1]
    eng = make_engine(spec, sd, torch.float32, max_batch=3)
    eng.set_gen_params(max_length=20, min_new_tokens=19)
    with pytest.raises(ValueError, match="no continuous session"):
        eng.B, eng.P, eng.session_N = 3, N_PROMPT, N_ENC
        _admit(eng, 0, pool, 0, gen=REC_A)
    eng.begin_session(3, N_ENC, N_PROMPT)
    _admit(eng, 1, pool, 0, max_length=11, gen=GREEDY)
    bad = [(dict(temperature=0.0), "temperature must be finite and > 0"), (dict(temperature=-1.0), "temperature must be finite and > 0"),
           (dict(temperature=float("inf")), "temperature must be finite and > 0"), (dict(temperature=float("nan")), "temperature must be finite and > 0"),
           (dict(do_sample=False, temperature=0.0), "temperature must be finite and > 0"),
           (dict(top_p=0.0), r"top_p must be in \(0, 1\]"), (dict(top_p=1.5), r"top_p must be in \(0, 1\]"), (dict(top_k=-1), "top_k must be >= 0"),
           (dict(min_new_tokens=-1), "min_new_tokens must be >= 0")]
    for fields, msg in bad:
        with pytest.raises(ValueError, match=msg):
            _admit(eng, 0, pool, 1, gen=dict(REC_A, **fields))
    with pytest.raises(ValueError, match="unknown per-request generation parameters"):
        _admit(eng, 0, pool, 1, gen=dict(REC_A, max_length=12))
    with pytest.raises(ValueError, match="differs from the max_length argument"):
        _raw_admit_gen(eng, 0, pool, 1, 9, N.PttsGenParams(7, 0, 1, 0.7, 20, 0.9, 1, 5))
    with pytest.raises(ValueError, match="still holds a request"):
        _admit(eng, 1, pool, 1, gen=REC_A)
    with pytest.raises(ValueError, match="outside the session"):
        _admit(eng, 3, pool, 1, gen=REC_A)
    with pytest.raises(ValueError, match="exceeds the session's"):
        _admit(eng, 0, pool, 1, max_length=21, gen=REC_A)
    # no refusal touched the session: slot 0 is still idle and takes a request (gp->max_length equal to the argument is accepted), the
    # greedy request in slot 1 runs to its end and equals the same request in a session of its own
    _raw_admit_gen(eng, 0, pool, 1, 9, N.PttsGenParams(9, 19, 0, 1.0, 0, 1.0, 1, 0))
    eng.decode_steps(12)
    cur, live = eng.row_state()
    assert cur == [9, 11, 1] and live == [False, False, False]
    got = eng.row_ids(1, 11).cpu()
    eng.set_gen_params(max_length=20, min_new_tokens=0)  # a plain greedy session with the record's min_new_tokens
    eng.begin_session(3, N_ENC, N_PROMPT)
    _admit(eng, 1, pool, 0, max_length=11)
    eng.decode_steps(12)
    assert torch.equal(eng.row_ids(1, 11).cpu(), got)
    eng.prefill(pool[2][:3], pool[3][:3], pool[4][:3], pool[5][:3])  # a static batch ends the session, as before
    with pytest.raises(ValueError, match="no continuous session"):
        _admit(eng, 0, pool, 1, gen=REC_A)
    eng.close()


@pytest.mark.parametrize("slots", [3, 12])
def test_an_admission_with_a_record_replays_the_cached_step_graph(slots):
    pool = _pool()
    spec, sd = pool[0], pool[1]
    nodes = {}
    for with_record in (False, True):
        eng = make_engine(spec, sd, torch.float32, max_batch=slots)
        eng.set_gen_params(**SESSION)
        eng.begin_session(slots, N_ENC, N_PROMPT)
        _admit(eng, 0, pool, 0)
        eng.decode_steps(2)  # warm: the step graph of this bucket exists
        warm = eng.graph_nodes()
        assert warm > 0
        _admit(eng, 1, pool, 1, gen=REC_A if with_record else None)
        eng.decode_steps(1)
        _admit(eng, 2, pool, 2, gen=GREEDY if with_record else None)
        eng.decode_steps(1)
        assert eng.graph_nodes() == warm
        cur, live = eng.row_state()
        assert cur[:3] == [6, 4, 3] and all(live[:3])
        nodes[with_record] = warm
        eng.close()
    assert nodes[True] == nodes[False]  # the step with per-slot records has the nodes of the step without


# ---- end to end: ContinuousBatcher, both modes -------------------------------------------------------------------------------------------
def _e2e():
    import test_continuous_batching_gpu as TB

    m, spec, sd, dsd = C.tiny_model(seed=TB.E2E_SEEDS[0])
    return m.to("cuda"), TB._e2e_requests(TB.E2E_SEEDS[1])[:6], TB


def _run_with_ids(cb, reqs):
    """run() plus the raw ids of every request as the batcher read them from its slot: {index: ids}, and the slot each request ran in."""
    ids, slot_of, decode, admit = {}, {}, cb._decode_group, cb.eng.admit_row

    def decode_group(group):
        for r, x in group:
            ids[r.ticket] = x.cpu().clone()
        return decode(group)

    def admit_row(row, *a, **k):
        slot_of[len(slot_of)] = row  # FIFO: the i-th admission is ticket i
        return admit(row, *a, **k)

    cb._decode_group, cb.eng.admit_row = decode_group, admit_row
    try:
        out = cb.run(reqs)
    finally:
        cb.eng.admit_row = admit
    return out, ids, slot_of


def test_continuous_batcher_per_request_options_end_to_end_in_both_modes():
    """Six requests through 3 slots of a session that samples: two ask for greedy decoding and get the waveforms of an all-greedy batcher; the
    four sampled ones carry a seed and give the same ids when the six are submitted in reverse order (another slot, another time: every context
    stays inside one 64-position fetch bucket, so the launch shapes - and with them the logits - are those of the first run); streaming
    delivers the same waveforms in chunks."""
    import parler_tts_amd as P

    m, reqs, TB = _e2e()
    base = dict(slots=3, max_description_tokens=TB.E2E_N, max_prompt_tokens=TB.E2E_P, poll_steps=5, max_new_tokens=30, min_new_tokens=30)
    greedy = (1, 4)
    opts = [dict(do_sample=False) if i in greedy else dict(temperature=0.7 + 0.1 * i, top_k=40, seed=100 + i) for i in range(6)]
    mixed = [dict(r, **o) for r, o in zip(reqs, opts)]
    ref = P.ContinuousBatcher(m, do_sample=False, **base).run(reqs)
    sampling = dict(base, do_sample=True, temperature=1.0, top_k=50)
    torch.manual_seed(3)
    out, ids, slot_of = _run_with_ids(P.ContinuousBatcher(m, **sampling), mixed)
    for i in greedy:
        assert out[i][1] == ref[i][1] == out[i][0].shape[0]
        err = float((out[i][0] - ref[i][0]).pow(2).mean().sqrt())
        assert err <= 1e-4, (i, err)  # the e2e bar of tests/test_continuous_batching_gpu.py
    sampled = [i for i in range(6) if i not in greedy]
    assert any(out[i][0].shape != ref[i][0].shape or float((out[i][0] - ref[i][0]).abs().max()) > 1e-3 for i in sampled)  # sampling is on
    # the same six in reverse order under another session seed
    torch.manual_seed(4)
    out_r, ids_r, slot_r = _run_with_ids(P.ContinuousBatcher(m, **sampling), mixed[::-1])
    moved = 0
    for i in range(6):
        j = 5 - i
        moved += slot_of[i] != slot_r[j]
        assert torch.equal(ids[i], ids_r[j]), (i, slot_of[i], slot_r[j], torch.nonzero(ids[i] != ids_r[j])[:4])
        assert out[i][1] == out_r[j][1] and torch.equal(out[i][0], out_r[j][0])
    assert moved >= 3, (slot_of, slot_r)
    # streaming: the concatenated chunks of each request are the non-streaming waveform
    torch.manual_seed(3)
    cb = P.ContinuousBatcher(m, stream_chunk_frames=4, stream_first_chunk_frames=2, **sampling)
    tickets = [cb.submit(**r) for r in mixed]
    by = {t: [] for t in tickets}
    closed = set()
    for t, c, last in cb.chunks():
        assert t not in closed
        by[t].append(c)
        if last:
            closed.add(t)
    assert closed == set(tickets)
    worst = 0.0
    for i, t in enumerate(tickets):
        w = torch.cat(by[t])
        assert w.shape[0] == out[i][1], (i, w.shape, out[i][1])
        worst = max(worst, float((w - out[i][0]).abs().max()))
    log_parity(f"ContinuousBatcher per-request options, 3 slots: greedy requests == all-greedy batcher, seeded requests torch.equal in reverse order "
               f"({moved} of 6 in another slot), streaming vs run() max|d| {worst:.3e}, pieces {[len(by[t]) for t in tickets]}", LOG)
    assert worst <= 1e-5, worst  # the bar of tests/test_continuous_streaming_gpu.py
