"""Batched admission on the GPU (ptts_admit_rows / DecoderEngine.admit_rows / ContinuousBatcher(admit_batch=N)): n requests go into n idle
slots of a session with ONE prefill pass on the engine's spare arena rows, and one kernel moves each spare row to its slot.

Contracts (they follow from the design, they are not tuned):
  * admit_rows of requests r_0 .. r_{n-1} runs the launches ptts_prefill runs for that batch of n: the step-0 logits of slot rows[j] are
    torch.equal to row j of the static prefill of the same requests on the same engine;
  * n = 1 is bit-identical to admit_row;
  * a request admitted in a group is held to the engine's contract against the oracle on the request alone: fp32 logits 2e-5, bf16 2e-2
    against DecoderOracle(precision="bf16") (tests/test_lm_gpu.py), free-running fp32 ids bit-equal on requests whose oracle top-2 margin
    is asserted >= cases.MARGIN;
  * the other slots are bit-identical across a batched admission.
Shapes: the pool of tests/test_continuous_batching_gpu.py (cases.batch_case(20), N_ENC, N_PROMPT = 9, 4, per-request lengths 11..20) on
engines of 12 slots + 4 spare rows (MFMA-strip step) and 3 slots + 2 spare rows (max_batch 5, the class of up to 8 utterances). Into the 2
spare rows of the small engine a group has at most 2 requests (3 would be PTTS_E_CAPACITY, which the refusal test pins), so its groups are
[2, 0] - unsorted, slot 0 and the last slot - and [1]."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cases as C
import sampler_cases as SC
import slot_gen_cases as GC
import test_continuous_batching_gpu as TB
from helpers import make_engine
from oracle import decoder_oracle as DO
from parler_tts_amd import _native

pytestmark = pytest.mark.gpu

LENGTHS, N_ENC, N_PROMPT = TB.LENGTHS, TB.N_ENC, TB.N_PROMPT
TOL = {"fp32": 2e-5, "bf16": 2e-2}
DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16}
FORCED = 3  # teacher-forced columns after the admission: the moved self and cross K/V rows are read back


def _admit_rows(eng, rows, pool, reqs, sample=True, max_lengths=None, gens=None):
    _, _, enc, enc_mask, prompt, prompt_mask, _ = pool
    i = torch.tensor(reqs, dtype=torch.long)
    eng.admit_rows(rows, enc[i], enc_mask[i], prompt[i], prompt_mask[i], max_lengths=[LENGTHS[r] for r in reqs] if max_lengths is None else max_lengths,
                   sample=sample, gens=gens)


@functools.lru_cache(maxsize=None)
def _gqa_pool(precision):
    """cases.gqa_case(12): 2 layers, RoPE, 4 heads on 2 self and 1 cross K/V head; the oracle's trace of the first 4 requests alone."""
    spec, sd, enc, enc_mask, prompt, prompt_mask, _ = C.gqa_case(12)
    orc = DO.DecoderOracle(spec, sd, precision=precision)
    refs = []
    with torch.no_grad():
        for i in range(4):
            sl = slice(i, i + 1)
            refs.append(DO.sample_loop(orc, enc[sl], enc_mask[sl], prompt[sl], prompt_mask[sl], DO.GenParams(max_length=FORCED + 3, min_new_tokens=FORCED + 2),
                                       keep_logits=True))
    return spec, sd, enc, enc_mask, prompt, prompt_mask, refs


def _equals_static_prefill(eng, pool, slots, n_enc, n_prompt, rows, reqs, tol, max_lengths):
    """One admit_rows(sample=False) of `reqs` into `rows`: step-0 logits against the static prefill of the same requests (bitwise), then
    FORCED teacher-forced columns against the oracle's logits of each request alone (`max_lengths`: those of the oracle's runs - the delay
    pattern a slot embeds follows its request's own length). Returns the worst logit error."""
    spec, _, enc, enc_mask, prompt, prompt_mask, refs = pool
    K, V = spec.num_codebooks, spec.vocab_size
    i = torch.tensor(reqs)
    eng.prefill(enc[i], enc_mask[i], prompt[i], prompt_mask[i], sample=False)
    static = eng.logits().cpu().view(len(reqs), K, V).clone()
    eng.begin_session(slots, n_enc, n_prompt)
    eng.admit_rows(rows, enc[i], enc_mask[i], prompt[i], prompt_mask[i], max_lengths=max_lengths, sample=False)
    worst = 0.0
    for col in range(1, FORCED + 2):
        lg = eng.logits().cpu().view(slots, K, V)
        tokens = torch.zeros(slots * K, dtype=torch.long)
        for j, (s, r) in enumerate(zip(rows, reqs)):
            if col == 1:
                assert torch.equal(lg[s], static[j]), (s, r, float((lg[s] - static[j]).abs().max()))
            err = float((lg[s] - refs[r].step_logits[col - 1]).abs().max())
            worst = max(worst, err)
            assert err < tol, (s, r, col, err)
            tokens[s * K:(s + 1) * K] = refs[r].sequences[:, col]
        if col == 1:  # the slots that were not listed are as the session opened them
            idle = [s for s in range(slots) if s not in rows]
            assert not lg[idle].any()
        eng.push_tokens(tokens)
        cur, live = eng.row_state()
        assert cur == [col + 1 if s in rows else 1 for s in range(slots)] and live == [s in rows for s in range(slots)]
        eng.step_forward()
    return worst


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("slots,spare,rows", [(12, 4, [11, 0, 5]), (12, 4, [3, 9, 1, 7]), (12, 4, [6]), (3, 2, [2, 0]), (3, 2, [1])])
def test_equals_the_static_prefill_bitwise_and_the_oracle_within_tolerance(slots, spare, rows, prec):
    pool = TB._pool(prec)
    reqs = [7, 9, 2, 13][: len(rows)]  # ragged masks b % 4 = 3, 1, 2, 1
    eng = make_engine(pool[0], pool[1], DTYPE[prec], max_batch=slots + spare)
    eng.set_gen_params(max_length=20, min_new_tokens=19)
    worst = _equals_static_prefill(eng, pool, slots, N_ENC, N_PROMPT, rows, reqs, TOL[prec], [LENGTHS[r] for r in reqs])
    eng.close()
    print(f"[admit_rows {prec} {slots}+{spare} rows={rows}] == static prefill; {FORCED + 1} columns vs oracle max |d| {worst:.2e}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("slots,spare,rows", [(12, 4, [11, 0, 5]), (3, 2, [2, 0])])
def test_two_layers_grouped_query_heads_and_rope(slots, spare, rows, prec):
    """The layer and K/V-head strides of the relocation: self K/V on 2 heads, cross K/V on 1, 21 description and 24 self positions."""
    pool = _gqa_pool(prec)
    spec, sd, enc = pool[0], pool[1], pool[2]
    N, Pw = enc.shape[1], pool[4].shape[1]
    eng = make_engine(spec, sd, DTYPE[prec], max_batch=slots + spare, max_ctx=64, max_enc=N + 3, max_prompt=Pw + 1)
    eng.set_gen_params(max_length=FORCED + 3, min_new_tokens=FORCED + 2)
    worst = _equals_static_prefill(eng, pool, slots, N, Pw, rows, [3, 1, 2][: len(rows)], TOL[prec], [FORCED + 3] * len(rows))
    eng.close()
    print(f"[admit_rows GQA {prec} {slots}+{spare} rows={rows}] max |d| {worst:.2e}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("slots,spare,slot", [(12, 4, 5), (3, 2, 2)])
def test_a_group_of_one_equals_admit_row(slots, spare, slot, prec):
    """Same slot, same request: step-0 logits, the first token and 8 decoded columns are torch.equal."""
    pool = TB._pool(prec)
    spec = pool[0]
    K, V = spec.num_codebooks, spec.vocab_size
    eng = make_engine(spec, pool[1], DTYPE[prec], max_batch=slots + spare)
    eng.set_gen_params(max_length=20, min_new_tokens=19)
    got = []
    for batched in (False, True):
        eng.begin_session(slots, N_ENC, N_PROMPT)
        if batched:
            _admit_rows(eng, [slot], pool, [9])
        else:
            TB._admit(eng, slot, pool, 9)
        lg0 = eng.logits().cpu().view(slots, K, V)[slot].clone()
        first = eng.row_ids(slot, 2).cpu()
        eng.decode_steps(8)
        cur, live = eng.row_state()
        assert cur[slot] == 10 and live[slot]
        got.append((lg0, first, eng.row_ids(slot, 10).cpu(), eng.logits().cpu().view(slots, K, V)[slot].clone()))
    eng.close()
    for a, b in zip(*got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("chunk", [1, 16])
def test_free_run_in_groups_against_the_oracle(chunk):
    """The 20 requests through 12 slots + 4 spare rows, admitted in groups of up to 4 whenever slots free up (idle slots ascending, queue in
    FIFO order): every request's ids equal the oracle's run of that request alone."""
    pool = TB._pool()
    spec, sd, refs = pool[0], pool[1], pool[6]
    for i, ref in enumerate(refs):
        assert ref.min_margin >= C.MARGIN, (i, ref.min_margin)
    slots, spare = 12, 4
    eng = make_engine(spec, sd, torch.float32, max_batch=slots + spare)
    eng.set_gen_params(max_length=20, min_new_tokens=19)
    eng.begin_session(slots, N_ENC, N_PROMPT)
    queue, in_slot, out, log, sizes, polls = list(range(20)), [None] * slots, {}, [], [], 0
    while queue or any(r is not None for r in in_slot):
        idle = [s for s in range(slots) if in_slot[s] is None][: len(queue)]
        for g0 in range(0, len(idle), spare):
            rows = idle[g0:g0 + spare]
            reqs = [queue.pop(0) for _ in rows]
            _admit_rows(eng, rows, pool, reqs)
            sizes.append(len(rows))
            for s, r in zip(rows, reqs):
                in_slot[s] = r
                log.append((r, s))
        eng.decode_steps(chunk)
        cur, live = eng.row_state()
        for s in range(slots):
            if in_slot[s] is not None and not live[s]:
                out[in_slot[s]] = eng.row_ids(s, cur[s]).cpu()
                eng.retire_row(s)
                in_slot[s] = None
        polls += 1
        assert polls < 2000, "the session does not drain"
    eng.close()
    assert sorted(out) == list(range(20)) and [r for r, _ in log] == list(range(20))  # FIFO
    assert sizes[:3] == [4, 4, 4] and max(sizes) <= spare and sum(sizes) == 20
    for i, ref in enumerate(refs):
        assert out[i].shape == ref.sequences.shape, (i, out[i].shape, ref.sequences.shape)
        assert torch.equal(out[i], ref.sequences), i


def test_bystanders_are_untouched_by_a_batched_admission():
    """Slot 1's request twice on 12 + 4 slots, once with a 3-request admit_rows into its neighbours and the last slot after 3 steps: its ids
    and final logits are identical, and no slot outside the list was written."""
    pool = TB._pool()
    spec, sd = pool[0], pool[1]
    K, V = spec.num_codebooks, spec.vocab_size
    slots, spare = 12, 4

    def run(extra):
        eng = make_engine(spec, sd, torch.float32, max_batch=slots + spare)
        eng.set_gen_params(max_length=20, min_new_tokens=19)
        eng.begin_session(slots, N_ENC, N_PROMPT)
        TB._admit(eng, 1, pool, 9, max_length=20)
        eng.decode_steps(3)
        if extra:
            _admit_rows(eng, [2, 11, 0], pool, [0, 1, 2], max_lengths=[20, 20, 20])
        eng.decode_steps(4)
        eng.decode_steps(5)
        cur, live = eng.row_state()
        ids = eng.row_ids(1, cur[1]).cpu()
        lg = eng.logits().cpu().view(slots, K, V).clone()
        eng.close()
        return cur, live, ids, lg

    cur_a, live_a, ids_a, lg_a = run(False)
    cur_b, live_b, ids_b, lg_b = run(True)
    assert cur_a == [1, 14] + [1] * 10 and live_a == [s == 1 for s in range(slots)]
    assert cur_b == [11, 14, 11] + [1] * 8 + [11] and live_b == [s in (0, 1, 2, 11) for s in range(slots)]
    assert torch.equal(ids_a, ids_b) and torch.equal(ids_a, pool[6][9].sequences[:, :14])
    assert torch.equal(lg_a[1], lg_b[1])


# ---- sampler records ------------------------------------------------------------------------------------------------------------------
SESSION = dict(max_length=20, min_new_tokens=19, do_sample=True, temperature=0.9, top_k=50, top_p=1.0, seed=7)
GREEDY = dict(min_new_tokens=19, do_sample=False)
REC_A = dict(min_new_tokens=2, do_sample=True, temperature=0.7, top_k=20, top_p=1.0, seed=0x5EEDA0000001)  # temperature and top-k only:
REC_B = dict(min_new_tokens=19, do_sample=True, temperature=1.3, top_k=40, top_p=1.0, seed=0xB0B0000000000002)  # no top-p mass band enters


def _gen_of(d):
    return SC.Gen(max_length=20, min_new_tokens=d.get("min_new_tokens", 0), do_sample=d.get("do_sample", False), temperature=d.get("temperature", 1.0),
                  top_k=d.get("top_k", 0), top_p=d.get("top_p", 1.0), use_eos_gate=True), d.get("seed", 0)


def test_sampler_records_arrive_in_their_own_slots():
    """One call admits a request without a record, a greedy one and two sampled ones with seeds into slots [7, 2, 10, 0] of a session that
    samples. Every slot's first token - and every column of 5 decode steps - is what the host restatement (tests/sampler_model.py through
    slot_gen_cases.SlotSession) makes of that slot's own logits read back from the engine: the sampled slots on (their seed, column, codebook),
    the record-less slot on (session seed, column, slot * K + codebook); the greedy slot runs to the oracle's ids."""
    pool = TB._pool()
    spec, sd, refs = pool[0], pool[1], pool[6]
    K, V = spec.num_codebooks, spec.vocab_size
    slots, spare = 12, 4
    rows, reqs, recs = [7, 2, 10, 0], [5, 3, 7, 9], [None, GREEDY, REC_A, REC_B]
    assert refs[3].min_margin >= C.MARGIN
    eng = make_engine(spec, sd, torch.float32, max_batch=slots + spare)
    eng.set_gen_params(**SESSION)
    eng.begin_session(slots, N_ENC, N_PROMPT)
    ses_gp, ses_seed = _gen_of(SESSION)
    model = GC.SlotSession(slots, K, V, 24, ses_gp, ses_seed, special_ids=(spec.eos_token_id, spec.pad_token_id, spec.bos_token_id), P=N_PROMPT)
    for b in range(slots):
        model.reset(b, 0, 20, None)

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
            assert np.array_equal(dev[b], f.ids[b * K:(b + 1) * K, :cur[b]]), (what, b)

    _admit_rows(eng, rows, pool, reqs, max_lengths=[20, LENGTHS[3], 20, 20], gens=recs)
    for s, L, rec in zip(rows, [20, LENGTHS[3], 20, 20], recs):
        model.reset(s, 1, L, None if rec is None else _gen_of(rec))
    check(rows, "the admission's own tokens")
    assert sorted(model.own) == [0, 2, 10]
    for step in range(5):
        eng.decode_steps(1)
        check(None, f"step {step}")
    eng.decode_steps(LENGTHS[3])
    cur, live = eng.row_state()
    assert not live[2] and torch.equal(eng.row_ids(2, cur[2]).cpu(), refs[3].sequences)
    eng.close()
    st = model.stats
    assert st["draws"] >= 3 * 6 * K and st["ambiguous"] / st["draws"] <= SC.AMBIGUOUS_CAP, st


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_admit_nothing():
    pool = TB._pool()
    spec, sd, refs = pool[0], pool[1], pool[6]
    slots, spare = 3, 2
    eng = make_engine(spec, sd, torch.float32, max_batch=slots + spare)
    eng.set_gen_params(max_length=20, min_new_tokens=19)
    with pytest.raises(ValueError, match="no continuous session"):
        eng.B, eng.P, eng.session_N = slots, N_PROMPT, N_ENC
        _admit_rows(eng, [0], pool, [0])
    eng.begin_session(slots, N_ENC, N_PROMPT)
    TB._admit(eng, 1, pool, 0)
    state = eng.row_state()
    bad_rec = dict(REC_A, temperature=0.0)
    refused = [(lambda: _admit_rows(eng, [], pool, []), "at least 1"),
               (lambda: _admit_rows(eng, [0, 0], pool, [1, 2]), "listed twice"),
               (lambda: _admit_rows(eng, [0, 1], pool, [1, 2]), "still holds a request"),
               (lambda: _admit_rows(eng, [0, 3], pool, [1, 2]), "outside the session"),
               (lambda: _admit_rows(eng, [-1, 2], pool, [1, 2]), "outside the session"),
               (lambda: _admit_rows(eng, [0, 2], pool, [1, 2], max_lengths=[12, 21]), "exceeds the session's"),
               (lambda: _admit_rows(eng, [0, 2], pool, [1, 2], max_lengths=[1, 12]), "max_length must be"),
               (lambda: _admit_rows(eng, [0, 2], pool, [1, 2], gens=[None, bad_rec]), "temperature must be finite and > 0")]
    for call, msg in refused:
        with pytest.raises(ValueError, match=msg):
            call()
        assert eng.row_state() == state, msg  # nothing was admitted
    # n above the spare rows: 3 requests into the 2 spare rows of this engine, and any group on an engine without spare rows
    tight = make_engine(spec, sd, torch.float32, max_batch=slots)
    tight.set_gen_params(max_length=20, min_new_tokens=19)
    tight.begin_session(slots, N_ENC, N_PROMPT)
    with pytest.raises(ValueError, match="spare rows"):
        _admit_rows(tight, [0, 2], pool, [1, 2])
    assert tight.row_state() == ([1, 1, 1], [False, False, False])
    tight.close()
    eng.retire_row(1)
    with pytest.raises(ValueError, match="spare rows"):
        _admit_rows(eng, [0, 1, 2], pool, [1, 2, 3])
    assert eng.row_state() == ([1, 1, 1], [False, False, False])
    TB._admit(eng, 1, pool, 0)
    eng.set_audio_prefix(torch.randint(0, 1024, (1, spec.num_codebooks, 3)))
    with pytest.raises(NotImplementedError, match="voice prompt"):
        _admit_rows(eng, [0, 2], pool, [1, 2])
    eng.set_audio_prefix(None)
    assert eng.row_state() == state
    # the refusals left the session intact: a valid call works, and the request admitted before them still runs to its oracle ids
    _admit_rows(eng, [2, 0], pool, [1, 2])
    eng.decode_steps(12)
    cur, live = eng.row_state()
    assert cur == [LENGTHS[2], LENGTHS[0], LENGTHS[1]] and live == [False, False, False]
    for s, r in ((1, 0), (2, 1), (0, 2)):
        assert refs[r].min_margin >= C.MARGIN
        assert torch.equal(eng.row_ids(s, cur[s]).cpu(), refs[r].sequences), (s, r)
    eng.close()


def _engine_addresses(eng):
    """The device addresses behind ptts_logits, ptts_ids and ptts_debug_hidden."""
    logits, hidden, rows = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32()
    _native.check(eng.lib.ptts_logits(eng._h, ctypes.byref(logits)), "ptts_logits")
    _native.check(eng.lib.ptts_debug_hidden(eng._h, ctypes.byref(hidden), ctypes.byref(rows)), "ptts_debug_hidden")
    return logits.value, eng.ids_buffer()[0], hidden.value


def test_the_engine_does_not_move():
    """An admission runs its prefill on a view of the engine, and no call - accepted or refused - leaves the engine itself aimed anywhere else:
    the addresses behind ptts_logits, ptts_ids and ptts_debug_hidden are the same after session begin, admit_row, admit_rows of 2, refused
    group and single admissions, retire_row and decode_steps, and the live slots end on the ids of the same sequence without the refused calls.
    The capacity refusal (3 requests into 2 spare rows) comes right after session begin: the per-entry checks run before it and a 3-slot
    session has three distinct idle slots only then; after the admissions the same group of 3 is refused on its busy slots instead."""
    pool = TB._pool()
    spec, sd = pool[0], pool[1]
    slots, spare = 3, 2

    def run(refusals):
        eng = make_engine(spec, sd, torch.float32, max_batch=slots + spare)
        eng.set_gen_params(max_length=20, min_new_tokens=19)
        where = _engine_addresses(eng)
        assert all(where)

        def call(what, fn, refused=None):
            if refused is None:
                fn()
            elif refusals:
                with pytest.raises(ValueError, match=refused):
                    fn()
            assert _engine_addresses(eng) == where, what

        call("begin_session", lambda: eng.begin_session(slots, N_ENC, N_PROMPT))
        call("admit_rows of 3, refused", lambda: _admit_rows(eng, [0, 1, 2], pool, [1, 2, 3]), refused="spare rows")
        call("admit_row", lambda: TB._admit(eng, 1, pool, 0))
        call("admit_rows of 2", lambda: _admit_rows(eng, [2, 0], pool, [1, 2]))
        call("admit_rows of 3 into busy slots, refused", lambda: _admit_rows(eng, [0, 1, 2], pool, [1, 2, 3]), refused="still holds a request")
        call("admit_row into a busy slot, refused", lambda: TB._admit(eng, 1, pool, 3), refused="still holds a request")
        call("retire_row", lambda: eng.retire_row(1))
        call("decode_steps", lambda: eng.decode_steps(3))
        cur, live = eng.row_state()
        ids = [eng.row_ids(s, cur[s]).cpu() for s in (0, 2)]
        eng.close()
        return cur, live, ids

    cur_a, live_a, ids_a = run(True)
    cur_b, live_b, ids_b = run(False)
    assert cur_a == cur_b == [5, 1, 5] and live_a == live_b == [True, False, True]
    assert all(torch.equal(a, b) for a, b in zip(ids_a, ids_b))


# ---- end to end: ContinuousBatcher(admit_batch=4) on the tiny model ---------------------------------------------------------------------
def test_continuous_batcher_with_group_admissions_end_to_end():
    """The 8 requests of tests/test_continuous_batching_gpu.py's end-to-end case through 5 slots with admit_batch=4 (3 spare rows: the class of
    up to 8 utterances): fp32 waveforms and lengths equal those of admit_batch=1 (same ids) and are within RMS 1e-4 of the oracle pipeline on
    each request alone; in streaming mode the chunks of each ticket concatenate to the non-streaming waveform (the 1e-5 bar of
    tests/test_continuous_streaming_gpu.py); cancel() drops a queued and an admitted request."""
    import parler_tts_amd as P
    from oracle import dac_oracle as DA

    ms, isd = TB.E2E_SEEDS
    m, spec, sd, dsd = C.tiny_model(seed=ms)
    m = m.to("cuda")
    reqs = TB._e2e_requests(isd)
    refs = [TB._e2e_reference(m, spec, sd, dsd, r, "cuda") for r in reqs]
    for i, (tr, _) in enumerate(refs):
        assert tr.min_margin >= C.MARGIN, (i, tr.min_margin)
    base = dict(slots=5, max_description_tokens=TB.E2E_N, max_prompt_tokens=TB.E2E_P, poll_steps=5, do_sample=False, max_new_tokens=30, min_new_tokens=30)
    single = P.ContinuousBatcher(m, **base).run(reqs)
    cb = P.ContinuousBatcher(m, admit_batch=4, **base)
    assert cb.spare == 3 and cb.eng.cfg.max_batch >= 8
    out = cb.run(reqs)
    assert cb.admissions == 8 and cb.admission_groups[:2] == [3, 2] and max(cb.admission_groups) <= 3
    hop = DA.DAC_TINY.hop_length
    for i, ((wav, n), (wav1, n1), (tr, ref)) in enumerate(zip(out, single, refs)):
        cols = TB.E2E_NEW[i] + 1
        assert n == n1 == wav.shape[0] == ref.shape[0] == hop * (cols - 9 if cols >= 17 else cols - 1), (i, n, n1, ref.shape)
        assert torch.equal(wav, wav1), (i, float((wav - wav1).abs().max()))
        err = float((wav.cpu() - ref).pow(2).mean().sqrt())
        assert err <= 1e-4, (i, err)
    # streaming
    cs = P.ContinuousBatcher(m, admit_batch=4, stream_chunk_frames=4, stream_first_chunk_frames=2, **base)
    tickets = [cs.submit(**r) for r in reqs]
    by, closed = {t: [] for t in tickets}, set()
    for t, c, last in cs.chunks():
        assert t not in closed
        by[t].append(c)
        if last:
            closed.add(t)
    assert closed == set(tickets) and cs.admission_groups[:2] == [3, 2]
    for i, t in enumerate(tickets):
        w = torch.cat(by[t])
        assert w.shape[0] == out[i][1], (i, w.shape, out[i][1])
        assert float((w - out[i][0]).abs().max()) <= 1e-5, i
    # cancel: ticket 6 is still queued after the first poll's admissions (5 slots), ticket 1 sits in a slot
    cc = P.ContinuousBatcher(m, admit_batch=4, **base)
    tickets = [cc.submit(**r) for r in reqs]
    it = iter(cc)
    first = next(it)  # one poll at least has run: 5 admitted, 3 queued or just admitted behind the first retirement
    assert cc.cancel(tickets[7]) and not cc.cancel(999)
    in_slot = [r.ticket for r in cc._slot if r is not None]
    victim = next(t for t in in_slot if t != first[0])
    assert cc.cancel(victim)
    rest = [first] + list(it)
    got = {t: (w, n) for t, w, n in rest}
    assert sorted(got) == sorted(set(tickets) - {tickets[7], victim})
    for t, (w, n) in got.items():  # the codec batches differ from the full run's (another schedule): the bar against the oracle pipeline
        assert n == out[t][1] and float((w.cpu() - refs[t][1]).pow(2).mean().sqrt()) <= 1e-4, t
