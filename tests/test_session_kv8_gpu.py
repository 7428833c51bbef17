"""Continuous sessions on the e4m3 self-attention cache (ptts_session_begin_kv8 / DecoderEngine.begin_session(kv_fp8=True) /
ContinuousBatcher on a model with enable_fp8_kv_cache()), on the GPU.

Bars (none is new): logits within 2e-2 of DecoderOracle(precision="bf16") with ``kv_fp8 = True`` (the SAME quantiser, oracle/fp8_oracle.py) -
the bf16 bar of tests/test_lm_gpu.py::test_e4m3_kv_cache_mode; everything a relocation or a view offset decides is compared bit for bit,
cache bytes and scales included (DecoderEngine.self_kv).
Shapes: bf16, Mini-v1 width, 2 layers, N = 13 description and P = 5 prompt positions (P + 1 = 6 scales per head: no multiple of 16 bytes),
max_ctx 64, ragged masks; kv_fp8 needs max_batch > 8, so the smallest session has 12 slots.
The oracle runs the requests of one max_length as one batch: its rows are independent (the reference's own property, see
tests/test_continuous_batching_gpu.py), so a row of it is the oracle on that request alone."""
import functools
import inspect
import types

import pytest
import torch

import cases as C
import test_continuous_batching_gpu as TB
from helpers import log_parity, make_engine
from oracle import decoder_oracle as DO

pytestmark = pytest.mark.gpu

SPEC = DO.DecoderSpec(num_hidden_layers=2, max_position_embeddings=512)
K, V = SPEC.num_codebooks, SPEC.vocab_size
N_ENC, N_PROMPT = 13, 5
LENGTH_CYCLE = (12, 20, 14, 17, 19)  # per-request max_length: both sides of the 2K - 1 = 17 delay-pattern threshold
TOL = 2e-2
PARITY = "session_kv8_parity.txt"


@functools.lru_cache(maxsize=None)
def _weights():
    return DO.make_decoder_weights(SPEC, seed=29)


def _oracle(kv_fp8):
    orc = DO.DecoderOracle(SPEC, _weights(), precision="bf16")
    orc.kv_fp8 = kv_fp8
    return orc


@functools.lru_cache(maxsize=None)
def _pool(n_req, P=N_PROMPT, plain=False, lengths=None, seed=7):
    """n_req requests and, per request, the quantised-cache oracle's greedy trace (EOS blocked: each runs to its own max_length). ``plain``:
    also, for the requests of the largest max_length (``sub``; every fifth request of the default cycle), the bf16-cache oracle's logits
    teacher-forced on the SAME ids - what the kv8 engine must be farther from."""
    lengths = list(lengths) if lengths is not None else [LENGTH_CYCLE[i % len(LENGTH_CYCLE)] for i in range(n_req)]
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(n_req, N_ENC, SPEC.hidden_size, generator=g)
    prompt = torch.randn(n_req, P, SPEC.hidden_size, generator=g) * 0.5 if P else None
    enc_mask, prompt_mask = C.ragged_masks(n_req, N_ENC, max(P, 1), enc_step=2)
    prompt_mask = prompt_mask if P else None
    enc = enc * enc_mask[..., None]
    refs, plain_refs = [None] * n_req, [None] * n_req
    with torch.no_grad():
        for L in sorted(set(lengths)):
            idx = torch.tensor([i for i in range(n_req) if lengths[i] == L])
            pr, pm = (prompt[idx], prompt_mask[idx]) if P else (None, None)
            tr = DO.sample_loop(_oracle(True), enc[idx], enc_mask[idx], pr, pm, DO.GenParams(max_length=L, min_new_tokens=L - 1), keep_logits=True)
            pl = DO.teacher_forced_logits(_oracle(False), enc[idx], enc_mask[idx], pr, pm, tr.sequences, L) if plain and L == max(lengths) else None
            for j, i in enumerate(idx.tolist()):
                rows = slice(j * K, (j + 1) * K)
                refs[i] = types.SimpleNamespace(sequences=tr.sequences[rows], step_logits=[s[rows] for s in tr.step_logits])
                if pl is not None:
                    plain_refs[i] = types.SimpleNamespace(sequences=tr.sequences[rows], step_logits=[s[rows] for s in pl])
    return types.SimpleNamespace(enc=enc, enc_mask=enc_mask, prompt=prompt, prompt_mask=prompt_mask, lengths=lengths, refs=refs, plain=plain_refs,
                                 reqs=(enc, enc_mask, prompt, prompt_mask), sub=[i for i in range(n_req) if plain_refs[i] is not None])


def _engine(max_batch, kv_fp8=True, P=N_PROMPT, max_ctx=64, max_length=20):
    eng = make_engine(SPEC, _weights(), torch.bfloat16, max_batch=max_batch, max_ctx=max_ctx, max_enc=N_ENC, max_prompt=P + 1, kv_fp8=kv_fp8)
    eng.set_gen_params(max_length=max_length, min_new_tokens=max_length - 1)
    return eng


def _opens_kv8(eng):
    """TB._teacher_forced_session opens its session with the three-argument call: on this engine that call carries kv_fp8=True."""
    assert list(inspect.signature(TB._teacher_forced_session).parameters)[:4] == ["eng", "slots", "n_enc", "n_prompt"]
    eng.begin_session = functools.partial(eng.begin_session, kv_fp8=True)
    return eng


def _recorded(eng):
    """[(logits of the slots that hold a request [n, K, V], their mask [slots])] per iteration of TB._teacher_forced_session, which reads
    logits() once and, behind push_tokens, row_state() once per iteration, in that order: a slot that held a request when the logits were
    read holds more than the BOS column afterwards. Any other call order fails here, by name."""
    seen, inner_logits, inner_state = [], eng.logits, eng.row_state

    def logits():
        assert not seen or len(seen[-1]) == 2, "_recorded: two logits() without a row_state() between them (TB._teacher_forced_session changed?)"
        t = inner_logits()
        seen.append([t.cpu().view(-1, K, V)])
        return t

    def row_state():
        assert seen and len(seen[-1]) == 1, "_recorded: row_state() without a logits() before it (TB._teacher_forced_session changed?)"
        cur, live = inner_state()
        held = torch.tensor(cur) > 1
        seen[-1] = [seen[-1][0][held].clone(), held]
        return cur, live

    eng.logits, eng.row_state = logits, row_state
    return seen


def _admit(eng, slot, pool, i, sample=True, max_length=None):
    eng.admit_row(slot, pool.enc[i], pool.enc_mask[i], None if pool.prompt is None else pool.prompt[i], None if pool.prompt_mask is None else pool.prompt_mask[i],
                  max_length=pool.lengths[i] if max_length is None else max_length, sample=sample)


def _admit_rows(eng, rows, pool, reqs, sample=True, max_lengths=None):
    i = torch.tensor(reqs, dtype=torch.long)
    eng.admit_rows(rows, pool.enc[i], pool.enc_mask[i], None if pool.prompt is None else pool.prompt[i],
                   None if pool.prompt_mask is None else pool.prompt_mask[i], max_lengths=[pool.lengths[r] for r in reqs] if max_lengths is None else max_lengths,
                   sample=sample)


def _self_kv(eng):
    """[(k, v, kscale, vscale)] of every layer, on the host; the scales as their int32 bit patterns, so that comparisons are bit for bit
    wherever the arena was never written (what is there may read as NaN)."""
    torch.cuda.synchronize()
    return [tuple((t if t.dtype == torch.uint8 else t.view(torch.int32)).cpu() for t in eng.self_kv(l)) for l in range(SPEC.num_hidden_layers)]


def _rows(kv, slot, n):
    """Positions [0, n) of one slot: the e4m3 bytes and the scales of every layer, K and V."""
    return [t[slot, :, :n] for layer in kv for t in layer]


def _all_equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [12, 70])
def test_each_request_against_the_oracle_on_that_request_alone_mixed_ages(slots):
    """1.5 x slots requests of max_length 12..20 through 12 slots (8-row LayerNorm nodes) and 70 slots (16-row nodes, exact-length fetch),
    teacher-forced, admitted at mixed ages: every (row, step) logit < 2e-2 against the quantised-cache oracle; the same session on a bf16-cache
    engine differs by > 1e-3 somewhere (the mode is on); the kv8 session is closer to the quantised oracle (worst of all requests) than to the
    plain one (worst of the requests of max_length 20, run again as a session of their own)."""
    pool = _pool(slots * 3 // 2, plain=True)
    total = sum(L - 1 for L in pool.lengths)
    eng = _opens_kv8(_engine(slots))
    rec_q = _recorded(eng)
    err_q, checked = TB._teacher_forced_session(eng, slots, N_ENC, N_PROMPT, pool.reqs, pool.refs, pool.lengths, TOL, K)
    assert checked == total
    sub = torch.tensor(pool.sub)
    err_cross, _ = TB._teacher_forced_session(eng, slots, N_ENC, N_PROMPT, tuple(t[sub] for t in pool.reqs), [pool.plain[i] for i in pool.sub],
                                              [pool.lengths[i] for i in pool.sub], float("inf"), K)
    eng.close()
    plain = _engine(slots, kv_fp8=False)
    rec_p = _recorded(plain)
    TB._teacher_forced_session(plain, slots, N_ENC, N_PROMPT, pool.reqs, pool.refs, pool.lengths, float("inf"), K)
    plain.close()
    assert len(rec_q) > len(rec_p) > 0 and all(len(r) == 2 for r in rec_q + rec_p)
    rec_q = rec_q[: len(rec_p)]  # the first of the two kv8 sessions: the same schedule as the bf16-cache one
    assert all(torch.equal(a[1], b[1]) for a, b in zip(rec_q, rec_p))
    on = max(float((a[0] - b[0]).abs().max()) for a, b in zip(rec_q, rec_p) if a[1].any())
    log_parity(f"[kv8 session, {slots} slots, {len(pool.lengths)} requests] {checked} (row, step) logits: max |d| vs the quantised-cache oracle {err_q:.2e}; "
               f"vs the bf16-cache oracle {err_cross:.2e}; kv8 session vs bf16-cache session {on:.2e}", PARITY)
    assert err_q < TOL, err_q
    assert on > 1e-3, "the kv8 session produced the bf16-cache session's logits: the mode is not on"
    assert err_q < err_cross, (err_q, err_cross)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_prefill_aimed_at_slot_7_writes_slot_7s_rows_and_scales():
    """What the view offsets decide: a request admitted into slot 7 of 12 leaves in slot 7, positions [0, P + 1), the bytes and scales the same
    request leaves in slot 0 of a fresh session, and slot 0 keeps the zeros of session open (a static batch of 12 has dirtied the arena first)."""
    pool = _pool(18, plain=True)
    n = N_PROMPT + 1
    eng = _engine(12)
    eng.prefill(pool.enc[:12], pool.enc_mask[:12], pool.prompt[:12], pool.prompt_mask[:12], sample=False)
    assert any(bool(t.any()) for t in _rows(_self_kv(eng), 0, n))
    eng.begin_session(12, N_ENC, N_PROMPT, kv_fp8=True)
    _admit(eng, 7, pool, 3, sample=False)
    first = _self_kv(eng)
    lg7 = eng.logits().cpu().view(12, K, V)[7].clone()
    eng.begin_session(12, N_ENC, N_PROMPT, kv_fp8=True)
    _admit(eng, 0, pool, 3, sample=False)
    second = _self_kv(eng)
    lg0 = eng.logits().cpu().view(12, K, V)[0].clone()
    eng.close()
    assert first[0][0].dtype == torch.uint8 and first[0][0].shape == (12, SPEC.kv_heads, 64, 64) and first[0][2].shape == (12, SPEC.kv_heads, 64)
    assert _all_equal(_rows(first, 7, n), _rows(second, 0, n))
    assert all(bool(t.any()) for t in _rows(first, 7, n))
    for s in [s for s in range(12) if s != 7]:
        assert not any(bool(t.any()) for t in _rows(first, s, n)), s  # as session open left them
    assert torch.equal(lg7, lg0)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_context_growth_across_fetch_buckets_while_short_requests_cycle():
    """One request of 140 columns (contexts 5 .. 144: the fetch bound moves 64 -> 128 -> the arena end) in slot 0 while short requests cycle
    through the other slots at every age, teacher-forced: every step of every request < 2e-2, the steps either side of contexts 64 and 128
    included (every step is compared)."""
    L = 140
    long = _pool(1, lengths=(L,), seed=11)
    short = _pool(18, plain=True)
    n_short = 66  # one admission every second step: short requests are live up to the long request's column ~150
    idx = [i % 18 for i in range(n_short)]
    cat = lambda a, b: torch.cat([a, b[idx]])
    reqs = (cat(long.enc, short.enc), cat(long.enc_mask, short.enc_mask), cat(long.prompt, short.prompt), cat(long.prompt_mask, short.prompt_mask))
    refs = long.refs + [short.refs[i] for i in idx]
    lengths = [L] + [short.lengths[i] for i in idx]
    eng = _opens_kv8(_engine(12, max_ctx=N_PROMPT + L + 3, max_length=L))
    worst, checked = TB._teacher_forced_session(eng, 12, N_ENC, N_PROMPT, reqs, refs, lengths, TOL, K)
    eng.close()
    log_parity(f"[kv8 session, context growth to {N_PROMPT + L - 1}] {checked} (row, step) logits, max |d| vs the quantised-cache oracle {worst:.2e}", PARITY)
    assert checked == sum(x - 1 for x in lengths) and worst < TOL


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [False, True])
def test_bystanders_are_untouched_by_an_admission(group):
    """Six long requests in slots 0..5 of 12 (+ 4 spare rows), the same schedule with and without an admission after 4 steps - one admit_row into
    slot 6, or one admit_rows of 3 into slots [6, 11, 7]: ids and last logits of the six are identical, and across the admission itself their
    cache bytes and scales over the P + 1 + 4 positions they had written are identical."""
    pool = _pool(18, plain=True)
    stay = [1, 6, 11, 16, 2, 7]
    written = N_PROMPT + 1 + 4
    eng = _engine(16)

    def run(extra):
        eng.begin_session(12, N_ENC, N_PROMPT, kv_fp8=True)
        for s, i in enumerate(stay):
            _admit(eng, s, pool, i, max_length=20)
        eng.decode_steps(4)
        before = _self_kv(eng)
        if extra and group:
            _admit_rows(eng, [6, 11, 7], pool, [0, 3, 5])
        elif extra:
            _admit(eng, 6, pool, 0)
        after = _self_kv(eng)
        eng.decode_steps(3)
        eng.decode_steps(5)
        cur, live = eng.row_state()
        ids = [eng.row_ids(s, cur[s]).cpu() for s in range(len(stay))]
        lg = eng.logits().cpu().view(12, K, V)[: len(stay)].clone()
        return cur, live, ids, lg, before, after

    cur_a, live_a, ids_a, lg_a, _, _ = run(False)
    cur_b, live_b, ids_b, lg_b, before, after = run(True)
    eng.close()
    assert cur_a[:6] == cur_b[:6] == [14] * 6 and all(live_a[:6]) and all(live_b[:6])
    assert cur_a[6] == 1 and cur_b[6] == 10  # the admitted slot holds BOS + its first token + 8 steps
    assert _all_equal(ids_a, ids_b) and torch.equal(lg_a, lg_b)
    for s in range(len(stay)):
        assert _all_equal(_rows(before, s, written), _rows(after, s, written)), s
    assert all(bool(t.any()) for t in _rows(after, 6, N_PROMPT + 1))  # the admission did write its own slot


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [N_PROMPT, 0])
def test_group_admission_equals_the_static_prefill_bit_for_bit(P):
    """12 slots + 4 spare rows. The static prefill of 4 requests, then the same 4 through one admit_rows into slots [9, 2, 11, 5]: each slot's
    step-0 logits and its cache bytes and scales over [0, P + 1) equal its request's row of the static batch bit for bit (P = 0: ONE scale per
    head is moved); 6 teacher-forced steps then stay < 2e-2 against the oracle on each request alone. With P = 5 also: a group of one equals
    admit_row bit for bit."""
    pool = _pool(4, P=P, lengths=(12, 12, 12, 12), seed=9) if P == 0 else _pool(18, plain=True)
    rows, reqs, n = [9, 2, 11, 5], [0, 1, 2, 3], P + 1
    i = torch.tensor(reqs)
    eng = _engine(16, P=P)
    eng.prefill(pool.enc[i], pool.enc_mask[i], None if P == 0 else pool.prompt[i], None if P == 0 else pool.prompt_mask[i], sample=False)
    static_lg = eng.logits().cpu().view(4, K, V).clone()
    static_kv = _self_kv(eng)
    eng.begin_session(12, N_ENC, P, kv_fp8=True)
    _admit_rows(eng, rows, pool, reqs, sample=False)
    kv = _self_kv(eng)
    worst = 0.0
    for col in range(1, 8):
        lg = eng.logits().cpu().view(12, K, V)
        tokens = torch.zeros(12 * K, dtype=torch.long)
        for j, (s, r) in enumerate(zip(rows, reqs)):
            if col == 1:
                assert torch.equal(lg[s], static_lg[j]), (s, r, float((lg[s] - static_lg[j]).abs().max()))
                assert _all_equal(_rows(kv, s, n), _rows(static_kv, j, n)), (s, r)
            err = float((lg[s] - pool.refs[r].step_logits[col - 1]).abs().max())
            worst = max(worst, err)
            assert err < TOL, (s, r, col, err)
            tokens[s * K:(s + 1) * K] = pool.refs[r].sequences[:, col]
        if col == 1:  # the slots that were not listed are as the session opened them
            idle = [s for s in range(12) if s not in rows]
            assert not lg[idle].any() and not any(bool(t.any()) for s in idle for t in _rows(kv, s, n))
        eng.push_tokens(tokens)
        eng.step_forward()
    log_parity(f"[kv8 session, admit_rows of 4, P = {P}] == static prefill (logits, e4m3 rows, scales); 4 x 7 (row, step) logits, max |d| vs the "
               f"quantised-cache oracle {worst:.2e}", PARITY)
    if P:
        got = []
        for batched in (False, True):
            eng.begin_session(12, N_ENC, P, kv_fp8=True)
            for s, r in zip(rows[:3], reqs[:3]):
                if batched:
                    _admit_rows(eng, [s], pool, [r])
                else:
                    _admit(eng, s, pool, r)
            lg0 = eng.logits().cpu().view(12, K, V)[rows[:3]].clone()
            kv0 = [t for s in rows[:3] for t in _rows(_self_kv(eng), s, n)]
            eng.decode_steps(6)
            cur, _ = eng.row_state()
            got.append([lg0] + kv0 + [eng.row_ids(s, cur[s]).cpu() for s in rows[:3]])
        assert _all_equal(*got)
    eng.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_idle_slots_compute_on_defined_values():
    """A fresh engine, session open, nothing admitted, 3 decode steps: every logit is finite; and again after a request ran to its end in one
    slot and was retired."""
    pool = _pool(18, plain=True)
    eng = _engine(12)
    eng.begin_session(12, N_ENC, N_PROMPT, kv_fp8=True)
    eng.decode_steps(3)
    assert bool(torch.isfinite(eng.logits()).all())
    assert eng.row_state() == ([1] * 12, [False] * 12)
    _admit(eng, 4, pool, 0)
    eng.decode_steps(pool.lengths[0])
    cur, live = eng.row_state()
    assert cur[4] == pool.lengths[0] and not any(live)
    eng.retire_row(4)
    eng.decode_steps(3)
    assert bool(torch.isfinite(eng.logits()).all())
    eng.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_values():
    pool = _pool(18, plain=True)
    # the kv8 entry point on a bf16-cache engine: refused, and the engine then opens an ordinary session and runs a request within the bf16 bar
    plain = _engine(12, kv_fp8=False)
    with pytest.raises(ValueError, match="ptts_session_begin"):
        plain.begin_session(12, N_ENC, N_PROMPT, kv_fp8=True)
    one = pool.sub[:1]
    worst, checked = TB._teacher_forced_session(plain, 12, N_ENC, N_PROMPT, tuple(t[one] for t in pool.reqs), [pool.plain[one[0]]], [pool.lengths[one[0]]], TOL, K)
    assert checked == pool.lengths[one[0]] - 1
    plain.close()
    eng = _engine(14)
    with pytest.raises(NotImplementedError, match="kv_fp8"):  # the entry point of ptts.h keeps refusing this engine
        eng.begin_session(12, N_ENC, N_PROMPT)
    eng.set_audio_prefix(torch.randint(0, 1024, (1, K, 3)))
    with pytest.raises(NotImplementedError, match="voice prompt"):
        eng.begin_session(12, N_ENC, N_PROMPT, kv_fp8=True)
    eng.set_audio_prefix(None)
    with pytest.raises(ValueError, match="max_batch"):
        eng.begin_session(15, N_ENC, N_PROMPT, kv_fp8=True)
    # 3 requests into 2 spare rows: PTTS_E_CAPACITY, and no slot, byte or scale has changed
    eng.begin_session(12, N_ENC, N_PROMPT, kv_fp8=True)
    _admit(eng, 1, pool, 0)
    eng.decode_steps(2)
    state, kv, lg = eng.row_state(), _self_kv(eng), eng.logits().cpu()
    with pytest.raises(ValueError, match="spare rows"):
        _admit_rows(eng, [0, 2, 3], pool, [1, 2, 3])
    assert eng.row_state() == state and torch.equal(eng.logits().cpu(), lg)
    assert all(_all_equal(a, b) for a, b in zip(kv, _self_kv(eng)))
    _admit_rows(eng, [0, 2], pool, [1, 2])  # the refusal left the session intact
    eng.decode_steps(3)
    cur, live = eng.row_state()
    assert cur[:3] == [5, 7, 5] and live[:3] == [True, True, True]
    eng.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
E2E_NEW = [30, 12, 22, 17, 26, 10, 19, 24, 14, 28, 11, 21, 16, 30, 13, 25]


def _by_hand(eng, slots, spare, queued, poll_steps):
    """ContinuousBatcher's schedule through the engine API: idle slots ascending take the queue FIFO (groups of up to `spare` through admit_rows,
    a group of one and admit_batch = 1 through admit_row), steps up to the nearest max_length end or `poll_steps`, finished slots retired."""
    eng.begin_session(slots, TB.E2E_N, TB.E2E_P, kv_fp8=True)
    queue, in_slot, cols, out = list(queued), [None] * slots, [0] * slots, {}
    while queue or any(r is not None for r in in_slot):
        idle = [s for s in range(slots) if in_slot[s] is None][: len(queue)]
        pairs = [(s, queue.pop(0)) for s in idle]
        for g0 in range(0, len(pairs), max(spare, 1)):
            grp = pairs[g0:g0 + max(spare, 1)]
            if len(grp) == 1:
                s, r = grp[0]
                eng.admit_row(s, r.enc, r.enc_mask, r.prompt, r.prompt_mask, max_length=r.max_length, sample=True)
            else:
                st = lambda ts: torch.stack(list(ts))
                eng.admit_rows([s for s, _ in grp], st(r.enc for _, r in grp), st(r.enc_mask for _, r in grp), st(r.prompt for _, r in grp),
                               st(r.prompt_mask for _, r in grp), max_lengths=[r.max_length for _, r in grp], sample=True)
            for s, r in grp:
                in_slot[s], cols[s] = r, 2
        busy = [s for s in range(slots) if in_slot[s] is not None]
        n = max(0, min(min(in_slot[s].max_length - cols[s] for s in busy), poll_steps))
        if n:
            eng.decode_steps(n)
            for s in busy:
                cols[s] = min(cols[s] + n, in_slot[s].max_length)
        cur, live = eng.row_state()
        for s in busy:
            if not live[s]:
                out[in_slot[s].ticket] = eng.row_ids(s, cur[s]).cpu()
                eng.retire_row(s)
                in_slot[s] = None
    return out


@pytest.mark.parametrize("admit_batch", [1, 4])
def test_continuous_batcher_reaches_the_kv8_session(admit_batch):
    """Glue: a bf16 tiny model with enable_fp8_kv_cache(), 12 slots, 16 requests of mixed max_new_tokens (EOS blocked). The batcher's engine has
    the e4m3 cache, every waveform has the length its max_new_tokens gives, and every request's ids equal those of the same schedule driven by
    hand through the engine API. With admit_batch = 1 also one streaming run: the chunks of a ticket concatenate to the non-streaming waveform
    (the 1e-5 bar of tests/test_continuous_streaming_gpu.py). The numerics of the session are pinned by the tests above."""
    import parler_tts_amd as P
    from oracle import dac_oracle as DA

    m, spec, sd, dsd = C.tiny_model(seed=TB.E2E_SEEDS[0])
    m = m.to("cuda").to(dtype=torch.bfloat16).enable_fp8_kv_cache()
    g = torch.Generator().manual_seed(TB.E2E_SEEDS[1])
    reqs = [dict(input_ids=torch.randint(3, 128, (TB.E2E_N - i % 3,), generator=g), prompt_input_ids=torch.randint(3, 128, (TB.E2E_P - i % 2,), generator=g),
                 max_new_tokens=n) for i, n in enumerate(E2E_NEW)]
    base = dict(slots=12, max_description_tokens=TB.E2E_N, max_prompt_tokens=TB.E2E_P, poll_steps=5, do_sample=False, max_new_tokens=30, min_new_tokens=30)
    cb = P.ContinuousBatcher(m, admit_batch=admit_batch, **base)
    assert cb.eng.kv_fp8 and cb.spare == (0 if admit_batch == 1 else 4) and cb.eng.cfg.max_batch >= 12 + cb.spare
    tickets = [cb.submit(**r) for r in reqs]
    queued = list(cb._queue)
    ids, inner = {}, cb._decode_group

    def spy(group):
        for r, x in group:
            ids[r.ticket] = x.cpu()
        inner(group)

    cb._decode_group = spy
    out = {t: (w, n) for t, w, n in cb}
    assert sorted(out) == tickets == sorted(ids)
    if admit_batch > 1:
        assert cb.admission_groups[:3] == [4, 4, 4]
    hop = DA.DAC_TINY.hop_length
    for t, new in enumerate(E2E_NEW):
        cols = new + 1
        assert out[t][1] == out[t][0].shape[0] == hop * (cols - 9 if cols >= 17 else cols - 1), (t, out[t][1])
        assert ids[t].shape == (spec.num_codebooks, cols)
    hand = _by_hand(cb.eng, 12, cb.spare, queued, 5)
    for t in tickets:
        assert torch.equal(hand[t], ids[t]), t
    if admit_batch == 1:
        cs = P.ContinuousBatcher(m, stream_chunk_frames=4, stream_first_chunk_frames=2, **base)
        assert cs.eng.kv_fp8
        st = [cs.submit(**r) for r in reqs]
        by, closed = {t: [] for t in st}, set()
        for t, c, last in cs.chunks():
            assert t not in closed
            by[t].append(c)
            if last:
                closed.add(t)
        assert closed == set(st)
        for t in st:
            w = torch.cat(by[t])
            assert w.shape[0] == out[t][1], (t, w.shape, out[t][1])
            assert float((w.float() - out[t][0].float()).abs().max()) <= 1e-5, t
