"""Voice prompts per request in a continuous session on the GPU (ptts_admit_row_voice / DecoderEngine.admit_row(voice=) /
ContinuousBatcher.submit(input_values= | decoder_input_ids=)), judged against the static path of the same engine bit for bit and against the
CPU oracle on every request ALONE (``sample_loop(decoder_input_ids=)``).

Bars (none is new): fp32 logits 2e-5, bf16 2e-2 against the matching oracle (tests/test_lm_gpu.py), kv_fp8 2e-2 against the oracle with the
same quantiser (profiles/session_kv8_parity.txt), codec RMS 1e-4 (tests/test_generate_gpu.py). Free-running ids are compared bit for bit
on requests whose oracle margin is asserted >= cases.MARGIN (tests/session_voice_cases.py: scanned with and without the prefix).
Shapes: DO.TINY (K = 9, pattern threshold 2K - 1 = 17), N = 9, P = 4 unless a test names another spec."""
import ctypes
import dataclasses
import functools

import pytest
import torch

import cases as C
import session_voice_cases as VC
from helpers import log_parity, make_engine
from oracle import dac_oracle as DA
from oracle import decoder_oracle as DO
from parler_tts_amd import _native
from parler_tts_amd.engine import _stream_ptr

pytestmark = pytest.mark.gpu

SPEC = DO.TINY
K, V = SPEC.num_codebooks, SPEC.vocab_size
LOG = "session_voice_parity.txt"


def _admit(eng, slot, req, L, sample=True, gen=None, voice=True):
    enc, enc_mask, prompt, prompt_mask, pre = req
    kw = {} if gen is None else {"gen": gen}
    if voice and pre is not None:
        kw["voice"] = pre
    eng.admit_row(slot, enc, enc_mask, prompt, prompt_mask, max_length=L, sample=sample, **kw)


def _raw_admit_voice(eng, slot, req, codes, T, L, sample=0):
    """ptts_admit_row_voice itself, with whatever `codes` / `T` the caller wants to try; returns the status."""
    enc, enc_mask, prompt, prompt_mask, _ = req
    keep = [enc.cuda().float().contiguous(), enc_mask.cuda().int().contiguous(), prompt.cuda().float().contiguous(), prompt_mask.cuda().int().contiguous()]
    cp = ctypes.c_void_p(codes.data_ptr()) if codes is not None else ctypes.c_void_p()
    rc = eng.lib.ptts_admit_row_voice(eng._h, slot, *[ctypes.c_void_p(t.data_ptr()) for t in keep], cp, T, L, sample, None, _stream_ptr(device=eng.device))
    torch.cuda.synchronize()
    return rc


# ---- bit-equal to the static path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [3, 12])
def test_step0_logits_equal_the_static_prefill_of_the_same_request(slots):
    """T = 7 into slot `slots - 2` of an fp32 session, beside a live slot: the step-0 logits are those of ptts_set_audio_prefix + ptts_prefill
    at batch 1 on the same engine, bit for bit (P + 1 + T = 12 rows either way); T = 0 through the new entry point is ptts_admit_row."""
    sd = VC.weights()
    req = VC.request(741, 7)
    enc, enc_mask, prompt, prompt_mask, pre = req
    L, s = 24, slots - 2
    eng = make_engine(SPEC, sd, torch.float32, max_batch=slots)
    eng.set_gen_params(max_length=L, min_new_tokens=0)
    eng.set_audio_prefix(pre[None])
    eng.prefill(enc[None], enc_mask[None], prompt[None], prompt_mask[None], sample=False)
    static = eng.logits().cpu().clone()
    static_ids = eng.ids().cpu().clone()
    eng.set_gen_params(max_length=30, min_new_tokens=0)
    eng.prefill(enc[None], enc_mask[None], prompt[None], prompt_mask[None], sample=False)
    plain = eng.logits().cpu().clone()
    eng.begin_session(slots, VC.N, VC.P)
    _admit(eng, 0, VC.request(742, 0), 20)
    eng.decode_steps(3)
    _admit(eng, s, req, L, sample=False)
    cur, live = eng.row_state()
    assert cur[s] == 8 and live[s] and eng.slot_voice()[s] == 7
    got = eng.logits().cpu().view(slots, K, V)[s]
    assert torch.equal(got.view(torch.int32), static.view(torch.int32))
    assert torch.equal(eng.row_ids(s, 8).cpu(), static_ids)  # the id columns the static prefill wrote
    eng.retire_row(s)
    assert _raw_admit_voice(eng, s, req, None, 0, 0) == _native.PTTS_OK  # T == 0, codes NULL: ptts_admit_row_gen
    assert eng.slot_voice()[s] == 0 and eng.row_state()[0][s] == 1
    got0 = eng.logits().cpu().view(slots, K, V)[s].clone()
    eng.retire_row(s)
    _admit(eng, s, req, 0, sample=False, voice=False)
    assert torch.equal(got0.view(torch.int32), eng.logits().cpu().view(slots, K, V)[s].view(torch.int32))
    assert torch.equal(got0.view(torch.int32), plain.view(torch.int32))
    eng.close()


# ---- free-running against the oracle on each request alone ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _free_pool():
    sd = VC.weights()
    reqs = [VC.request(seed, T) for T, L, seed in VC.FREE_RUNNING]
    refs = [VC.oracle_run(SPEC, sd, r, L) for r, (T, L, _) in zip(reqs, VC.FREE_RUNNING)]
    bare = [VC.oracle_run(SPEC, sd, r, L, with_prefix=False) for r, (T, L, _) in zip(reqs, VC.FREE_RUNNING)]
    return sd, reqs, refs, bare


@pytest.mark.parametrize("poll", [1, 16])
@pytest.mark.parametrize("slots", [3, 12])
def test_free_running_requests_with_and_without_prompts(slots, poll):
    """12 requests, half of them with T in {1, 8, 9, 11}, their own max_length on both sides of 17 and at T + 2, FIFO through 3 slots (GEMV
    step) and 12 slots (MFMA strips; a second round of the list reuses every slot): raw ids equal sample_loop(...).sequences bit for bit."""
    sd, reqs, refs, bare = _free_pool()
    for i, (a, b) in enumerate(zip(refs, bare)):
        assert min(a.min_margin, b.min_margin) >= C.MARGIN, (i, a.min_margin, b.min_margin)
    n = len(reqs)
    order = list(range(n)) + ([(i + 5) % n for i in range(n)] if slots == 12 else [])  # 12 slots: a second round, so that slots are reused
    eng = make_engine(SPEC, sd, torch.float32, max_batch=slots)
    eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=0)
    eng.begin_session(slots, VC.N, VC.P)
    queue, in_slot, out, history, polls = list(order), [None] * slots, [], [[] for _ in range(slots)], 0
    while queue or any(r is not None for r in in_slot):
        for s in range(slots):
            if in_slot[s] is None and queue:
                in_slot[s] = queue.pop(0)
                _admit(eng, s, reqs[in_slot[s]], VC.FREE_RUNNING[in_slot[s]][1])
                history[s].append(VC.FREE_RUNNING[in_slot[s]][0])
        assert eng.slot_voice() == [0 if r is None else VC.FREE_RUNNING[r][0] for r in in_slot]
        eng.decode_steps(poll)
        cur, live = eng.row_state()
        for s in range(slots):
            if in_slot[s] is not None and not live[s]:
                out.append((in_slot[s], eng.row_ids(s, cur[s]).cpu()))
                eng.retire_row(s)
                in_slot[s] = None
        polls += 1
        assert polls < 2000, "the session does not drain"
    assert eng.slot_voice() == [0] * slots
    eng.close()
    assert sorted(i for i, _ in out) == sorted(order)
    for i, ids in out:
        assert ids.shape == refs[i].sequences.shape, (i, ids.shape, refs[i].sequences.shape)
        assert torch.equal(ids, refs[i].sequences), i
    # a voice request behind a request without one in the same slot, and the reverse: the prefix length does not leak
    follows = {(a > 0, b > 0) for h in history for a, b in zip(h, h[1:])}
    assert (False, True) in follows and (True, False) in follows, history


# ---- teacher-forced ---------------------------------------------------------------------------------------------------------------------------
def _teacher_forced(eng, slots, plan, reqs, refs, tol, n_enc=VC.N, n_prompt=VC.P, session_kw=None, max_steps=None):
    """Manual path. plan: [(slot, admission step, request, max_length)]; every live slot is fed the oracle's own tokens and its logits are compared
    with the oracle's at the slot's own step, right behind its admission and behind every forward. Returns (worst |d|, comparisons)."""
    eng.begin_session(slots, n_enc, n_prompt, **(session_kw or {}))
    in_slot, col, fed = [None] * slots, [0] * slots, [0] * slots
    todo, worst, checked, step = list(plan), 0.0, 0, 0
    while todo or any(i is not None for i in in_slot):
        for p in [p for p in todo if p[1] == step]:
            s, _, i, L = p
            _admit(eng, s, reqs[i], L, sample=False)
            T = 0 if reqs[i][4] is None else reqs[i][4].shape[1]
            in_slot[s], col[s], fed[s] = (i, L), 1 + T, 0
            todo.remove(p)
        lg = eng.logits().cpu().view(slots, K, -1)
        tokens = torch.zeros(slots * K, dtype=torch.long)
        for s, it in enumerate(in_slot):
            if it is None:
                continue
            i, L = it
            err = float((lg[s] - refs[i].step_logits[fed[s]]).abs().max())
            worst, checked = max(worst, err), checked + 1
            assert err < tol, (i, s, col[s], err)
            tokens[s * K:(s + 1) * K] = refs[i].sequences[:, col[s]]
        eng.push_tokens(tokens)
        cur, live = eng.row_state()
        for s, it in enumerate(in_slot):
            if it is None:
                assert cur[s] == 1 and not live[s]
                continue
            i, L = it
            col[s] += 1
            fed[s] += 1
            assert cur[s] == col[s]
            if col[s] == L or (max_steps is not None and fed[s] > max_steps):
                assert live[s] == (col[s] < L)
                eng.retire_row(s)
                in_slot[s] = None
            else:
                assert live[s]
        eng.step_forward()
        step += 1
        assert step < 500
    return worst, checked


@pytest.mark.parametrize("dtype,prec,tol", [(torch.float32, "fp32", 2e-5), (torch.bfloat16, "bf16", 2e-2)])
@pytest.mark.parametrize("slots", [3, 12])
def test_teacher_forced_logits_behind_a_prefix(slots, dtype, prec, tol):
    """embed_kernel<WT, true> behind a prefix, while codebooks 1..K-1 are still fed prompt codes: logits at each slot's own step, with slots of
    T in {0, 1, 8, 11} admitted at different steps and a voice request reusing the slot of a plain one (and the reverse)."""
    sd = VC.weights()
    cases = [(8, 24, 701), (0, 20, 700), (11, 20, 724), (1, 17, 717), (0, 12, 703), (8, 16, 707)]
    reqs = [VC.request(seed, T) for T, L, seed in cases]
    refs = [VC.oracle_run(SPEC, sd, r, L, min_new=L, precision=prec, keep_logits=True) for r, (T, L, _) in zip(reqs, cases)]
    last = slots - 1
    plan = [(0, 0, 0, 24), (1, 2, 1, 20), (last, 3, 2, 20), (0, 20, 4, 12), (1, 24, 5, 16), (last, 14, 3, 17)]
    eng = make_engine(SPEC, sd, dtype, max_batch=slots)
    eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=VC.SESSION_MAX_LENGTH)
    worst, checked = _teacher_forced(eng, slots, plan, reqs, refs, tol)
    eng.close()
    log_parity(f"teacher-forced behind a prefix {prec} slots={slots}: {checked} (slot, step) logits, max |d| {worst:.2e} (bar {tol:.0e})", LOG)
    assert checked == sum(L - 1 - T for T, L, _ in cases)


# ---- min_new_tokens --------------------------------------------------------------------------------------------------------------------------------
def test_min_new_tokens_counts_from_the_given_columns():
    """EOS-favouring weights. Slot 0: T = 4 on the session's min_new_tokens = 3; slot 1: no prompt, its own record (5); slots 2 and 3: the same
    T = 4 request with its own records, 4 and 5 - the oracle ends its first codebook at column 1 + T + 4 under the one and a column later under
    the other, so a count that is off by one in either direction changes one of them. Ids equal the oracle's."""
    sd = VC.weights(eos_gain=6.0)
    L, s0 = VC.MIN_NEW_MAX_LENGTH, VC.MIN_NEW_SEED
    plan = [(VC.request(s0, 4), 3, None), (VC.request(s0 + 1, 0), 5, 5), (VC.request(s0 + 2, 4), 4, 4), (VC.request(s0 + 2, 4), 5, 5)]
    refs = [VC.oracle_run(SPEC, sd, r, L, min_new=mn) for r, mn, _ in plan]
    for (r, mn, _), ref in zip(plan, refs):
        assert min(ref.min_margin, VC.oracle_run(SPEC, sd, r, L, min_new=mn, with_prefix=False).min_margin) >= C.MARGIN
    eos = SPEC.eos_token_id
    first = [int((ref.sequences[0] == eos).nonzero()[0]) for ref in refs]
    assert first[2] == 1 + 4 + 4 and first[3] == first[2] + 1  # the bound of slot 2 / slot 3 is what ends their first codebook
    for (r, mn, _), ref in zip(plan, refs):
        T = 0 if r[4] is None else 4
        assert not bool((ref.sequences[:, 1 + T:1 + T + mn] == eos).any())  # EOS blocked for exactly min_new_tokens new columns
    eng = make_engine(SPEC, sd, torch.float32, max_batch=4, max_ctx=64)
    eng.set_gen_params(max_length=L, min_new_tokens=3)
    eng.begin_session(4, VC.N, VC.P)
    for s, (r, mn, own) in enumerate(plan):
        _admit(eng, s, r, L, gen=None if own is None else dict(min_new_tokens=own))
        eng.decode_steps(2)  # slots of different ages
    eng.decode_steps(L)
    cur, live = eng.row_state()
    assert not any(live)
    for s, ref in enumerate(refs):
        assert cur[s] == ref.sequences.shape[1] and torch.equal(eng.row_ids(s, cur[s]).cpu(), ref.sequences), s
    eng.close()


# ---- bystanders --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [3, 12])
def test_bystanders_are_untouched_by_a_voice_admission(slots):
    sd = VC.weights()
    stay = [VC.request(700, 0), VC.request(701, 8)] + ([VC.request(713, 9), VC.request(711, 0), VC.request(724, 11)] if slots == 12 else [])
    extra = VC.request(741, 7)

    def run(with_extra):
        eng = make_engine(SPEC, sd, torch.float32, max_batch=slots)
        eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=VC.SESSION_MAX_LENGTH)
        eng.begin_session(slots, VC.N, VC.P)
        for s, r in enumerate(stay):
            _admit(eng, s, r, VC.SESSION_MAX_LENGTH)
        eng.decode_steps(4)
        if with_extra:
            _admit(eng, slots - 1, extra, 24)
        eng.decode_steps(3)
        eng.decode_steps(5)
        cur, live = eng.row_state()
        ids = [eng.row_ids(s, cur[s]).cpu() for s in range(len(stay))]
        lg = eng.logits().cpu().view(slots, K, V)[: len(stay)].clone()
        last = cur[slots - 1]
        eng.close()
        return cur[: len(stay)], live[: len(stay)], ids, lg, last

    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1] and a[4] == 1 and b[4] == 1 + 7 + 1 + 8
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))


# ---- row-count classes of the one-slot prefill ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [12, 64])
def test_prefill_row_classes_12_and_64(rows):
    """P + 1 + T = 12 (fused LN nodes) and 64 (strips), fp32: step-0 plus four step logits of the voice slot, beside two live slots."""
    sd = VC.weights()
    T = rows - VC.P - 1
    L = T + K + 6
    reqs = [VC.request(750, T), VC.request(700, 0), VC.request(701, 8)]
    refs = [VC.oracle_run(SPEC, sd, r, Lr, min_new=Lr, keep_logits=True) for r, Lr in zip(reqs, (L, 20, 24))]
    eng = make_engine(SPEC, sd, torch.float32, max_batch=3, max_ctx=128, max_prompt=max(rows, 16))
    eng.set_gen_params(max_length=max(L, 24), min_new_tokens=max(L, 24))
    worst, checked = _teacher_forced(eng, 3, [(0, 0, 1, 20), (1, 1, 2, 24), (2, 3, 0, L)], reqs, refs, 2e-5, max_steps=6)
    eng.close()
    log_parity(f"one-slot prefill of {rows} rows (T = {T}) fp32: {checked} logits, max |d| {worst:.2e} (bar 2e-05)", LOG)
    assert checked >= 3 * 5


def test_prefill_row_class_265_bf16():
    """P + 1 + T = 265 rows (above 256: LDS-DMA GEMM and MFMA attention), bf16, cases.block_case's 2-layer H = 256 widths with room for 300
    positions, 12 slots (the MFMA-strip step of block_case's batch), beside two live slots: step-0 plus four step logits of every slot < 2e-2
    against the bf16 oracle."""
    spec = dataclasses.replace(C.block_case()[0], max_position_embeddings=512)
    sd = DO.make_decoder_weights(spec, seed=C.BLOCK_SEEDS[0])
    N, P, T = 40, 23, 241
    L = T + K + 6
    reqs = [VC.request(760, T, N, P, spec), VC.request(761, 0, N, P, spec), VC.request(762, 5, N, P, spec)]
    refs = [VC.oracle_run(spec, sd, r, Lr, min_new=Lr, precision="bf16", keep_logits=True) for r, Lr in zip(reqs, (L, 20, 24))]
    eng = make_engine(spec, sd, torch.bfloat16, max_batch=12, max_ctx=320, max_enc=N, max_prompt=P + 1 + T)
    eng.set_gen_params(max_length=L, min_new_tokens=L)
    worst, checked = _teacher_forced(eng, 12, [(0, 0, 1, 20), (1, 1, 2, 24), (7, 3, 0, L)], reqs, refs, 2e-2, n_enc=N, n_prompt=P, max_steps=6)
    eng.close()
    log_parity(f"one-slot prefill of 265 rows (T = {T}) bf16 H=256: {checked} logits, max |d| {worst:.2e} (bar 2e-02)", LOG)
    assert checked >= 3 * 5


# ---- kv8 session ---------------------------------------------------------------------------------------------------------------------------------
def test_kv8_session_voice_admission():
    """12 slots on a kv_fp8 engine, T = 8: logits within 2e-2 of the oracle with the same quantiser; the slot's e4m3 rows and scales of positions
    [0, P + 1 + T) equal the static kv8 prefill of the same request bit for bit; no other slot's bytes move."""
    import test_session_kv8_gpu as T8

    spec, sd = T8.SPEC, T8._weights()
    N, P, T, L, slots, s = T8.N_ENC, T8.N_PROMPT, 8, 24, 12, 5
    reqs = [VC.request(770, T, N, P, spec), VC.request(771, 0, N, P, spec)]
    enc, enc_mask, prompt, prompt_mask, pre = reqs[0]
    with torch.no_grad():
        refs = [DO.sample_loop(T8._oracle(True), r[0][None], r[1][None], r[2][None], r[3][None], DO.GenParams(max_length=Lr, min_new_tokens=Lr),
                               decoder_input_ids=r[4], keep_logits=True) for r, Lr in zip(reqs, (L, 20))]
    def engine():
        e = make_engine(spec, sd, torch.bfloat16, max_batch=slots, max_ctx=64, max_enc=N, max_prompt=P + 1 + T, kv_fp8=True)
        e.set_gen_params(max_length=L, min_new_tokens=L - 1)
        return e

    eng = engine()
    n = P + 1 + T
    eng.set_audio_prefix(pre[None])
    eng.prefill(enc[None], enc_mask[None], prompt[None], prompt_mask[None], sample=False)
    static = T8._rows(T8._self_kv(eng), 0, n)
    eng.begin_session(slots, N, P, kv_fp8=True)
    _admit(eng, 3, reqs[1], 20)
    eng.decode_steps(2)
    before = T8._self_kv(eng)
    _admit(eng, s, reqs[0], L, sample=False)
    after = T8._self_kv(eng)
    assert T8._all_equal(T8._rows(after, s, n), static)
    others = [b for b in range(slots) if b != s]
    assert all(torch.equal(x[others], y[others]) for lb, la in zip(before, after) for x, y in zip(lb, la))
    eng.close()
    eng = engine()
    worst, checked = _teacher_forced(eng, slots, [(3, 0, 1, 20), (s, 2, 0, L)], reqs, refs, T8.TOL, n_enc=N, n_prompt=P, session_kw=dict(kv_fp8=True), max_steps=6)
    eng.close()
    log_parity(f"kv8 session, T = 8 into slot {s} of {slots}: rows and scales of {n} positions == static kv8 prefill; {checked} logits, max |d| {worst:.2e} "
               f"(bar {T8.TOL:.0e})", LOG)
    assert checked >= 10


# ---- refusals through the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    sd = VC.weights()
    slots = 3
    eng = make_engine(SPEC, sd, torch.float32, max_batch=slots, max_prompt=16)
    eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=0)
    eng.begin_session(slots, VC.N, VC.P)
    busy, idle = VC.request(701, 8), VC.request(724, 11)
    _admit(eng, 0, busy, 24)
    eng.decode_steps(2)

    def state():
        cur, live = eng.row_state()
        return cur, live, [eng.row_ids(s, 14).cpu() for s in range(slots)], eng.slot_voice(), eng.logits().cpu().view(torch.int32)

    def same(a, b):
        return a[0] == b[0] and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and a[3] == b[3] and torch.equal(a[4], b[4])

    s0 = state()
    assert s0[3] == [8, 0, 0]
    codes = idle[4].cuda().contiguous()
    big = torch.zeros(K, 12, dtype=torch.long).cuda()
    tries = [
        (lambda: _raw_admit_voice(eng, 1, idle, codes, -1, 24), _native.PTTS_E_INVALID, "T < 0"),
        (lambda: _raw_admit_voice(eng, 1, idle, None, 11, 24), _native.PTTS_E_INVALID, "NULL codes with T > 0"),
        (lambda: _raw_admit_voice(eng, 1, idle, big, 12, 24), _native.PTTS_E_CAPACITY, "P + 1 + T > max_prompt"),
        (lambda: _raw_admit_voice(eng, 1, idle, codes, 11, 12), _native.PTTS_E_INVALID, "T + 2 > max_length"),
        (lambda: _raw_admit_voice(eng, 1, idle, codes, 11, 31), _native.PTTS_E_CAPACITY, "max_length above the session's"),
        (lambda: _raw_admit_voice(eng, 1, idle, codes, 11, 1), _native.PTTS_E_INVALID, "max_length 1"),
        (lambda: _raw_admit_voice(eng, 0, idle, codes, 11, 24), _native.PTTS_E_INVALID, "busy slot"),
        (lambda: _raw_admit_voice(eng, 3, idle, codes, 11, 24), _native.PTTS_E_INVALID, "slot outside the session"),
    ]
    for call, want, what in tries:
        assert call() == want, what
        assert same(s0, state()), what
    eng.set_audio_prefix(idle[4][None])  # a pending static prefix stays refused by the session
    assert _raw_admit_voice(eng, 1, idle, codes, 11, 24) == _native.PTTS_E_UNSUPPORTED
    assert same(s0, state())
    eng.set_audio_prefix(None)
    assert _raw_admit_voice(eng, 1, idle, codes, 11, 13) == _native.PTTS_OK  # T + 2 == max_length: one generated token
    cur, live = eng.row_state()
    assert cur[1] == 12 and live[1] and eng.slot_voice() == [8, 11, 0]
    # no session: refused too
    eng.prefill(busy[0][None], busy[1][None], busy[2][None], busy[3][None], sample=False)
    assert _raw_admit_voice(eng, 1, idle, codes, 11, 24) == _native.PTTS_E_INVALID
    eng.close()


# ---- ContinuousBatcher end to end --------------------------------------------------------------------------------------------------------------------
def test_continuous_batcher_equals_generate_on_each_request_alone():
    """Tiny T5 + decoder + codec: requests with a waveform prompt, with codes and without any, through 2 slots; per request the raw ids are those
    of model.generate() on that request alone and the waveform is within the codec's bar (RMS 1e-4) of it, the prompt's frames included.
    Requests WITH a prompt have max_length >= 2K - 1 here (17 among them): below it the static prefill of generate() writes BOS-shifted prompt
    columns where the reference keeps the prompt as given (no pattern); the session follows the reference there, which
    test_free_running_requests_with_and_without_prompts checks against the oracle."""
    import parler_tts_amd as P

    ms, isd = C.GEN_VOICE_SEEDS
    m, spec, sd, dsd = C.tiny_model(seed=ms)
    m = m.to("cuda")
    desc, prompt_ids, voice, syn, gp = C.gen_voice_inputs(isd)
    base = dict(input_ids=desc.cuda(), prompt_input_ids=prompt_ids.cuda())
    extras = [dict(input_values=voice.cuda()), {}, dict(decoder_input_ids=syn.cuda()), dict(decoder_input_ids=torch.cat([torch.full((9, 1), 1025), syn], 1).cuda()),
              dict(input_values=voice.cuda()), {}]
    news = [20, 12, 20, 10, 12, 20]
    refs = []
    for ex, n in zip(extras, news):
        out = m.generate(**base, **ex, do_sample=False, max_new_tokens=n, min_new_tokens=n, return_dict_in_generate=True)
        refs.append((out.sequences[0, : out["audios_length"][0]].cpu(), m._engine.ids().cpu().clone()))
    seen = []
    cb = P.ContinuousBatcher(m, slots=2, max_description_tokens=8, max_prompt_tokens=5, poll_steps=4, do_sample=False, max_new_tokens=20, min_new_tokens=20,
                             max_voice_frames=6)
    row_ids = cb.eng.row_ids
    cb.eng.row_ids = lambda s, n: (seen.append((cb._slot[s].ticket, row_ids(s, n).cpu())), seen[-1][1].cuda())[1]
    out = cb.run([dict(input_ids=desc[0], prompt_input_ids=prompt_ids[0], max_new_tokens=n, **ex) for ex, n in zip(extras, news)])
    got_ids = dict(seen)
    hop = DA.DAC_TINY.hop_length
    for i, ((wav, n), (ref_wav, ref_ids)) in enumerate(zip(out, refs)):
        assert torch.equal(got_ids[i], ref_ids), i
        assert n == wav.shape[0] == ref_wav.shape[0], (i, n, ref_wav.shape)
        rms = float((wav.cpu() - ref_wav).pow(2).mean().sqrt())
        assert rms <= 1e-4, (i, rms)
    T = [6, 0, 6, 6, 6, 0]
    assert [n for _, n in out] == [hop * ((nn + 1 + t - 9) if nn + 1 + t >= 17 else nn + t) for nn, t in zip(news, T)]
    cb.close()
