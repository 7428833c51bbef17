"""Groups of voice-prompt requests admitted into a continuous session with ONE prefill pass (ptts_admit_rows_voice /
DecoderEngine.admit_rows(voices=) / ContinuousBatcher(admit_voice_groups=True)), judged against the static path of the same engine bit for
bit where the launches are the same, and against the CPU oracle on every request ALONE (``sample_loop(decoder_input_ids=)``).

Bars (none is new): fp32 logits 2e-5, bf16 2e-2 against the matching oracle (tests/test_lm_gpu.py), kv_fp8 2e-2 against the oracle with the
same quantiser (profiles/session_kv8_parity.txt), codec RMS 1e-4 (tests/test_generate_gpu.py). Free-running ids are compared bit for bit on
requests whose oracle margin is asserted >= cases.MARGIN (tests/session_voice_cases.py: scanned with and without the prefix).
Shapes: DO.TINY (K = 9, pattern threshold 2K - 1 = 17), N = 9, P = 4; 12 slots + 4 spare rows (MFMA-strip step) and 3 slots + 2 spare rows
(GEMV step)."""
import ctypes
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
LAYERS = SPEC.num_hidden_layers
LOG = "session_voice_groups_parity.txt"
N, P = VC.N, VC.P


def _stack(reqs):
    return [torch.stack([r[i] for r in reqs]) for i in range(4)]


def _admit_group(eng, rows, reqs, Ls, sample=True, gens=None):
    enc, enc_mask, prompt, prompt_mask = _stack(reqs)
    eng.admit_rows(rows, enc, enc_mask, prompt, prompt_mask, max_lengths=list(Ls), sample=sample, gens=gens, voices=[r[4] for r in reqs])


def _admit_one(eng, slot, req, L, sample=True):
    kw = {} if req[4] is None else {"voice": req[4]}
    eng.admit_row(slot, req[0], req[1], req[2], req[3], max_length=L, sample=sample, **kw)


def _raw(eng, rows, reqs, codes, Ts, Ls, sample=0, n=None):
    """ptts_admit_rows_voice itself with whatever lists the caller wants to try (codes: device tensors or None per entry); returns the status."""
    n = len(rows) if n is None else n
    keep = [t.cuda().contiguous() for t in _stack(reqs)]
    keep = [keep[0].float(), keep[1].int(), keep[2].float(), keep[3].int()]
    cp = (ctypes.c_void_p * len(rows))(*[None if c is None else c.data_ptr() for c in codes])
    i32 = lambda xs: (ctypes.c_int32 * len(xs))(*xs)
    rc = eng.lib.ptts_admit_rows_voice(eng._h, n, i32(rows), *[ctypes.c_void_p(t.data_ptr()) for t in keep], cp, i32(Ts), i32(Ls), sample, None,
                                       _stream_ptr(device=eng.device))
    torch.cuda.synchronize()
    return rc


def _engine(prec, slots, spare, max_prompt=16, max_ctx=128):
    """prec: "fp32", "bf16" or "kv8" (bf16 on the e4m3 self-attention cache)."""
    dtype = torch.float32 if prec == "fp32" else torch.bfloat16
    return make_engine(SPEC, VC.weights(), dtype, max_batch=slots + spare, max_ctx=max_ctx, max_prompt=max_prompt, kv_fp8=prec == "kv8")


def _begin(eng, prec, slots):
    eng.begin_session(slots, N, P, **({"kv_fp8": True} if prec == "kv8" else {}))


def _self_kv(eng):
    """[(k, v, kscale, vscale)] of every layer on the host, floats as int32 bit patterns; kscale / vscale None off the e4m3 cache."""
    torch.cuda.synchronize()
    return [tuple(None if t is None else (t if t.dtype == torch.uint8 else t.view(torch.int32)).cpu() for t in eng.self_kv(l)) for l in range(LAYERS)]


def _slot_rows(kv, slot, lo, hi):
    return [t[slot, :, lo:hi] for layer in kv for t in layer if t is not None]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _paint_self_kv(eng, seed):
    """Every byte of the self K/V arena (and every scale) to a seeded pattern of finite small values in every format the arena is read in
    (bytes 0x38..0x3d: fp32 / bf16 around 1e-4..0.1, e4m3 1..1.6): what an admission must leave alone is then recognisable."""
    g = torch.Generator().manual_seed(seed)
    hip = _native.hip_runtime()
    keep = []
    for l in range(LAYERS):
        k, v, ks, vs = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        rb, nkv, cap = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _native.check(eng.lib.ptts_debug_self_kv(eng._h, l, ctypes.byref(k), ctypes.byref(v), ctypes.byref(ks), ctypes.byref(vs), ctypes.byref(rb),
                                                 ctypes.byref(nkv), ctypes.byref(cap)))
        units = eng.cfg.max_batch * nkv.value * cap.value
        for ptr, nbytes in ((k, units * rb.value), (v, units * rb.value), (ks, units * 4), (vs, units * 4)):
            if ptr.value:
                src = torch.randint(0x38, 0x3E, (nbytes,), generator=g, dtype=torch.uint8).cuda()
                keep.append(src)
                assert hip.hipMemcpyAsync(ptr, ctypes.c_void_p(src.data_ptr()), nbytes, 3, _stream_ptr(device=eng.device)) == 0
    torch.cuda.synchronize()


def _oracle(prec):
    orc = DO.DecoderOracle(SPEC, VC.weights(), precision="fp32" if prec == "fp32" else "bf16")
    if prec == "kv8":
        orc.kv_fp8 = True
    return orc


def _ref(prec, req, L, min_new=0, keep_logits=True):
    with torch.no_grad():
        return DO.sample_loop(_oracle(prec), req[0][None], req[1][None], req[2][None], req[3][None], DO.GenParams(max_length=L, min_new_tokens=min_new),
                              decoder_input_ids=req[4], keep_logits=keep_logits)


TOL = {"fp32": 2e-5, "bf16": 2e-2, "kv8": 2e-2}


# ---- 1: equal lengths are the static prefill of the group -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "kv8"])
def test_equal_lengths_equal_the_static_prefill_of_the_group(prec):
    """T = 7, n = 3 into slots [11, 2, 5] of 12 (+ 4 spare) beside a live slot: logits and id columns are those of ptts_set_audio_prefix +
    ptts_prefill at batch 3 on the same engine bit for bit; on the e4m3 cache so are the bytes and scales of positions [0, P + 1 + T)."""
    reqs = [VC.request(741 + i, 7) for i in range(3)]
    rows, L, slots, n_pos = [11, 2, 5], 24, 12, P + 1 + 7
    eng = _engine(prec, slots, 4)
    eng.set_gen_params(max_length=L, min_new_tokens=0)
    enc, enc_mask, prompt, prompt_mask = _stack(reqs)
    eng.set_audio_prefix(torch.stack([r[4] for r in reqs]))
    eng.prefill(enc, enc_mask, prompt, prompt_mask, sample=False)
    static = eng.logits().cpu().view(3, K, V).clone()
    static_ids = eng.ids().cpu().reshape(3, K, -1).clone()
    static_kv = _self_kv(eng)
    assert static_ids.shape[2] == 8
    _begin(eng, prec, slots)
    _admit_one(eng, 0, VC.request(700, 0), 20)
    eng.decode_steps(3)
    before = _self_kv(eng)
    _admit_group(eng, rows, reqs, [L] * 3, sample=False)
    cur, live = eng.row_state()
    voice = eng.slot_voice()
    got = eng.logits().cpu().view(slots, K, V)
    after = _self_kv(eng)
    for j, s in enumerate(rows):
        assert cur[s] == 8 and live[s] and voice[s] == 7
        assert torch.equal(got[s].view(torch.int32), static[j].view(torch.int32)), (j, s)
        assert torch.equal(eng.row_ids(s, 8).cpu(), static_ids[j]), (j, s)
        assert _same(_slot_rows(after, s, 0, n_pos), _slot_rows(static_kv, j, 0, n_pos)), (j, s)
    others = [b for b in range(slots) if b not in rows]
    assert all(x is None or torch.equal(x[others], y[others]) for lb, la in zip(before, after) for x, y in zip(lb, la))
    assert [voice[s] for s in others] == [0] * len(others)
    eng.close()


# ---- 2: the two degenerate groups are the calls that exist for them -----------------------------------------------------------------------------
def test_a_group_of_one_is_admit_row_voice_and_a_group_without_prompts_is_admit_rows():
    slots = 12
    req = VC.request(724, 11)
    plain = [VC.request(700 + i, 0) for i in range(3)]
    eng = _engine("fp32", slots, 4)
    eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=VC.SESSION_MAX_LENGTH)

    def snapshot(rows, cols):
        lg0 = eng.logits().cpu().view(slots, K, V)[rows].clone().view(torch.int32)
        eng.decode_steps(6)
        cur, live = eng.row_state()
        return lg0, [eng.row_ids(s, cols + 6).cpu() for s in rows], cur, live, eng.slot_voice(), eng.logits().cpu().view(slots, K, V)[rows].clone().view(torch.int32)

    got = []
    for grouped in (False, True):
        _begin(eng, "fp32", slots)
        if grouped:
            _admit_group(eng, [5], [req], [20])
        else:
            _admit_one(eng, 5, req, 20)
        got.append(snapshot([5], 13))
    for a, b in zip(*got):
        assert _same(a, b) if isinstance(a, list) and torch.is_tensor(a[0]) else (torch.equal(a, b) if torch.is_tensor(a) else a == b)
    got = []
    for through_voice_entry in (False, True):
        _begin(eng, "fp32", slots)
        if through_voice_entry:  # every T == 0, no code pointer at all
            assert _raw(eng, [7, 1, 4], plain, [None] * 3, [0] * 3, [20, 17, 12], sample=1) == _native.PTTS_OK
        else:
            enc, enc_mask, prompt, prompt_mask = _stack(plain)
            eng.admit_rows([7, 1, 4], enc, enc_mask, prompt, prompt_mask, max_lengths=[20, 17, 12], sample=True)
        got.append(snapshot([7, 1, 4], 2))
    for a, b in zip(*got):
        assert _same(a, b) if isinstance(a, list) and torch.is_tensor(a[0]) else (torch.equal(a, b) if torch.is_tensor(a) else a == b)
    eng.close()


# ---- 3: a ragged group ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "kv8"])
def test_a_row_of_a_ragged_group_does_not_depend_on_the_others_and_no_padding_reaches_a_slot(prec):
    """T = (11, 8, 1, 0) into slots [9, 1, 4, 0]; then the other three requests replaced and their lengths changed to (0, 8, 11, 5), n and Tmax
    kept: slot 1's logits, its self K/V rows [0, P + 1 + 8) and slot_voice are bit-identical. The arena was painted before each call: every
    destination slot's rows at and beyond P + 1 + T_j (16, 13, 6, 5 positions moved: scale counts that are and are not multiples of four) are
    the paint, and so is every slot that was not listed."""
    slots, rows = 12, [9, 1, 4, 0]
    keepr = VC.request(701, 8)
    groups = [
        ([VC.request(724, 11), keepr, VC.request(717, 1), VC.request(700, 0)], [20, 24, 17, 20]),
        ([VC.request(703, 0), keepr, VC.request(705, 11), VC.request(751, 5)], [12, 24, 13, 30]),
    ]
    seen = []
    for reqs, Ls in groups:
        eng = _engine(prec, slots, 4)
        eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=0)
        _begin(eng, prec, slots)
        _paint_self_kv(eng, seed=5)
        before = _self_kv(eng)
        _admit_group(eng, rows, reqs, Ls, sample=False)
        after = _self_kv(eng)
        Ts = [0 if r[4] is None else r[4].shape[1] for r in reqs]
        cur, _ = eng.row_state()
        voice = eng.slot_voice()
        assert [voice[s] for s in rows] == Ts and [cur[s] for s in rows] == [t + 1 for t in Ts]
        cap = before[0][0].shape[2]
        for s, t in zip(rows, Ts):
            assert _same(_slot_rows(after, s, P + 1 + t, cap), _slot_rows(before, s, P + 1 + t, cap)), (s, t)  # no padded position arrived
            assert not _same(_slot_rows(after, s, 0, P + 1 + t), _slot_rows(before, s, 0, P + 1 + t)), (s, t)
        idle = [b for b in range(slots) if b not in rows]
        assert all(x is None or torch.equal(x[idle], y[idle]) for lb, la in zip(before, after) for x, y in zip(lb, la))
        lg = eng.logits().cpu().view(slots, K, V).clone()
        ref = _ref(prec, keepr, 24)
        err = float((lg[1] - ref.step_logits[0]).abs().max())
        assert err < TOL[prec], err
        seen.append((lg[1].view(torch.int32), _slot_rows(after, 1, 0, P + 1 + 8), voice[1], eng.row_ids(1, 9).cpu()))
        eng.close()
    a, b = seen
    assert torch.equal(a[0], b[0]) and _same(a[1], b[1]) and a[2] == b[2] == 8 and torch.equal(a[3], b[3])


# ---- 4: free-running against the oracle on each request alone -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _free_pool():
    sd = VC.weights()
    reqs = [VC.request(seed, T) for T, L, seed in VC.FREE_RUNNING]
    refs = [VC.oracle_run(SPEC, sd, r, L) for r, (T, L, _) in zip(reqs, VC.FREE_RUNNING)]
    bare = [VC.oracle_run(SPEC, sd, r, L, with_prefix=False) for r, (T, L, _) in zip(reqs, VC.FREE_RUNNING)]
    return reqs, refs, bare


@pytest.mark.parametrize("poll", [1, 16])
@pytest.mark.parametrize("slots,spare", [(12, 4), (3, 2)])
def test_free_running_in_groups_against_the_oracle(slots, spare, poll):
    """The 12 VC.FREE_RUNNING requests FIFO in groups of up to `spare` - requests with and without prompts in the same group - through 12
    slots (two rounds: every slot is reused) and 3 slots: raw ids equal sample_loop on each request alone; slot_voice returns to zeros."""
    reqs, refs, bare = _free_pool()
    for i, (a, b) in enumerate(zip(refs, bare)):
        assert min(a.min_margin, b.min_margin) >= C.MARGIN, (i, a.min_margin, b.min_margin)
    n = len(reqs)
    order = list(range(n)) + ([(i + 5) % n for i in range(n)] if slots == 12 else [])
    eng = _engine("fp32", slots, spare)
    eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=0)
    _begin(eng, "fp32", slots)
    queue, in_slot, out, sizes, admitted, polls = list(order), [None] * slots, [], [], [], 0
    while queue or any(r is not None for r in in_slot):
        idle = [s for s in range(slots) if in_slot[s] is None][: len(queue)]
        for g0 in range(0, len(idle), spare):
            rows = idle[g0:g0 + spare]
            took = [queue.pop(0) for _ in rows]
            _admit_group(eng, rows, [reqs[i] for i in took], [VC.FREE_RUNNING[i][1] for i in took])
            sizes.append(len(rows))
            admitted += took
            for s, i in zip(rows, took):
                in_slot[s] = i
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
    assert admitted == order and sizes[0] == spare and max(sizes) <= spare
    assert sorted(i for i, _ in out) == sorted(order)
    for i, ids in out:
        assert ids.shape == refs[i].sequences.shape, (i, ids.shape, refs[i].sequences.shape)
        assert torch.equal(ids, refs[i].sequences), i


# ---- 5 / 6: teacher-forced ------------------------------------------------------------------------------------------------------------------------
def _teacher_forced(eng, prec, slots, plan, reqs, refs, tol, max_steps=None):
    """Manual path. plan: [(admission step, [(slot, request, max_length), ...])], each entry ONE admit_rows(voices=); every live slot is fed the
    oracle's own tokens and its logits are compared with the oracle's at the slot's own step. Returns (worst |d|, comparisons)."""
    _begin(eng, prec, slots)
    in_slot, col, fed = [None] * slots, [0] * slots, [0] * slots
    todo, worst, checked, step = list(plan), 0.0, 0, 0
    while todo or any(i is not None for i in in_slot):
        for p in [p for p in todo if p[0] == step]:
            _admit_group(eng, [s for s, _, _ in p[1]], [reqs[i] for _, i, _ in p[1]], [L for _, _, L in p[1]], sample=False)
            for s, i, L in p[1]:
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
                continue
            i, L = it
            col[s] += 1
            fed[s] += 1
            assert cur[s] == col[s]
            if col[s] == L or (max_steps is not None and fed[s] > max_steps):
                eng.retire_row(s)
                in_slot[s] = None
        eng.step_forward()
        step += 1
        assert step < 500
    return worst, checked


@pytest.mark.parametrize("prec", ["bf16", "kv8"])
def test_teacher_forced_logits_behind_group_admissions_through_context_growth(prec):
    """12 slots + 4 spare. A ragged group of four (one request of 70 columns: its context P + columns crosses the 64-position fetch bucket
    while it is live) and two later groups that reuse slots, teacher-forced: the logits of every (slot, step) against the oracle of the same
    precision (kv8: with the same quantiser) on each request alone."""
    slots = 12
    cases = [(8, 70, 701), (0, 20, 700), (11, 20, 724), (1, 17, 717), (0, 12, 703), (8, 16, 707), (9, 30, 713), (11, 13, 705)]
    reqs = [VC.request(seed, T) for T, L, seed in cases]
    refs = [_ref(prec, r, L, min_new=L) for r, (T, L, _) in zip(reqs, cases)]
    plan = [(0, [(11, 0, 70), (3, 1, 20), (0, 2, 20), (7, 3, 17)]), (2, [(5, 4, 12), (1, 5, 16)]), (22, [(3, 6, 30), (0, 7, 13), (9, 4, 12)])]
    eng = _engine(prec, slots, 4)
    eng.set_gen_params(max_length=70, min_new_tokens=70)
    worst, checked = _teacher_forced(eng, prec, slots, plan, reqs, refs, TOL[prec])
    eng.close()
    log_parity(f"teacher-forced behind group voice admissions {prec} 12+4: {checked} (slot, step) logits, max |d| {worst:.2e} (bar {TOL[prec]:.0e})", LOG)
    assert checked == sum(L - 1 - cases[i][0] for _, g in plan for _, i, L in g)


def test_a_group_above_256_prefill_rows():
    """n = 12 requests with T from {20, 13, 5, 0} (one at 20): 12 x (P + 1 + 20) = 300 prefill rows, the row class above 256. Step-0 and three
    teacher-forced steps of every slot, fp32 within 2e-5 of the oracle on each request alone."""
    Ts = [13, 5, 0, 20, 13, 0, 5, 5, 13, 0, 13, 5]
    L, slots = 40, 12
    reqs = [VC.request(780 + i, T) for i, T in enumerate(Ts)]
    refs = [_ref("fp32", r, L, min_new=L) for r in reqs]
    eng = _engine("fp32", slots, 12, max_prompt=25)
    eng.set_gen_params(max_length=L, min_new_tokens=L)
    rows = [5, 0, 11, 2, 7, 1, 9, 3, 10, 4, 8, 6]
    worst, checked = _teacher_forced(eng, "fp32", slots, [(0, [(s, i, L) for i, s in enumerate(rows)])], reqs, refs, 2e-5, max_steps=3)
    eng.close()
    log_parity(f"group voice admission of 12 x 25 = 300 prefill rows fp32: {checked} logits, max |d| {worst:.2e} (bar 2e-05)", LOG)
    assert checked == 12 * 4


# ---- 7: two chunks of the slot list -----------------------------------------------------------------------------------------------------------
def test_66_requests_take_two_launches_of_the_slot_list_and_equal_the_static_prefill():
    n, T, L = 66, 2, 20
    reqs = [VC.request(800 + i, T) for i in range(n)]
    eng = _engine("fp32", n, n)
    eng.set_gen_params(max_length=L, min_new_tokens=0)
    enc, enc_mask, prompt, prompt_mask = _stack(reqs)
    eng.set_audio_prefix(torch.stack([r[4] for r in reqs]))
    eng.prefill(enc, enc_mask, prompt, prompt_mask, sample=False)
    static = eng.logits().cpu().view(n, K, V).clone()
    static_ids = eng.ids().cpu().reshape(n, K, -1).clone()
    _begin(eng, "fp32", n)
    rows = list(range(n - 1, -1, -1))
    _admit_group(eng, rows, reqs, [L] * n, sample=False)
    got = eng.logits().cpu().view(n, K, V)
    cur, live = eng.row_state()
    assert cur == [T + 1] * n and all(live) and eng.slot_voice() == [T] * n
    for j, s in enumerate(rows):
        assert torch.equal(got[s].view(torch.int32), static[j].view(torch.int32)), (j, s)
        assert torch.equal(eng.row_ids(s, T + 1).cpu(), static_ids[j]), (j, s)
    eng.close()


# ---- 8: bystanders ----------------------------------------------------------------------------------------------------------------------------
def test_bystanders_are_untouched_by_a_group_voice_admission():
    slots = 12
    stay = [VC.request(700, 0), VC.request(701, 8), VC.request(713, 9), VC.request(711, 0), VC.request(724, 11)]
    extra = [VC.request(741, 7), VC.request(742, 0), VC.request(743, 11)]

    def run(with_extra):
        eng = _engine("fp32", slots, 4)
        eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=VC.SESSION_MAX_LENGTH)
        _begin(eng, "fp32", slots)
        for s, r in enumerate(stay):
            _admit_one(eng, s, r, VC.SESSION_MAX_LENGTH)
        eng.decode_steps(4)
        if with_extra:
            _admit_group(eng, [11, 6, 8], extra, [24, 20, 30])
        eng.decode_steps(3)
        eng.decode_steps(5)
        cur, live = eng.row_state()
        ids = [eng.row_ids(s, cur[s]).cpu() for s in range(len(stay))]
        lg = eng.logits().cpu().view(slots, K, V)[: len(stay)].clone()
        last = [cur[s] for s in (11, 6, 8)]
        eng.close()
        return cur[: len(stay)], live[: len(stay)], ids, lg, last

    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1] and a[4] == [1, 1, 1] and b[4] == [1 + 7 + 1 + 8, 1 + 0 + 1 + 8, 1 + 11 + 1 + 8]
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))


# ---- 9: refusals through the C ABI --------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    slots, spare = 3, 2
    eng = _engine("fp32", slots, spare, max_prompt=16)
    eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=0)
    _begin(eng, "fp32", slots)
    busy, a, b = VC.request(701, 8), VC.request(724, 11), VC.request(717, 1)
    _admit_one(eng, 0, busy, 24)
    eng.decode_steps(2)

    def state():
        cur, live = eng.row_state()
        return cur, live, [eng.row_ids(s, 14).cpu() for s in range(slots)], eng.slot_voice(), eng.logits().cpu().view(torch.int32)

    def same(x, y):
        return x[0] == y[0] and x[1] == y[1] and _same(x[2], y[2]) and x[3] == y[3] and torch.equal(x[4], y[4])

    s0 = state()
    assert s0[3] == [8, 0, 0]
    ca, cb = a[4].cuda().contiguous(), b[4].cuda().contiguous()
    big = torch.zeros(K, 12, dtype=torch.long).cuda()
    pair = [a, b]
    E = _native
    tries = [
        (lambda: _raw(eng, [1, 2], pair, [ca, cb], [11, -1], [24, 24]), E.PTTS_E_INVALID, "T < 0"),
        (lambda: _raw(eng, [1, 2], pair, [ca, None], [11, 1], [24, 24]), E.PTTS_E_INVALID, "NULL codes with T > 0"),
        (lambda: _raw(eng, [1, 2], pair, [big, cb], [12, 1], [24, 24]), E.PTTS_E_CAPACITY, "P + 1 + Tmax > max_prompt"),
        (lambda: _raw(eng, [1, 2], pair, [ca, cb], [11, 1], [12, 24]), E.PTTS_E_INVALID, "T + 2 > max_length"),
        (lambda: _raw(eng, [1, 2], pair, [ca, cb], [11, 1], [24, 31]), E.PTTS_E_CAPACITY, "max_length above the session's"),
        (lambda: _raw(eng, [1, 2], pair, [ca, cb], [11, 1], [24, 1]), E.PTTS_E_INVALID, "max_length 1"),
        (lambda: _raw(eng, [1, 0], pair, [ca, cb], [11, 1], [24, 24]), E.PTTS_E_INVALID, "busy slot"),
        (lambda: _raw(eng, [1, 3], pair, [ca, cb], [11, 1], [24, 24]), E.PTTS_E_INVALID, "slot outside the session"),
        (lambda: _raw(eng, [1, 1], pair, [ca, cb], [11, 1], [24, 24]), E.PTTS_E_INVALID, "slot listed twice"),
        (lambda: _raw(eng, [1, 2], pair, [ca, cb], [11, 1], [24, 24], n=0), E.PTTS_E_INVALID, "n = 0"),
        (lambda: _raw(eng, [1, 2, 1], [a, b, a], [ca, cb, ca], [11, 1, 11], [24, 24, 24]), E.PTTS_E_INVALID, "three requests, one slot twice"),
    ]
    for call, want, what in tries:
        assert call() == want, what
        assert same(s0, state()), what
    eng.set_audio_prefix(a[4][None])  # a pending static prefix stays refused by the session
    assert _raw(eng, [1, 2], pair, [ca, cb], [11, 1], [24, 24]) == E.PTTS_E_UNSUPPORTED
    assert same(s0, state())
    eng.set_audio_prefix(None)
    eng.close()
    # more requests than spare rows, on a session with three idle slots
    eng = _engine("fp32", 4, 2, max_prompt=16)
    eng.set_gen_params(max_length=VC.SESSION_MAX_LENGTH, min_new_tokens=0)
    _begin(eng, "fp32", 4)
    _admit_one(eng, 0, busy, 24)
    eng.decode_steps(2)
    slots = 4
    s0 = state()
    assert _raw(eng, [1, 2, 3], [a, b, a], [ca, cb, ca], [11, 1, 11], [24, 24, 24]) == E.PTTS_E_CAPACITY
    assert same(s0, state())
    assert _raw(eng, [3, 1], pair, [ca, cb], [11, 1], [13, 3], sample=1) == E.PTTS_OK  # T + 2 == max_length: one generated token each
    cur, live = eng.row_state()
    assert cur[3] == 13 and cur[1] == 3 and not live[3] and not live[1] and eng.slot_voice() == [8, 1, 0, 11]
    eng.prefill(busy[0][None], busy[1][None], busy[2][None], busy[3][None], sample=False)  # no session: refused too
    assert _raw(eng, [1, 2], pair, [ca, cb], [11, 1], [24, 24]) == E.PTTS_E_INVALID
    eng.close()


# ---- 10: ContinuousBatcher end to end -------------------------------------------------------------------------------------------------------------
def _batcher_case():
    ms, isd = C.GEN_VOICE_SEEDS
    m, spec, sd, dsd = C.tiny_model(seed=ms)
    m = m.to("cuda")
    desc, prompt_ids, voice, syn, gp = C.gen_voice_inputs(isd)
    extras = [dict(input_values=voice.cuda()), dict(decoder_input_ids=syn[:, :3].cuda()), dict(decoder_input_ids=syn.cuda()), {}, {},
              dict(decoder_input_ids=torch.cat([torch.full((9, 1), 1025), syn[:, :5]], 1).cuda()), dict(input_values=voice.cuda())]
    news = [20, 14, 20, 12, 20, 12, 13]
    Ts = [6, 3, 6, 0, 0, 5, 6]
    return m, desc, prompt_ids, extras, news, Ts


def test_continuous_batcher_with_voice_groups_equals_generate_on_each_request_alone():
    """Tiny T5 + decoder + codec, 10 slots + 4 spare rows: seven requests (waveform prompts, code prompts of 3, 5 and 6 frames, none) are
    admitted as [0, 1, 2] | [3, 4] | [5, 6] - runs by kind, FIFO. Per request the raw ids are those of model.generate() on that request alone
    and the waveform is within the codec's bar (RMS 1e-4); the streaming batcher's chunks ("emit", and "skip" behind the prompt's samples)
    concatenate to the same waveform. Requests with a prompt have max_length >= 2K - 1 (see tests/test_session_voice_gpu.py)."""
    import parler_tts_amd as PT

    m, desc, prompt_ids, extras, news, Ts = _batcher_case()
    base = dict(input_ids=desc.cuda(), prompt_input_ids=prompt_ids.cuda())
    refs = []
    for ex, n in zip(extras, news):
        out = m.generate(**base, **ex, do_sample=False, max_new_tokens=n, min_new_tokens=n, return_dict_in_generate=True)
        refs.append((out.sequences[0, : out["audios_length"][0]].cpu(), m._engine.ids().cpu().clone()))
    kw = dict(slots=10, max_description_tokens=8, max_prompt_tokens=5, poll_steps=4, do_sample=False, max_new_tokens=20, min_new_tokens=20,
              admit_batch=4, max_voice_frames=11, admit_voice_groups=True)
    submit = [dict(input_ids=desc[0], prompt_input_ids=prompt_ids[0], max_new_tokens=n, **ex) for ex, n in zip(extras, news)]
    seen = []
    cb = PT.ContinuousBatcher(m, **kw)
    assert cb.spare == 4
    row_ids = cb.eng.row_ids
    cb.eng.row_ids = lambda s, n: (seen.append((cb._slot[s].ticket, row_ids(s, n).cpu())), seen[-1][1].cuda())[1]
    out = cb.run(submit)
    assert cb.admission_groups == [3, 2, 2] and cb.admissions == 7
    got_ids = dict(seen)
    hop = DA.DAC_TINY.hop_length
    for i, ((wav, n), (ref_wav, ref_ids)) in enumerate(zip(out, refs)):
        assert torch.equal(got_ids[i], ref_ids), i
        assert n == wav.shape[0] == ref_wav.shape[0], (i, n, ref_wav.shape)
        rms = float((wav.cpu() - ref_wav).pow(2).mean().sqrt())
        assert rms <= 1e-4, (i, rms)
    assert [n for _, n in out] == [hop * ((nn + 1 + t - 9) if nn + 1 + t >= 17 else nn + t) for nn, t in zip(news, Ts)]
    cb.eng.row_ids = row_ids
    cb.close()
    whole = [w.cpu() for w, _ in out]
    for mode in ("emit", "skip"):
        cs = PT.ContinuousBatcher(m, **kw, stream_chunk_frames=4, stream_voice_prompts=mode)
        tickets = [cs.submit(**r) for r in submit]
        parts, last = {t: [] for t in tickets}, {t: 0 for t in tickets}
        for t, chunk, is_last in cs.chunks():
            parts[t].append(chunk.cpu())
            last[t] += bool(is_last)
        assert cs.admission_groups == [3, 2, 2]
        for i, t in enumerate(tickets):
            got = torch.cat(parts[t])
            skip = 0 if mode == "emit" or Ts[i] == 0 else whole[i].shape[0] - got.shape[0]
            assert last[t] == 1 and (mode == "emit" or Ts[i] == 0 or skip == hop * Ts[i]), (mode, i, skip)
            assert got.shape[0] == whole[i].shape[0] - skip, (mode, i)
            worst = float((got - whole[i][skip:]).abs().max()) if got.shape[0] else 0.0
            assert worst <= 1e-5, (mode, i, worst)  # the streaming bar of tests/test_continuous_streaming_voice_gpu.py
        cs.close()


# ---- 11: an engine without spare rows ----------------------------------------------------------------------------------------------------------
def test_one_voice_request_runs_in_its_slot_and_needs_no_spare_row():
    """2 slots on an engine of max_batch 2, T = 3: admit_row(voice=) and admit_rows([r], voices=[v]) both run their pass in the slot itself, and
    each slot's step-0 logits are those of ptts_set_audio_prefix + ptts_prefill of the request alone on the same engine, bit for bit. The same
    list without a voice prompt runs on a spare row and is refused for want of one."""
    slots, L = 2, 24
    reqs = [VC.request(751, 3), VC.request(752, 3)]
    eng = _engine("fp32", slots, 0)
    eng.set_gen_params(max_length=L, min_new_tokens=0)
    static = []
    for r in reqs:
        eng.set_audio_prefix(r[4][None])
        eng.prefill(r[0][None], r[1][None], r[2][None], r[3][None], sample=False)
        static.append(eng.logits().cpu().view(K, V).clone())
    _begin(eng, "fp32", slots)
    with pytest.raises(ValueError, match="spare rows"):
        eng.admit_rows([1], *[t[None] for t in reqs[1][:4]], max_lengths=[L], sample=False)
    assert eng.row_state() == ([1, 1], [False, False]) and eng.slot_voice() == [0, 0]
    _admit_one(eng, 0, reqs[0], L, sample=False)
    _admit_group(eng, [1], [reqs[1]], [L], sample=False)
    got = eng.logits().cpu().view(slots, K, V)
    for s in range(slots):
        assert torch.equal(got[s].view(torch.int32), static[s].view(torch.int32)), s
    assert eng.row_state() == ([4, 4], [True, True]) and eng.slot_voice() == [3, 3]
    eng.close()
