"""CPU: the float64 restatement of the decode-step kernels (tests/step_model.py) against independent statements, the exactness proofs that the
GPU tests' constructions rest on (tests/test_step_kernels_gpu.py), on the very inputs tests/step_cases.py generates, and negative controls: each
kind of slip the GPU tests exist to catch must exceed their bars."""
import math

import pytest
import torch
import torch.nn.functional as F

import step_cases as SC
import step_harness as SH
import step_model as SM
from oracle import decoder_oracle as DO
from oracle import fp8_oracle as FP8

F64 = torch.float64


# ---- the model against independent statements -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (384, 512, 1024, 1536))
def test_layer_norm_gelu_and_strip_statistics_against_torch(K):
    x, gamma, beta = SC.ln_inputs(17, K, 1)
    ref = F.layer_norm(x.to(F64), (K,), gamma.to(F64), beta.to(F64), 1e-5)
    y = SM.layer_norm64(x, gamma, beta)
    assert float((y - ref).abs().max()) <= 1e-13
    assert float((SM.gelu_erf64(x) - F.gelu(x.to(F64))).abs().max()) <= 1e-15
    st = SM.strip_stats64(x)
    xs = x.to(F64).view(17, K // 16, 16)
    assert torch.allclose(st[..., 0], xs.mean(dim=2), rtol=0, atol=1e-15) and torch.allclose(st[..., 1], xs.var(dim=2, unbiased=False) * 16, rtol=1e-13, atol=0)
    mean, var = SM.combine_strip_stats64(st)
    assert float((mean[:, 0] - x.to(F64).mean(dim=1)).abs().max()) <= 1e-14
    assert torch.allclose(var[:, 0], x.to(F64).var(dim=1, unbiased=False), rtol=1e-12, atol=0)
    assert float((SM.lns_layer_norm64(x, st, gamma, beta) - ref).abs().max()) <= 1e-12  # Chan's combination of exact partials is the LayerNorm


def test_e4m3_rows_against_the_oracle_and_torch():
    W = torch.randn(32, 128, generator=SC.gen(2)) * 3.0
    b, scale, deq = SM.e4m3_rows(W)
    ref, rs = FP8.quantize_rows(W)
    assert torch.equal(scale, rs) and torch.equal(deq, ref.to(F64))
    assert torch.equal(b.view(torch.float8_e4m3fn).to(F64) * scale.to(F64)[:, None], deq)  # what the strips compute from bytes and scales
    assert bool((torch.log2(scale) == torch.round(torch.log2(scale))).all())
    # integers |v| <= 8, also scaled by powers of two (the GELU constructions), are exact in e4m3 x a power-of-two row scale
    Wi = SC.ints((48, 256), 3)
    Ws, _ = SC.scale_into_gelu_range(Wi, SC.ints((5, 256), 4) @ Wi.t())
    for Wx in (Wi, Ws):
        assert torch.equal(SM.e4m3_rows(Wx)[2], Wx)


@pytest.mark.parametrize("rope", (False, True))
@pytest.mark.parametrize("n_rep", (1, 2))
def test_cross_block_against_the_oracles_decoder_layer(rope, n_rep):
    """The cross block of one oracle decoder layer (oracle/decoder_oracle.py: encoder_attn_layer_norm, q_proj, the quirk of rotating q only,
    repeat_kv, the additive mask, softmax) on a tiny shape in fp32, against cross_block64."""
    nh, B, N, P = 4, 3, 7, 2
    H = nh * 64
    spec = DO.DecoderSpec(hidden_size=H, num_hidden_layers=1, num_attention_heads=nh, ffn_dim=2 * H, max_position_embeddings=64, rope_embeddings=rope,
                          num_key_value_heads=nh // n_rep, num_cross_attention_key_value_heads=nh // n_rep)
    sd = DO.make_decoder_weights(spec, seed=5)
    orc = DO.DecoderOracle(spec, sd)
    lp = "model.decoder.layers.0."
    g = SC.gen(6)
    x = torch.randn(B, H, generator=g)
    enc = torch.randn(B, N, H, generator=g)
    mask = (torch.rand(B, N, generator=g) < 0.7).int()
    mask[:, 0] = 1
    cur_len = torch.tensor([1, 4, 9])
    # the oracle's steps (forward(), cross-attention block), one utterance at a time because every utterance sits at its own position
    nkc = spec.cross_kv_heads
    Kc = orc._heads(orc._linear(enc, lp + "encoder_attn.k_proj.weight"), B, N, nkc)
    Vc = orc._heads(orc._linear(enc, lp + "encoder_attn.v_proj.weight"), B, N, nkc)
    ref = torch.zeros(B, H)
    for b in range(B):
        hn = orc._ln(x[b:b + 1, None], lp + "encoder_attn_layer_norm")
        q = orc._heads(orc._linear(hn, lp + "encoder_attn.q_proj.weight"), 1, 1)
        if rope:
            pos = P + int(cur_len[b]) - 1
            q = q * orc.cos[pos][None, None, None] + DO._rotate_half(q) * orc.sin[pos][None, None, None]
        add = ((1.0 - mask[b:b + 1].float()) * torch.finfo(torch.float32).min)[:, None, None, :]
        ref[b] = orc._attend(q, orc._repeat_kv(Kc[b:b + 1]), orc._repeat_kv(Vc[b:b + 1]), add, causal=False).transpose(1, 2).reshape(H)
    cap = N + 3
    Kp, Vp = torch.full((B, nkc, cap, 64), float("nan"), dtype=F64), torch.full((B, nkc, cap, 64), float("nan"), dtype=F64)
    Kp[:, :, :N], Vp[:, :, :N] = Kc.to(F64), Vc.to(F64)
    m = SM.cross_block64(x, orc.w[lp + "encoder_attn_layer_norm.weight"], orc.w[lp + "encoder_attn_layer_norm.bias"], orc.w[lp + "encoder_attn.q_proj.weight"],
                         Kp, Vp, n_rep=n_rep, N=N, P=P, cur_len=cur_len, mask=mask, scale=0.125, cos=orc.cos if rope else None,
                         sin=orc.sin if rope else None, bf16=False)
    assert float((m["out"] - ref.to(F64)).abs().max()) <= 2e-5 * float(ref.abs().max())
    # a row without a visible key yields 0 (the oracle's additive finfo.min would give the uniform mean: the kernels' rule is the restated one)
    mask[1] = 0
    m = SM.cross_block64(x, orc.w[lp + "encoder_attn_layer_norm.weight"], orc.w[lp + "encoder_attn_layer_norm.bias"], orc.w[lp + "encoder_attn.q_proj.weight"],
                         Kp, Vp, n_rep=n_rep, N=N, P=P, cur_len=cur_len, mask=mask, scale=0.125, cos=orc.cos if rope else None,
                         sin=orc.sin if rope else None, bf16=False)
    assert float(m["out"][1].abs().max()) == 0.0 and float(m["out"][0].abs().max()) > 0


def test_fragment_order_round_trip():
    for bf16 in SC.ENGINES:
        for M in (9, 16, 33):
            x = torch.randn(M, 128, generator=SC.gen(M))
            buf = SM.to_fo(x, bf16)
            assert buf.numel() == (M + 15) // 16 * 16 * 128 and int(torch.isnan(buf).sum()) == buf.numel() - M * 128
            assert torch.equal(SM.from_fo(buf, M, 128, bf16), x)


# ---- exactness proofs ----------------------------------------------------------------------------------------------------------------------------
def _sum32(terms, order):
    """fp32 sum of terms [..., K] over the last axis in the given order of K (sequential)."""
    acc = torch.zeros(terms.shape[:-1], dtype=torch.float32)
    for k in order:
        acc = acc + terms[..., k]
    return acc


@pytest.mark.parametrize("K", (384, 1024, 1536))
def test_construction_a_is_exact_in_any_accumulation_order(K):
    x, gamma, beta = SC.exact_ln_inputs(8, K, 800)
    # gamma = 0: the fp32 LayerNorm is beta exactly, whatever x and its statistics are
    y = F.layer_norm(x, (K,), gamma, beta, 1e-5)
    assert torch.equal(y, beta[None, :].expand(8, K)) and bool(torch.isfinite(x).all())
    W = SC.ints((16, K), 810)
    ref = beta.to(F64) @ W.t()
    assert float((beta.to(F64).abs() @ W.abs().t()).max()) < 2 ** 24  # every partial sum of any order stays an integer below 2^24
    terms = (W.float() * beta[None, :])                                 # [16, K] products, exact
    for order in (range(K), reversed(range(K)), torch.randperm(K, generator=SC.gen(1)).tolist()):
        assert torch.equal(_sum32(terms, order).to(F64), ref)
    # through a GELU the rows are scaled by powers of two into (-3, 3]: still exact
    Ws, acc = SC.scale_into_gelu_range(W, ref[None, :])
    assert torch.equal((Ws.float() * beta[None, :]).to(F64).sum(dim=1), acc[0]) and float(acc.abs().max()) <= 3.0
    assert bool((torch.log2((W / Ws)[W != 0]) % 1 == 0).all())


def test_float32_gelu_stays_inside_the_fp32_evaluation_bound():
    """0.5 x (1 + erf(x / sqrt 2)) evaluated in float32 step by step on the accumulators of construction (a), with an erf that is correctly rounded
    (float64's, rounded once) and with one that is 4 ulps off: both stay inside step_model.gelu_bound_fp32, and even the correctly rounded one is
    tens of fp32 ulps of the result away in the negative tail, where 1 + erf cancels - one fp32 ulp is not what this formula gives in fp32.
    (torch's own float32 gelu on this CPU is further off than either: its vectorised erf is ~6 ulps off at |erf| ~ 1.)"""
    beta = SC.ints((1536,), 801)
    W = SC.ints((256, 1536), 810)
    _, acc = SC.scale_into_gelu_range(W, (beta @ W.t())[None, :])
    assert float(acc.abs().max()) <= 3.0 and float(acc.abs().max()) > 1.5 and float(acc.min()) < -1.5
    x = acc.float()
    ref = SM.gelu_erf64(acc)
    # what gelu_erf_wt<float> computes instead for engine-dtype outputs: 0.5 x erfc(-x / sqrt 2) in double, rounded once - within one fp32 ulp
    wt = (0.5 * acc * torch.erfc(-acc / math.sqrt(2.0))).float().to(F64)
    assert float(((wt - ref).abs() / SM.ulp(ref, False)).max()) <= 0.51
    arg = x * torch.tensor(0.70710678118654752440, dtype=torch.float32)
    for off in (0.0, 4.0, -4.0):
        e = torch.erf(arg.to(F64)).float() + off * 2.0 ** -24
        err = (((0.5 * x) * (1.0 + e)).to(F64) - ref).abs()
        assert bool((err <= SM.gelu_bound_fp32(acc)).all()), off
        if off == 0.0:
            assert float((err / SM.ulp(ref, False)).max()) > 16.0


def test_construction_b_exposes_the_staged_rows_exactly():
    K, N, M = 1024, 256, 5
    x, gamma, beta, = SC.ln_inputs(M, K, 820)
    sel = SC.selection_weights(N, K, 830)
    assert len(sel) == K // N and set(torch.cat([pi for _, pi, _ in sel]).tolist()) == set(range(K))  # every column is selected
    for bf16 in SC.ENGINES:
        y = F.layer_norm(x, (K,), gamma, beta, 1e-5)
        y = y.bfloat16().float() if bf16 else y
        rows = torch.zeros(M, K, dtype=F64)
        for W, pi, c in sel:
            assert int((W != 0).sum()) == N and bool((W[torch.arange(N), pi] == c).all())
            out = y @ W.float().t()  # fp32: one non-zero product per output, the other K - 1 terms are exact zeros
            rows[:, pi] = out.to(F64) / c[None, :]
        assert torch.equal(rows, y.to(F64))


@pytest.mark.parametrize("M", SC.ROWS_LNS)
def test_strip_statistics_construction_is_exact(M):
    K, Kin = 1024, 512
    x = SC.ints((M, Kin), 700 + M, -2, 2)
    W = SC.sparse_int_weights(K, Kin, 700 + M + 3)
    r = SC.ints((M, K), 700 + M + 5, -8, 8)
    h = r + x @ W.t()
    assert float(h.abs().max()) <= 32
    ref = SM.strip_stats64(h)
    hs = h.float().view(M, K // 16, 16)
    for order in (list(range(16)), list(reversed(range(16))), [0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15]):
        mean = _sum32(hs, order) * 0.0625
        d = hs - mean[..., None]
        m2 = _sum32(d * d, order)
        assert torch.equal(mean.to(F64), ref[..., 0]) and torch.equal(m2.to(F64), ref[..., 1])


def test_exact_split_kv_partials_combine_exactly():
    for S in (2, 4):
        for K in (384, 1024):
            part, stats, rows = SC.exact_attn_partials(9, K, S, 300)
            nh = K // 64
            m = stats[..., 0]
            assert bool(torch.isinf(m[:, 1, 0]).all()) and bool(torch.isinf(m[:, :, nh - 1]).all()) and bool(torch.isnan(part[:, 1, :64]).all())
            for order in (range(S), reversed(range(S))):  # the kernel's fp32 recipe with the empty splits selected away
                mx = m.amax(dim=1)
                den, o = torch.zeros(9, nh), torch.zeros(9, K)
                for s in order:
                    live = ~torch.isinf(m[:, s])
                    w = torch.where(live, torch.exp2(m[:, s] - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)), torch.zeros(()))
                    den = den + torch.where(live, w * stats[:, s, :, 1], torch.zeros(()))
                    o = o + torch.where(live.repeat_interleave(64, dim=1), w.repeat_interleave(64, dim=1) * part[:, s], torch.zeros(()))
                inv = torch.where(den > 0, 1.0 / den, torch.zeros(()))
                got = o * inv.repeat_interleave(64, dim=1)
                assert torch.equal(got.to(F64), rows)
            for bf16 in SC.ENGINES:  # and the rows are representable in the engine dtype
                assert torch.equal(SM.round_engine(rows, bf16), rows)
            assert float(rows[:, -64:].abs().max()) == 0.0 and float(rows.abs().max()) > 0


def test_e4m3_case_rows_select_their_instances():
    for table in (SC.W8_CASES, SC.W8_FALLBACK):
        for (pro, epi, mtp), (M, fo) in table.items():
            assert SC.mtp_of(pro, M, fo) == mtp, (pro, epi, mtp, M, fo)
            assert M <= (32 if pro == SH.PRO_LNS else 8) or pro == SH.PRO_COPY
    assert not set(SC.W8_CASES) & set(SC.W8_FALLBACK)
    # PRO_LNS serves every row count of the list except 32 rows of the fp32 engine at hidden 1536 (LDS), which the GPU test expects to be declined
    assert [(M, K, bf) for K in SC.WIDTHS_FULL for bf in SC.ENGINES for M in SC.ROWS_LNS if not SC.lns_fits(M, K, bf)] == [(32, 1536, False)]
    # the row lists reach both pass sizes of msplit_rows and a ragged last pass
    assert {SC.mtp_of(SH.PRO_COPY, M, 1) for M in SC.ROWS_COPY_FO} == {1, 2}
    assert any(M % 16 for M in SC.ROWS_COPY_FO if M <= 64) and any(M % 32 for M in SC.ROWS_COPY_FO if M > 64)


def _flip_sets():
    """(family, [(M, K, seed)]) as tests/test_step_kernels_gpu.py aggregates the bf16 flip share."""
    out = []
    for K in (512, 1024, 1536):
        out.append((f"rows_prep K={K}", [(M, K, 100 + M) for M in SC.ROWS_COPY_FO] + [(27, K, 127)]))
    out.append(("fused", [(M, K, 500 + M) for K in (384, 512, 1024, 1536) for M in SC.ROWS_FUSED]))
    for K in SC.WIDTHS_FULL:  # (the PRO_LNS consumer's rows are produced on the device: no CPU restatement of its inputs)
        out.append((f"lnproj K={K}", [(M, K, 100 + M if M in SC.ROWS_COPY_FO else 820 + M) for Ms in SC.LNPROJ_ROWS.values() for M in Ms]))
    return out


@pytest.mark.parametrize("fam,cases", _flip_sets(), ids=[f for f, _ in _flip_sets()])
def test_float32_restatement_flips_at_most_half_the_cap(fam, cases):
    """The bf16 rows may differ from RNE(float64) in at most 1e-3 of their elements; the plain float32 LayerNorm rounded to bf16 stays at or below
    5e-4 on the same inputs, so the cap cannot hide a kernel worse than twice the reference. The fp32 bar of each case is 4 x the measured error
    of that restatement, floored at 4 fp32 ulps of the largest |y64|."""
    flips = n = 0
    for M, K, seed in cases:
        x, gamma, beta = SC.ln_inputs(M, K, seed)
        y64 = SM.layer_norm64(x, gamma, beta)
        y32 = F.layer_norm(x, (K,), gamma, beta, 1e-5)
        flips += int((y32.bfloat16().to(F64) != SM.round_engine(y64, True)).sum())
        n += y32.numel()
        bar, err = SM.ln_tolerance_fp32(x, gamma, beta, y64)
        assert bar == max(4 * err, 4 * float(SM.ulp(y64.abs().max().reshape(1), False)))
    print(f"{fam}: {flips} / {n} = {flips / n:.2e}")
    assert flips <= 5e-4 * n, f"{fam}: the float32 restatement flips {flips} of {n} elements"


# ---- negative controls: each must exceed the bars of the GPU tests ----------------------------------------------------------------------------------------
def test_negative_control_wrong_strip_columns():
    _, gamma, beta = SC.ln_inputs(1, 1024, 1)
    h, _, _ = SC.ln_inputs(9, 1024, 729)
    ref, bm, b2 = SM.strip_stats_bounds(h)
    good = SM.strip_stats64(h.float())
    assert bool(((good[..., 0] - ref[..., 0]).abs() <= bm).all()) and bool(((good[..., 1] - ref[..., 1]).abs() <= b2).all())
    wrong = SM.strip_stats64(torch.roll(h, -4, dims=1))  # statistics over columns 4 .. 19 instead of 0 .. 15
    assert bool(((wrong[..., 0] - ref[..., 0]).abs() > bm).any()) and bool(((wrong[..., 1] - ref[..., 1]).abs() > b2).any())
    # and a consumer fed the wrong strip's partials leaves the LayerNorm bound
    y64 = SM.layer_norm64(h, gamma, beta)
    bar, _ = SM.ln_tolerance_fp32(h, gamma, beta, y64)
    st = ref.clone()
    st[:, 0] = st[:, 1]
    for bf16 in SC.ENGINES:
        y = SM.round_engine(SM.lns_layer_norm64(h, st, gamma, beta), bf16)
        assert bool(((y - y64).abs() > SM.ln_rows_bound(y64, bar, bf16)).any())


def test_negative_control_neighbouring_utterance():
    M, K = 16, 1024
    x, gamma, beta = SC.ln_inputs(M, K, 116)
    y64 = SM.layer_norm64(x, gamma, beta)
    bar, _ = SM.ln_tolerance_fp32(x, gamma, beta, y64)
    for bf16 in SC.ENGINES:
        y = SM.round_engine(F.layer_norm(x, (K,), gamma, beta, 1e-5), bf16)
        assert bool(((y - y64).abs() <= SM.ln_rows_bound(y64, bar, bf16)).all())
        swapped = y.clone()
        swapped[[8, 9]] = y[[9, 8]]  # wave 0 of a group of 8 stages its neighbour's row
        bad = (swapped - y64).abs() > SM.ln_rows_bound(y64, bar, bf16)
        assert bool(bad[8].any()) and bool(bad[9].any()) and not bool(bad[:8].any())


def test_negative_control_swapped_fragments():
    M, K = 17, 1024
    x, gamma, beta = SC.ln_inputs(M, K, 117)
    y64 = SM.layer_norm64(x, gamma, beta)
    bar, _ = SM.ln_tolerance_fp32(x, gamma, beta, y64)
    for bf16 in SC.ENGINES:
        y = SM.round_engine(F.layer_norm(x, (K,), gamma, beta, 1e-5), bf16)
        buf = SM.to_fo(y, bf16)
        per = 64 * (8 if bf16 else 4)                     # elements of one fragment (64 lanes x 16 B)
        frag = buf.view(-1, per).clone()
        frag[[2, 3]] = frag[[3, 2]]                       # fragments 2 and 3 of row tile 0 change places
        got = SM.from_fo(frag.reshape(-1), M, K, bf16)
        bad = (got - y64).abs() > SM.ln_rows_bound(y64, bar, bf16)
        assert bool(bad[:16].any()) and not bool(bad[16:].any())
        # through an integer GEMM the slip is not exact any more either
        ints = SC.ints((M, K), 5)
        f2 = SM.to_fo(ints, bf16, fill=0.0).view(-1, per).clone()
        f2[[2, 3]] = f2[[3, 2]]
        W = SC.ints((16, K), 6)
        assert not torch.equal(SM.from_fo(f2.reshape(-1), M, K, bf16) @ W.t(), ints @ W.t())


def test_negative_control_empty_split_given_weight_one():
    g = SC.gen(77)
    M, S, K = 19, 4, 512
    nh = K // 64
    part = torch.randn(M, S, K, generator=g).float()
    stats = torch.stack((torch.randn(M, S, nh, generator=g) * 4.0, torch.rand(M, S, nh, generator=g) * 30.0 + 1.0), dim=3).float()
    stats[:, 2, 1, 0], stats[:, 2, 1, 1] = -math.inf, 0.0
    for bf16 in SC.ENGINES:
        ref, tol = SM.combine_tolerance(part, stats, bf16)
        assert bool(((SM.round_engine(ref, bf16) - ref).abs() <= tol).all())
        # the empty split taken with weight 1 (its maximum read as the head's): its partial row leaks into head 1
        leak = stats.clone()
        leak[:, 2, 1, 0] = stats[:, :, 1, 0].amax(dim=1)
        bad = (SM.combine_splits(part, leak) - ref).abs() > tol
        assert bool(bad[:, 64:128].any()) and not bool(bad[:, :64].any()) and not bool(bad[:, 128:].any())


@pytest.mark.parametrize("bf16", SC.ENGINES, ids=lambda b: "bf16" if b else "fp32")
@pytest.mark.parametrize("K", (512, 1024, 1536))
def test_negative_controls_of_the_fused_cross_block(K, bf16):
    """The random case of xattn_fused_kernel on the inputs the GPU test generates: an evaluation that differs from float64 only by fp32 arithmetic
    passes step_model.xattn_tolerance; the rotation one position late, no rotation, the neighbouring utterance's x, the mean of the visible V rows
    (q = 0), LN2 without its affine part and an all-zero output each exceed it - in both engine dtypes and at every width."""
    B, N, n_rep, P = 9, 17, 2, 3
    x, gamma, beta, Wq, Kc, Vc, cur_len, mask = SC.xattn_random_inputs(K, B, n_rep, bf16, 1110 + B)
    cos, sin = SC.rope_tables(P + 20)
    y = SM.round_engine(F.layer_norm(x, (K,), gamma, beta, 1e-5), bf16)  # the rows a float32 LayerNorm stages (the GPU test takes rows_prep_kernel's)
    kw = dict(n_rep=n_rep, N=N, P=P, cur_len=cur_len, mask=mask, scale=0.125, cos=cos, sin=sin, bf16=bf16)
    m = SM.cross_block64(x, gamma, beta, Wq, Kc, Vc, y=y, **kw)
    tol = SM.xattn_tolerance(m, Wq, Kc, N=N, n_rep=n_rep, scale=0.125, bf16=bf16)

    def ratio(out):
        return float(((out - m["out"]).abs() / tol).max())
    # fp32 arithmetic on the same staged rows: q in float32, then the float64 attention on that q - inside the bound, and far inside without rounding
    q32 = (y.float() @ Wq.float().t()).to(F64)
    from attn_model import decoder_attention
    fp32ish = decoder_attention(q32.view(B, K // 64, 64), Kc, Vc, Q=1, cross=True, **{k: v for k, v in kw.items()})["out"]
    assert ratio(SM.round_engine(fp32ish, bf16)) <= 1.0
    controls = {
        "rotation at P + cur_len": SM.cross_block64(x, gamma, beta, Wq, Kc, Vc, y=y, **{**kw, "cur_len": cur_len + 1})["out"],
        "no rotation": SM.cross_block64(x, gamma, beta, Wq, Kc, Vc, y=y, **{**kw, "cos": None, "sin": None})["out"],
        "the neighbouring utterance's x": SM.cross_block64(x, gamma, beta, Wq, Kc, Vc, y=torch.roll(y, 1, dims=0), **kw)["out"],
        "q = 0": SM.cross_block64(x, gamma, beta, Wq, Kc, Vc, y=torch.zeros_like(y), **kw)["out"],
        "gamma = 1, beta = 0": SM.cross_block64(x, gamma, beta, Wq, Kc, Vc, y=SM.round_engine(F.layer_norm(x, (K,)), bf16), **kw)["out"],
        "zero output": torch.zeros_like(m["out"]),
    }
    for name, out in controls.items():
        r = ratio(SM.round_engine(out, bf16))
        print(f"K={K} {'bf16' if bf16 else 'fp32'} {name}: error / bound {r:.1f}; median bound {float(tol.median()):.2e}")
        assert r > 4.0, name
