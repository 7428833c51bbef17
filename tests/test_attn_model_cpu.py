"""CPU: the float64 restatement of the attention kernels (tests/attn_model.py) against independent statements of the same operations - torch's
scaled_dot_product_attention with boolean masks, the RoPE of oracle/decoder_oracle.py, the T5 attention of oracle/t5_oracle.py, the e4m3 cache
quantiser of oracle/fp8_oracle.py - and the derived error bound of the random-data GPU tests against a plain fp32 evaluation of the reference."""
import math

import pytest
import torch
import torch.nn.functional as F

import attn_cases as AC
import attn_model as AM
from oracle import decoder_oracle as DO
from oracle import fp8_oracle as FO
from oracle import t5_oracle as TO

F64 = torch.float64


def _sdpa(c):
    """float64 scaled_dot_product_attention of a prefill / cross DecCase without RoPE: boolean masks, grouped-query by repeat_interleave."""
    n_rep = AC.NH // c.kv_heads
    L = c.N if c.cross else c.Q
    q = c.heads_q().to(F64).view(c.B, c.Q, AC.NH, 64).transpose(1, 2)
    K = c.K[:, :, :L].repeat_interleave(n_rep, dim=1)
    V = c.V[:, :, :L].repeat_interleave(n_rep, dim=1)
    keep = torch.ones(c.B, 1, c.Q, L, dtype=torch.bool)
    if not c.cross:
        keep &= torch.tril(torch.ones(c.Q, L, dtype=torch.bool))[None, None]
    ml = L if c.cross else c.P
    if c.mask is not None:
        keep[..., :ml] &= (c.mask[:, None, None, :ml] != 0)
    K, V = torch.nan_to_num(K), torch.nan_to_num(V)  # masked rows may hold anything: the mask must hide them
    o = F.scaled_dot_product_attention(q, K, V, attn_mask=keep, scale=c.scale)
    return o.transpose(1, 2).reshape(c.B * c.Q, AC.H), keep.any(dim=-1).expand(c.B, AC.NH, c.Q).transpose(1, 2).reshape(c.B * c.Q, AC.NH)


@pytest.mark.parametrize("kv_heads", [4, 2, 1])
@pytest.mark.parametrize("cross", [False, True])
def test_model_equals_sdpa_with_boolean_masks(kv_heads, cross):
    c = AC.dec_case(mode="random", bf16=True, decode=False, cross=cross, Ls=[0, 0, 0], Q=11, N=13, P=4, kv_heads=kv_heads, seed=kv_heads)
    m = c.model()
    ref, any_key = _sdpa(c)
    seen = any_key[..., None].expand(-1, -1, 64).reshape(ref.shape)
    if cross:
        assert not any_key[c.Q:2 * c.Q].any() and any_key[:c.Q].all() and any_key[2 * c.Q:].all()  # utterance 1 is fully masked: rows without a key
    else:
        assert not any_key[c.Q:c.Q + 2].any() and any_key[c.Q + 2:].all() and any_key[:c.Q].all()  # left padding of 2: its first two rows see nothing
    assert float((m["out"] - ref)[seen].abs().max()) <= 1e-12
    assert float(m["out"][~seen].abs().max() if (~seen).any() else 0.0) == 0.0
    assert torch.equal(m["count"] > 0, any_key)


def test_model_rope_equals_the_decoder_oracle():
    cos, sin = DO.rope_tables(64, 10000.0, 40)
    x = torch.randn(5, 7, 64, generator=torch.Generator().manual_seed(1), dtype=F64)
    pos = torch.tensor([0, 1, 17, 38, 39])
    ref = x * cos.to(F64)[pos][:, None] + DO._rotate_half(x) * sin.to(F64)[pos][:, None]
    assert float((AM.rope(x, cos, sin, pos[:, None].expand(5, 7)) - ref).abs().max()) <= 1e-12
    # the exact tables: the rotation of integers is exact and unrope inverts it
    ec, es = AC.exact_rope_tables(40)
    y = torch.randint(-8, 9, (5, 7, 64), generator=torch.Generator().manual_seed(2)).to(F64)
    raw = AC.unrope(y, ec, es, pos[:, None].expand(5, 7))
    assert torch.equal(raw, raw.round()) and float(raw.abs().max()) <= 16
    assert torch.equal(AM.rope(raw, ec, es, pos[:, None].expand(5, 7)), y)


@pytest.mark.parametrize("mask_kind", [None, "right", "left", "row"])
def test_model_t5_attention_equals_the_t5_oracle(mask_kind):
    spec = TO.T5Spec(vocab_size=32, d_model=64, d_kv=64, d_ff=64, num_layers=1, num_heads=AC.NH)
    orc = TO.T5Oracle(spec, TO.make_t5_weights(spec, seed=3))
    c = AC.t5_case(mode="random", B=2, N=19, mask_kind=mask_kind, seed=5)
    N = c.N
    pb = orc.position_bias(N).to(F64)  # [heads, query, key]
    table = torch.zeros(AC.NH, c.bias_ld, dtype=F64)
    for d in range(-(N - 1), N):
        table[:, d + c.bias_zero] = pb[:, max(0, -d), max(0, -d) + d]
    c.bias = table.float()
    x = c.qkv[:2 * N, :3 * AC.H].reshape(2, N, 3, AC.NH, 64).to(F64)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    bias = orc.position_bias(N)[None].to(F64)
    if c.mask is not None:
        bias = bias + (1.0 - c.mask[:, None, None, :].to(F64)) * torch.finfo(torch.float32).min  # T5Oracle.encode
    ref = (torch.softmax(q @ k.transpose(2, 3) + bias, dim=-1) @ v).transpose(1, 2).reshape(2, N, AC.H)
    assert float((AC.t5_model(c)["out"] - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("S,NW,bf16", [(2, 4, True), (4, 4, True), (8, 4, False), (4, 1, False)])
def test_split_combine_equals_the_unsplit_result(S, NW, bf16):
    L = 2 * AM.span(S, NW, bf16) // (4 if S == 8 else 1) + 3
    c = AC.dec_case(mode="random", bf16=bf16, Ls=[L, 3, L // 2], kv_heads=2, rope="real", S=S, NW=NW, seed=S)
    m = c.model(S=S, NW=NW)
    assert float((AM.combine_splits(m["part"], m["stats"]) - m["out"]).abs().max()) <= 1e-12
    assert bool((m["stats"][1, 1:, :, 0] == -math.inf).all()) and bool((m["stats"][1, 1:, :, 1] == 0).all())  # 3 keys: every split but the first is empty
    # a row whose splits are all empty yields 0
    part, stats = torch.zeros(1, S, AC.H, dtype=F64), torch.zeros(1, S, AC.NH, 2, dtype=F64)
    stats[..., 0] = -math.inf
    assert float(AM.combine_splits(part, stats).abs().max()) == 0.0


def test_kv8_quantiser_edge_rows_equal_the_fp8_oracle():
    x = AC.kv8_edge_rows()
    b, s = AM.kv8_quantize(x)
    assert torch.equal(AM.kv8_dequantize(b, s).float(), FO.quantize_kv_rows(x))
    assert float(s[9, 0]) == 1.0 and int(b[9].max()) == 0          # the all-zero row: scale 1, bytes 0
    assert [float(v) for v in s[0:3, 0]] == [0.125, 0.25, 0.125]   # amax = 448 / 8, one float above, one below
    t = AM.kv8_dequantize(b[10], s[10])[:8]
    assert t.tolist() == [448.0, 16.0, 20.0, 28.0, 64.0, 80.0, 1.0, -16.0]  # ties to even
    r = torch.randn(50, 64, generator=torch.Generator().manual_seed(9)) * 3
    b, s = AM.kv8_quantize(r)
    assert torch.equal(AM.kv8_dequantize(b, s).float(), FO.quantize_kv_rows(r))


@pytest.mark.parametrize("bf16", [True, False])
def test_fragment_order_index(bf16):
    M, K = 21, AC.H
    idx = AM.fo_elem_index(M, K, bf16)
    assert idx.unique().numel() == M * K and int(idx.max()) < 32 * K
    KT, EPL = (32, 8) if bf16 else (16, 4)
    for m, k in ((0, 0), (5, 9), (17, 255), (20, 100)):  # X_fo[M/16 tiles][K/KT fragments][64 lanes][16 B], lane = ((k % KT) / EPL) * 16 + (m & 15)
        lane = ((k % KT) // EPL) * 16 + (m & 15)
        assert int(idx[m, k]) == (((m // 16) * (K // KT) + k // KT) * 64 + lane) * EPL + k % EPL


def test_exact_cases_have_separated_score_tiers_and_integer_sums():
    for mode, rope in (("uniform", None), ("onehot", "exact"), ("onehot", None)):
        c = AC.dec_case(mode=mode, bf16=True, Ls=[70, 67, 35], kv_heads=2, rope=rope, decoy="hot", S=2, NW=4)
        m = c.model(S=2, NW=4)
        AC.assert_tiers(m)
        assert torch.equal(m["num"].float().double(), m["num"].float().double().round())
        if mode == "onehot":  # the hot key wins where it is visible: the output is its V row
            (b, kvh), t = next(iter(c.hot.items()))
            nr = c.new_rows()
            v = nr["v"][b, kvh] if t == c.lens[b] - 1 else c.V[b, kvh, t]
            assert torch.equal(AC.exact_out(m["num"], m["den"], False)[b, kvh * 2 * 64:kvh * 2 * 64 + 64].double(), v)


@pytest.mark.parametrize("cfg", AC.ATTN_CONFIGS, ids=lambda c: f"{'bf16' if c[0] else 'fp32'}{'-e4m3' if c[1] else ''}-S{c[2]}-NW{c[3]}")
def test_one_hot_rounds_make_every_candidate_hot_in_every_utterance(cfg):
    """The rounds the GPU tests run place the hot key at position 0, L - 1, the first and last position of every split and loop iteration, 63 and
    64 - for EVERY utterance of the case, the longest included."""
    bf16, kv8, S, NW = cfg
    for L in AC.attn_lengths(S, NW, bf16):
        big = AC.is_big(S, NW, bf16)
        Ls = AC.ragged(L, big)
        kv_heads = 2 if big else 4 if L % 2 else 1
        seen = [set() for _ in Ls]
        for r in range(AC.hot_rounds(Ls, kv_heads, S, NW, bf16)):
            c = AC.dec_case(mode="onehot", bf16=bf16, kv8=kv8, Ls=Ls, kv_heads=kv_heads, hot_round=r, S=S, NW=NW, masked=False)
            for (b, kvh), t in c.hot.items():
                seen[b].add(t)
        for b, x in enumerate(Ls):
            assert seen[b] == set(AC.hot_candidates(x, S, NW, bf16)), (L, b, sorted(set(AC.hot_candidates(x, S, NW, bf16)) - seen[b]))
    for N in AC.CROSS_N:  # decode cross-attention: utterance 0 sees every key
        seen = set()
        for r in range(AC.hot_rounds([N] * 3, 2, 1, NW, bf16)):
            c = AC.dec_case(mode="onehot", bf16=bf16, cross=True, Ls=[0, 0, 0], N=N, kv_heads=2, hot_round=r, NW=NW)
            seen |= {t for (b, kvh), t in c.hot.items() if b == 0}
        assert seen == set(AC.hot_candidates(N, 1, NW, bf16)), (N, seen)


def test_fp32_reference_stays_inside_the_derived_bound():
    """Before any GPU run: a plain fp32 torch evaluation of the same attention is inside `tol` on every input of part C - as fp32, and rounded to
    bf16 against the bound of a bf16 output. If it were not, the derivation of the bound would be wrong."""
    worst = {False: 0.0, True: 0.0}

    def check(name, ref, m, tol_of):
        for bf16_out in (False, True):
            got = ref.bfloat16().double() if bf16_out else ref.double()
            r = float(((got - m["out"].reshape(got.shape)).abs() / tol_of(bf16_out).reshape(got.shape).clamp_min(1e-300)).max())
            assert r <= 1.0, (name, bf16_out, r)
            worst[bf16_out] = max(worst[bf16_out], r)

    for name, kind, c, S, NW in AC.random_dec_cases():
        m = c.model(S=S, NW=NW)
        check(name, AC.fp32_attention(c), m, lambda b: AC.dec_tolerance(c, m, S, NW, bf16_out=b))
    for name, c in AC.random_t5_cases():
        m = AC.t5_model(c)
        check(name, AC.fp32_t5_attention(c), m, lambda b: AC.t5_tolerance(c, m, bf16_out=b))
    print(f"fp32 torch reference: largest error / bound {worst[False]:.3f}, rounded to bf16 {worst[True]:.3f}")
    assert worst[True] > 0.5, "the bf16 term is not slack either: half an ulp is reached"
