"""CPU: tests/dac_kernel_model.py - the float64 restatement the DAC kernel tests compare against - pinned against torch.nn.functional in float64
and against oracle/dac_oracle.py's stage functions. On dyadic data (small integers times a power of two) every sum is exact, so the comparison
is `==`; where a Snake is involved the two float64 evaluations agree to a few float64 ulps."""
import pytest
import torch
import torch.nn.functional as F

import dac_kernel_model as M
from oracle import dac_oracle as DA

F64 = torch.float64


def _ints(g, shape, lo, hi, scale):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64) * scale


@pytest.mark.parametrize("k,dil,stride,pad", [(1, 1, 1, -1), (7, 1, 1, -1), (7, 3, 1, -1), (7, 9, 1, -1), (3, 1, 1, 1), (4, 1, 2, 1), (16, 1, 8, 4)])
def test_conv_equals_torch_conv1d_exactly(k, dil, stride, pad):
    g = torch.Generator().manual_seed(k * 100 + dil)
    B, T, Cin, Cout = 2, 41, 16, 32
    x, w, b = _ints(g, (B, T, Cin), -4, 4, 0.25), _ints(g, (Cout, Cin, k), -3, 3, 0.125), _ints(g, (Cout,), -8, 8, 0.125)
    skip = None
    out, written = M.conv(x, w, b, k, dil=dil, stride=stride, pad=pad, skip=skip)
    p = pad if pad >= 0 else (k - 1) * dil // 2
    ref = F.conv1d(x.transpose(1, 2), w, b, stride=stride, dilation=dil, padding=p).transpose(1, 2)
    assert out.shape == ref.shape and torch.equal(out, ref)
    assert written.all()


@pytest.mark.parametrize("s", [2, 4, 8])
def test_transposed_conv_by_phases_equals_torch_exactly(s):
    g = torch.Generator().manual_seed(s)
    B, T, Cin, Cout = 2, 19, 32, 16
    x, w, b = _ints(g, (B, T, Cin), -4, 4, 0.25), _ints(g, (Cin, Cout, 2 * s), -3, 3, 0.125), _ints(g, (Cout,), -8, 8, 0.125)
    out, written = M.conv(x, w, b, 2 * s, stride=s, transposed=True)
    ref = F.conv_transpose1d(x.transpose(1, 2), w, b, stride=s, padding=(s + 1) // 2).transpose(1, 2)
    assert out.shape == ref.shape == (B, T * s, Cout) and torch.equal(out, ref)
    assert written.all()


def test_lens_rows_beyond_read_as_zeros_and_are_not_written():
    g = torch.Generator().manual_seed(9)
    B, T, C = 3, 12, 16
    x, w, b = _ints(g, (B, T, C), -4, 4, 0.25), _ints(g, (C, C, 7), -3, 3, 0.125), _ints(g, (C,), -8, 8, 0.125)
    lens, mul = [2, 0, 9], 2  # 4, 0 and 12 (clamped from 18) valid rows
    poisoned = x.clone()
    poisoned[0, 4:], poisoned[1, :] = float("nan"), float("nan")
    out, written = M.conv(poisoned, w, b, 7, dil=3, lens=lens, len_mul=mul)
    assert written.sum(1).tolist() == [4, 0, 12]
    for bi, n in enumerate([4, 0, 12]):
        xz = x[bi:bi + 1].clone()
        xz[:, n:] = 0
        ref = F.conv1d(xz.transpose(1, 2), w, b, dilation=3, padding=9).transpose(1, 2)
        assert torch.equal(out[bi:bi + 1, :n], ref[:, :n])
    assert not torch.isnan(out).any()
    # a transposed conv writes lens * len_mul * stride rows
    wt = _ints(g, (C, C, 4), -3, 3, 0.125)
    out, written = M.conv(poisoned, wt, b, 4, stride=2, transposed=True, lens=lens, len_mul=mul)
    assert written.sum(1).tolist() == [8, 0, 24] and not torch.isnan(out).any()
    # negative lengths clamp to zero
    assert M.valid_rows(10, [-3, 4], 2, 2) == [0, 8]


def test_skip_bias_and_bf16_rounding():
    g = torch.Generator().manual_seed(3)
    x, w, b = _ints(g, (1, 5, 16), -4, 4, 0.25), _ints(g, (16, 16, 1), -3, 3, 0.125), _ints(g, (16,), -8, 8, 0.125)
    skip = _ints(g, (1, 5, 16), -16, 16, 0.0625)
    out, _ = M.conv(x, w, b, 1, skip=skip)
    assert torch.equal(out, torch.einsum("btc,oc->bto", x, w[:, :, 0]) + b + skip)
    # round-to-nearest-even at the bf16 boundary: 1 + 2^-8 is a tie -> 1 (even), 1 + 3 * 2^-8 -> 1 + 2^-6... ties go to the even mantissa
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 2.0 ** -8)])
    assert M.rb(t).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0]
    a = torch.tensor([0.25, 0.3125, 0.375, 1.0])
    assert torch.equal(M.inv_alpha(a), (1.0 / (a + torch.tensor(1e-9, dtype=torch.float32))).to(torch.float32))


def _tiny():
    spec = DA.DAC_TINY
    sd = DA.make_dac_weights(spec, seed=4321, with_encoder=True)
    return spec, DA.DacOracle(spec, sd), DA.DacOracle(spec, sd, precision="bf16")


def test_model_matches_the_oracle_stage_functions():
    """Every decoder stage of the tiny codec, fp32 and bf16-operand precision: the model's conv / transposed conv / fused unit / final conv on the
    oracle's own stage inputs, in float64, against the oracle's fp32 torch evaluation (<= 2e-5: the oracle's own rounding)."""
    spec, o32, o16 = _tiny()
    g = torch.Generator().manual_seed(11)
    codes = torch.randint(0, spec.codebook_size, (2, spec.num_codebooks, 9), generator=g)
    for o in (o32, o16):
        bf = o.precision == "bf16"
        w, d, n = o.w, "decoder.model.", len(spec.decoder_rates)
        z = o.from_codes(codes)
        act, raw = (M.rb(z) if bf else z), None
        for s in range(o.n_stages()):
            exp_raw, exp_act, exp_y = o.stage(s, act, raw)
            cl = lambda t: t.transpose(1, 2)
            if s == 0:
                got, _ = M.conv(cl(act), w[d + "0.weight"], w[d + "0.bias"], 7)
            else:
                bi, k = divmod(s - 1, 4)
                b = f"{d}{bi + 1}.block."
                if k == 0:
                    st = spec.decoder_rates[bi]
                    got, _ = M.conv(cl(act), w[b + "1.weight"], w[b + "1.bias"], 2 * st, stride=st, transposed=True)
                else:
                    r = f"{b}{k + 1}.block."
                    if bf:
                        u = M.resunit(cl(act), w[r + "1.weight"], w[r + "1.bias"], w[r + "2.alpha"].flatten(), w[r + "3.weight"], w[r + "3.bias"],
                                      torch.ones(act.shape[1]), cl(raw), (1, 3, 9)[k - 1])
                        got = u["raw"]
                        # the inner activation: bf16 values, equal but for a rounding flip where the fp32 and float64 Snake straddle a boundary
                        dy = (u["y"] - cl(exp_y)).abs()
                        assert float((dy > 0).to(F64).mean()) <= 1e-2 and bool((dy <= 2.0 ** -7 * cl(exp_y).abs() + 1e-30).all())
                    else:
                        y, _ = M.conv(cl(act), w[r + "1.weight"], w[r + "1.bias"], 7, dil=(1, 3, 9)[k - 1])
                        y = M.snake64(y, w[r + "2.alpha"].flatten())
                        got, _ = M.conv(y, w[r + "3.weight"], w[r + "3.bias"], 1, skip=cl(raw))
            tol = 2e-5 * float(exp_raw.abs().max()) + (2e-2 if bf and s > 0 and (s - 1) % 4 else 0.0)  # bf16 units: an inner flip moves the sum
            assert got.shape == cl(exp_raw).shape and float((got - cl(exp_raw)).abs().max()) <= tol, (o.precision, s)
            act, raw = exp_act, exp_raw
        acc, wav, emitted = M.conv_out(act.transpose(1, 2), w[f"{d}{n + 2}.weight"], w[f"{d}{n + 2}.bias"], 0, act.shape[2])
        assert emitted.all() and float((wav - o.final_stage(act)[:, 0]).abs().max()) <= 2e-6


def test_conv_out_emit_ranges():
    g = torch.Generator().manual_seed(5)
    x, w, b = _ints(g, (2, 20, 8), -4, 4, 0.25), _ints(g, (1, 8, 7), -3, 3, 0.125), _ints(g, (1,), -8, 8, 0.125)
    acc, wav, emitted = M.conv_out(x, w, b, [3, 0], [18, 7], lens=[5, 9], len_mul=2)
    assert emitted[0].nonzero().flatten().tolist() == list(range(3, 10)) and emitted[1].nonzero().flatten().tolist() == list(range(0, 7))
    xz = x.clone()
    xz[0, 10:], xz[1, 18:] = 0, 0
    assert torch.equal(acc, F.conv1d(xz.transpose(1, 2), w, b, padding=3)[:, 0])


def test_conv_in_is_conv1d_of_the_waveform():
    g = torch.Generator().manual_seed(6)
    wave, w, b = _ints(g, (2, 33), -8, 8, 0.125), _ints(g, (16, 1, 7), -3, 3, 0.25), _ints(g, (16,), -8, 8, 0.125)
    alpha = torch.tensor([0.25, 0.3125, 0.375, 0.5] * 4)
    raw, act = M.conv_in(wave, w, b, alpha)
    assert torch.equal(raw, F.conv1d(wave[:, None], w, b, padding=3).transpose(1, 2))
    assert float((act - DA.snake1d(raw, alpha.to(F64))).abs().max()) <= 1e-7  # inv is the fp32 1 / (alpha + 1e-9) here


def test_rvq_table_gather_and_encode_match_the_oracle():
    spec, o32, _ = _tiny()
    K, w = spec.num_codebooks, o32.w
    g = torch.Generator().manual_seed(12)
    codes = torch.randint(0, spec.codebook_size, (2, K, 7), generator=g)
    q = "quantizer.quantizers.%d."
    table = torch.stack([M.rvq_table(w[q % i + "codebook.weight"], w[q % i + "out_proj.weight"], w[q % i + "out_proj.bias"]) for i in range(K)])
    z, written = M.rvq_gather(codes, table, spec.codebook_size)
    assert written.all() and float((z.transpose(1, 2) - o32.from_codes(codes)).abs().max()) <= 1e-5
    # clamping of ids and the ragged rows
    wild = codes.clone()
    wild[0, 0, 0], wild[1, 2, 3] = -5, spec.codebook_size + 7
    fixed = codes.clone()
    fixed[0, 0, 0], fixed[1, 2, 3] = 0, spec.codebook_size - 1
    z2, written = M.rvq_gather(wild, table, spec.codebook_size, lens=[7, 4])
    assert torch.equal(z2, M.rvq_gather(fixed, table, spec.codebook_size)[0]) and written.sum(1).tolist() == [7, 4]
    # the stream variant reads tab[slot][k][start + t]
    tab = torch.randint(0, spec.codebook_size, (3, K, 16), generator=g)
    zs, ws = M.rvq_gather_stream(tab, [2, 0], [5, 1], [4, 7], 16, table, spec.codebook_size, 7)
    assert torch.equal(zs[0, :4], M.rvq_gather(tab[2:3, :, 5:9], table, spec.codebook_size)[0][0]) and ws.sum(1).tolist() == [4, 7]
    # encode: the oracle's codes wherever its top-2 margin is clear of fp32 noise
    zlat = o32.from_codes(codes) + 0.05 * torch.randn(2, spec.latent_dim, 7, generator=g)
    ref, margin = o32.quantize(zlat)
    got, gaps = M.rvq_encode(zlat.transpose(1, 2), torch.stack([w[q % i + "in_proj.weight"][:, :, 0] for i in range(K)]),
                             torch.stack([w[q % i + "in_proj.bias"] for i in range(K)]), torch.stack([w[q % i + "codebook.weight"] for i in range(K)]),
                             torch.stack([w[q % i + "out_proj.weight"][:, :, 0] for i in range(K)]), torch.stack([w[q % i + "out_proj.bias"] for i in range(K)]), K)
    ok = margin >= 1e-4
    assert ok.any() and torch.equal(got.permute(0, 2, 1)[ok], ref.permute(0, 2, 1)[ok])
    # nq stages are a prefix of all stages; ties go to the lowest index
    assert torch.equal(M.rvq_encode(zlat.transpose(1, 2), *_enc_args(w, K), 4)[0], got[:, :4])
    cb = torch.stack([w[q % 0 + "codebook.weight"]]).clone()
    cb[0, 300] = cb[0, 17]
    zz = (cb[0, 17] @ torch.linalg.pinv(w[q % 0 + "in_proj.weight"][:, :, 0]).t())[None, None]
    one = M.rvq_encode(zz, torch.stack([w[q % 0 + "in_proj.weight"][:, :, 0]]), torch.zeros(1, spec.codebook_dim), cb,
                       torch.stack([w[q % 0 + "out_proj.weight"][:, :, 0]]), torch.stack([w[q % 0 + "out_proj.bias"]]), 1)
    assert int(one[0][0, 0, 0]) == 17 and float(one[1][0, 0, 0]) == 0.0


def _enc_args(w, K):
    q = "quantizer.quantizers.%d."
    return (torch.stack([w[q % i + "in_proj.weight"][:, :, 0] for i in range(K)]), torch.stack([w[q % i + "in_proj.bias"] for i in range(K)]),
            torch.stack([w[q % i + "codebook.weight"] for i in range(K)]), torch.stack([w[q % i + "out_proj.weight"][:, :, 0] for i in range(K)]),
            torch.stack([w[q % i + "out_proj.bias"] for i in range(K)]))
