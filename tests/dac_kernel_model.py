"""Float64 restatement of what the DAC codec's kernels compute (parler_tts_amd/csrc/ptts_dac_kernels.h), one function per launch the harness
(tests/dac_harness.py) can make. Plain torch / numpy; tests/test_dac_kernel_model_cpu.py pins it against torch.nn.functional and the oracle's stage
functions, tests/test_dac_kernels_gpu.py compares the kernels with it.

Layout as the kernels': activations channels-last [B][T][C]; weights in the checkpoint's layout, [Cout][Cin][k] and [Cin][Cout][k] for a transposed
convolution. Ragged `lens`: utterance b has min(T, max(lens[b], 0) * len_mul) valid input rows; rows beyond read as zeros whatever they hold, outputs
beyond are NOT written - every function returns the values and a boolean mask [B][Tout] of the rows the kernel writes.

The Snake is x + inv * sin(alpha * x)^2 with inv = fp32(1 / (alpha + 1e-9)) as inv_alpha_kernel stores it; `snake=` lets the GPU test substitute
the device's own fp32 evaluation (the dh_snake probe) where the model has to reproduce a rounding."""
import numpy as np
import torch

F64 = torch.float64


def inv_alpha(alpha):
    """inv_alpha_kernel: 1.0f / (alpha + 1e-9f), correctly rounded fp32."""
    a = np.asarray(alpha, dtype=np.float32)
    return torch.from_numpy((np.float32(1.0) / (a + np.float32(1e-9))).astype(np.float32))


def snake64(v, alpha, inv=None):
    """float64 Snake of v [..., C] with the fp32 parameters the kernels hold."""
    inv = inv_alpha(alpha) if inv is None else inv
    a, i = alpha.to(F64), inv.to(F64)
    return v.to(F64) + i * torch.sin(a * v.to(F64)) ** 2


def rb(x):
    """fp32 -> bf16 round-to-nearest-even -> fp32 (f32_to_bf16 / v_cvt_pk_bf16_f32)."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def bf16_bits(x):
    return x.to(torch.float32).to(torch.bfloat16).view(torch.int16)


def valid_rows(T, lens, len_mul, B):
    """valid_rows(): min(T, max(lens[b], 0) * len_mul) per utterance, T without lens."""
    if lens is None:
        return [T] * B
    return [min(T, max(int(n), 0) * len_mul) for n in lens]


def _masked_input(x, Tv):
    x = x.to(F64).clone()
    for b, n in enumerate(Tv):
        x[b, n:] = 0.0  # rows beyond the utterance read as the zero padding (NaN poison included)
    return x


def conv(x, w, bias, ksize, dil=1, stride=1, transposed=False, pad=-1, lens=None, len_mul=1, skip=None):
    """Conv1d / ConvTranspose1d as conv_mfma_kernel / conv_lds_kernel evaluate it: out[t][co] = bias[co] + sum_{tap, ci} W * x[t * stride + off(tap)][ci]
    (+ skip). A stride-s transposed convolution is s interleaved 2-tap phase convolutions (kernel size 2s, padding ceil(s / 2)).
    -> (raw [B][Tout][Cout] float64, written [B][Tout] bool)."""
    B, Tin, Cin = x.shape
    Tv = valid_rows(Tin, lens, len_mul, B)
    xm = _masked_input(x, Tv)
    w = w.to(F64)

    def rows(t_idx):  # xm rows at the integer indices t_idx (a tensor), zeros outside [0, Tin)
        ok = (t_idx >= 0) & (t_idx < Tin)
        return xm[:, t_idx.clamp(0, Tin - 1)] * ok.to(F64)[None, :, None]

    if not transposed:
        p = pad if pad >= 0 else (ksize - 1) * dil // 2
        Tn = (Tin + 2 * p - ksize) // stride + 1 if stride > 1 else Tin
        assert stride == 1 or lens is None, "the strided convolutions (encoder) never run ragged"
        Cout = w.shape[0]
        out = torch.zeros(B, Tn, Cout, dtype=F64)
        j = torch.arange(Tn)
        for tap in range(ksize):
            out += torch.einsum("btc,oc->bto", rows(j * stride + tap * dil - p), w[:, :, tap])
        Tout, Tw = Tn, Tv if lens is not None else [Tn] * B
    else:
        s = stride
        assert ksize == 2 * s
        p = (s + 1) // 2
        Cout = w.shape[1]
        out = torch.zeros(B, Tin * s, Cout, dtype=F64)
        j = torch.arange(Tin)
        for ph in range(s):
            r, c0 = (ph + p) % s, (ph + p) // s
            out[:, ph::s] = torch.einsum("btc,co->bto", rows(j + c0), w[:, :, r]) + torch.einsum("btc,co->bto", rows(j + c0 - 1), w[:, :, r + s])
        Tout, Tw = Tin * s, [n * s for n in Tv]
    out += bias.to(F64)
    if skip is not None:
        out += skip.to(F64)
    written = torch.zeros(B, Tout, dtype=torch.bool)
    for b, n in enumerate(Tw):
        written[b, :n] = True
    return out, written


def act_of(raw, alpha, bf16, snake=None):
    """The epilogue's activation output: Snake of the fp32 result, rounded to bf16 unless the layer feeds the final convolution (bf16=False).
    `snake(v32, alpha)` -> fp32 replaces the float64 evaluation rounded to fp32."""
    v32 = raw.to(torch.float32)
    s = snake(v32, alpha) if snake is not None else snake64(v32, alpha).to(torch.float32)
    return rb(s) if bf16 else s


def resunit(x, w7, b7, alpha7, w1, b1, alpha1, skip, dil, lens=None, len_mul=1, act_f32=False, alpha_in=None, snake=None):
    """resunit_lds_kernel: y = bf16(Snake_a7(conv_k7_dil(x) + b7)); raw = skip + conv_k1(y) + b1; act = Snake_a1(raw) (bf16 unless act_f32).
    alpha_in: an XIN unit - x is the fp32 stream and the unit's input is bf16(Snake_alpha_in(x)).
    -> dict(y_pre, y, raw, act, written)."""
    B, T, C = x.shape
    Tv = valid_rows(T, lens, len_mul, B)
    if alpha_in is not None:
        x = act_of(_masked_input(x, Tv), alpha_in, True, snake)
    y_pre, written = conv(x, w7, b7, 7, dil=dil, lens=lens, len_mul=len_mul)
    y = act_of(y_pre, alpha7, True, snake)
    # the k1 GEMM reads the y tile of the workgroup's own rows only: rows beyond the utterance are computed but never stored
    raw = torch.einsum("btc,oc->bto", y.to(F64), w1.to(F64)[:, :, 0]) + b1.to(F64) + _masked_input(skip, Tv)
    act = act_of(raw, alpha1, not act_f32, snake)
    return dict(y_pre=y_pre, y=y, raw=raw, act=act, written=written)


def conv_out(x, w, bias, skip, t_end, lens=None, len_mul=1):
    """conv_out_tanh*_kernel: tanh(Conv1d(C -> 1, k7, pad 3)) of x [B][T][C]; samples [skip[b], min(t_end[b], Tv[b])) of utterance b go to out[b][t - skip[b]].
    skip / t_end: ints or per-row lists. -> (pre-tanh accumulator [B][T] float64, tanh of it, emitted [B][T] bool)."""
    B, T, C = x.shape
    Tv = valid_rows(T, lens, len_mul, B)
    acc, _ = conv(x, w, bias, 7, lens=lens, len_mul=len_mul)
    acc = acc[:, :, 0]
    sk = [skip] * B if isinstance(skip, int) else list(skip)
    te = [t_end] * B if isinstance(t_end, int) else list(t_end)
    emitted = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        emitted[b, max(sk[b], 0):max(min(te[b], Tv[b]), 0)] = True
    return acc, torch.tanh(acc), emitted


def conv_in(wave, w, bias, alpha):
    """conv_in_kernel: Conv1d(1 -> C, k7, pad 3) of wave [B][L] -> (raw [B][L][C], exact-sinf Snake of it in float64)."""
    raw, _ = conv(wave[:, :, None], w, bias, 7)
    return raw, snake64(raw.to(torch.float32), alpha)


def rvq_table(cb, w, bias):
    """rvq_table_kernel: table[code][c] = bias[c] + sum_d W[c][d] * codebook[code][d]."""
    return cb.to(F64) @ w.to(F64).reshape(w.shape[0], -1).t() + bias.to(F64)


def rvq_gather(codes, table, ncodes, lens=None, bf16=False):
    """rvq_gather_kernel: z[b][t] = sum_i table[i][clamp(codes[b][i][t], 0, ncodes - 1)] for t < lens[b]. table [K][ncodes][latent]; codes [B][K][T].
    -> (z [B][T][latent] float64 (bf16-rounded values if bf16), written [B][T])."""
    B, K, T = codes.shape
    c = codes.clamp(0, ncodes - 1)
    z = torch.zeros(B, T, table.shape[2], dtype=F64)
    for i in range(K):
        z += table[i].to(F64)[c[:, i]]
    written = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        written[b, :T if lens is None else max(0, min(T, int(lens[b])))] = True
    return (rb(z).to(F64) if bf16 else z), written


def rvq_gather_stream(tab, slot, start, lens, cap, table, ncodes, T, bf16=False):
    """rvq_gather_kernel<STREAM>: row b reads codes tab[slot[b]][k][start[b] + t], t < lens[b]. tab [slots][K][cap]."""
    B = len(slot)
    K = tab.shape[1]
    codes = torch.zeros(B, K, T, dtype=torch.int64)
    for b in range(B):
        n = max(0, min(T, int(lens[b])))
        codes[b, :, :n] = tab[slot[b], :, start[b]:start[b] + n]
    return rvq_gather(codes, table, ncodes, lens, bf16)


def cb_normalize(cb):
    """cb_normalize_kernel in float64: rows c / max(||c||, 1e-12) and their squared norms."""
    cb = cb.to(F64)
    n = cb / cb.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return n, (n * n).sum(1)


def rvq_encode(z, in_w, in_b, cb, out_w, out_b, nq):
    """rvq_encode_kernel in float64: per frame and stage p = in_proj(residual); idx = argmax_c -(|e|^2 - 2 e.c + |c|^2) over the normalised codebook
    (LOWEST index on ties); residual -= out_proj(p + (codebook[idx] - p)). z [B][T][latent]; in_w [K][cdim][latent]; cb [K][codes][cdim];
    out_w [K][latent][cdim]. -> (codes [B][nq][T], top-2 score gap [B][nq][T])."""
    B, T, _ = z.shape
    res = z.to(F64).clone()
    codes = torch.zeros(B, nq, T, dtype=torch.int64)
    gaps = torch.zeros(B, nq, T, dtype=F64)
    for i in range(nq):
        p = res @ in_w[i].to(F64).t() + in_b[i].to(F64)
        e = p / p.norm(dim=2, keepdim=True).clamp_min(1e-12)
        cbn, cbn_sq = cb_normalize(cb[i])
        score = -(((e * e).sum(2, keepdim=True) - 2.0 * (e @ cbn.t())) + cbn_sq)
        best = score.max(dim=2, keepdim=True).values
        idx = (score == best).to(torch.int64).argmax(dim=2)  # first (lowest) index holding the maximum
        top2 = score.topk(2, dim=2).values
        codes[:, i], gaps[:, i] = idx, top2[..., 0] - top2[..., 1]
        c = cb[i].to(F64)[idx]
        q = p + (c - p)
        res = res - (q @ out_w[i].to(F64).t() + out_b[i].to(F64))
    return codes, gaps
