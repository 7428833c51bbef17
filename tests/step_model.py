"""TEST INFRASTRUCTURE ONLY - float64 restatement of the contracts of the batched decode-step kernels (csrc/ptts_lm_kernels.h: rows_prep_kernel,
gemm_strip_kernel's prologues and epilogues, lnproj_fused_kernel, xattn_fused_kernel; csrc/ptts_lm_w8.hip), on the operands as the kernels read
them. Plain torch float64 on whatever device the operands live on; no product code. The attention rules, the fragment order, the split-KV
combination, the engine-dtype rounding and the attention error bound are tests/attn_model.py's.

  LayerNorm            nn.LayerNorm over the last axis, eps 1e-5, biased variance.
  strip statistics     EPI_RESID + stats_out: per (row, 16-column strip of the updated residual row) the strip mean and the strip sum of squared
                       deviations from that mean.
  PRO_LNS              the LayerNorm whose mean / variance are the exact combination of those K / 16 partials (Chan's update: equal counts of 16).
  e4m3 strips          weight = e4m3 byte (OCP FN, oracle/fp8_oracle.py) * a power-of-two scale per output row.
  fused cross block    LN2 -> rows in the engine dtype -> q = Wq y -> RoPE on q at position P + cur_len[b] - 1 (keys not rotated) -> softmax over the
                       N description keys that the additive mask leaves (masked = -inf), query head h reads K/V head h // n_rep; a row without a
                       visible key yields 0."""
import math
import os
import sys

import torch

from attn_model import F64, LOG2E, combine_splits, decoder_attention, fo_elem_index, rope, round_engine, tolerance  # noqa: F401  (re-exported to the tests)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import fp8_oracle as FP8  # noqa: E402

EPS = 1e-5
U32 = 2.0 ** -24  # unit roundoff of fp32


def layer_norm64(x, gamma, beta, eps=EPS):
    x = x.to(F64)
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)


def strip_stats64(h):
    """h [M, N] -> [M, N / 16, 2]: (mean, sum of squared deviations) of every 16-column strip."""
    M, N = h.shape
    s = h.to(F64).view(M, N // 16, 16)
    mean = s.mean(dim=2)
    return torch.stack((mean, ((s - mean[..., None]) ** 2).sum(dim=2)), dim=2)


def combine_strip_stats64(lnstat):
    """[M, NS, 2] strip partials (16 elements each) -> (mean [M, 1], biased variance [M, 1]) of the whole rows: Chan's update, folded over equal counts."""
    st = lnstat.to(F64)
    ns = st.shape[1]
    mean = st[..., 0].mean(dim=1, keepdim=True)
    m2 = st[..., 1].sum(dim=1, keepdim=True) + 16.0 * ((st[..., 0] - mean) ** 2).sum(dim=1, keepdim=True)
    return mean, m2 / (16.0 * ns)


def lns_layer_norm64(h, lnstat, gamma, beta, eps=EPS):
    mean, var = combine_strip_stats64(lnstat)
    return (h.to(F64) - mean) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)


def gelu_erf64(u):
    u = u.to(F64)
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_bound_fp32(u):
    """Per element, what an fp32 evaluation of 0.5 u (1 + erf(u / sqrt 2)) may differ from float64 by, as an fp32 value (EPI_GELU, the fp32
    intermediate the strips write at up to 8 rows; the engine-dtype outputs of EPI_GELU_WT are held to one ulp instead): the erf value carries the
    rounding of its argument (|d erf| <= 0.5 * 2^-24) and the function's own error (taken as 4 ulp at |erf| <= 1: 4 * 2^-24), 1 + erf one more
    rounding (2^-24 at values below 2); that absolute error E = 5.5 * 2^-24 is then multiplied by |u| / 2, and the two products round once each
    (2 * 2^-24 relative). For u < 0 the sum 1 + erf cancels, so in ulps of the small result the error is large (tens of ulps at u = -2.5): the
    formula's, not a kernel's. tests/test_step_model_cpu.py holds a step-by-step float32 evaluation to this bound on the GPU cases' accumulators."""
    u = u.to(F64)
    return 0.5 * u.abs() * 5.5 * U32 + 2.0 * U32 * gelu_erf64(u).abs()


def ulp(v, bf16):
    """Spacing of the engine dtype at |v| (float64 tensor)."""
    a = v.abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - (7 if bf16 else 23))


def e4m3_rows(W):
    """W [N, K] -> (bytes uint8 [N, K], scale fp32 [N], dequantised float64 [N, K]): the product's weight-only e4m3 mode, rounded by
    oracle/fp8_oracle.py; the bytes are those values' encodings (exact: they are representable)."""
    deq, scale = FP8.quantize_rows(W.float().cpu())
    q = deq / scale[:, None]
    b = q.to(torch.float8_e4m3fn)
    assert torch.equal(b.float(), q), "fp8_oracle produced a value e4m3 cannot hold"
    return b.view(torch.uint8), scale, deq.to(F64)


def to_fo(x, bf16, fill=float("nan")):
    """Row-major [M, K] -> the flat fragment-order buffer of ceil(M / 16) * 16 rows; the rows past M hold `fill`."""
    M, K = x.shape
    Mp = (M + 15) // 16 * 16
    buf = torch.full((Mp * K,), fill, dtype=x.dtype, device=x.device)
    buf[fo_elem_index(M, K, bf16).to(x.device).reshape(-1)] = x.reshape(-1)
    return buf


def from_fo(buf, M, K, bf16):
    """The inverse: rows [M, K] out of a flat fragment-order buffer."""
    return buf[fo_elem_index(M, K, bf16).to(buf.device)]


def ln_tolerance_fp32(x, gamma, beta, y64):
    """The fp32 LayerNorm bar of one case (a scalar): 4 x the largest error of the plain float32 torch restatement against float64 on the same
    inputs - the kernels' one-pass shifted variance and torch's two-pass variance differ in summation order and in one rsqrtf, not in kind -
    floored at 4 fp32 ulps of the case's largest |y64|. Returns (bar, error of the float32 restatement)."""
    xf = x.float().cpu()
    y32 = torch.nn.functional.layer_norm(xf, (xf.shape[-1],), gamma.float().cpu(), beta.float().cpu(), EPS)
    err = float((y32.to(F64) - y64.cpu()).abs().max())
    floor = 4.0 * float(ulp(y64.abs().max().reshape(1).cpu(), False))
    return max(4.0 * err, floor), err


def ln_rows_bound(y64, bar, bf16):
    """Per element of the exposed normalised rows: the fp32 bar; a bf16 row adds one bf16 ulp of the float64 value."""
    return ulp(y64, True) + bar if bf16 else torch.full_like(y64, bar)


def strip_stats_bounds(h):
    """(float64 statistics [M, N / 16, 2] of the rows h, bound on the mean, bound on M2).
    Mean: 16 fp32 additions of values up to max|h| of the strip. M2: the same relative bound on sum d^2; the kernel's deviations are taken from ITS
    mean, off by delta <= the mean's bound, and sum (d + delta)^2 = sum d^2 + 16 delta^2 because sum d = 0."""
    M, N = h.shape
    ref = strip_stats64(h)
    bm = 16 * U32 * h.to(F64).abs().view(M, N // 16, 16).amax(dim=2)
    return ref, bm, 16 * U32 * ref[..., 1] + 16 * bm * bm


def combine_tolerance(part, stats, bf16):
    """(attn_model.combine_splits of the partials, its error bound): attn_model.tolerance for the combine alone - no dot product (the spread of the
    split maxima takes absdot's place: the exponent's argument is one fp32 subtraction of that size), no keys, S terms."""
    M, S, K = part.shape
    nh = K // 64
    ref = combine_splits(part, stats)
    m = stats[..., 0].to(F64)
    top = m.amax(dim=1, keepdim=True)
    spread = (top - torch.where(torch.isinf(m), top.expand_as(m), m)).amax(dim=1)
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - torch.where(torch.isinf(top), torch.zeros_like(top), top)))
    den = (w * stats[..., 1].to(F64)).sum(dim=1)
    vmax = ((w[..., None] * part.to(F64).view(M, S, nh, 64).abs()).sum(dim=1) / den.clamp_min(1e-300)[..., None]).amax(dim=2)
    return ref, tolerance(spread, vmax, torch.zeros(M, nh, dtype=torch.int64), ref, S=S, NW=0, bf16=bf16)


def flip_share(y, y64):
    """Share of the bf16 elements of y that differ from round-to-nearest-even of y64."""
    return float((y.to(F64) != round_engine(y64, True).to(y.device)).double().mean())


def gemm_bound(W, x):
    """Per element of x W^T, the fp32 accumulation bound of tests/test_gemm_kernels_gpu.py: K 2^-24 sum_k |W||x|."""
    return W.shape[1] * U32 * (x.abs().to(F64) @ W.abs().to(F64).t())


def cross_block64(x, gamma, beta, Wq, K, V, *, n_rep, N, P, cur_len, mask, scale, cos, sin, bf16, y=None):
    """xattn_fused_kernel on x [B, H] fp32 rows: Wq [H, H] and K, V [B, kv_heads, cap, 64] float64 as the kernel reads them (engine-dtype values).
    y: the staged rows, if known, in place of the engine-dtype rounding of LayerNorm(x). Returns attn_model.decoder_attention's dict (out
    [B, H], absdot, vmax, count, ...) plus q [B, H] and y."""
    B, H = x.shape
    if y is None:
        y = round_engine(layer_norm64(x, gamma, beta).cpu(), bf16)
    q = y.to(F64).cpu() @ Wq.to(F64).cpu().t()
    r = decoder_attention(q.view(B, H // 64, 64), K.cpu(), V.cpu(), Q=1, n_rep=n_rep, P=P, N=N, cur_len=cur_len if cos is not None else None,
                          cross=True, mask=mask, scale=scale, cos=cos, sin=sin, bf16=bf16)
    r["q"], r["y"] = q, y
    return r


def xattn_tolerance(m, Wq, Kc, *, N, n_rep, scale, bf16):
    """attn_model.tolerance for the fused cross block on the rows y it really staged (m = cross_block64(..., y=y)), plus what the q projection
    itself rounds: q_d is an fp32 sum of the nnz non-zero products of row d of Wq (zero products add exactly), so |dq_d| <= nnz 2^-24 sum_k |W_dk||y_k|;
    the rotation mixes two q elements with |cos| + |sin| <= 2, and the score error sum_d |dq_d| max_t |k_td| (in the score's log2 units) joins
    tolerance's own dot-product term. Nothing here comes from a LayerNorm bound: y is the kernel's own LayerNorm (rows_prep_kernel<PRO_LN>)."""
    B, K = m["y"].shape
    nnz = int((Wq != 0).sum(dim=1).max())
    dq = nnz * U32 * (m["y"].abs().to(F64) @ Wq.abs().to(F64).t())                                       # [B, K]
    kabs = Kc[:, :, :N].abs().amax(dim=2).repeat_interleave(n_rep, dim=1)                              # [B, heads, 64]
    dscore = scale * LOG2E * 2.0 * (dq.reshape(B, K // 64, 64) * kabs).sum(dim=2)
    return tolerance(m["absdot"] + dscore / (66.0 * U32), m["vmax"], m["count"], m["out"], S=1, NW=8, bf16=bf16)
