"""TEST INFRASTRUCTURE ONLY - float64 restatement of the contracts of the attention kernels (csrc/ptts_lm_kernels.h: attn_kernel,
prefill_attn_kernel, prefill_attn_mfma_kernel, kv_append_kernel; csrc/ptts_t5_kernels.h: t5_attn_kernel, t5_attn_mfma_kernel), on the operands
as the kernels read them: cache rows already in the engine dtype (or e4m3 x scale), q in fp32. Everything here is float64 torch on the CPU.

Decode / prefill attention (attn_kernel's rules; the prefill kernels promise the same function at S = 1):
  pos = P + cur_len[b] - 1 + qi (decode) or qi (prefill); L = N (cross) or pos + 1 (self); the mask applies to positions < P (self) or < L (cross);
  query head h reads K/V head h // n_rep; RoPE from the SUPPLIED tables on q (also in the cross block) and on the appended k; softmax over the
  visible keys only, a row without one yields 0. Scores are in log2 units: (rot(q) * scale * log2 e) . k.
  Split-KV: key t belongs to split ((t // RPI) % (S * NW)) // NW (RPI = 8 rows per wave instruction for bf16 / e4m3, 4 for fp32); a split hands
  over the unnormalised sum relative to ITS maximum and (max, sumexp) in log2 units; an empty split has max = -inf and weight 0."""
import math

import torch

LOG2E = 1.44269504088896340736
FLT_MAX = 3.402823466e38
E4M3_MAX = 448.0
F64 = torch.float64


def rpi(bf16):
    return 8 if bf16 else 4


def span(S, NW, bf16):
    """Positions one loop iteration of attn_kernel covers: S workgroups x NW waves x 8 row groups in flight x RPI rows."""
    return S * NW * 8 * rpi(bf16)


def rotate_half(x):
    return torch.cat((-x[..., 32:], x[..., :32]), dim=-1)


def rope(x, cos, sin, pos):
    """x [..., 64] at position(s) pos (int or index tensor broadcasting against x's leading axes): x * cos + rotate_half(x) * sin."""
    if cos is None:
        return x.to(F64)
    x = x.to(F64)
    return x * cos.to(F64)[pos] + rotate_half(x) * sin.to(F64)[pos]


def round_engine(x, bf16):
    """RNE into the engine dtype, returned as float64 (fp32 first: the kernels hold the value in fp32 before they store it)."""
    x = x.to(torch.float32)
    return (x.bfloat16() if bf16 else x).to(F64)


def kv8_quantize(x):
    """Rows of 64 (last axis) -> (e4m3 bytes as uint8, scale fp32 [..., 1]): scale = 2^ceil(log2(max|x| / 448)) (1 for an all-zero row) from the
    exponent of max|x| / 448, bytes = RNE e4m3 of x / scale (torch's float8_e4m3fn cast)."""
    x = x.to(torch.float32)
    amax = x.abs().amax(dim=-1, keepdim=True)
    m, e = torch.frexp(amax / torch.tensor(E4M3_MAX, dtype=torch.float32))
    e = torch.where(m == 0.5, e - 1, e)
    scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax))
    return (x / scale).to(torch.float8_e4m3fn).view(torch.uint8), scale


def kv8_dequantize(bytes_u8, scale):
    return bytes_u8.view(torch.float8_e4m3fn).to(F64) * scale.to(F64)


def fo_elem_index(M, K, bf16):
    """[M, K] int64: where element (m, k) of a row-major activation sits in MFMA B-fragment order (fo_vec_index of ptts_lm_kernels.h):
    X_fo[M/16 tiles][K/KT fragments][64 lanes][16 B], lane l of fragment (mt, t) = row mt*16 + (l & 15), k = t*KT + (l >> 4)*EPL + e.
    The buffer holds ceil(M / 16) * 16 * K elements."""
    KT, EPL = (32, 8) if bf16 else (16, 4)
    m = torch.arange(M)[:, None]
    k = torch.arange(K)[None, :]
    vec = ((m >> 4) * (K // KT) + k // KT) * 64 + ((k % KT) // EPL) * 16 + (m & 15)
    return vec * EPL + k % EPL


def append_rows(knew, vnew, cos, sin, pos, bf16, kv8):
    """The cache rows an append writes: knew / vnew [..., 64] fp32 at position(s) pos -> dict with the rows as attention then sees them (float64)
    and, for the e4m3 cache, bytes and scales."""
    k = rope(knew, cos, sin, pos).to(torch.float32)
    v = vnew.to(torch.float32)
    if kv8:
        kb, ks = kv8_quantize(k)
        vb, vs = kv8_quantize(v)
        return dict(k=kv8_dequantize(kb, ks), v=kv8_dequantize(vb, vs), kbytes=kb, vbytes=vb, kscale=ks[..., 0], vscale=vs[..., 0])
    return dict(k=round_engine(k, bf16), v=round_engine(v, bf16))


def decoder_attention(q, K, V, *, Q, n_rep, P, N, cur_len, cross, mask, scale, cos, sin, bf16, S=1, NW=4, new_k=None, new_v=None, qscale=None):
    """q [B*Q, heads, 64] fp32; K, V [B, kv_heads, cap, 64] float64 as the cache holds them (rows no query may see can hold anything);
    cur_len [B] ints or None (prefill); mask [B, mask_ld] (1 = keep) or None; new_k / new_v [B, kv_heads, 64] float64: the appended row as
    attention sees it (decode self-attention, Q = 1), placed at pos before anything is read. qscale: the factor on the rotated query in place of
    scale * log2 e (the exact tests pass the power of two that the kernel's fp32 product gives).
    Returns float64 tensors: out [rows, heads*64], num / den (out = num / den relative to the row's maximum), part [rows, S, heads*64],
    stats [rows, S, heads, 2], and what the error bound needs: absdot (max over visible keys of sum_d |qhat_d k_td|), vmax, count; pos [rows]."""
    rows, nheads, _ = q.shape
    B = rows // Q
    H = nheads * 64
    R = rpi(bf16)
    out = torch.zeros(rows, H, dtype=F64)
    num = torch.zeros(rows, H, dtype=F64)
    den = torch.zeros(rows, nheads, dtype=F64)
    part = torch.zeros(rows, S, H, dtype=F64)
    stats = torch.zeros(rows, S, nheads, 2, dtype=F64)
    absdot = torch.zeros(rows, nheads, dtype=F64)
    vmax = torch.zeros(rows, nheads, dtype=F64)
    count = torch.zeros(rows, nheads, dtype=torch.int64)
    poss = torch.zeros(rows, dtype=torch.int64)
    scores = {}
    qs = float(scale) * LOG2E if qscale is None else qscale
    for b in range(B):  # the Q rows of an utterance at once: hidden keys are excluded by a visibility matrix, never by what their rows hold
        r0 = b * Q
        pos = (P + int(cur_len[b]) - 1 if cur_len is not None else 0) + torch.arange(Q)
        poss[r0:r0 + Q] = pos
        Lr = torch.full((Q,), N) if cross else pos + 1
        Lmax = int(Lr.max())
        t = torch.arange(Lmax)
        vis = t[None, :] < Lr[:, None]                                   # [Q, Lmax]
        if mask is not None:
            ml = Lr if cross else torch.clamp(Lr, max=P)                 # flags count for positions < P (self) or < L (cross)
            flags = torch.ones(Lmax, dtype=torch.bool)
            n = min(Lmax, mask.shape[1])
            flags[:n] = mask[b, :n] != 0
            vis &= (t[None, :] >= ml[:, None]) | flags[None, :]
        Kb, Vb = K[b, :, :Lmax], V[b, :, :Lmax]
        if new_k is not None:
            Kb, Vb = Kb.clone(), Vb.clone()
            Kb[:, int(pos[0])], Vb[:, int(pos[0])] = new_k[b], new_v[b]
        hid = ~vis.any(dim=0)                                            # keys no row of the utterance sees may hold NaN: taken out, not multiplied
        Kh = torch.where(hid[None, :, None], torch.zeros((), dtype=F64), Kb).repeat_interleave(n_rep, dim=0)  # [heads, Lmax, 64]: head h reads h // n_rep
        Vh = torch.where(hid[None, :, None], torch.zeros((), dtype=F64), Vb).repeat_interleave(n_rep, dim=0)
        qh = rope(q[r0:r0 + Q], cos, sin, pos[:, None].expand(Q, nheads)) * qs                                 # [Q, heads, 64]
        v3 = vis[:, None, :]
        sc = torch.where(v3, torch.einsum("hkd,qhd->qhk", Kh, qh), torch.full((), -math.inf, dtype=F64))
        absdot[r0:r0 + Q] = torch.where(v3, torch.einsum("hkd,qhd->qhk", Kh.abs(), qh.abs()), torch.zeros((), dtype=F64)).amax(dim=2)
        vmax[r0:r0 + Q] = torch.where(v3, Vh.abs().amax(dim=2)[None], torch.zeros((), dtype=F64)).amax(dim=2)
        count[r0:r0 + Q] = vis.sum(dim=1)[:, None]
        split_of = ((t // R) % (S * NW)) // NW

        def softmax_terms(sel):
            """(max, p, sum p, p V) over the keys `sel` [Q, 1, Lmax] of every (row, head); rows without such a key: (-inf, 0, 0, 0)."""
            s_ = torch.where(sel, sc, torch.full((), -math.inf, dtype=F64))
            m_ = s_.amax(dim=2)
            p_ = torch.where(sel, torch.exp2(s_ - torch.where(torch.isinf(m_), torch.zeros_like(m_), m_)[..., None]), torch.zeros((), dtype=F64))
            return m_, p_.sum(dim=2), torch.einsum("qhk,hkd->qhd", p_, Vh)

        _, l_, n_ = softmax_terms(v3)
        num[r0:r0 + Q], den[r0:r0 + Q] = n_.reshape(Q, H), l_
        out[r0:r0 + Q] = torch.where(l_[..., None] > 0, n_ / l_.clamp_min(1e-300)[..., None], torch.zeros_like(n_)).reshape(Q, H)
        for s in range(S):
            m_, l_, n_ = softmax_terms(v3 & (split_of == s)[None, None, :])
            part[r0:r0 + Q, s], stats[r0:r0 + Q, s, :, 0], stats[r0:r0 + Q, s, :, 1] = n_.reshape(Q, H), m_, l_
        for qi in range(Q):
            if bool(vis[qi].any()):
                scores[r0 + qi] = (t[vis[qi]], sc[qi][:, vis[qi]])
    return dict(out=out, num=num, den=den, part=part, stats=stats, absdot=absdot, vmax=vmax, count=count, pos=poss, scores=scores)


def combine_splits(part, stats):
    """part [rows, S, heads*64], stats [rows, S, heads, 2] (max, sumexp in log2 units) -> the normalised output [rows, heads*64]; a row whose
    splits are all empty yields 0."""
    rows, S, H = part.shape
    nheads = H // 64
    m = stats[..., 0].to(F64)                                   # [rows, S, heads]
    M = m.amax(dim=1, keepdim=True)
    w = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), torch.exp2(m - torch.where(torch.isinf(M), torch.zeros_like(M), M)))
    lsum = (w * stats[..., 1].to(F64)).sum(dim=1)               # [rows, heads]
    o = (w[..., None] * part.to(F64).view(rows, S, nheads, 64)).sum(dim=1)
    return torch.where(lsum[..., None] > 0, o / lsum.clamp_min(1e-300)[..., None], torch.zeros_like(o)).reshape(rows, H)


def t5_attention(qkv, bias, bias_zero, mask):
    """qkv [B, N, 3, heads, 64] fp32 (q, k, v), bias [heads, bias_ld] with entry (key - query) + bias_zero, mask [B, N] (1 = keep) or None.
    No scale; a masked key has the score -FLT_MAX, so a fully masked row is uniform over all N keys; keys >= N do not exist.
    Returns out = num / den [B, N, heads*64] float64 (den [B, N, heads], relative to the row's maximum), scores [B, heads, N, N] and absdot / vmax [B, N, heads] for the error bound (natural-log units)."""
    B, N, _, nheads, _ = qkv.shape
    x = qkv.to(F64)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)  # [B, heads, N, 64]
    rel = torch.arange(N)[None, :] - torch.arange(N)[:, None] + bias_zero  # [query, key]
    bb = bias.to(F64)[:, rel]                                              # [heads, N, N]
    sc = q @ k.transpose(2, 3) + bb[None]
    absdot = q.abs() @ k.abs().transpose(2, 3) + bb[None].abs()
    if mask is not None:
        sc = torch.where(mask[:, None, None, :] != 0, sc, torch.full_like(sc, -FLT_MAX))
    p = torch.exp(sc - sc.amax(dim=-1, keepdim=True))
    num, den = p @ v, p.sum(dim=-1)                                        # [B, heads, N, 64], [B, heads, N]
    out = (num / den[..., None]).transpose(1, 2).reshape(B, N, nheads * 64)
    return dict(out=out, num=num.transpose(1, 2).reshape(B, N, nheads * 64), den=den.transpose(1, 2), absdot=absdot.amax(dim=-1).transpose(1, 2),
                vmax=v.abs().amax(dim=(2, 3))[:, None, :].expand(B, N, nheads), scores=sc)


# ---- the derived error bound of the random-data tests -------------------------------------------------------------------------------------
def tolerance(absdot, vmax, count, out, *, S, NW, bf16, log2_units=True):
    """Per element of out [..., heads*64], from float64-side quantities only (absdot, vmax, count: [..., heads]):
      delta = 66 * 2^-24 * max_t sum_d |qhat_d k_td|       the fp32 dot product of 64 terms + the rotation and scale roundings, in the score's units
      eps_p = 2 * ln2 * delta + 4 * 2^-24                  the exponent's argument on numerator and running maximum + the exponential at ~1 ulp
                                                           (T5: scores in natural-log units, so the factor ln2 is 1)
      tol   = max|V_visible| * (2 * eps_p + (L_visible + S + NW + 8) * 2^-24)
    A bf16 output adds its own rounding: bf16 carries 8 significant bits, so RNE moves a value x in [2^e, 2^(e+1)) by at most half an ulp =
    2^(e-8) <= 2^-8 |x|, and the value rounded is the kernel's, within tol of o: + 2^-8 (|o| + tol). (2^-9 |o| is the bound only at the top of a
    binade: a plain fp32 evaluation rounded to bf16 already exceeds it by up to 1.8 x on these inputs, tests/test_attn_model_cpu.py.)"""
    u = 2.0 ** -24
    delta = 66.0 * u * absdot.to(F64)
    eps_p = 2.0 * (math.log(2.0) if log2_units else 1.0) * delta + 4.0 * u
    t = vmax.to(F64) * (2.0 * eps_p + (count.to(F64) + S + NW + 8) * u)
    t = t[..., None].expand(*t.shape, 64).reshape(out.shape)
    return t + (2.0 ** -8) * (out.abs() + t) if bf16 else t
