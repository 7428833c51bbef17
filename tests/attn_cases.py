"""The inputs of the attention-kernel tests (tests/test_attn_kernels_gpu.py runs them on the GPU, tests/test_attn_model_cpu.py checks the random
ones against a plain fp32 evaluation), built on the CPU, deterministic per seed. Geometry: 4 query heads x 64, K/V heads 4 / 2 / 1, ragged
utterances, q / k / v rows wider than their data with NaN in the gap, a cache capacity just above the longest length.

Exact modes: `scale` is the fp32 number whose fp32 product with the kernels' log2(e) constant is exactly 2^-3, queries and keys are small integers,
so every score is an exact multiple of 1/8 whatever the summation order. Scores come in tiers at least 200 log2-units apart (asserted on the float64
side): the probabilities are then exactly 1 on the row's top tier and 0 below it, and the output is the exact mean of the top tier's V rows -
  uniform: q = 0, every visible key is in the top tier;
  one-hot: the rotated query is A e_j (j per query head), cold keys are 0 in those components, the hot key of a K/V head holds HOT there; a decoy
           twice as hot sits just beyond L and on masked positions (`decoy="hot"`), or those rows hold NaN (`decoy="nan"`).
Exact RoPE: tables with (cos, sin) in {(1, 0), (0, 1), (0, -1), (0.5, 0.5)}, the pattern chosen by (position + d) % 4, the same for d and d + 32:
the rotation of integers is exact and invertible in integers, so a query / new key row is given RAW such that its rotation is the wanted row."""
import numpy as np
import torch

import attn_model as AM

NH, HD = 4, 64
H = NH * HD
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
A_Q, HOT = 64.0, 32.0           # hot score A_Q * HOT / 8 = 256 log2-units above the cold tier, the decoy another 256 above
JQ = (3, 10, 17, 24)            # the component of query head h that is not zero after rotation
EXACT_QSCALE = 0.125
EXACT_SCALE = float(np.float32(0.125) / np.float32(1.44269504088896340736))
assert np.float32(np.float32(EXACT_SCALE) * np.float32(1.44269504088896340736)) == np.float32(0.125)
TIER_GAP = 200.0


def exact_rope_tables(npos):
    d = torch.arange(64) % 32
    pat = (torch.arange(npos)[:, None] + d[None, :]) % 4
    cos = torch.tensor([1.0, 0.0, 0.0, 0.5])[pat]
    sin = torch.tensor([0.0, 1.0, -1.0, 0.5])[pat]
    return cos.to(F32), sin.to(F32)


def real_rope_tables(npos):
    from oracle.decoder_oracle import rope_tables

    return rope_tables(64, 10000.0, npos)


def unrope(y, cos, sin, pos):
    """The raw row whose rotation at `pos` is y: x = (c y - s rotate_half(y)) / (c^2 + s^2)."""
    if cos is None:
        return y.clone()
    c, s = cos.to(F64)[pos], sin.to(F64)[pos]
    y = y.to(F64)
    return ((c * y - s * AM.rotate_half(y)) / (c * c + s * s)).to(y.dtype)


def _ints(gen, *shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F64)


def _round_cache(x, bf16, kv8):
    """Gaussian rows as an engine-dtype / e4m3 cache holds them (float64 values)."""
    if kv8:
        b, s = AM.kv8_quantize(x.to(F32))
        return AM.kv8_dequantize(b, s)
    return AM.round_engine(x, bf16)


class DecCase:
    """One launch of the decoder attention kernels, CPU side. Tensors: q [rows, q_ld] fp32, knew / vnew [rows, kv_ld] fp32 or None,
    K / V [B, kv_heads, cap, 64] float64 as the cache holds them BEFORE the launch (NaN where nobody may look), mask [B, mask_ld] int32 or None,
    cos / sin [npos, 64] fp32 or None; scalars as AttnArgs names them."""

    def heads_q(self):
        """q as the model takes it: [rows, heads, 64]."""
        return self.q[:, :H].reshape(-1, NH, HD)

    def new_rows(self):
        """The rows a fused append writes, as attention sees them: dict of append_rows, tensors [B, kv_heads, 64]."""
        if not self.fused_append:
            return None
        kvh = self.kv_heads
        pos = torch.tensor([self.P + c - 1 for c in self.cur_len])[:, None].expand(self.B, kvh)
        return AM.append_rows(self.knew[:, :kvh * 64].reshape(self.B, kvh, 64), self.vnew[:, :kvh * 64].reshape(self.B, kvh, 64), self.cos, self.sin, pos,
                              self.bf16, self.kv8)

    def model(self, S=1, NW=4):
        nr = self.new_rows()
        return AM.decoder_attention(self.heads_q(), self.K, self.V, Q=self.Q, n_rep=NH // self.kv_heads, P=self.P, N=self.N, cur_len=self.cur_len,
                                    cross=self.cross, mask=self.mask, scale=self.scale, cos=self.cos, sin=self.sin, bf16=self.bf16 or self.kv8, S=S, NW=NW,
                                    new_k=nr["k"] if nr else None, new_v=nr["v"] if nr else None, qscale=EXACT_QSCALE if self.exact else None)


def hot_candidates(L, S, NW, bf16):
    """Where a hot key must be tried for a context of L keys: position 0 and L - 1, the first and last position of every split and of every loop
    iteration of attn_kernel, the last key of a 64-key tile and the first of the next."""
    R, TW = AM.rpi(bf16), S * NW
    sp = AM.span(S, NW, bf16)
    c = {0, L - 1, 63, 64}
    t = np.arange(L)
    split = ((t // R) % TW) // NW
    for s in range(S):
        ts = t[split == s]
        if ts.size:
            c |= {int(ts[0]), int(ts[-1])}
    for k in range(1, (L + sp - 1) // sp + 1):
        c |= {k * sp - 1, k * sp}
    return sorted(x for x in c if 0 <= x < L)


def hot_rounds(Ls, kv_heads, S, NW, bf16):
    """Rounds of one-hot cases (hot_round = 0 .. rounds - 1) after which every utterance has had every one of its candidates as a hot key:
    round r makes candidate (r * kv_heads + kvh) % n the hot key of K/V head kvh."""
    return max((len(hot_candidates(L, S, NW, bf16)) + kv_heads - 1) // kv_heads for L in Ls)


def dec_case(*, mode, bf16, kv8=False, cross=False, decode=True, Ls=None, Q=1, N=0, P=None, kv_heads=4, rope=None, decoy="nan", hot_round=0, S=1, NW=4,
             masked=True, prefill_kernel=False, cap=None, seed=0):
    """mode: "uniform" | "onehot" | "random". decode self: Ls = the context length of every utterance after the append. decode cross: Ls gives B only
    (ragged cur_len), N keys. prefill (decode=False): Q rows per utterance, self (P prompt positions) or cross (N keys).
    prefill_kernel: the case is also meant for the tiled prefill kernels, which multiply p = 0 into the V rows of masked keys: those rows hold large
    finite values instead of NaN."""
    g = torch.Generator().manual_seed(1000 + seed)
    c = DecCase()
    B = len(Ls)
    c.B, c.Q, c.bf16, c.kv8, c.cross, c.kv_heads, c.exact, c.mode = B, Q, bf16, kv8, int(cross), kv_heads, mode != "random", mode
    c.fused_append = int(decode and not cross)
    rows = B * Q
    if decode and not cross:
        c.P = min(5, min(Ls) - 1) if P is None else P
        c.cur_len = [L - c.P for L in Ls]
        c.N, lens = 0, list(Ls)
    elif decode:
        c.P = 3 if P is None else P
        c.cur_len = [2 + 3 * b for b in range(B)]
        c.N, lens = N, [N] * B
    else:
        c.P = 0 if P is None else P
        c.cur_len = None
        c.N, lens = (N, [N] * B) if cross else (0, [Q] * B)
    maxL = max(lens)
    c.cap = maxL + 2 if cap is None else cap  # just above the longest length, unless the case sets it
    assert c.cap >= maxL
    c.lens = lens
    c.q_ld, c.kv_ld = H + 8, kv_heads * 64 + 12
    npos = (c.P + max(c.cur_len) if decode else Q) + 1
    c.scale = EXACT_SCALE if c.exact else 0.125
    c.cos, c.sin = (None, None) if rope is None else exact_rope_tables(npos) if rope == "exact" else real_rope_tables(npos)
    assert not (rope == "exact" and not c.exact) and not (rope == "real" and c.exact)
    # the mask: utterance 0 keeps everything, 1 is padded on the left (cross: fully masked), 2 on the right; flags beyond the masked range are 0 - a
    # flag read for a position that has none would hide a key
    mask_len = c.N if cross else c.P
    c.mask, c.mask_ld = None, 0
    if masked:
        c.mask_ld = mask_len + 3
        m = torch.zeros(B, c.mask_ld, dtype=torch.int32)
        m[:, :mask_len] = 1
        if B > 1:
            m[1, :(mask_len if cross else min(2, mask_len))] = 0
        if B > 2:
            m[2, max(mask_len - 2, 1 if cross else 0):mask_len] = 0
        c.mask = m
    vis = torch.zeros(B, c.cap, dtype=torch.bool)  # positions some query of the utterance may see
    for b in range(B):
        vis[b, :lens[b]] = True
        if c.mask is not None:
            vis[b, :mask_len] &= c.mask[b, :mask_len] != 0
    pos_of = lambda b, qi: (c.P + c.cur_len[b] - 1 if decode else 0) + qi  # noqa: E731
    qpos = torch.tensor([pos_of(b, qi) for b in range(B) for qi in range(Q)])
    # ---- q, K, V --------------------------------------------------------------------------------------------------------------------------------
    if mode == "random":
        qrot_raw = torch.randn(rows, NH, HD, generator=g, dtype=F64).to(F32)
        K = _round_cache(torch.randn(B, kv_heads, c.cap, HD, generator=g, dtype=F64), bf16, kv8)
        V = _round_cache(torch.randn(B, kv_heads, c.cap, HD, generator=g, dtype=F64), bf16, kv8)
        qraw = qrot_raw
        knew = torch.randn(rows, kv_heads, HD, generator=g, dtype=F64).to(F32)
        vnew = torch.randn(rows, kv_heads, HD, generator=g, dtype=F64).to(F32)
        c.hot = {}
    else:
        K, V = _ints(g, B, kv_heads, c.cap, HD), _ints(g, B, kv_heads, c.cap, HD)
        qrot = torch.zeros(rows, NH, HD, dtype=F64)
        c.hot = {}
        if mode == "onehot":
            for j in JQ:
                K[..., j] = 0.0
            for h in range(NH):
                qrot[:, h, JQ[h]] = A_Q
            for b in range(B):
                cands = [t for t in hot_candidates(lens[b], S, NW, bf16 or kv8) if vis[b, t]]
                for kvh in range(kv_heads):
                    if not cands:
                        continue
                    t = cands[(hot_round * kv_heads + kvh) % len(cands)]  # each utterance walks its own list: hot_rounds() rounds cover it
                    c.hot[(b, kvh)] = t
                    for h in range(kvh * (NH // kv_heads), (kvh + 1) * (NH // kv_heads)):
                        K[b, kvh, t, JQ[h]] = HOT
        qraw = unrope(qrot, c.cos, c.sin, qpos[:, None].expand(rows, NH)).to(F32)
        knew = _ints(g, rows, kv_heads, HD)
        vnew = _ints(g, rows, kv_heads, HD).to(F32)
        if c.fused_append:  # the appended row is the key at L - 1: cold, or the hot key where that position was chosen
            for b in range(B):
                for kvh in range(kv_heads):
                    knew[b, kvh] = K[b, kvh, lens[b] - 1]
            knew = unrope(knew, c.cos, c.sin, qpos[:, None].expand(rows, kv_heads))
        knew = knew.to(F32)
    # ---- what nobody may see -------------------------------------------------------------------------------------------------------------------
    big = 2.0 * HOT if c.exact else 3.0
    for b in range(B):
        L = lens[b]
        K[b, :, L:], V[b, :, L:] = NAN, NAN
        hidden = (~vis[b, :L]).nonzero().flatten()
        if prefill_kernel or decoy == "hot":
            K[b, :, hidden] = 0.0 if c.exact else big
            V[b, :, hidden] = 7.0 if c.exact else big
            if c.exact:
                for j in JQ:
                    K[b][:, hidden, j] = big
        else:
            K[b, :, hidden], V[b, :, hidden] = NAN, NAN
        if decoy == "hot" and c.exact and L < c.cap:  # a hotter key just beyond the context
            K[b, :, L], V[b, :, L] = 0.0, 5.0
            for j in JQ:
                K[b, :, L, j] = big
        if c.fused_append:
            K[b, :, L - 1], V[b, :, L - 1] = NAN, NAN  # the stale content of the row the launch appends
    c.K, c.V = K, V
    c.q = torch.full((rows, c.q_ld), NAN, dtype=F32)
    c.q[:, :H] = qraw.reshape(rows, H)
    c.knew = c.vnew = None
    if c.fused_append:
        c.knew = torch.full((rows, c.kv_ld), NAN, dtype=F32)
        c.vnew = torch.full((rows, c.kv_ld), NAN, dtype=F32)
        c.knew[:, :kv_heads * 64] = knew.reshape(rows, -1)
        c.vnew[:, :kv_heads * 64] = vnew.reshape(rows, -1)
    return c


def assert_tiers(model):
    """Exact modes: the visible scores of every (row, head) lie in tiers at least TIER_GAP log2-units apart, so that p is exactly 1 or 0 in fp32 - for
    the whole row and for every split of it."""
    for row, (idx, sc) in model["scores"].items():
        for h in range(sc.shape[0]):
            u = torch.unique(sc[h])
            assert u.numel() == 1 or float((u[1:] - u[:-1]).min()) >= TIER_GAP, (row, h, u)


def exact_out(num, den, bf16):
    """RNE into the engine dtype of float32(num) / float32(den) (one IEEE division), 0 where den = 0; num [rows, heads*64], den [rows, heads]."""
    n = num.to(F32).view(num.shape[0], -1, 64)
    d = den.to(F32)[..., None]
    o = torch.where(d > 0, n / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(n)).reshape(num.shape)
    return o.bfloat16() if bf16 else o


def fp32_attention(c):
    """A plain fp32 torch evaluation of a DecCase (softmax in natural units, fp32 matmuls): the reference alone, for the check that it stays inside
    the derived bound. Returns [rows, heads*64] fp32."""
    nr = c.new_rows()
    out = torch.zeros(c.B * c.Q, H, dtype=F32)
    n_rep = NH // c.kv_heads
    for b in range(c.B):
        for qi in range(c.Q):
            row = b * c.Q + qi
            pos = (c.P + c.cur_len[b] - 1 if c.cur_len is not None else 0) + qi
            L = c.N if c.cross else pos + 1
            ml = L if c.cross else min(c.P, L)
            vis = torch.ones(L, dtype=torch.bool)
            if c.mask is not None and ml > 0:
                vis[:ml] = c.mask[b, :ml] != 0
            for h in range(NH):
                kvh = h // n_rep
                Kh, Vh = c.K[b, kvh, :L].clone(), c.V[b, kvh, :L].clone()
                if nr:
                    Kh[pos], Vh[pos] = nr["k"][b, kvh], nr["v"][b, kvh]
                Kh, Vh = Kh[vis].to(F32), Vh[vis].to(F32)
                if Kh.shape[0] == 0:
                    continue
                qh = c.q[row, h * 64:h * 64 + 64]
                if c.cos is not None:
                    qh = qh * c.cos[pos] + AM.rotate_half(qh) * c.sin[pos]
                p = torch.softmax((Kh @ qh) * np.float32(c.scale), dim=0)
                out[row, h * 64:h * 64 + 64] = p @ Vh
    return out


# ---- T5 ----------------------------------------------------------------------------------------------------------------------------------------
class T5Case:
    pass


T5_HOT = 400.0  # natural-log units: 577 log2-units above the cold tier


def t5_case(*, mode, B, N, mask_kind, offset_round=0, seed=0):
    """qkv [B*N + 1 guard row of NaN, ld] fp32 (q | k | v of 4 heads x 64, NaN in the gap), bias [heads, bias_ld], mask [B, N] int32 or None.
    mask_kind: None | "right" | "left" | "row" (utterance B - 1 fully masked). one-hot: q = 0 and one large bias entry per head, at the relative
    offsets -(N - 1), N - 1, 0, and one that moves with offset_round."""
    g = torch.Generator().manual_seed(2000 + seed)
    c = T5Case()
    c.B, c.N, c.mode, c.exact = B, N, mode, mode != "random"
    c.inner, c.ld = H, 3 * H + 8
    c.bias_zero = N + 2            # the table is wider than the offsets need: bias_zero is not N - 1
    c.bias_ld = c.bias_zero + N + 4
    qkv = torch.full((B * N + 1, c.ld), NAN, dtype=F32)
    if mode == "random":
        x = torch.randn(B * N, 3 * H, generator=g, dtype=F64).to(F32)
        x[:, :H] *= 0.5
        c.bias = torch.randn(NH, c.bias_ld, generator=g, dtype=F64).to(F32)
    else:
        x = _ints(g, B * N, 3 * H).to(F32)
        x[:, :H] = 0.0
        c.bias = torch.zeros(NH, c.bias_ld, dtype=F32)
        if mode == "onehot":
            offs = [-(N - 1), N - 1, 0, (offset_round * 5 + 1) % (2 * N - 1) - (N - 1)]
            for h in range(NH):
                c.bias[h, offs[h] + c.bias_zero] = T5_HOT
            c.offs = offs
    qkv[:B * N, :3 * H] = x
    c.qkv = qkv
    c.mask = None
    if mask_kind is not None:
        m = torch.ones(B, N, dtype=torch.int32)
        if mask_kind == "right":
            m[0, N - (N + 2) // 3:] = 0
        elif mask_kind == "left":
            m[B - 1, :(N + 1) // 2] = 0
        else:
            m[B - 1, :] = 0
        c.mask = m
    return c


def t5_model(c):
    return AM.t5_attention(c.qkv[:c.B * c.N, :3 * H].reshape(c.B, c.N, 3, NH, HD), c.bias, c.bias_zero, c.mask)


def fp32_t5_attention(c):
    x = c.qkv[:c.B * c.N, :3 * H].reshape(c.B, c.N, 3, NH, HD)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    rel = torch.arange(c.N)[None, :] - torch.arange(c.N)[:, None] + c.bias_zero
    sc = q @ k.transpose(2, 3) + c.bias[:, rel][None]
    if c.mask is not None:
        sc = sc + (1.0 - c.mask[:, None, None, :].float()) * torch.finfo(F32).min
    return (torch.softmax(sc, dim=-1) @ v).transpose(1, 2).reshape(c.B, c.N, H)


# ---- the shapes --------------------------------------------------------------------------------------------------------------------------------
ATTN_CONFIGS = [  # (engine dtype bf16?, e4m3 cache?, S, NW) - every attn_kernel instance, and the splits S_self can take
    (True, False, 1, 1), (True, False, 1, 2), (True, False, 1, 4), (True, False, 2, 4), (True, False, 4, 4), (True, False, 8, 4),
    (True, True, 1, 4), (True, True, 4, 4),
    (False, False, 1, 1), (False, False, 1, 2), (False, False, 1, 4), (False, False, 2, 4), (False, False, 4, 4), (False, False, 8, 4)]
PREFILL_Q = (1, 7, 8, 9, 15, 16, 17, 33, 48, 49, 64, 65, 130)
PREFILL_N = (1, 63, 64, 65, 140)
CROSS_N = (1, 31, 32, 33, 64, 65)
T5_SHAPES = ((1, 1), (2, 7), (2, 8), (3, 9), (1, 63), (2, 64), (2, 65), (1, 140))


def attn_lengths(S, NW, bf16):
    R, sp = AM.rpi(bf16), AM.span(S, NW, bf16)
    return [1, 2, R - 1, R, R + 1, sp - 1, sp, sp + 1, 2 * sp + 3]


def ragged(L, big):
    """The context lengths of the utterances of a decode case whose longest is L: B = 3 (B = 1 where the cache would get large)."""
    return [L] if big else [L, max(1, L - 3), max(1, (L + 1) // 2)]


def is_big(S, NW, bf16):
    return AM.span(S, NW, bf16) >= 2048


def random_dec_cases():
    """(name, launch kind "attn" | "prefill", case, S, NW) of part C for the decoder kernels."""
    out = []
    for i, (bf16, kv8, S, NW) in enumerate([(True, False, 1, 1), (True, False, 1, 4), (True, False, 4, 4), (True, True, 1, 4), (True, True, 4, 4),
                                            (False, False, 1, 2), (False, False, 2, 4)]):
        sp = AM.span(S, NW, bf16)
        for k, L in enumerate((1, sp + 1, 2 * sp + 3)):
            c = dec_case(mode="random", bf16=bf16, kv8=kv8, Ls=ragged(L, False), kv_heads=(4, 2, 1)[k], rope="real", S=S, NW=NW, seed=10 * i + k)
            out.append((f"decode self {'bf16' if bf16 else 'fp32'}{' e4m3' if kv8 else ''} S={S} NW={NW} L={L}", "attn", c, S, NW))
    for k, NW in enumerate((1, 2, 4)):
        for bf16 in (True, False):
            c = dec_case(mode="random", bf16=bf16, cross=True, Ls=[0, 0, 0], N=65, kv_heads=(4, 2, 1)[k], rope="real", seed=100 + k)
            out.append((f"decode cross {'bf16' if bf16 else 'fp32'} NW={NW} N=65", "attn", c, 1, NW))
    for k, Q in enumerate((9, 33, 130)):
        for bf16, kv8 in ((True, False), (False, False), (True, True)):
            c = dec_case(mode="random", bf16=bf16, kv8=kv8, decode=False, Ls=[0, 0, 0], Q=Q, P=3, kv_heads=(4, 2, 1)[k], rope="real", prefill_kernel=True,
                         seed=200 + k)
            out.append((f"prefill self {'bf16' if bf16 else 'fp32'}{' e4m3' if kv8 else ''} Q={Q}", "prefill", c, 1, 4))
        for bf16 in (True, False):
            c = dec_case(mode="random", bf16=bf16, decode=False, cross=True, Ls=[0, 0, 0], Q=Q, N=140 if k else 65, kv_heads=(4, 2, 1)[k], rope="real",
                         prefill_kernel=True, seed=300 + k)
            out.append((f"prefill cross {'bf16' if bf16 else 'fp32'} Q={Q} N={c.N}", "prefill", c, 1, 4))
    return out


def random_t5_cases():
    return [(f"t5 B=2 N={N}", t5_case(mode="random", B=2, N=N, mask_kind=("right", "left", "row")[k], seed=k)) for k, N in enumerate((9, 65, 140))]


def dec_tolerance(c, m, S, NW, bf16_out):
    return AM.tolerance(m["absdot"], m["vmax"], m["count"], m["out"], S=S, NW=NW, bf16=bf16_out)


def t5_tolerance(c, m, bf16_out):
    n = torch.full(m["absdot"].shape, c.N)
    return AM.tolerance(m["absdot"], m["vmax"], n, m["out"], S=1, NW=4, bf16=bf16_out, log2_units=False)


def kv8_edge_rows():
    """Rows [n, 64] fp32 at the edges of the e4m3 cache quantiser: amax exactly 448 * 2^k, one float above and one below it, an all-zero row,
    values exactly halfway between e4m3 grid points (ties to even), results in the subnormal range of e4m3."""
    g = torch.Generator().manual_seed(7)
    rows = []
    base = (torch.rand(64, generator=g) * 2 - 1).to(F32)
    for k in (-3, 0, 2):
        a = np.float32(448.0 * 2.0 ** k)
        for amax in (a, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(0))):
            r = base * float(amax) * 0.9
            r[5] = -float(amax)
            rows.append(r)
    rows.append(torch.zeros(64))
    # scale 1 (amax 448): halfway points between neighbours of the grid - 17 (16 | 18), 19 (18 | 20), 27 (26 | 28), 68 (64 | 72), 76 (72 | 80), 1.0625 (1 | 1.125)
    ties = torch.zeros(64)
    ties[:8] = torch.tensor([448.0, 17.0, 19.0, 27.0, 68.0, 76.0, 1.0625, -17.0])
    rows.append(ties)
    # subnormal results (grid 2^-9 below 2^-6 at scale 1): exact grid points, halfway points, values that round to zero and to the smallest subnormal
    sub = torch.zeros(64)
    sub[:10] = torch.tensor([448.0, 2.0 ** -9, 3 * 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -11, -7 * 2.0 ** -10, 2.0 ** -7 + 2.0 ** -10, 1e-8])
    rows.append(sub)
    rows.append(sub * 0.25)   # the same at scale 2^-2
    return torch.stack(rows).to(F32)
