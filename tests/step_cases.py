"""Shapes, seeds, edge lists and input constructions of the decode-step kernel tests (tests/test_step_kernels_gpu.py, tests/test_step_model_cpu.py):
the smallest shapes at which each path of ptts_lm.hip::strip_path begins and ends, not the workload's. Everything is generated on the CPU from a
seed, so the CPU proofs run on the very inputs the GPU tests use."""
import math

import torch

import step_harness as SH

F64 = torch.float64
WIDTHS_FULL = (1024, 1536)        # register-resident LayerNorm, PRO_LNS, lnproj_fused_kernel, xattn G < 8
WIDTH_GENERIC = 512               # two-pass rows_prep, non-FULL fused prologues, xattn_fused_kernel<WT, 8, 2>
ENGINES = (True, False)           # bf16, fp32

ROWS_FUSED = (1, 3, 8)                          # strips with fused prologues (PRO_LN / PRO_ATTN / PRO_PLAIN)
ROWS_LNS = (9, 16, 17, 32)                      # PRO_LNS; EPI_RESID + stats_out: one and two row tiles, ragged last tile
ROWS_COPY_FO = (9, 16, 17, 33, 48, 64, 65, 128)  # rows_prep + PRO_COPY on fragment-order rows, decode = 1: 16- and 32-row passes on both sides of
                                                 # msplit_rows' edges (<= 64 | above), ragged last pass
LNPROJ_ROWS = {8: (9, 40), 16: (41, 56, 128), 4: (9, 13)}   # utterances per workgroup -> rows
LNPROJ_PREFILL = dict(B=3, Q=11)                # EPI_STORE with the cache append
XATTN_ROWS = {8: (1, 3, 8, 9, 70), 4: (9, 33, 64), 2: (9, 13, 32)}  # utterances per workgroup -> utterances
XATTN_CAP = 72                                  # max_enc of the cross K/V arena: above the 64 (bf16) / 32 (fp32) positions of the first batch of loads
XATTN_DESC = (1, 17, 64, XATTN_CAP)             # description tokens
N_COLS = (64, 256)                              # projection rows: one and four 64-row blocks

# (PRO, EPI, MTP) of ptts_lm_w8.hip -> (rows, fragment-order rows) that select the instance in launch_gemm. On fragment-order rows with decode = 1 a
# pass has 16 rows up to 64 utterances and 32 above (1 / 2 tiles); 4 tiles are a pass of 33..64 rows: row-major prepared rows (one pass of M rows),
# or in the product the 64-row passes of prefill-sized rows and of the LM heads.
W8_CASES = {
    (SH.PRO_LN, SH.EPI_STORE, 1): (8, 0), (SH.PRO_ATTN, SH.EPI_RESID, 1): (5, 0), (SH.PRO_LN, SH.EPI_GELU, 1): (7, 0), (SH.PRO_PLAIN, SH.EPI_RESID, 1): (8, 0),
    (SH.PRO_COPY, SH.EPI_STORE, 1): (13, 1), (SH.PRO_COPY, SH.EPI_STORE, 2): (70, 1), (SH.PRO_COPY, SH.EPI_STORE, 4): (40, 0),
    (SH.PRO_COPY, SH.EPI_RESID, 1): (16, 1), (SH.PRO_COPY, SH.EPI_RESID, 2): (65, 1), (SH.PRO_COPY, SH.EPI_RESID, 4): (49, 0),
    (SH.PRO_COPY, SH.EPI_GELU_WT, 4): (64, 0), (SH.PRO_LNS, SH.EPI_GELU_WT, 1): (16, 0), (SH.PRO_LNS, SH.EPI_GELU_WT, 2): (17, 0),
}
# combinations outside that list: launch_gemm falls back to the bf16 strips on W, with the same exact result
W8_FALLBACK = {(SH.PRO_COPY, SH.EPI_GELU_WT, 1): (16, 1), (SH.PRO_COPY, SH.EPI_GELU_WT, 2): (70, 1), (SH.PRO_LNS, SH.EPI_STORE, 1): (9, 0)}


def lns_fits(M, K, bf16):
    """The product's condition for PRO_LNS (ptts_step_plan.h: pro_lns_fits; held equal to it by tests/test_step_harness_cpu.py): 9..32 rows that all fit in LDS beside the reduction buffer, hidden 1024 / 1536.
    The fp32 engine at hidden 1536 fits 23 rows: its 32-row case stays on rows_prep + PRO_COPY."""
    return 8 < M <= 32 and K in (1024, 1536) and M * (K * (2 if bf16 else 4) + 16) + 16 * 1024 <= 159 * 1024


def mtp_of(pro, M, x_fo, N=256, decode=True):
    """Row tiles per pass that launch_gemm picks (ptts_gemm_launch.h: msplit_rows, max_rows, tiles), restated for the case lists."""
    if pro == SH.PRO_COPY and x_fo:
        if not decode and not (N // 16) * ((M + 63) // 64) < 256:
            rows = 64 if M > 32 else 32
        elif N >= 8192:
            rows = 64 if M > 32 else 32
        else:
            rows = 16 if M <= 64 else 32
        rpp = min(M, rows)
    else:
        rpp = min(M, 128 if (pro == SH.PRO_COPY and M > 32) else 32)
    return 8 if rpp > 64 else 4 if rpp > 32 else 2 if rpp > 16 else 1


# ---- which template instances the case lists reach, by the launch functions' own selection rules -------------------------------------------------
# hidden 1024 has 16-fragment K halves in both engine dtypes ((1024 / KT) / 2 = 16 or 32), so the <WT, 8, 4, ...> instances that launch_lnproj and
# launch_xattn_fused also instantiate are never selected by any width the product supports
UNREACHABLE = {
    "lnproj_fused_kernel": {(bf, 8, 4, g, e) for bf in (0, 1) for g in (4, 8, 16) for e in (SH.EPI_STORE, SH.EPI_GELU_WT)},
    "xattn_fused_kernel": {(bf, 8, 4, 8) for bf in (0, 1)},
    "rows_prep_kernel": set(),
    "gemm_strip_kernel_w8": set(),
}


def reached_instances(name):
    out = set()
    if name == "lnproj_fused_kernel":
        for bf in ENGINES:
            for K in WIDTHS_FULL:
                for g in LNPROJ_ROWS:
                    for e in (SH.EPI_STORE, SH.EPI_GELU_WT):
                        out.add((int(bf), 16 if K == 1024 else 8, K // 256, g, e))
    elif name == "xattn_fused_kernel":
        for bf in ENGINES:
            for K in WIDTHS_FULL:
                for g in XATTN_ROWS:
                    out.add((int(bf), 16 if K == 1024 else 8, K // 256, g))
            out.add((int(bf), 8, WIDTH_GENERIC // 256, 8))
    elif name == "rows_prep_kernel":
        out = {(int(bf), p) for bf in ENGINES for p in (SH.PRO_LN, SH.PRO_ATTN)}
    elif name == "gemm_strip_kernel_w8":
        out = set(W8_CASES)
    return out


# ---- input constructions ------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def ln_inputs(M, K, seed):
    """fp32 rows that differ per row, with row scales (0.04 .. 4) and offsets (0.03 .. 3, either sign) spread over two decades; gamma around 1, beta
    around 0."""
    g = gen(seed)
    scale = 4.0 * torch.pow(10.0, -2.0 * torch.rand(M, generator=g))
    off = 3.0 * torch.pow(10.0, -2.0 * torch.rand(M, generator=g)) * torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0)
    x = torch.randn(M, K, generator=g) * scale[:, None] + off[:, None]
    gamma = 1.0 + 0.25 * torch.randn(K, generator=g)
    beta = 0.25 * torch.randn(K, generator=g)
    return x.float(), gamma.float(), beta.float()


def ints(shape, seed, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).to(F64)


def exact_ln_inputs(M, K, seed):
    """Construction (a): gamma = 0, beta = small integers varying over k, x arbitrary finite Gaussians: the normalised row is beta exactly."""
    x, _, _ = ln_inputs(M, K, seed)
    return x, torch.zeros(K), ints((K,), seed + 1).float()


def scale_into_gelu_range(W, acc):
    """Scale the rows of W by powers of two (exact) so that the accumulators acc [M, N] land in (-3, 3]: the curved range of the GELU."""
    mx = acc.abs().amax(0).clamp(min=1.0)
    s = torch.exp2(-torch.clamp(torch.ceil(torch.log2(mx / 3.0)), min=0.0))
    return W * s[:, None], acc * s[None, :]


def selection_weights(N, K, seed):
    """Construction (b): launches of W [N, K] with one non-zero entry c(n) in {+-1, +-2, +-1/2} at column pi(n) per row; over the launches every
    column k is selected at least once. Returns [(W float64, pi int64 [N], c float64 [N])]."""
    g = gen(seed)
    perm = torch.randperm(K, generator=g)
    coef = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], dtype=F64)
    out = []
    for j in range((K + N - 1) // N):
        pi = perm[(j * N + torch.arange(N)) % K]
        c = coef[torch.randint(0, 6, (N,), generator=g)]
        W = torch.zeros(N, K, dtype=F64)
        W[torch.arange(N), pi] = c
        out.append((W, pi, c))
    return out


def sparse_int_weights(N, K, seed, nnz=3, lo=-2, hi=2):
    """A few small integers per W row: with |x| <= 2 and a residual |r| <= 8 the updated residual stays within |v| <= 32 (strip statistics exact)."""
    g = gen(seed)
    W = torch.zeros(N, K, dtype=F64)
    for _ in range(nnz):
        W[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = torch.randint(lo, hi + 1, (N,), generator=g).to(F64)
    return W


def rope_tables(npos, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, 64, 2, dtype=F64) / 64))
    f = torch.outer(torch.arange(npos, dtype=F64), inv)
    emb = torch.cat((f, f), dim=-1)
    return emb.cos().float(), emb.sin().float()


def exact_attn_partials(M, K, S, seed):
    """Split-KV partials whose combination is exact: every split of a head has the same maximum, sumexp is a power of two with a power-of-two total,
    the partial rows are integers. Split 1 of head 0 is empty (max = -inf) with NaN partials: weight 0, nothing may leak; the last head has every
    split empty: output 0. Returns part [M, S, K], stats [M, S, heads, 2] (fp32) and the combined rows [M, K] (float64)."""
    nh = K // 64
    g = gen(seed)
    part = torch.randint(-8, 9, (M, S, K), generator=g).to(F64)
    mx = torch.randint(-20, 21, (M, 1, nh), generator=g).to(F64).expand(M, S, nh).clone()
    e = torch.randint(0, 4, (M, 1, nh), generator=g).to(F64).expand(M, S, nh).clone()  # sumexp 2^e in every split: total S 2^e
    ls = torch.exp2(e)
    live = torch.ones(M, S, nh, dtype=torch.bool)
    live[:, 1, 0] = False
    live[:, :, nh - 1] = False
    # head 0 keeps a power-of-two total over its S - 1 live splits: S = 2 -> one split; S = 4 -> sumexp (2, 1, 1) 2^e
    if S == 4:
        ls[:, 0, 0] *= 2.0
    lv = live[..., None].expand(M, S, nh, 64).reshape(M, S, K)
    den = (ls * live).sum(dim=1)                                                   # [M, nh]
    num = torch.where(lv, part, torch.zeros((), dtype=F64)).sum(dim=1)              # [M, K]
    rows = torch.where(den > 0, 1.0 / den.clamp_min(1e-300), torch.zeros_like(den)).repeat_interleave(64, dim=1) * num
    part = torch.where(lv, part, torch.full((), float("nan"), dtype=F64))
    stats = torch.stack((torch.where(live, mx, torch.full((), -math.inf, dtype=F64)), torch.where(live, ls, torch.zeros((), dtype=F64))), dim=3)
    return part.float(), stats.float(), rows


def quarter_turn_tables(npos):
    """RoPE tables whose rotation is exact: position p turns every pair by (p mod 4) quarter turns, so cos / sin are 0 or +-1 and a rotated integer
    q is q, rotate_half(q), -q or -rotate_half(q) - a different vector at each of four consecutive positions."""
    p = torch.arange(npos) % 4
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[p][:, None].expand(npos, 64).contiguous()
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[p][:, None].expand(npos, 64).contiguous()
    return cos, sin


def xattn_random_inputs(K, B, n_rep, bf16, seed, nnz=16):
    """The random case of xattn_fused_kernel: LayerNorm inputs that differ per utterance (ln_inputs), Gaussian K / V in the engine dtype, and a Wq
    with nnz Gaussian entries per row (engine dtype): q depends on real LN2 rows of this utterance, and its fp32 rounding stays a few ulps (the dense
    K reduction is the exact cases' business), so the attention bound is not drowned by a worst-case K 2^-24 sum |W||y|.
    Returns x, gamma, beta, Wq [K, K], Kc, Vc [B, heads / n_rep, XATTN_CAP, 64] (float64 values of the engine dtype), cur_len [B], mask [B, XATTN_CAP]."""
    dt = torch.bfloat16 if bf16 else torch.float32
    x, gamma, beta = ln_inputs(B, K, seed)
    g = gen(seed + 1)
    nkv = K // 64 // n_rep
    Wq = torch.zeros(K, K)
    cols = torch.stack([torch.randperm(K, generator=g)[:nnz] for _ in range(K)])
    Wq[torch.arange(K)[:, None], cols] = torch.randn(K, nnz, generator=g) / math.sqrt(nnz)
    Kc = torch.randn(B, nkv, XATTN_CAP, 64, generator=g).to(dt).to(F64)
    Vc = torch.randn(B, nkv, XATTN_CAP, 64, generator=g).to(dt).to(F64)
    cur_len = torch.randint(1, 20, (B,), generator=g).int()
    mask = (torch.rand(B, XATTN_CAP, generator=g) < 0.7).int()
    mask[:, 0] = 1
    return x, gamma, beta, Wq.to(dt).to(F64), Kc, Vc, cur_len, mask
