"""Shapes, instance selection and input constructions of the GEMV decode-step tests (tests/test_gemv_kernels_gpu.py, tests/test_gemv_harness_cpu.py).
Everything is generated on the CPU from a seed.

nodes() is the table of gemv_kernel launches the case lists are built from, for the widths the product is built for. It is tied to the product by
the product's own plan (ptts_step_plan.h: gemv_plan, read through the harness): tests/test_gemv_harness_cpu.py sweeps the plan over these widths,
batch sizes, contexts and switches and requires the launches it lists to be exactly nodes() minus UNREACHED_NODES. instance_of() restates
ptts_gemv_launch.inc's selection (pick_rows, the MB / STG choice), naming the gemv_kernel template instance a launch lands on; gemv_cases() is the
table of test shapes: one per reached instance at the smallest N that selects it and exercises the row clamp, plus the product's own widths named
by the issue (the LM heads' 9 * 1088 rows, a grouped-query QKV width)."""
import functools
import math

import torch

import gemv_harness as GH
import step_model as SM
from gemv_harness import (GV_ATTN, GV_ATTN2, GV_BF16, GV_BF16_W8, GV_COPY, GV_F32, GV_GELU_WT, GV_LN, GV_LNP, GV_RESID, GV_SOFTMAX, GV_STORE)
from step_cases import gen, ints, ln_inputs, scale_into_gelu_range, selection_weights  # noqa: F401  (shared constructions)

F64 = torch.float64
# (hidden, heads, ffn) the product is built for (Mini / Large-v1 class widths and the 512 parity width), each also with half as many K/V heads
WIDTHS = ((512, 8, 1024), (1024, 16, 4096), (1536, 24, 6144))
LM_HEAD_ROWS = 9 * 1088
GV_MAX_ROWS, GV_PMAX = 8, 24
SUP_ROWS = (1, 2, 3, 4, 5, 6, 8, 10)
NCH_BUILT = (1, 2, 3, 4, 6, 8, 12, 16, 24)


def epl(mode):
    return 4 if mode == GV_F32 else 8


def qa_ok(H, mode):
    """ptts_qkvattn_ok / ptts_xqattn_ok."""
    return H in ((512, 1024) if mode == GV_F32 else (512, 1024, 1536))


def xfold_ok(H, nh, mode):
    """ptts_xfoldattn_ok."""
    return nh <= GV_PMAX and H in ((512,) if mode == GV_F32 else (512, 1024, 1536))


def rows_per_split(mode):
    return 8 * 4 * (4 if mode == GV_F32 else 8)


# ---- the nodes gemv_step issues ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nodes():
    """{(pro, epi, S, M, N, K, mode)}: the ptts_gemv_launch calls of gemv_step over WIDTHS x {all K/V heads, half} x M = 1..8 x the three modes,
    with both sides of each of its switches (fused / two-node self-attention, folded / fused / plain cross block, every split count it can pick)."""
    out = set()
    for H, nh, F in WIDTHS:
        for nkv in (nh, nh // 2):
            QKV = H + 2 * nkv * 64
            for mode in GH.MODES:
                for M in range(1, (1 if mode == GV_F32 else GV_MAX_ROWS) + 1):
                    def add(pro, epi, S, N, K, mode=mode, M=M):
                        out.add((pro, epi, S, M, N, K, mode))
                    if qa_ok(H, mode):  # fuse_qa: S_f doubles up to S_cap
                        for S in (1, 2, 4, 8):
                            if S <= (8 if M == 1 else 4 if M <= 4 else 2):
                                add(GV_ATTN2, GV_RESID, S, H, H)
                    add(GV_LN, GV_STORE, 1, QKV, H)                      # LN1 + QKV
                    add(GV_COPY, GV_RESID, 1, H, H)                      # out_proj (one split), cross out_proj
                    for S in (2, 4, 8):
                        add(GV_ATTN, GV_RESID, S, H, H)                  # combine + out_proj
                    if M == 1:
                        fm = GV_F32 if mode == GV_F32 else GV_BF16       # the folded matrices are in the engine dtype, never e4m3
                        add(GV_LN, GV_STORE, 1, nh * 64, H, mode=fm)     # LN2 + folded scores
                        add(GV_SOFTMAX, GV_RESID, 1, H, nh * 64, mode=fm)
                        if xfold_ok(H, nh, fm):
                            add(GV_LNP, GV_GELU_WT, 1, F, H)             # partial rows + LN3 + fc1
                    add(GV_LN, GV_STORE, 1, H, H)                        # LN2 + cross q
                    add(GV_LN, GV_GELU_WT, 1, F, H)                      # LN3 + fc1
                    add(GV_COPY, GV_RESID, 1, H, F)                      # fc2
                    add(GV_LN, GV_STORE, 1, LM_HEAD_ROWS, H)             # final LayerNorm + LM heads
    return frozenset(out)


# the nodes of the table that no engine's plan issues: a two-node self-attention runs on S_self = 256 / (max_batch * heads) splits (a power of two), so a
# GV_ATTN combine of S splits needs S * M * heads <= 256 - eight utterances of 24 heads never split, one utterance of 8 heads reaches every count
UNREACHED_NODES = frozenset((GV_ATTN, GV_RESID, S, M, H, H, mode) for H, nh, _ in WIDTHS for mode in GH.MODES for S in (2, 4, 8)
                            for M in range(1, (1 if mode == GV_F32 else GV_MAX_ROWS) + 1) if S * M * nh > 256)
assert len(UNREACHED_NODES) == 60 and UNREACHED_NODES < nodes()


# ---- ptts_gemv_launch.inc restated ------------------------------------------------------------------------------------------------------------------
def pick_rows(N, nch, rcap):
    want = (N + 1023) // 1024
    maxr = min(rcap, max(1, 40 // nch))
    r = 1
    for s in SUP_ROWS:
        if s <= maxr:
            r = s
            if s >= want:
                break
    return r


def mb_of(M):
    return 1 if M == 1 else 4 if M <= 4 else 8


def row_cap(pro, mode, M):
    """(RCAP of the dispatch, the cap launch_nch hands pick_rows)."""
    rcap = 10 if pro in (GV_LN, GV_LNP) else 2
    mb, w8 = mb_of(M), mode == GV_BF16_W8
    return rcap, (min(rcap, 3 if w8 else 4) if mb >= 8 else min(rcap, 64 // mb) if mb > 1 else rcap)


def dispatch_ok(pro, epi, S, M, mode):
    """The (prologue, epilogue, S, M) combinations GV_FN dispatches (fp32 without GV_MULTI: one utterance)."""
    if not 1 <= M <= GV_MAX_ROWS or (mode == GV_F32 and M != 1):
        return False
    if pro == GV_LN:
        return epi in (GV_STORE, GV_GELU_WT) and S == 1
    if pro == GV_COPY:
        return epi == GV_RESID and S == 1
    if pro == GV_SOFTMAX:
        return epi == GV_RESID and S == 1 and M == 1
    if pro == GV_ATTN:
        return epi == GV_RESID and S in (2, 4, 8)
    if pro == GV_LNP:
        return epi == GV_GELU_WT and S == 1 and M == 1
    if pro == GV_ATTN2:
        return epi == GV_RESID and (S in (1, 2) or (S == 4 and M <= 4) or (S == 8 and M == 1))
    return False


def instance_of(pro, epi, S, M, N, K, mode):
    """The gemv_kernel instance (bf16, NCH, R, PRO, EPI, S, MB, W8, STG) the launch lands on, or None where the dispatch has none."""
    e = epl(mode)
    if not dispatch_ok(pro, epi, S, M, mode) or K % (64 * e) or K // (64 * e) not in NCH_BUILT:
        return None
    nch, mb, w8 = K // (64 * e), mb_of(M), mode == GV_BF16_W8
    rcap, cap = row_cap(pro, mode, M)
    R = pick_rows(N, nch, cap)
    if not (R * nch <= 40 and R <= rcap and mb * R <= 64 and (mb < 8 or R <= (3 if w8 else 4)) and (pro == GV_COPY or nch * e <= 32)):
        return None
    stg = pro == GV_COPY and mb == 8 and mb * nch > 40 and mb * nch * 1024 <= 64 * 1024
    return (int(mode != GV_F32), nch, R, pro, epi, S, mb, int(w8), int(stg))


def groups_of(inst):
    """(MG utterances per register group, NG groups) of an MB instance (gemv_kernel's MG / NG)."""
    _, nch, _, _, _, _, mb, _, _ = inst
    mg = mb if (mb <= 4 or mb * nch <= 40) else (mb // 2 if (mb // 2) * nch <= 40 else mb // 4)
    return mg, mb // mg


def symbol_of(inst):
    """The mangled-name prefix of the instance (tests/test_gemv_harness_cpu.py looks the instances up by name)."""
    bf, nch, R, pro, epi, S, mb, w8, stg = inst
    return f"_Z11gemv_kernelI{'t' if bf else 'f'}Li{nch}ELi{R}ELi{pro}ELi{epi}ELi{S}ELi{mb}ELb{w8}ELb{stg}EE"


@functools.lru_cache(maxsize=None)
def reached_by_nodes():
    """{instance: [nodes]} over nodes(). Every node of the table has an instance."""
    out = {}
    for n in nodes():
        inst = instance_of(*n)
        assert inst is not None, n
        out.setdefault(inst, []).append(n)
    return out


def smallest_n(pro, epi, S, M, K, mode, inst):
    """The smallest N that selects `inst`, spans more than one workgroup and is no multiple of R or 4 R: the last wave clamps rows inside itself and
    the last workgroup has waves whose rows are all clamped."""
    R = inst[2]
    for N in range(4 * R + 1, 16384):
        if N % (4 * R) and (R == 1 or N % R) and instance_of(pro, epi, S, M, N, K, mode) == inst:
            return N
    raise AssertionError(f"no N selects {inst}")


@functools.lru_cache(maxsize=None)
def gemv_cases():
    """[(pro, epi, S, M, N, K, mode)]: per reached instance one case at smallest_n, with the largest M among its nodes that is not a whole MB (so
    utterances past M exist where the instance has any) - and the product's own LM-head and grouped-query QKV widths at 1, 3 and 8 utterances."""
    out = []
    for inst, ns in sorted(reached_by_nodes().items()):
        pro, epi, S, _, _, K, mode = ns[0]
        Ms = sorted({n[3] for n in ns})
        M = max([m for m in Ms if m != mb_of(m)] or Ms)
        modes = sorted({n[6] for n in ns})
        assert modes == [mode], (inst, modes)
        out.append((pro, epi, S, M, smallest_n(pro, epi, S, M, K, mode, inst), K, mode))
    for H, nh, _ in WIDTHS:
        for mode in GH.MODES:
            for M in ((1,) if mode == GV_F32 else (1, 3, 8)):
                out.append((GV_LN, GV_STORE, 1, M, LM_HEAD_ROWS, H, mode))
    out.append((GV_LN, GV_STORE, 1, 1, 1024 + 2 * 8 * 64, 1024, GV_BF16))  # QKV with 8 of 16 K/V heads
    out.append((GV_LN, GV_STORE, 1, 3, 1024 + 2 * 8 * 64, 1024, GV_BF16_W8))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    for c in uniq:  # the clamp is exercised wherever the product's own N leaves rows over (the LM heads at R = 10: 9792 = 244 * 40 + 32)
        assert instance_of(*c) is not None, c
    return tuple(uniq)


def reached_by_cases():
    return {instance_of(*c) for c in gemv_cases()}


def group_cases():
    """(pro, epi, S, M, N, K, mode) at M = 5 and 8 on the staged MB = 8 instance (fc2 of hidden 1024: K = 4096) and on the instances whose
    activations pass through the registers in several groups (K = 4096: two groups of 4; K = 6144: four groups of 2)."""
    out = []
    for K in (4096, 6144):
        for mode in (GV_BF16, GV_BF16_W8):
            for M in (5, 8):
                c = (GV_COPY, GV_RESID, 1, M, 1029, K, mode)
                assert groups_of(instance_of(*c))[1] > 1 and instance_of(*c)[8] == int(K == 4096)
                out.append(c)
    return out


# ---- input constructions -------------------------------------------------------------------------------------------------------------------------
def exact_combine_partials(M, K, S, seed, new_slot):
    """Split-KV partials whose combination is exact (step_cases.exact_attn_partials, with the new position's slot of GV_ATTN2): every live slot of a
    head has the same maximum mx; the live cache splits carry sumexp 2^e except the first, which carries what makes the head's total a power of two
    (the new position counts 1); the partial rows are integers. Split 1 of head 0 is empty (max = -inf, sumexp 0) and holds large finite partials: its
    weight is 0 (the producers write zeros there); the last head has every cache split empty - with the new slot its output is the V row, without it 0.
    new_slot: slot S holds the V row as partial and the two half dot products (s0, mx - s0) as statistics.
    Returns part [M, S (+ 1), K], stats [M, S (+ 1), heads, 2] (fp32) and the combined rows [M, K] (float64)."""
    nh = K // 64
    g = gen(seed)
    slots = S + int(new_slot)
    part = torch.randint(-8, 9, (M, slots, K), generator=g).to(F64)
    mx = torch.randint(-20, 21, (M, nh), generator=g).to(F64)
    e = torch.randint(1, 4, (M, nh), generator=g).to(F64)
    live = torch.ones(M, S, nh, dtype=torch.bool)
    if S >= 2:
        live[:, 1, 0] = False
    live[:, :, nh - 1] = False
    live[M // 2, :, 1 % nh] = False                                    # one utterance: a second head without cache rows
    nlive = live.sum(dim=1)                                            # [M, nh]
    p2 = torch.exp2(torch.ceil(torch.log2(nlive.clamp(min=1).to(F64))))
    ls = torch.exp2(e)[:, None, :].expand(M, S, nh).clone()
    first = live & (live.cumsum(dim=1) == 1)
    extra = torch.exp2(e) * (1.0 + p2 - nlive) - (1.0 if new_slot else 0.0)
    ls = torch.where(first, extra[:, None, :].expand(M, S, nh), ls)
    ls = torch.where(live, ls, torch.zeros((), dtype=F64))
    lv = live[..., None].expand(M, S, nh, 64).reshape(M, S, K)
    num = torch.where(lv, part[:, :S], torch.zeros((), dtype=F64)).sum(dim=1)
    den = ls.sum(dim=1)
    st = torch.stack((torch.where(live, mx[:, None, :].expand(M, S, nh), torch.full((), -math.inf, dtype=F64)), ls), dim=3)
    if new_slot:
        num, den = num + part[:, S], den + 1.0
        s0 = torch.randint(-30, 31, (M, nh), generator=g).to(F64)
        st = torch.cat((st, torch.stack((s0, mx - s0), dim=2)[:, None]), dim=1)
    assert bool(((den == 0) | (torch.log2(den.clamp(min=1)) % 1 == 0)).all())
    rows = torch.where(den > 0, 1.0 / den.clamp_min(1e-300), torch.zeros_like(den)).repeat_interleave(64, dim=1) * num
    part[:, :S] = torch.where(lv, part[:, :S], torch.full((), 12345.0, dtype=F64))
    return part.float(), st.float(), rows


def random_combine_partials(M, K, S, seed, new_slot, pos0=False):
    """Gaussian partials, maxima spread over ~10 log2 units, one split of head 1 % heads empty (max = -inf, sumexp 0, partial 0 as the producers write
    it), the last head with every cache split empty; pos0: every cache split of every head empty (the first decode position)."""
    nh = K // 64
    g = gen(seed)
    slots = S + int(new_slot)
    part = torch.randn(M, slots, K, generator=g).float()
    stats = torch.stack((torch.randn(M, slots, nh, generator=g) * 4.0, torch.rand(M, slots, nh, generator=g) * 30.0 + 1.0), dim=3).float()
    dead = torch.zeros(M, slots, nh, dtype=torch.bool)
    dead[:, S - 1, 1 % nh] = True
    dead[:, :S, nh - 1] = True
    if pos0:
        dead[:, :S] = True
    if not new_slot:
        dead[:, :, nh - 1] = True
    else:
        dead[:, S] = False
    stats[..., 0] = torch.where(dead, torch.full((), -math.inf), stats[..., 0])
    stats[..., 1] = torch.where(dead, torch.zeros(()), stats[..., 1])
    part = torch.where(dead[..., None].expand(M, slots, nh, 64).reshape(M, slots, K), torch.zeros(()), part)
    return part, stats


def tiered_softmax(nh, ne, n_valid, seed, all_masked=False):
    """A base-2 softmax whose weights are exact without being equal. Of the positions below n_valid the mask keeps 15 (3, or 1, where n_valid has
    no more); the mask also keeps every position at or past n_valid, which n_valid cuts. In every head one kept position scores s_h, two s_h - 1,
    four s_h - 2, eight s_h - 3, in an order that differs per head: the exponentials are 2^-o, each tier sums to 1, the total is the number of
    tiers T in {4, 2, 1}, the weights are 2^-o / T. s_h = +-256 + h % 5 alternates in sign from head to head: a maximum (or a sum) that leaks
    from a neighbouring head turns a head's weights into 0 or inf, a reduction over the wrong lane group changes T, exp in place of exp2 leaves the
    powers of two, a permuted position moves a weight. all_masked: the mask keeps no position below n_valid - every weight is 0.
    Returns (s [nh] float64, o [nh, ne] int64 (tier of a visible position, -1 elsewhere), mask int32 [ne], p float64 [nh * ne])."""
    g = gen(seed)
    cnt = 15 if n_valid >= 15 else 3 if n_valid >= 3 else 1
    tiers = torch.tensor(([0] + [1] * 2 + [2] * 4 + [3] * 8)[:cnt])
    T = float(int(tiers.max()) + 1)
    mask = torch.zeros(ne, dtype=torch.int32)
    kept = torch.randperm(n_valid, generator=g)[:cnt]
    mask[n_valid:] = 1
    o = torch.full((nh, ne), -1, dtype=torch.int64)
    if not all_masked:
        mask[kept] = 1
        for h in range(nh):
            o[h, kept] = tiers[torch.randperm(cnt, generator=g)]
    s = torch.tensor([(256.0 if h % 2 == 0 else -256.0) + h % 5 for h in range(nh)], dtype=F64)
    p = torch.where(o >= 0, torch.exp2(-o.to(F64)) / T, torch.zeros((), dtype=F64)).reshape(-1)
    return s, o, mask, p


def tiered_scores(s, o, hidden=float("nan")):
    """The scores [nh * ne] fp32 of tiered_softmax: s_h - o at the visible positions, `hidden` (NaN, or a decoy above every visible score) elsewhere."""
    return torch.where(o >= 0, s[:, None] - o.to(F64), torch.full((), hidden, dtype=F64)).reshape(-1).float()


def exact_softmax_inputs(nh, ne, seed):
    """tiered_softmax at n_valid = ne - 3 for the instance table's exact GV_SOFTMAX cases. Returns scores, mask, n_valid, p."""
    s, o, mask, p = tiered_softmax(nh, ne, ne - 3, seed)
    return tiered_scores(s, o), mask, ne - 3, p


LNP_SHAPES = ((512, 8), (1024, 16), (1536, 24))   # (hidden, partial rows = heads) of the GV_LNP row cases
GELU_SLOPE = 1.13  # sup |d gelu / du| = Phi(u) + u phi(u) at u = sqrt 2: 0.9214 + 0.2076 = 1.1290 (its minimum is -0.129)


def lnp_inputs(K, npart):
    """x [K], part [npart, K] (fp32: a residual row and Gaussian per-head rows a third of its size), gamma, beta [K]."""
    x, gamma, beta = ln_inputs(1, K, 3500 + K)
    part = (torch.randn(npart, K, generator=gen(3500 + K)) * 0.3).float()
    return x[0], part, gamma, beta


def lnp_row_sum(x, part):
    """hsum of GV_LNP as an exact fp32 statement: x, then the partial rows added in index order, one fp32 addition each."""
    h = x.float().cpu().clone()
    for i in range(part.shape[0]):
        h = h + part[i].float().cpu()
    return h


def lnp_gelu_bound(y64, rows_bound, c, pi, bf16):
    """GV_LNP has one epilogue, GV_GELU_WT, so a selection launch shows the normalised row y as gelu(c y_pi) in the engine dtype. With the staged
    y within rows_bound (step_model.ln_rows_bound) of y64 and c a power of two (c y exact), the mean value theorem puts gelu(c y) within
    GELU_SLOPE |c| rows_bound of gelu(c y64); the output adds one engine-dtype ulp of the result (the fp32 engine's GELU is the one-ulp form) and,
    in the bf16 / e4m3 engines, the fp32 evaluation behind the bf16 rounding (step_model.gelu_bound_fp32). Every term is an existing bound; the
    float32 restatement is held to it on these inputs by tests/test_gemv_bounds_cpu.py. Returns (gelu64(c y64_pi), bound), [1, N] each."""
    u = c[None, :] * y64[:, pi]
    ref = SM.gelu_erf64(u)
    tol = GELU_SLOPE * c.abs()[None, :] * rows_bound[:, pi] + SM.ulp(ref, bf16)
    return ref, tol + SM.gelu_bound_fp32(u) if bf16 else tol


def sparse_rows(N, K, nnz, seed, dt):
    """N weight rows with nnz Gaussian entries each, in the dtype dt (step_cases.xattn_random_inputs' Wq: a projection whose fp32 rounding stays a few
    ulps, so that the attention bound is not drowned by K 2^-24 sum |W||y|)."""
    g = gen(seed)
    W = torch.zeros(N, K)
    cols = torch.stack([torch.randperm(K, generator=g)[:nnz] for _ in range(N)])
    W[torch.arange(N)[:, None], cols] = torch.randn(N, nnz, generator=g) / math.sqrt(nnz)
    return W.to(dt).to(F64)


# qkv_attn_kernel: (mode, H, heads, kv_heads, S, M) - bf16 at the three widths, fp32 at 512 / 1024, e4m3 at 512 / 1024; S in {1, 2, 4, 8};
# M in {1, 3, 8} (bf16); one grouped-query shape
QKV_SHAPES = (
    (GV_BF16, 512, 8, 8, 1, 1), (GV_BF16, 512, 8, 8, 2, 8), (GV_BF16, 1024, 16, 16, 4, 3), (GV_BF16, 1024, 16, 4, 2, 1), (GV_BF16, 1536, 24, 24, 8, 1),
    (GV_F32, 512, 8, 8, 2, 1), (GV_F32, 1024, 16, 16, 8, 1), (GV_BF16_W8, 512, 8, 4, 4, 1), (GV_BF16_W8, 1024, 16, 16, 1, 3),
)


def qkv_positions(mode, S, kv_bound):
    """New-token positions: 0, 1, one row group below / at / above S * rows_per_split (where a split's second K/V batch begins) where kv_bound
    leaves room, and the last position below kv_bound."""
    rpi = epl(mode)
    edge = S * rows_per_split(mode)
    return sorted({p for p in (0, 1, edge - rpi, edge, edge + rpi, kv_bound - 1) if 0 <= p < kv_bound})


def qkv_kv_bound(mode, S):
    """A context bucket that reaches into the second K/V batch of every split, kept small: one row group and a ragged row past S * rows_per_split."""
    return S * rows_per_split(mode) + 2 * epl(mode) + 3


# xfold_attn_kernel: (mode, H, heads); nur 2 and 4; n_valid in XFOLD_VALID
XFOLD_SHAPES = ((GV_F32, 512, 8), (GV_BF16, 512, 8), (GV_BF16, 1024, 16), (GV_BF16, 1536, 24))
XFOLD_VALID = (1, 37, 64)
# xq_attn_kernel: (mode, H, heads, kv_heads, M); description lengths XQ_DESC in an arena of XQ_CAP positions (300: a second K/V batch)
XQ_SHAPES = ((GV_BF16, 512, 8, 8, 1), (GV_BF16, 1024, 16, 8, 3), (GV_BF16, 1536, 24, 24, 8), (GV_F32, 512, 8, 8, 1), (GV_F32, 1024, 16, 16, 1),
             (GV_BF16_W8, 512, 8, 8, 8), (GV_BF16_W8, 1024, 16, 16, 3))
XQ_DESC = (1, 80, 300)
XQ_CAP = 320
