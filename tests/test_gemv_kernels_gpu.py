"""The row-per-wave GEMV decode step called directly (tests/native/gemv_harness.hip) against exact results and the float64 restatements of
tests/step_model.py / tests/attn_model.py, at the shapes of tests/gemv_cases.py: gemv_kernel on every template instance gemv_step reaches,
qkv_attn_kernel, xfold_attn_kernel and xq_attn_kernel. The pattern and the helpers (Guarded, twice, nanpad, assert_bits) are
tests/step_helpers.py's.

gemv_kernel is pinned by the three constructions of the step tests:
 (a) Exact: small-integer W (e4m3 mode: such values times a power-of-two row scale), integer activations or gamma = 0 with integer beta, exact
     split partials (gemv_cases.exact_combine_partials), equal scores over 2^j positions (exact_softmax_inputs), integer residual: every partial
     sum is a multiple of 2^-6 below 2^18, so the output equals the float64 product bit for bit in any order. GV_GELU_WT: weight rows scaled by
     powers of two so that the accumulators land in (-3, 3], output within one ulp of the engine dtype of the float64 function.
 (b) Selection: one non-zero c in {+-1, +-2, +-1/2} per W row at a permuted column exposes the prepared row of every utterance exactly.
 (c) Random: Gaussian W and rows against the float64 product of the rows really staged, within step_model.gemm_bound.
Every output buffer sits between sentinels and holds MB utterances' rows of which only the M live ones may change; input rows are padded with NaN;
weights are followed by NaN; every launch runs twice with bitwise equal results."""
import collections
import functools
import math
import time

import numpy as np
import pytest
import torch

import gemv_cases as GC
import gemv_harness as GH
import step_harness as SH
import step_model as SM
import step_helpers as T
from attn_model import combine_splits, decoder_attention
from gemv_harness import (GV_ATTN, GV_ATTN2, GV_BF16, GV_BF16_W8, GV_COPY, GV_F32, GV_GELU_WT, GV_LN, GV_LNP, GV_RESID, GV_SOFTMAX, GV_STORE, PTTS_OK)
from helpers import log_parity
from step_helpers import Guarded, assert_bits, nanpad

pytestmark = pytest.mark.gpu

LOG = "gemv_kernels_parity.txt"
DEV = "cuda"
F64 = torch.float64
EXACT = collections.Counter()   # kernel family -> exact launches (each run twice and compared whole)
WORST = {}                      # family -> largest error / bound
FLIPS = collections.defaultdict(lambda: [0, 0])
FLIP_CAP = 1e-3
EXACT_QSCALE = 0.125            # a.scale * log2(e) as the kernels' fp32 product gives it: exactly 2^-3 (tests/attn_cases.py)
EXACT_SCALE = float(np.float32(0.125) / np.float32(1.44269504088896340736))
assert np.float32(np.float32(EXACT_SCALE) * np.float32(1.44269504088896340736)) == np.float32(0.125)
STEP_EPI = {GV_STORE: SH.EPI_STORE, GV_RESID: SH.EPI_RESID, GV_GELU_WT: SH.EPI_GELU_WT}


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    t0 = time.time()
    h = GH.Harness(GH.build(str(tmp_path_factory.mktemp("gemv_harness"))))
    log_parity(f"[gemv harness] built in {time.time() - t0:.0f} s (product objects reused: {', '.join(GH.build.reused) or 'none'})", LOG)
    yield h
    for fam, n in sorted(EXACT.items()):
        log_parity(f"[exact] {fam}: {n} launches, each run twice and compared whole", LOG)
    for fam, r in sorted(WORST.items()):
        log_parity(f"[error / bound] {fam}: largest {r:.3e}", LOG)
    for fam, (f, n) in sorted(FLIPS.items()):
        log_parity(f"[flip share] {fam}: {f} of {n} bf16 elements differ from RNE(float64) = {f / max(n, 1):.2e} (cap {FLIP_CAP:.0e})", LOG)


@pytest.fixture(autouse=True)
def _wall(request):
    t0 = time.time()
    yield
    log_parity(f"[wall] {request.node.name}: {time.time() - t0:.1f} s", LOG)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bf(mode):
    return mode != GV_F32


def _edt(mode):
    return torch.bfloat16 if _bf(mode) else torch.float32


def _worst(fam, r):
    WORST[fam] = max(WORST.get(fam, 0.0), r)


def twice(H, fam, launch, outs, exact=True):
    T.twice(H, fam, launch, outs, exact=False)
    if exact:
        EXACT[fam] += 1


def dev(t, dtype=None):
    return t.to(device=DEV, dtype=dtype).contiguous()


def tail_nan(t, n=256):
    """A flat device copy of t followed by n NaN elements (bytes: 0x7f, the e4m3 NaN): a read past the end spreads into the results."""
    flat = t.reshape(-1)
    if flat.dtype == torch.uint8:
        b = torch.full((flat.numel() + n,), 0x7F, dtype=torch.uint8, device=DEV)
    else:
        b = torch.full((flat.numel() + n,), float("nan"), dtype=flat.dtype, device=DEV)
    b[:flat.numel()] = flat.to(DEV)
    return b


def weights(mode, W, exact):
    """W [N, K] float64 -> (device buffer, bytes described, wscale buffer or None, the float64 weights the kernel reads)."""
    if mode == GV_BF16_W8:
        b8, sc, deq = SM.e4m3_rows(W)
        if exact:
            assert torch.equal(deq, W), "the exact weights are representable in e4m3 x a power-of-two row scale"
        return tail_nan(b8), b8.numel(), tail_nan(sc.float()), deq
    dt = _edt(mode)
    Wd = W.to(dt)
    if exact:
        assert torch.equal(Wd.to(F64), W)
    return tail_nan(Wd), Wd.numel() * Wd.element_size(), None, Wd.to(F64)


@functools.lru_cache(maxsize=8)
def int_weights(N, K, lo, hi):
    return GC.ints((N, K), 7 * N + K, lo, hi)


class Node:
    """One gemv_kernel launch through gvh_gemv: its operands on the device, its output between sentinels with room for MB utterances."""

    def __init__(self, H, case, W, exact=True, separate_resid=False, resid=None):
        self.H, self.case = H, case
        self.pro, self.epi, self.S, self.M, self.N, self.K, self.mode = case
        pro, epi, S, M, N, K, mode = case
        self.inst = GC.instance_of(*case)
        assert self.inst is not None, case
        self.MB = self.inst[6]
        a = self.a = GH.GvhGemv()
        a.mode, a.pro, a.epi, a.S, a.M, a.N, a.K = mode, pro, epi, S, M, N, K
        self.keep = []
        self.wbuf, a.n_W, self.wsc, self.W = weights(mode, W, exact)
        a.W = self.wbuf.data_ptr()
        if self.wsc is not None:
            a.wscale, a.n_wscale = self.wsc.data_ptr(), N
        self.rows = None
        self.ld = N + 8
        odt = _edt(mode) if epi == GV_GELU_WT else torch.float32
        self.resid = None
        init = None
        if epi == GV_RESID:
            self.resid = resid if resid is not None else GC.ints((M, N), 11 * N + M, -1000, 1000)
            rdev = dev(self.resid, torch.float32)
            if separate_resid:  # out starts as sentinels; the residual operand is a buffer of its own, NaN past its logical width
                rb = torch.full((self.MB * self.ld,), float("nan"), device=DEV)
                rb.view(self.MB, self.ld)[:M, :N] = rdev
                a.resid, a.n_resid = rb.data_ptr(), rb.numel()
                self.keep.append(rb)
            else:
                ld = self.ld

                def init(v):
                    v.view(-1, ld)[:M, :N].copy_(rdev)
        self.out = Guarded(self.MB * self.ld, odt, init=init)
        a.out, a.out_ld, a.n_out = self.out.ptr(), self.ld, self.MB * self.ld
        self.outs = [self.out]
        self.hsum = None

    # ---- prologue operands ----
    def ln(self, x, gamma, beta, rows):
        a, K = self.a, self.K
        xb, gb, bb = nanpad(x, K + 8, torch.float32), tail_nan(gamma.float()), tail_nan(beta.float())
        a.x, a.x_ld, a.n_x, a.gamma, a.beta, a.n_gamma = xb.data_ptr(), K + 8, xb.numel(), gb.data_ptr(), bb.data_ptr(), K
        self.keep += [xb, gb, bb]
        self.rows = rows
        return self

    def copy(self, rows):
        a, K = self.a, self.K
        xb = nanpad(rows, K + 16, _edt(self.mode))
        a.xw, a.xw_ld, a.n_xw = xb.data_ptr(), K + 16, xb.numel()
        self.keep.append(xb)
        self.rows = xb[:, :K].double().cpu()
        return self

    def attn(self, part, stats, rows):
        a = self.a
        pb, sb = tail_nan(part.float()), tail_nan(stats.float())
        a.part, a.stats, a.n_part, a.n_stats, a.nheads = pb.data_ptr(), sb.data_ptr(), part.numel(), stats.numel(), self.K // 64
        self.keep += [pb, sb]
        self.rows = rows
        return self

    def softmax(self, scores, mask, n_valid, ne, rows):
        a = self.a
        xb, nv = tail_nan(scores.float()), torch.tensor([n_valid], dtype=torch.int32, device=DEV)
        a.x, a.n_x, a.n_valid, a.ne = xb.data_ptr(), self.K, nv.data_ptr(), ne
        self.keep += [xb, nv]
        if mask is not None:
            mb = dev(mask, torch.int32)
            a.mask, a.n_mask = mb.data_ptr(), mask.numel()
            self.keep.append(mb)
        self.rows = rows
        return self

    def lnp(self, x, part, gamma, beta, rows, part_ptr=None):
        a, K = self.a, self.K
        xb, gb, bb = tail_nan(x.float()), tail_nan(gamma.float()), tail_nan(beta.float())
        a.x, a.x_ld, a.n_x, a.gamma, a.beta, a.n_gamma = xb.data_ptr(), K, K, gb.data_ptr(), bb.data_ptr(), K
        self.keep += [xb, gb, bb]
        if part_ptr is None:
            pb = tail_nan(part.float())
            self.keep.append(pb)
            part_ptr = pb.data_ptr()
        a.part, a.n_part, a.npart = part_ptr, part.shape[0] * K, part.shape[0]
        self.hsum = Guarded(K, torch.float32)
        a.hsum, a.n_hsum = self.hsum.ptr(), K
        self.outs.append(self.hsum)
        self.rows = rows
        return self

    def family(self):
        return f"gemv<{GH.MODE_NAMES[self.mode]}, {GH.PRO_NAMES[self.pro]}, {GH.EPI_NAMES[self.epi]}>"

    def run(self, exact=True):
        twice(self.H, self.family(), lambda: self.H.gemv(self.a, _stream()), self.outs, exact=exact)
        return self

    def live(self):
        """The live rows [M, N] of the output as float64 on the CPU, after checking that nothing else was written."""
        idx = torch.arange(self.M)[:, None] * self.ld + torch.arange(self.N)[None, :]
        self.out.untouched_outside(idx, f"{self.family()} {self.case}")
        return self.out.t[idx.to(DEV)].double().cpu()

    def check_exact(self, tag):
        """(a): rows >= N, columns past N, utterances >= M and everything around stay sentinels; the rest equals the float64 result."""
        M, N, ld = self.M, self.N, self.ld
        acc = self.rows.to(F64) @ self.W.t()
        assert float((self.rows.to(F64).abs() @ self.W.abs().t()).max()) < 2 ** 18, "every partial sum stays exact in fp32"
        if self.epi == GV_GELU_WT:
            return T.check_epilogue(tag, self.out, M, N, ld, 0, STEP_EPI[self.epi], _bf(self.mode), acc)
        ref = acc + (self.resid if self.resid is not None else 0)
        assert float(ref.abs().max()) < 2 ** 24
        assert_bits(self.out.bits(), self.out.expected(lambda v: v.view(-1, ld)[:M, :N].copy_(ref.float())), f"{tag}: output")
        return "exact"


def exact_node(H, case, seed, separate_resid=False):
    """Construction (a) for one case."""
    pro, epi, S, M, N, K, mode = case
    narrow = pro in (GV_ATTN, GV_ATTN2, GV_SOFTMAX)
    W = int_weights(N, K, -4 if narrow else -8, 4 if narrow else 8)
    if pro == GV_LN:
        x, gamma, beta = GC.ln_inputs(M, K, seed)[0], torch.zeros(K), GC.ints((K,), seed + 1).float()
        rows = beta.to(F64)[None, :].expand(M, K)
    elif pro == GV_COPY:
        rows = GC.ints((M, K), seed)
    elif pro in (GV_ATTN, GV_ATTN2):
        part, stats, rows = GC.exact_combine_partials(M, K, S, seed, pro == GV_ATTN2)
    elif pro == GV_SOFTMAX:
        sc, mask, nv, p = GC.exact_softmax_inputs(K // 64, 64, seed)
        rows = p[None, :]
    else:
        x, gamma, beta = torch.randint(-8, 9, (K,), generator=GC.gen(seed)).float(), torch.zeros(K), GC.ints((K,), seed + 1).float()
        part = torch.randint(-8, 9, (K // 64, K), generator=GC.gen(seed + 2)).float()
        rows = beta.to(F64)[None, :]
    if epi == GV_GELU_WT:
        W, _ = GC.scale_into_gelu_range(W, rows.to(F64) @ W.t())
    n = Node(H, case, W, separate_resid=separate_resid)
    if pro == GV_LN:
        n.ln(x, gamma, beta, rows)
    elif pro == GV_COPY:
        n.copy(rows)
    elif pro in (GV_ATTN, GV_ATTN2):
        n.attn(part, stats, rows)
    elif pro == GV_SOFTMAX:
        n.softmax(sc, mask, nv, 64, rows)
    else:
        n.lnp(x, part, gamma, beta, rows)
        n.hsum_ref = lnp_row_sum(x, part)
    return n


lnp_row_sum = GC.lnp_row_sum


def check_hsum(n, ref, tag):
    assert_bits(n.hsum.bits(), n.hsum.expected(lambda v: v.copy_(ref.to(DEV))), f"{tag}: hsum against x + the partial rows in index order")


# ---- (a) every instance of the case table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", GH.MODES, ids=lambda m: GH.MODE_NAMES[m])
@pytest.mark.parametrize("pro", sorted(GH.PRO_NAMES), ids=lambda p: GH.PRO_NAMES[p])
def test_gemv_exact_on_every_reached_instance(H, pro, mode):
    cases = [c for c in GC.gemv_cases() if c[0] == pro and c[6] == mode]
    if not cases:
        assert pro == GV_SOFTMAX and mode == GV_BF16_W8  # the folded matrices are never e4m3: gemv_step has no such node
        return
    for i, case in enumerate(cases):
        for sep in ((False, True) if case[1] == GV_RESID else (False,)):
            n = exact_node(H, case, 2000 + i, separate_resid=sep).run()
            tag = f"{n.family()} S={case[2]} M={case[3]} N={case[4]} K={case[5]} instance {n.inst}{' resid apart' if sep else ''}"
            n.check_exact(tag)
            if pro == GV_LNP:
                check_hsum(n, n.hsum_ref, tag)


@pytest.mark.parametrize("pro", (GV_LN, GV_LNP), ids=lambda p: GH.PRO_NAMES[p])
def test_gelu_wt_of_the_fp32_engine_within_one_ulp(H, pro):
    """The regression case of gv_gelu_erf_wt<float>. With gv_gelu_erf - 0.5 x (1 + erff(x / sqrt 2)) in fp32, which cancels in 1 + erf for x < 0 -
    the fp32 engine's GV_GELU_WT outputs were 23.13 (GV_LN) and 6.22 (GV_LNP) fp32 ulps of the float64 value away on the first exact case of the
    instance table (N = 5, K = 512, measured on an MI355X); the bf16 and e4m3 engines' were within one bf16 ulp. Now 0.5 x erfc(-x / sqrt 2) in
    double, rounded once (the strip kernels' gelu_erf_wt<float>). Its bar is the one-ulp bar of every GV_GELU_WT case of the instance test above."""
    for N, K in ((5, 512), (1029, 512), (4099, 1024)):
        case = (pro, GV_GELU_WT, 1, 1, N, K, GV_F32)
        n = exact_node(H, case, 2600 + N).run()
        n.check_exact(f"{n.family()} N={N} K={K}, one ulp")


@pytest.mark.parametrize("case", GC.group_cases(), ids=lambda c: f"{GH.MODE_NAMES[c[6]]}-K{c[5]}-M{c[3]}")
def test_gemv_staged_and_register_group_instances(H, case):
    """The staged MB = 8 instance and the instances that pass the activations through the registers in groups, at 5 and 8 utterances: groups past
    the live batch leave no trace (their rows of the output stay sentinels), every live utterance gets its own row."""
    for sep in (False, True):
        n = exact_node(H, case, 2500 + case[3], separate_resid=sep).run()
        n.check_exact(f"{n.family()} M={case[3]} K={case[5]} instance {n.inst} groups {GC.groups_of(n.inst)}")


# ---- (b) the prepared rows ---------------------------------------------------------------------------------------------------------------------------
def expose(H, mode, pro, S, M, K, seed, stage, epi=None):
    """Construction (b): run the node once per selection matrix; stage(node) hands it the prologue operands. Returns rows [M, K] float64."""
    N = 256
    epi = epi if epi is not None else (GV_STORE if pro == GV_LN else GV_RESID)
    rows = torch.full((M, K), float("nan"), dtype=F64)
    for W, pi, c in GC.selection_weights(N, K, seed):
        n = Node(H, (pro, epi, S, M, N, K, mode), W, resid=torch.zeros(M, N, dtype=F64))
        stage(n)
        n.run(exact=False)
        rows[:, pi] = n.live() / c[None, :]
    assert not bool(torch.isnan(rows).any()), "a column was never selected, or a staged element is NaN"
    return rows


@functools.lru_cache(maxsize=None)
def ln_ref(M, K, seed):
    x, gamma, beta = GC.ln_inputs(M, K, seed)
    y64 = SM.layer_norm64(x, gamma, beta)
    bar, _ = SM.ln_tolerance_fp32(x, gamma, beta, y64)
    return x, gamma, beta, y64, bar


def check_rows(tag, fam, y, y64, bar, bf16):
    assert bool(torch.isfinite(y).all()), f"{tag}: NaN / inf in a prepared row"
    tol = SM.ln_rows_bound(y64, bar, bf16)
    err = (y - y64).abs()
    if bf16:
        FLIPS[fam][0] += int((y != SM.round_engine(y64, True)).sum())
        FLIPS[fam][1] += y.numel()
    r = float((err / tol).max())
    _worst(fam, r)
    print(f"{tag}: max |y - y64| {float(err.max()):.3e}, fp32 bar {bar:.3e}, error / bound {r:.3f}")
    assert r <= 1.0, f"{tag}: {int((err > tol).sum())} prepared elements beyond the bound, worst {r:.2f} x"


def staged_ln_rows(H, mode, M, K, seed):
    """The rows the GV_LN prologue stages for ln_inputs(M, K, seed), exposed by selection; cached per test session."""
    key = (mode, M, K, seed)
    if key not in staged_ln_rows.cache:
        x, gamma, beta, y64, _ = ln_ref(M, K, seed)
        staged_ln_rows.cache[key] = expose(H, mode, GV_LN, 1, M, K, seed + 1, lambda n: n.ln(x, gamma, beta, y64))
    return staged_ln_rows.cache[key]


staged_ln_rows.cache = {}


@pytest.mark.parametrize("mode", GH.MODES, ids=lambda m: GH.MODE_NAMES[m])
def test_gemv_layer_norm_rows_and_random(H, mode):
    """(b) and (c) of GV_LN: the staged rows of 1, 3 and 8 utterances (slab waves / MB = 4 / MB = 8) against float64 under step_model.ln_rows_bound,
    then Gaussian weights against the float64 product of those rows under step_model.gemm_bound."""
    fam = f"gemv<{GH.MODE_NAMES[mode]}, LN>"
    for K in (512, 1024, 1536):
        for M in ((1,) if mode == GV_F32 else (1, 3, 8)):
            x, gamma, beta, y64, bar = ln_ref(M, K, 3000 + M)
            y = staged_ln_rows(H, mode, M, K, 3000 + M)
            check_rows(f"{fam} K={K} M={M}", fam, y, y64, bar, _bf(mode))
            Wg = torch.randn(70, K, generator=GC.gen(3100 + M)).to(_edt(mode)).to(F64)
            n = Node(H, (GV_LN, GV_STORE, 1, M, 70, K, mode), Wg, exact=False).ln(x, gamma, beta, y).run(exact=False)
            r = float(((n.live() - y @ n.W.t()).abs() / SM.gemm_bound(n.W, y)).max())
            _worst(fam + " random", r)
            assert r <= 1.0, f"{fam} random K={K} M={M}: error / bound {r:.3f}"
    if _bf(mode):
        f, n_ = FLIPS[fam]
        assert f <= FLIP_CAP * n_, f"{fam}: {f} of {n_} bf16 elements differ from RNE(float64): above {FLIP_CAP:.0e}"


@pytest.mark.parametrize("mode", GH.MODES, ids=lambda m: GH.MODE_NAMES[m])
def test_gemv_copy_random(H, mode):
    """(c) of GV_COPY + GV_RESID: Gaussian weights, rows and residual; K = 4096 at 8 utterances is the staged instance."""
    fam = f"gemv<{GH.MODE_NAMES[mode]}, COPY> random"
    for K, M in ((512, 1), (1024, 3), (4096, 8), (6144, 5)) if mode != GV_F32 else ((512, 1), (4096, 1)):
        g = GC.gen(3200 + K + M)
        rows = torch.randn(M, K, generator=g).to(_edt(mode)).to(F64)
        Wg = (torch.randn(70, K, generator=g) / math.sqrt(K)).to(_edt(mode)).to(F64)
        rs = torch.randn(M, 70, generator=g).float().to(F64)
        n = Node(H, (GV_COPY, GV_RESID, 1, M, 70, K, mode), Wg, exact=False, resid=rs).copy(rows).run(exact=False)
        ref = rs + rows @ n.W.t()
        r = float(((n.live() - ref).abs() / (SM.gemm_bound(n.W, rows) + SM.U32 * ref.abs())).max())
        _worst(fam, r)
        assert r <= 1.0, f"{fam} K={K} M={M}: error / bound {r:.3f}"


def attn2_as_splits(part, stats):
    """GV_ATTN2's slot S as one more split: maximum s0 + s1 (the two half dot products), sumexp 1."""
    st = stats.to(F64).clone()
    st[:, -1, :, 0] = stats[:, -1, :, 0].to(F64) + stats[:, -1, :, 1].to(F64)
    st[:, -1, :, 1] = 1.0
    return part.to(F64), st


@pytest.mark.parametrize("mode", (GV_F32, GV_BF16), ids=lambda m: GH.MODE_NAMES[m])
@pytest.mark.parametrize("pro", (GV_ATTN, GV_ATTN2), ids=lambda p: GH.PRO_NAMES[p])
def test_gemv_split_combine_rows(H, pro, mode):
    """(b) of GV_ATTN (S = 2, 4, 8) and GV_ATTN2 (S = 1, 2, 4, 8) at M = 1 (slab waves), 3 and 8: the combined rows against
    attn_model.combine_splits under step_model.combine_tolerance; splits whose maximum is -inf, a head without cache rows, and (GV_ATTN2) every
    cache split empty: the first decode position."""
    fam = f"gemv<{GH.MODE_NAMES[mode]}, {GH.PRO_NAMES[pro]}>"
    new = pro == GV_ATTN2
    for K in (512, 1536):
        for S in ((1, 2, 4, 8) if new else (2, 4, 8)):
            for M in ((1,) if mode == GV_F32 else (1, 3, 8)):
                if not GC.dispatch_ok(pro, GV_RESID, S, M, mode):
                    continue
                for pos0 in ((False, True) if new else (False,)):
                    part, stats = GC.random_combine_partials(M, K, S, 3300 + S + M, new, pos0)
                    y = expose(H, mode, pro, S, M, K, 3310 + S, lambda n: n.attn(part, stats, None))
                    ps = attn2_as_splits(part, stats) if new else (part, stats)
                    ref, tol = SM.combine_tolerance(ps[0], ps[1], _bf(mode))
                    assert bool(torch.isfinite(y).all())
                    err = (y - ref).abs()  # a head without a live slot has the bound 0: its row must be 0 exactly
                    r = float(torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err))).max())
                    _worst(fam, r)
                    assert r <= 1.0, f"{fam} K={K} S={S} M={M} pos0={pos0}: error / bound {r:.3f}"
                    if pos0:  # nothing but the new position: the V row itself
                        assert torch.equal(y, SM.round_engine(part[:, S].to(F64), _bf(mode)))


@pytest.mark.parametrize("mode", (GV_F32, GV_BF16), ids=lambda m: GH.MODE_NAMES[m])
def test_gemv_softmax_rows_exact(H, mode):
    """(b) of GV_SOFTMAX with ne = 32 and 64 and n_valid in {1, ne - 3, ne}, on gemv_cases.tiered_softmax: scores that differ inside a head by
    whole units in an order of their own per head, head maxima 512 units apart from neighbour to neighbour, a mask with holes, NaN scores wherever
    no head may look - every exposed weight is 2^-o / T or 0 exactly; a mask without a kept position gives 0 everywhere. The mask and n_valid
    are shared by the heads: a masked head is a masked row. Scores at arbitrary real distances need a tolerance of their own (4 x a float32
    restatement) and its CPU proof; they are not part of this file."""
    fam = f"gemv<{GH.MODE_NAMES[mode]}, SOFTMAX>"
    for ne, nh in ((64, 8), (32, 16), (64, 24)):
        K = nh * ne
        if GC.instance_of(GV_SOFTMAX, GV_RESID, 1, 1, 256, K, mode) is None:
            continue
        for nv in (1, ne - 3, ne):
            for all_masked in (False, True):
                s, o, mask, p = GC.tiered_softmax(nh, ne, nv, 3400 + ne + nv, all_masked)
                sc = GC.tiered_scores(s, o)
                y = expose(H, mode, GV_SOFTMAX, 1, 1, K, 3410 + ne, lambda n: n.softmax(sc, mask, nv, ne, None))
                assert torch.equal(y, p[None, :]), f"{fam} ne={ne} n_valid={nv} all_masked={all_masked}: {int((y != p[None, :]).sum())} weights differ from 2^-o / T"
                EXACT[fam] += 1


@pytest.mark.parametrize("mode", GH.MODES, ids=lambda m: GH.MODE_NAMES[m])
def test_gemv_lnp_rows_and_row_sum(H, mode):
    """(b) of GV_LNP with npart = 8, 16, 24: hsum bit-equal to the fp32 statement (x, then the rows in index order). The node has one epilogue,
    GV_GELU_WT, so the normalised row y shows as gelu(c y) in the engine dtype: held to step_model.ln_rows_bound carried through the GELU
    (gemv_cases.lnp_gelu_bound; tests/test_gemv_bounds_cpu.py holds the float32 restatement to it on these inputs and shows that a row sum
    without its last partial row, or a LayerNorm without beta, exceeds it)."""
    fam = f"gemv<{GH.MODE_NAMES[mode]}, LNP>"
    bf = _bf(mode)
    for K, npart in GC.LNP_SHAPES:
        if GC.instance_of(GV_LNP, GV_GELU_WT, 1, 1, 256, K, mode) is None or (mode == GV_F32 and K != 512):
            continue
        x, part, gamma, beta = GC.lnp_inputs(K, npart)
        hs = lnp_row_sum(x, part)
        y64 = SM.layer_norm64(hs[None, :], gamma, beta)
        bar, _ = SM.ln_tolerance_fp32(hs[None, :], gamma, beta, y64)
        for W, pi, c in GC.selection_weights(256, K, 3510 + K):
            n = Node(H, (GV_LNP, GV_GELU_WT, 1, 1, 256, K, mode), W).lnp(x, part, gamma, beta, None).run(exact=False)
            check_hsum(n, hs, f"{fam} K={K} npart={npart}")
            got = n.live()
            ref, tol = GC.lnp_gelu_bound(y64, SM.ln_rows_bound(y64, bar, bf), c, pi, bf)
            assert bool(torch.isfinite(got).all())
            r = float(((got - ref).abs() / tol).max())
            _worst(fam, r)
            assert r <= 1.0, f"{fam} K={K} npart={npart}: error / bound {r:.3f}"


# ---- qkv_attn_kernel -----------------------------------------------------------------------------------------------------------------------------
class QkvRig:
    """Operands of one qkv_attn_kernel launch: M utterances whose new tokens sit at positions pos[b] in caches of cap > kv_bound rows. Every cache row
    at or past an utterance's new position holds NaN (the arena is uninitialised memory in the product)."""

    def __init__(self, H, shape, pos, seed):
        self.H = H
        self.mode, self.Hd, self.nh, self.nkv, self.S, self.M = shape
        mode, Hd, nh, nkv, S, M = shape
        self.bf, self.dt = _bf(mode), _edt(mode)
        self.kv_bound = GC.qkv_kv_bound(mode, S)
        self.cap = self.kv_bound + 8
        self.P = 5 if pos >= 5 else 0
        self.mask_ld = 8
        self.pos = [max(self.P, pos - 2 * b) for b in range(M)]
        self.cur_len = torch.tensor([p - self.P + 1 for p in self.pos], dtype=torch.int32)
        self.mask = torch.ones(M, self.mask_ld, dtype=torch.int32)
        self.mask[M - 1, :2] = 0                      # a padded head of the last utterance's prompt
        self.mask[:, self.P:] = 0                     # flags past the prompt do not count
        self.g = GC.gen(seed)
        self.rows = Hd + 2 * nkv * 64
        t = torch.arange(self.cap)
        self.before = torch.stack([t < p for p in self.pos])                                       # [M, cap]: rows in place
        self.vis = self.before & ((t[None, :] >= self.P) | (torch.nn.functional.pad(self.mask, (0, self.cap - self.mask_ld), value=1) != 0))

    def launch(self, x, gamma, beta, W, Kc, Vc, scale, fam, exact):
        """Kc / Vc [M, nkv, cap, 64] float64 (engine-dtype values); rows at or past pos[b] are overwritten with NaN. Returns (part [M, S + 1, H],
        stats [M, S + 1, heads, 2], K / V caches after the launch [M, nkv, cap, 64]) as float64 on the CPU; only row pos[b] of the caches may differ."""
        M, Hd, nh, nkv, S, cap = self.M, self.Hd, self.nh, self.nkv, self.S, self.cap
        nan = torch.full((), float("nan"), dtype=F64)
        keep = self.before[:, None, :, None]
        Kn, Vn = torch.where(keep, Kc, nan).to(self.dt), torch.where(keep, Vc, nan).to(self.dt)
        kdev, vdev = dev(Kn), dev(Vn)
        idt = torch.int16 if self.bf else torch.int32

        def seed_cache(src):
            return lambda v: v.copy_(src.reshape(-1))
        kc, vc = Guarded(Kn.numel(), self.dt, init=seed_cache(kdev)), Guarded(Vn.numel(), self.dt, init=seed_cache(vdev))
        part, stats = Guarded(M * (S + 1) * Hd, torch.float32), Guarded(M * (S + 1) * nh * 2, torch.float32)
        a = GH.GvhQkvAttn()
        wbuf, a.n_W, wsc, Wr = weights(self.mode, W, exact)
        xb, gb, bb = nanpad(x, Hd + 8, torch.float32), tail_nan(gamma.float()), tail_nan(beta.float())
        cl, Pd, mk = dev(self.cur_len), torch.tensor([self.P], dtype=torch.int32, device=DEV), dev(self.mask)
        self.keep = (wbuf, wsc, xb, gb, bb, cl, Pd, mk, kdev, vdev)
        a.W, a.x, a.gamma, a.beta, a.kcache, a.vcache = wbuf.data_ptr(), xb.data_ptr(), gb.data_ptr(), bb.data_ptr(), kc.ptr(), vc.ptr()
        if wsc is not None:
            a.wscale, a.n_wscale = wsc.data_ptr(), self.rows
        a.cur_len, a.P, a.mask, a.part, a.stats = cl.data_ptr(), Pd.data_ptr(), mk.data_ptr(), part.ptr(), stats.ptr()
        a.n_x, a.n_gamma, a.n_cache, a.n_cur_len, a.n_mask, a.n_part, a.n_stats = xb.numel(), Hd, Kn.numel(), M, mk.numel(), part.n, stats.n
        a.mode, a.S, a.M, a.H, a.nheads, a.kv_heads, a.x_ld = self.mode, S, M, Hd, nh, nkv, Hd + 8
        a.cap, a.kv_bound, a.mask_ld, a.scale = cap, self.kv_bound, self.mask_ld, scale
        twice(self.H, fam, lambda: self.H.qkvattn(a, _stream()), [kc, vc, part, stats], exact=exact)
        # (ii) nothing but row pos[b] of each K/V head changed, and nothing around the four buffers
        for cache, src, nm in ((kc, kdev, "K"), (vc, vdev, "V")):
            got = cache.buf.clone()
            exp = cache.expected(lambda v: None)
            for b in range(M):
                for kh in range(nkv):
                    o = cache.pre + ((b * nkv + kh) * cap + self.pos[b]) * 64
                    got[o:o + 64] = exp[o:o + 64]
            assert_bits(got, exp, f"{fam}: {nm} cache elements other than the new position's row changed")
        part.untouched_outside(torch.arange(part.n), fam)
        stats.untouched_outside(torch.arange(stats.n), fam)
        self.Wr = Wr
        return (part.t.view(M, S + 1, Hd).double().cpu(), stats.t.view(M, S + 1, nh, 2).double().cpu(),
                kc.t.view(M, nkv, cap, 64).double().cpu(), vc.t.view(M, nkv, cap, 64).double().cpu())

    def new_rows(self, cache):
        return torch.stack([cache[b, :, self.pos[b]] for b in range(self.M)])                      # [M, nkv, 64]


@pytest.mark.parametrize("shape", GC.QKV_SHAPES, ids=lambda s: f"{GH.MODE_NAMES[s[0]]}-H{s[1]}-kv{s[3]}-S{s[4]}-M{s[5]}")
def test_qkv_attn_exact(H, shape):
    """(i) - (iii), (v), (vi) on integer data: gamma = 0 and a sparse +-1 beta make the staged row exact, integer k / v rows give integer K / V
    rows (|k| <= 32 * 8 = 256: representable in bf16). Counting case: zero q rows give every visible position the score 0, so per head the summed
    sumexp of the cache splits is exactly the number of visible positions and the summed partial exactly the sum of their (integer) V rows: a row
    dropped or counted twice by the interleaved split assignment, or a position at / past the new one counted in, fails bit for bit. Then non-zero
    integer q rows at the scale that makes the kernels' fp32 product exactly 2^-3: the two half dot products of slot S are exact."""
    mode, Hd, nh, nkv, S, M = shape
    fam = f"qkv_attn<{GH.MODE_NAMES[mode]}>"
    n_rep = nh // nkv
    for pos in GC.qkv_positions(mode, S, GC.qkv_kv_bound(mode, S)):
        rig = QkvRig(H, shape, pos, 4000 + pos)
        g = rig.g
        x = GC.ln_inputs(M, Hd, 4001 + pos)[0]
        beta = torch.zeros(Hd)
        beta[torch.randperm(Hd, generator=g)[:32]] = torch.where(torch.rand(32, generator=g) < 0.5, -1.0, 1.0)
        Wkv = GC.ints((2 * nkv * 64, Hd), 4002)
        Kc = torch.randint(-8, 9, (M, nkv, rig.cap, 64), generator=g).to(F64)
        # V row t holds the three base-16 digits of t (+ 1) in its columns d % 3 == 0 / 1 / 2: the rows are distinct over the whole context
        # (cap < 16^3), and the column sums of an 8- or 4-row group name the group, so one group dropped and another counted twice cannot cancel.
        # Values stay <= 16 + 7 + 46 (exact in bf16), sums below 2^18 (exact in fp32).
        assert rig.cap < 16 ** 3
        digit = (torch.arange(rig.cap)[:, None] // (16 ** (torch.arange(64) % 3))[None, :]) % 16
        Vc = (1 + digit).to(F64)[None, None].expand(M, nkv, rig.cap, 64).clone()
        Vc = Vc + torch.arange(M)[:, None, None, None] + 2 * torch.arange(nkv)[None, :, None, None]    # distinct per utterance and K/V head
        for counting in ((True, False) if pos == GC.qkv_positions(mode, S, rig.kv_bound)[-1] else (True,)):
            Wq = torch.zeros(Hd, Hd, dtype=F64) if counting else GC.ints((Hd, Hd), 4003)
            W = torch.cat((Wq, Wkv))
            tag = f"{fam} H={Hd} kv={nkv} S={S} M={M} pos={rig.pos} {'counting' if counting else 'integer q'}"
            part, stats, Ka, Va = rig.launch(x, torch.zeros(Hd), beta, W, Kc, Vc, EXACT_SCALE, fam, True)
            qkv = beta.to(F64)[None, :] @ W.t()                                                     # [1, rows]: the same for every utterance
            q, k, v = qkv[0, :Hd], qkv[0, Hd:Hd + nkv * 64], qkv[0, Hd + nkv * 64:]
            k_row, v_row = SM.round_engine(k, rig.bf).view(nkv, 64), SM.round_engine(v, rig.bf).view(nkv, 64)
            assert torch.equal(k_row, k.view(nkv, 64)) and torch.equal(v_row, v.view(nkv, 64))
            # (i) the appended rows
            assert torch.equal(rig.new_rows(Ka), k_row[None].expand(M, nkv, 64)), f"{tag}: K row at the new position"
            assert torch.equal(rig.new_rows(Va), v_row[None].expand(M, nkv, 64)), f"{tag}: V row at the new position"
            # (vi)
            assert bool(torch.isfinite(part).all()) and bool((torch.isfinite(stats) | (stats == -math.inf)).all()), f"{tag}: NaN in part / stats"
            # (iii) slot S: the V row of the head's K/V head, and the two half dot products (q / 8) . k
            assert torch.equal(part[:, S], v_row.repeat_interleave(n_rep, dim=0).reshape(1, Hd).expand(M, Hd)), f"{tag}: slot S partial"
            halves = (q.view(nh, 2, 32) * EXACT_QSCALE * k_row.repeat_interleave(n_rep, dim=0).view(nh, 2, 32)).sum(dim=2)
            assert torch.equal(stats[:, S], halves[None].expand(M, nh, 2)), f"{tag}: slot S half dot products"
            if not counting:
                continue
            # (v) counting
            cnt = rig.vis.sum(dim=1).to(F64)                                                        # [M]
            vsum = (Vc * rig.vis[:, None, :, None]).sum(dim=2)                                      # [M, nkv, 64]
            assert torch.equal(stats[:, :S, :, 1].sum(dim=1), cnt[:, None].expand(M, nh)), f"{tag}: summed sumexp {stats[:, :S, :, 1].sum(dim=1)[:, 0]} != visible {cnt}"
            assert torch.equal(part[:, :S].sum(dim=1), vsum.repeat_interleave(n_rep, dim=1).reshape(M, Hd)), f"{tag}: summed partials != sum of the visible V rows"
            mx = stats[:, :S, :, 0]
            assert bool(((mx == 0) | ((mx == -math.inf) & (stats[:, :S, :, 1] == 0))).all()), f"{tag}: split maxima"


@pytest.mark.parametrize("shape", GC.QKV_SHAPES, ids=lambda s: f"{GH.MODE_NAMES[s[0]]}-H{s[1]}-kv{s[3]}-S{s[4]}-M{s[5]}")
def test_qkv_attn_random(H, shape):
    """(iv): Gaussian caches, a real LayerNorm on rows that differ per utterance, sparse Gaussian projection rows. The kernel's S + 1 slots, combined
    in float64, against attn_model.decoder_attention on the cache as the launch left it (the new position's rows included), evaluated on the rows the
    GV_LN prologue stages for the same x (the same gv_ln_row statistics: no LayerNorm term in the bound) - within step_model.xattn_tolerance:
    attn_model.tolerance plus the q-projection term."""
    mode, Hd, nh, nkv, S, M = shape
    fam = f"qkv_attn<{GH.MODE_NAMES[mode]}> random"
    n_rep = nh // nkv
    kvb = GC.qkv_kv_bound(mode, S)
    for pos in (GC.qkv_positions(mode, S, kvb)[-1], S * GC.rows_per_split(mode) - 3):
        rig = QkvRig(H, shape, pos, 4100 + pos)
        x, gamma, beta, _, _ = ln_ref(M, Hd, 3000 + M)
        y = staged_ln_rows(H, mode, M, Hd, 3000 + M)
        W = GC.sparse_rows(rig.rows, Hd, 16, 4101, rig.dt)
        Kc = torch.randn(M, nkv, rig.cap, 64, generator=rig.g).to(rig.dt).to(F64)
        Vc = torch.randn(M, nkv, rig.cap, 64, generator=rig.g).to(rig.dt).to(F64)
        part, stats, Ka, Va = rig.launch(x, gamma, beta, W, Kc, Vc, 0.125, fam, False)
        assert bool(torch.isfinite(part).all())
        got = combine_splits(*attn2_as_splits(part, stats))
        Wq = rig.Wr[:Hd]
        q = y @ Wq.t()
        m = decoder_attention(q.view(M, nh, 64), Kc, Vc, Q=1, n_rep=n_rep, P=rig.P, N=0, cur_len=rig.cur_len, cross=False, mask=rig.mask, scale=0.125,
                              cos=None, sin=None, bf16=rig.bf, S=1, NW=8, new_k=rig.new_rows(Ka), new_v=rig.new_rows(Va))
        m["y"] = y
        seen = (torch.arange(rig.cap)[None, :] <= torch.tensor(rig.pos)[:, None])[:, None, :, None]
        Kseen = torch.where(seen, torch.nan_to_num(Ka, nan=0.0), torch.zeros((), dtype=F64))
        # bf16=False: the partials and statistics are fp32 and are combined here in float64 - no output is rounded to the engine dtype (the
        # engine-dtype rounding of the K / V rows is in the cache the model reads)
        tol = SM.xattn_tolerance(m, Wq, Kseen, N=max(rig.pos) + 1, n_rep=n_rep, scale=0.125, bf16=False)
        r = float(((got - m["out"]).abs() / tol).max())
        print(f"{fam} H={Hd} S={S} M={M} pos={rig.pos}: error / bound {r:.3e}")
        _worst(fam, r)
        assert r <= 1.0


# ---- xfold_attn_kernel -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GC.XFOLD_SHAPES, ids=lambda s: f"{GH.MODE_NAMES[s[0]]}-H{s[1]}")
def test_xfold_attn_exact_and_chain_into_lnp(H, shape):
    """xpart[h] on exact data - gamma = 0 and a sparse +-1 beta stage an integer row, the rows of Mw give the scores of gemv_cases.tiered_softmax
    (they differ from position to position in an order of their own per head, head maxima 512 units apart between neighbours, decoys 50 units
    above the maximum on the positions that n_valid in {1, 37, 64} or the mask's holes hide), Uw holds small integers:
    xpart[h][n] = sum_t Uw[n][64 h + t] 2^-o[h][t] / T bit for bit, for nur = 2 and 4. Then the chain into GV_LNP on the kernel's own partial rows:
    hsum is bit-equal to x plus those rows in index order. Scores at arbitrary real distances against float64 need a tolerance of their own and
    its CPU proof; they are not part of this file."""
    mode, Hd, nh = shape
    fam = f"xfold_attn<{GH.MODE_NAMES[mode]}>"
    bf, dt = _bf(mode), _edt(mode)
    for nur in (2, 4):
        for nv in GC.XFOLD_VALID:
            g = GC.gen(5000 + Hd + nv)
            x = GC.ln_inputs(1, Hd, 5001 + nv)[0]
            beta = torch.zeros(Hd)
            cols = torch.randperm(Hd, generator=g)[:32]
            beta[cols] = torch.where(torch.rand(32, generator=g) < 0.5, -1.0, 1.0)
            beta[cols[0]] = 1.0
            # row (h, t) of Mw = +-8 beta + (h % 5 - o[h][t]) e_j with beta_j = 1: its score is s_h - o[h][t] (tiered_softmax), an integer; the rows
            # of the positions no head may look at score 50 above the head's maximum instead
            s, o, mask, p = GC.tiered_softmax(nh, 64, nv, 5005 + Hd + nv)
            sgn = torch.where(torch.arange(nh) % 2 == 0, 8.0, -8.0).to(F64)
            Mw = (sgn[:, None, None] * beta.to(F64)[None, None, :]).expand(nh, 64, Hd).clone()
            Mw[:, :, cols[0]] += (torch.arange(nh) % 5).to(F64)[:, None] + torch.where(o >= 0, -o.to(F64), torch.full((), 50.0, dtype=F64))
            assert torch.equal(Mw @ beta.to(F64), torch.where(o >= 0, s[:, None] - o.to(F64), s[:, None] + 50.0))
            Mw = Mw.reshape(nh * 64, Hd)
            Uw = GC.ints((Hd, nh * 64), 5003)
            a = GH.GvhXfold()
            mb, ub = tail_nan(Mw.to(dt)), tail_nan(Uw.to(dt))
            xb, gb, bb = tail_nan(x[0].float()), tail_nan(torch.zeros(Hd)), tail_nan(beta)
            nvd, mk = torch.tensor([nv], dtype=torch.int32, device=DEV), dev(mask)
            xpart = Guarded(nh * Hd, torch.float32)
            a.Mw, a.Uw, a.x, a.gamma, a.beta, a.n_valid, a.mask, a.xpart = mb.data_ptr(), ub.data_ptr(), xb.data_ptr(), gb.data_ptr(), bb.data_ptr(), nvd.data_ptr(), mk.data_ptr(), xpart.ptr()
            a.n_Mw, a.n_Uw, a.n_x, a.n_gamma, a.n_mask, a.n_xpart = Mw.numel(), Uw.numel(), Hd, Hd, 64, nh * Hd
            a.mode, a.H, a.nheads, a.nur = mode, Hd, nh, nur
            twice(H, fam, lambda: H.xfoldattn(a, _stream()), [xpart])
            ref = torch.einsum("nht,ht->hn", Uw.view(Hd, nh, 64), p.view(nh, 64))
            assert_bits(xpart.bits(), xpart.expected(lambda v: v.copy_(ref.float().reshape(-1))), f"{fam} H={Hd} nur={nur} n_valid={nv}: xpart")
            # the chain: GV_LNP reads the kernel's own rows
            mode_l = mode
            case = (GV_LNP, GV_GELU_WT, 1, 1, 70, Hd, mode_l)
            xr, gamma, bt = GC.ln_inputs(1, Hd, 5004 + nv)
            n = Node(H, case, torch.randn(70, Hd, generator=g).to(dt).to(F64), exact=False)
            n.lnp(xr[0], xpart.t.view(nh, Hd), gamma, bt, None, part_ptr=xpart.ptr()).run(exact=False)
            check_hsum(n, lnp_row_sum(xr[0], xpart.t.view(nh, Hd)), f"{fam} -> GV_LNP H={Hd} nur={nur} n_valid={nv}")
            assert bool(torch.isfinite(n.live()).all())


# ---- xq_attn_kernel ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GC.XQ_SHAPES, ids=lambda s: f"{GH.MODE_NAMES[s[0]]}-H{s[1]}-kv{s[3]}-M{s[4]}")
def test_xq_attn_random(H, shape):
    """Against step_model.cross_block64 (no rotation) on the rows the GV_LN prologue stages for the same x, under step_model.xattn_tolerance - the
    bound of the fused cross block of the step tests. Description lengths 1, 80 and 300 (a second K/V batch) in an arena of 320 positions whose rows
    past the length hold NaN; ragged masks; with 3 or more utterances one of them is fully masked and yields 0."""
    mode, Hd, nh, nkv, M = shape
    fam = f"xq_attn<{GH.MODE_NAMES[mode]}>"
    bf, dt, cap = _bf(mode), _edt(mode), GC.XQ_CAP
    n_rep = nh // nkv
    x, gamma, beta, _, _ = ln_ref(M, Hd, 3000 + M)
    y = staged_ln_rows(H, mode, M, Hd, 3000 + M)
    for N in GC.XQ_DESC:
        g = GC.gen(6000 + N + M)
        Wq = GC.sparse_rows(Hd, Hd, 16, 6001, dt)
        Kc = torch.randn(M, nkv, cap, 64, generator=g).to(dt).to(F64)
        Vc = torch.randn(M, nkv, cap, 64, generator=g).to(dt).to(F64)
        mask = (torch.rand(M, cap, generator=g) < 0.7).int()
        mask[:, 0] = 1
        if M >= 3:
            mask[1] = 0
        past = (torch.arange(cap) >= N)[None, None, :, None]
        nan = torch.full((), float("nan"), dtype=F64)
        a = GH.GvhXq()
        wbuf, a.n_W, wsc, Wr = weights(mode, Wq, False)
        xb, gb, bb = nanpad(x, Hd + 8, torch.float32), tail_nan(gamma.float()), tail_nan(beta.float())
        kd, vd = dev(torch.where(past, nan, Kc).to(dt)), dev(torch.where(past, nan, Vc).to(dt))
        mk, nvd = dev(mask), torch.tensor([N], dtype=torch.int32, device=DEV)
        out = Guarded(M * (Hd + 8), dt)
        a.W, a.x, a.gamma, a.beta, a.kcache, a.vcache, a.mask, a.n_valid, a.out = (wbuf.data_ptr(), xb.data_ptr(), gb.data_ptr(), bb.data_ptr(), kd.data_ptr(),
                                                                                   vd.data_ptr(), mk.data_ptr(), nvd.data_ptr(), out.ptr())
        if wsc is not None:
            a.wscale, a.n_wscale = wsc.data_ptr(), Hd
        a.n_x, a.n_gamma, a.n_cache, a.n_mask, a.n_out = xb.numel(), Hd, kd.numel(), mk.numel(), out.n
        a.mode, a.M, a.H, a.nheads, a.kv_heads, a.x_ld, a.out_ld, a.mask_ld, a.cap, a.scale = mode, M, Hd, nh, nkv, Hd + 8, Hd + 8, cap, cap, 0.125
        twice(H, fam, lambda: H.xqattn(a, _stream()), [out], exact=False)
        idx = torch.arange(M)[:, None] * (Hd + 8) + torch.arange(Hd)[None, :]
        out.untouched_outside(idx, fam)
        got = out.t[idx.to(DEV)].double().cpu()
        assert bool(torch.isfinite(got).all()), f"{fam} H={Hd} M={M} N={N}: NaN / inf in the output"
        m = SM.cross_block64(x, gamma, beta, Wr, Kc, Vc, n_rep=n_rep, N=N, P=0, cur_len=None, mask=mask, scale=0.125, cos=None, sin=None, bf16=bf, y=y)
        tol = SM.xattn_tolerance(m, Wr, Kc, N=N, n_rep=n_rep, scale=0.125, bf16=bf)
        if M >= 3:
            assert torch.equal(got[1], torch.zeros(Hd, dtype=F64)), f"{fam}: a fully masked utterance must yield 0"
        r = float(((got - m["out"]).abs() / tol.clamp_min(1e-300)).max()) if M < 3 else float(((got - m["out"]).abs()[[i for i in range(M) if i != 1]] / tol[[i for i in range(M) if i != 1]]).max())
        print(f"{fam} H={Hd} M={M} N={N}: error / bound {r:.3e}")
        _worst(fam, r)
        assert r <= 1.0
