"""The batched decode-step kernels called directly (tests/native/step_harness.hip) against exact results and a float64 restatement
(tests/step_model.py), at the shapes of tests/step_cases.py: rows_prep_kernel, the strip GEMMs with every prologue / epilogue pair of strip_path
(fragment-order rows, one M pass per blockIdx.z, strip statistics, PRO_LNS, the e4m3 strips), lnproj_fused_kernel and xattn_fused_kernel.

LayerNorm cannot be made integer-exact, so the LayerNorm + GEMM nodes are pinned by three constructions:
 (a) GEMM-exact: gamma = 0 and beta = small integers make the normalised row beta exactly, whatever the statistics; W holds small integers, so every
     partial sum of K <= 1536 products stays an integer below 2^24 and the output equals the float64 product bit for bit in any accumulation order
     (the argument of test_gemm_kernels_gpu.py). Through a GELU epilogue the weight rows are scaled by powers of two so that the accumulators land
     in (-3, 3]; an EPI_GELU_WT output is then within one ulp of the engine dtype of the float64 function (the fp32 intermediate of EPI_GELU:
     inside the bound of an fp32 evaluation of the formula, step_model.gelu_bound_fp32).
 (b) Selection: every W row has one non-zero entry c in {+-1, +-2, +-1/2} at column pi(n), so out[m][n] = c * (the normalised element the kernel
     staged), exactly: the rows that never reach memory become visible bit for bit, per utterance.
 (c) Random: Gaussian W and x against the float64 GEMM of the rows the kernel really staged, within K 2^-24 sum |W||x|.
The fp32 LayerNorm bar of a case is 4 x the error of the float32 torch restatement on the same inputs (step_model.ln_tolerance_fp32); bf16 rows are
within one bf16 ulp + that bar of float64, and at most 1e-3 of them differ from its round-to-nearest-even value (tests/test_step_model_cpu.py shows
the float32 restatement stays below 5e-4 on these inputs). Every buffer sits between sentinels that must survive - fragment-order buffers hold
ceil(M / 16) * 16 rows whose rows past M stay sentinels - and every launch runs twice with bitwise equal results."""
import collections
import functools
import math
import time

import pytest
import torch

import step_cases as SC
import step_harness as SH
import step_model as SM
from helpers import log_parity
from step_helpers import DEV, EXACT, F64, Guarded, _edt, act_rows, assert_bits, check_epilogue, nanpad, twice
from step_harness import (EPI_GELU, EPI_GELU_WT, EPI_RESID, EPI_STORE, PRO_ATTN, PRO_COPY, PRO_LN, PRO_LNS, PRO_PLAIN, PTTS_OK)

pytestmark = pytest.mark.gpu

LOG = "step_kernels_parity.txt"
WORST = {}                          # family -> largest error / bound of the random cases
FLIPS = collections.defaultdict(lambda: [0, 0])  # family -> [bf16 elements that differ from RNE(float64), elements]
FLIP_CAP = 1e-3


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    t0 = time.time()
    h = SH.Harness(SH.build(str(tmp_path_factory.mktemp("step_harness"))))
    log_parity(f"[step harness] built in {time.time() - t0:.0f} s ({len(SH.parts())} parts)", LOG)
    yield h
    for fam, n in sorted(EXACT.items()):
        log_parity(f"[exact] {fam}: {n} launches, each run twice and compared whole", LOG)
    for fam, r in sorted(WORST.items()):
        log_parity(f"[random] {fam}: largest error / bound {r:.3e}", LOG)
    for fam, (f, n) in sorted(FLIPS.items()):
        log_parity(f"[flip share] {fam}: {f} of {n} bf16 elements differ from RNE(float64) = {f / max(n, 1):.2e} (cap {FLIP_CAP:.0e})", LOG)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _eng(bf16):
    return "bf16" if bf16 else "fp32"


def _worst(fam, r):
    WORST[fam] = max(WORST.get(fam, 0.0), r)


def pack(H, bf16, W):
    N, K = W.shape
    p = torch.empty(N * K, device=DEV, dtype=_edt(bf16))
    Wf = W.to(device=DEV, dtype=torch.float32).contiguous()
    assert H.pack(bf16, Wf.data_ptr(), p.data_ptr(), N, K, _stream()) == PTTS_OK, H.error()
    torch.cuda.synchronize()
    return p


def pack_w8(H, b8):
    N, K = b8.shape
    src = b8.to(DEV).contiguous()
    dst = torch.empty(N * K, device=DEV, dtype=torch.uint8)
    assert H.pack_w8(src.data_ptr(), dst.data_ptr(), N, K, _stream()) == PTTS_OK, H.error()
    torch.cuda.synchronize()
    return dst


def act_size(M, K, ld, fo):
    return (M + 15) // 16 * 16 * K if fo else M * ld


# ---- LayerNorm references, computed once per (M, K, seed) -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_ref(M, K, seed):
    x, gamma, beta = SC.ln_inputs(M, K, seed)
    y64 = SM.layer_norm64(x, gamma, beta)
    bar, err32 = SM.ln_tolerance_fp32(x, gamma, beta, y64)
    return x, gamma, beta, y64, bar, err32


def check_ln_rows(tag, fam, y, y64, bar, bf16):
    """The exposed normalised rows y (engine-dtype values as float64, on the CPU) against float64."""
    assert bool(torch.isfinite(y).all()), f"{tag}: NaN / inf in a real row"
    err = (y - y64).abs()
    tol = SM.ln_rows_bound(y64, bar, bf16)
    if bf16:
        FLIPS[fam][0] += int((y != SM.round_engine(y64, True)).sum())
        FLIPS[fam][1] += y.numel()
    r = float((err / tol).max())
    log_parity(f"[ln rows] {tag}: max |y - y64| {float(err.max()):.3e}, fp32 bar {bar:.3e}, error / bound {r:.3f}", LOG)
    assert r <= 1.0, f"{tag}: {int((err > tol).sum())} normalised elements beyond the bound, worst {r:.2f} x"


def check_flips(fam):
    f, n = FLIPS[fam]
    print(f"{fam}: flip share {f} / {n}")
    assert f <= FLIP_CAP * n, f"{fam}: {f} of {n} bf16 elements differ from RNE(float64): above {FLIP_CAP:.0e}"


# ---- one strip GEMM with any prologue / epilogue -----------------------------------------------------------------------------------------------------
class Strip:
    """One strip GEMM out[m][n] = epilogue(sum_k W[n][k] rows[m][k]) through sh_gemm, with the operands of its prologue on the device."""

    def __init__(self, H, bf16, pro, epi, M, N, K, seed, x_fo=0, out_fo=0, w8=0, decode=1, S=2, rows=None, W=None, ln=None, stats=False, resid=None):
        self.H, self.bf16, self.pro, self.epi, self.M, self.N, self.K = H, bf16, pro, epi, M, N, K
        self.x_fo, self.out_fo, self.w8 = x_fo, out_fo, w8
        dt = _edt(bf16)
        a = self.a = SH.ShGemm()
        a.M, a.N, a.K, a.decode, a.x_row_mul, a.x_fo, a.out_fo = M, N, K, decode, 1, x_fo, out_fo
        self.keep = []
        if pro in (PRO_LN, PRO_LNS):  # construction (a) unless the caller brings (x, gamma, beta) and the rows they give
            x, gamma, beta = ln if ln is not None else SC.exact_ln_inputs(M, K, seed)
            self.rows = rows if rows is not None else beta.to(F64)[None, :].expand(M, K)
            xb = nanpad(x, K + 8, torch.float32)
            gb, bb = gamma.to(DEV), beta.to(DEV)
            a.x, a.x_ld, a.gamma, a.beta = xb.data_ptr(), K + 8, gb.data_ptr(), bb.data_ptr()
            self.keep += [xb, gb, bb]
            if pro == PRO_LNS and ln is None:  # any finite statistics do: the row is beta whatever they are
                st = torch.rand(M, K // 16, 2, generator=SC.gen(seed + 7)).float().to(DEV) + 0.5
                a.lnstat = st.data_ptr()
                self.keep.append(st)
        elif pro == PRO_ATTN:
            part, stats_in, self.rows = SC.exact_attn_partials(M, K, S, seed)
            pb, sb = part.to(DEV), stats_in.to(DEV)
            a.part, a.stats, a.S, a.nheads = pb.data_ptr(), sb.data_ptr(), S, K // 64
            self.keep += [pb, sb]
        else:
            self.rows = rows if rows is not None else SC.ints((M, K), seed, -2 if stats else -8, 2 if stats else 8)
            if pro == PRO_PLAIN:
                xb = nanpad(self.rows, K + 8, torch.float32)
                a.x_ld = K + 8
            elif x_fo:
                xb = SM.to_fo(self.rows.to(dt), bf16).to(DEV)
                a.x_ld = K
            else:
                xb = nanpad(self.rows, K + 16, dt)
                a.x_ld = K + 16
            a.x = xb.data_ptr()
            self.keep.append(xb)
        self.W = W if W is not None else (SC.sparse_int_weights(N, K, seed + 3) if stats else SC.ints((N, K), seed + 3))
        self.acc = self.rows @ self.W.t()
        if W is None and epi in (EPI_GELU, EPI_GELU_WT):
            self.W, self.acc = SC.scale_into_gelu_range(self.W, self.acc)
        Wdev = self.W
        if w8:  # e4m3 strips: bytes + row scales carry the weights; W carries them only for the fallback (w8 = 2), else a different matrix
            b8, sc, deq = SM.e4m3_rows(self.W)
            assert torch.equal(deq, self.W), "the exact weights are representable in e4m3 x a power-of-two row scale"
            if w8 == 2:
                b8 = SM.e4m3_rows(self.W + torch.sign(self.W) * self.W.abs().amax(dim=1, keepdim=True))[0]  # different bytes: a used W8 would show
            else:
                Wdev = self.W + 1.0
            p8, scd = pack_w8(H, b8), sc.float().to(DEV)
            a.W8, a.wscale = p8.data_ptr(), scd.data_ptr()
            self.keep += [p8, scd]
        self.packed = pack(H, bf16, Wdev)
        a.W = self.packed.data_ptr()
        wt = epi == EPI_GELU_WT
        self.out_ld = N if out_fo else N + 8
        self.resid = None
        if epi == EPI_RESID:
            self.resid = resid if resid is not None else SC.ints((M, N), seed + 5, -8 if stats else -1000, 8 if stats else 1000)
        init = None
        if self.resid is not None:  # the pad columns keep their sentinel: only the residual columns are initialised
            rdev, ld = self.resid.float().to(DEV), self.out_ld

            def init(v):
                v.view(M, ld)[:, :N].copy_(rdev)
        self.out = Guarded(act_size(M, N, self.out_ld, out_fo), dt if wt else torch.float32, init=init)
        a.out, a.out_ld = self.out.ptr(), self.out_ld
        self.outs = [self.out]
        self.stats_out = None
        if stats:
            self.stats_out = Guarded(M * (N // 16) * 2, torch.float32)
            a.stats_out = self.stats_out.ptr()
            self.outs.append(self.stats_out)

    def family(self):
        return f"gemm_strip<{_eng(self.bf16)}{', e4m3' if self.w8 == 1 else ''}, {SH.PRO_NAMES[self.pro]}, {SH.EPI_NAMES[self.epi]}>"

    def run(self, exact=True):
        twice(self.H, self.family(), lambda: self.H.gemm(self.bf16, self.pro, self.epi, self.a, _stream()), self.outs, exact=exact)
        return self

    def check(self, tag):
        msg = check_epilogue(tag, self.out, self.M, self.N, self.out_ld, self.out_fo, self.epi, self.bf16, self.acc, self.resid)
        if self.stats_out is not None:
            st = SM.strip_stats64(self.acc + self.resid)
            assert_bits(self.stats_out.bits(), self.stats_out.expected(lambda v: v.copy_(st.float().reshape(-1))), f"{tag}: strip statistics")
        return msg


def expose_rows(H, bf16, M, K, seed, launch_with):
    """Construction (b): run the node under test once per selection matrix and put the normalised rows it staged back together, exactly.
    launch_with(packed W, N, out Guarded, out_ld) -> status. Returns rows [M, K] float64 (CPU)."""
    N = 256
    rows = torch.full((M, K), float("nan"), dtype=F64)
    for W, pi, c in SC.selection_weights(N, K, seed):
        p = pack(H, bf16, W)
        out = Guarded(M * (N + 8), torch.float32)
        twice(H, "selection", lambda: launch_with(p, N, out, N + 8), [out], exact=False)
        o = out.t.view(M, N + 8)
        assert_bits(out.bits(), out.expected(lambda v: v.view(M, N + 8)[:, :N].copy_(o[:, :N])), "selection: writes outside the output")
        rows[:, pi] = o[:, :N].double().cpu() / c[None, :]
    assert not bool(torch.isnan(rows).any()), "a column was never selected, or a staged element is NaN"
    return rows


# ---- rows_prep_kernel<PRO_LN> --------------------------------------------------------------------------------------------------------------------
def prep_ln(H, bf16, M, K, x, gamma, beta, fo, row_mul=1, row_off=0):
    """rows_prep_kernel<WT, PRO_LN> on rows m * row_mul + row_off of x; returns (Guarded dst, rows [M, K] on the device, flat positions)."""
    dt = _edt(bf16)
    xb = nanpad(x, K + 8, torch.float32)
    gb, bb = gamma.to(DEV), beta.to(DEV)
    dst = Guarded(act_size(M, K, K, fo), dt)
    a = SH.ShGemm()
    a.x, a.x_ld, a.gamma, a.beta, a.dst = xb.data_ptr(), K + 8, gb.data_ptr(), bb.data_ptr(), dst.ptr()
    a.M, a.K, a.x_row_mul, a.x_row_off, a.out_fo = M, K, row_mul, row_off, fo
    twice(H, f"rows_prep<{_eng(bf16)}, LN>", lambda: H.rows_prep(bf16, PRO_LN, a, _stream()), [dst], exact=False)
    rows, idx = act_rows(dst, M, K, K, fo, bf16)
    dst.untouched_outside(idx, f"rows_prep M={M} K={K} fo={fo}")
    return dst, rows, idx


@pytest.mark.parametrize("bf16", SC.ENGINES, ids=_eng)
@pytest.mark.parametrize("K", (SC.WIDTH_GENERIC,) + SC.WIDTHS_FULL)
def test_rows_prep_layer_norm(H, K, bf16):
    fam = f"rows_prep<{_eng(bf16)}, LN> K={K}"
    for M in SC.ROWS_COPY_FO:
        x, gamma, beta, y64, bar, _ = ln_ref(M, K, 100 + M)
        _, rm, _ = prep_ln(H, bf16, M, K, x, gamma, beta, 0)
        _, fo, _ = prep_ln(H, bf16, M, K, x, gamma, beta, 1)
        assert torch.equal(rm.view(torch.int16 if bf16 else torch.int32), fo.view(torch.int16 if bf16 else torch.int32)), "row-major and fragment-order rows differ"
        check_ln_rows(f"{fam} M={M}", fam, rm.double().cpu(), y64, bar, bf16)
    # the LM heads' row selection: output row m reads input row 3 m + 2
    x, gamma, beta, y64, bar, _ = ln_ref(27, K, 127)
    _, sel, _ = prep_ln(H, bf16, 9, K, x, gamma, beta, 1, row_mul=3, row_off=2)
    check_ln_rows(f"{fam} rows 3 m + 2", fam, sel.double().cpu(), y64[2::3], bar, bf16)
    if bf16:
        check_flips(fam)


# ---- rows_prep_kernel<PRO_ATTN> and the fused split-KV combine -----------------------------------------------------------------------------------------
def prep_attn(H, bf16, M, K, S, part, stats, fo):
    dt = _edt(bf16)
    pb, sb = part.to(DEV), stats.to(DEV)
    dst = Guarded(act_size(M, K, K, fo), dt)
    a = SH.ShGemm()
    a.part, a.stats, a.S, a.nheads, a.dst, a.M, a.K, a.out_fo, a.x_row_mul = pb.data_ptr(), sb.data_ptr(), S, K // 64, dst.ptr(), M, K, fo, 1
    a.keep = (pb, sb)  # the struct holds raw pointers only
    return dst, a


@pytest.mark.parametrize("bf16", SC.ENGINES, ids=_eng)
@pytest.mark.parametrize("K", (SC.WIDTH_GENERIC, 1024))
def test_split_kv_combine(H, K, bf16):
    fam = f"rows_prep<{_eng(bf16)}, ATTN>"
    for S in (2, 4):
        for M in (9, 17, 33):  # above 8 rows: the rows_prep node; the exact rows are representable in the engine dtype (integers / 2^k)
            part, stats, rows = SC.exact_attn_partials(M, K, S, 300 + M + S)
            for fo in (0, 1):
                dst, a = prep_attn(H, bf16, M, K, S, part, stats, fo)
                twice(H, fam, lambda: H.rows_prep(bf16, PRO_ATTN, a, _stream()), [dst])
                idx = SM.fo_elem_index(M, K, bf16) if fo else torch.arange(M * K).view(M, K)

                def fill(v, idx=idx, rows=rows):
                    v[idx.to(DEV).reshape(-1)] = rows.to(v.dtype).to(DEV).reshape(-1)
                assert_bits(dst.bits(), dst.expected(fill), f"{fam} exact M={M} S={S} fo={fo}")
        for M in SC.ROWS_FUSED:  # up to 8 rows: fused into the out_proj strip
            Strip(H, bf16, PRO_ATTN, EPI_RESID, M, 64, K, 320 + M + S, S=S).run().check(f"gemm_strip<ATTN, RESID> M={M} K={K} S={S}")
    # random partials against attn_model.combine_splits, inside attn_model.tolerance's bound for the combine alone: no dot product (the spread of the
    # split maxima takes absdot's place: the exponent's argument is one fp32 subtraction), no keys, S terms
    g = SC.gen(77)
    M, S, nh = 19, 4, K // 64
    part = torch.randn(M, S, K, generator=g).float()
    stats = torch.stack((torch.randn(M, S, nh, generator=g) * 4.0, torch.rand(M, S, nh, generator=g) * 30.0 + 1.0), dim=3).float()
    stats[:, 2, 1, 0], stats[:, 2, 1, 1] = -math.inf, 0.0
    ref, tol = SM.combine_tolerance(part, stats, bf16)
    for fo in (0, 1):
        dst, a = prep_attn(H, bf16, M, K, S, part, stats, fo)
        twice(H, fam, lambda: H.rows_prep(bf16, PRO_ATTN, a, _stream()), [dst], exact=False)
        rows, idx = act_rows(dst, M, K, K, fo, bf16)
        dst.untouched_outside(idx, f"{fam} random fo={fo}")
        r = float(((rows.double().cpu() - ref).abs() / tol).max())
        print(f"{fam} random K={K} fo={fo}: error / bound {r:.3e}")
        _worst(fam, r)
        assert r <= 1.0


# ---- strips with fused prologues, 1..8 rows ------------------------------------------------------------------------------------------------------
# 384: K % 256 != 0, the non-FULL instances (by value where PTTS_STRIP_PRELOAD says so: the harness launches what launch_strip picks)
@pytest.mark.parametrize("bf16", SC.ENGINES, ids=_eng)
@pytest.mark.parametrize("K", (384, SC.WIDTH_GENERIC) + SC.WIDTHS_FULL)
def test_fused_prologue_strips(H, K, bf16):
    for M in SC.ROWS_FUSED:
        for pro, epi in ((PRO_LN, EPI_STORE), (PRO_LN, EPI_GELU), (PRO_LN, EPI_GELU_WT), (PRO_PLAIN, EPI_RESID)):
            for N in SC.N_COLS:
                for out_fo in ((0, 1) if epi == EPI_GELU_WT and M == 8 else (0,)):
                    Strip(H, bf16, pro, epi, M, N, K, 400 + M + N, out_fo=out_fo).run().check(
                        f"gemm_strip<{SH.PRO_NAMES[pro]}, {SH.EPI_NAMES[epi]}> {_eng(bf16)} M={M} N={N} K={K} out_fo={out_fo}")


@pytest.mark.parametrize("bf16", SC.ENGINES, ids=_eng)
def test_fused_layer_norm_rows(H, bf16):
    """(b) and (c) for the fused LayerNorm prologue at 1..8 rows. One family over the four widths: 12 rows of a single width are too few elements for
    a share of 1e-3 to mean anything (tests/test_step_model_cpu.py aggregates the float32 restatement the same way)."""
    fam = f"gemm_strip<{_eng(bf16)}, LN> fused"
    for K in (384, SC.WIDTH_GENERIC) + SC.WIDTHS_FULL:
        for M in SC.ROWS_FUSED:
            # (b) the rows the fused LayerNorm staged
            x, gamma, beta, y64, bar, _ = ln_ref(M, K, 500 + M)

            def launch_with(p, N, out, out_ld):
                s = Strip(H, bf16, PRO_LN, EPI_STORE, M, N, K, 0, ln=(x, gamma, beta), rows=y64, W=torch.zeros(N, K, dtype=F64))
                s.a.W, s.a.out, s.a.out_ld = p.data_ptr(), out.ptr(), out_ld
                launch_with.keep = s
                return H.gemm(bf16, PRO_LN, EPI_STORE, s.a, _stream())
            y = expose_rows(H, bf16, M, K, 510 + M, launch_with)
            check_ln_rows(f"{fam} M={M}", fam, y, y64, bar, bf16)
            # (c) Gaussian weights against the float64 GEMM of the rows really staged
            Wg = torch.randn(64, K, generator=SC.gen(520 + M)).to(_edt(bf16)).to(F64)
            s = Strip(H, bf16, PRO_LN, EPI_STORE, M, 64, K, 0, ln=(x, gamma, beta), rows=y, W=Wg).run(exact=False)
            got = s.out.t.view(M, 72)[:, :64].double().cpu()
            r = float(((got - s.acc).abs() / SM.gemm_bound(Wg, y)).max())
            print(f"{fam} random M={M}: error / bound {r:.3e}")
            _worst(fam, r)
            assert r <= 1.0
    if bf16:
        check_flips(fam)


# ---- rows_prep + PRO_COPY on fragment-order rows, one M pass per blockIdx.z ---------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", SC.ENGINES, ids=_eng)
@pytest.mark.parametrize("K", SC.WIDTHS_FULL)
def test_copy_strips_on_fragment_order_rows(H, K, bf16):
    for M in SC.ROWS_COPY_FO:
        for epi, N in ((EPI_STORE, 64), (EPI_RESID, 256), (EPI_GELU_WT, 64)):
            for out_fo in ((0, 1) if epi == EPI_GELU_WT else (0,)):
                Strip(H, bf16, PRO_COPY, epi, M, N, K, 600 + M, x_fo=1, out_fo=out_fo).run().check(
                    f"gemm_strip<COPY, {SH.EPI_NAMES[epi]}> {_eng(bf16)} fo M={M} N={N} K={K} out_fo={out_fo}")
        # the two-node path as strip_path chains it: rows_prep writes beta (construction (a)) in fragment order, the strip reads it
        x, gamma, beta = SC.exact_ln_inputs(M, K, 620 + M)
        dst, rows, _ = prep_ln(H, bf16, M, K, x, gamma, beta, 1)
        assert torch.equal(rows.double().cpu(), beta.to(F64)[None, :].expand(M, K)), "rows_prep with gamma = 0 must write beta exactly"
        s = Strip(H, bf16, PRO_COPY, EPI_STORE, M, 64, K, 630 + M, x_fo=1, rows=beta.to(F64)[None, :].expand(M, K).clone())
        s.a.x = dst.ptr()
        s.keep.append(dst)
        s.run().check(f"rows_prep -> gemm_strip<COPY, STORE> {_eng(bf16)} M={M} K={K}")
    for M in (9, 40, 128):  # row-major prepared rows: one pass of up to 32 rows, 4 row tiles, 8 row tiles
        for epi in (EPI_STORE, EPI_RESID, EPI_GELU_WT):
            Strip(H, bf16, PRO_COPY, epi, M, 64, K, 640 + M, x_fo=0).run().check(f"gemm_strip<COPY, {SH.EPI_NAMES[epi]}> {_eng(bf16)} row-major M={M} K={K}")
    # (c) Gaussian data on real LayerNorm rows, K 2^-24 sum |W||x|
    fam = f"gemm_strip<{_eng(bf16)}, COPY> K={K}"
    for M in (17, 65, 128):
        x, gamma, beta, _, _, _ = ln_ref(M, K, 100 + M)
        dst, rows, _ = prep_ln(H, bf16, M, K, x, gamma, beta, 1)
        y = rows.double().cpu()
        Wg = torch.randn(64, K, generator=SC.gen(650 + M)).to(_edt(bf16)).to(F64)
        for epi in (EPI_STORE, EPI_RESID):
            rs = torch.randn(M, 64, generator=SC.gen(660 + M)).to(F64) if epi == EPI_RESID else None
            s = Strip(H, bf16, PRO_COPY, epi, M, 64, K, 0, x_fo=1, rows=y, W=Wg, resid=rs)
            s.a.x = dst.ptr()
            s.run(exact=False)
            got = s.out.t.view(M, 72)[:, :64].double().cpu()
            ref = s.acc + (rs.float().to(F64) if rs is not None else 0)
            bound = SM.gemm_bound(Wg, y) + (SM.U32 * ref.abs() if rs is not None else 0)  # + the rounding of the residual sum
            r = float(((got - ref).abs() / bound).max())
            print(f"{fam} random {SH.EPI_NAMES[epi]} M={M}: error / bound {r:.3e}")
            _worst(fam, r)
            assert r <= 1.0


# ---- EPI_RESID + stats_out, and the PRO_LNS consumer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", SC.ENGINES, ids=_eng)
@pytest.mark.parametrize("K", SC.WIDTHS_FULL)
def test_strip_statistics_and_lns(H, K, bf16):
    fam = f"gemm_strip<{_eng(bf16)}, LNS> K={K}"
    Kin = 512
    for M in SC.ROWS_LNS:
        # producer, exact: sparse integer data, residual + accumulator within |v| <= 32 (step_cases.sparse_int_weights): out and statistics bit for bit
        Strip(H, bf16, PRO_COPY, EPI_RESID, M, K, Kin, 700 + M, x_fo=1, stats=True).run().check(f"gemm_strip<COPY, RESID> + stats_out {_eng(bf16)} M={M} N={K}")
        # producer, random: the statistics against float64 on the kernel's own output rows
        g = SC.gen(710 + M)
        xr = torch.randn(M, Kin, generator=g).to(_edt(bf16)).to(F64)
        Wg = (torch.randn(K, Kin, generator=g) / math.sqrt(Kin)).to(_edt(bf16)).to(F64)
        h0, _, _ = SC.ln_inputs(M, K, 720 + M)  # the residual rows: scales and offsets over two decades
        p = Strip(H, bf16, PRO_COPY, EPI_RESID, M, K, Kin, 0, x_fo=1, stats=True, rows=xr, W=Wg, resid=h0.to(F64)).run(exact=False)
        h = p.out.t.view(M, K + 8)[:, :K].double().cpu()
        assert bool(((h - (p.acc + h0.to(F64))).abs() <= SM.gemm_bound(Wg, xr) + SM.U32 * h.abs()).all())
        st = p.stats_out.t.view(M, K // 16, 2).double().cpu()
        ref, bm, b2 = SM.strip_stats_bounds(h)
        r = max(float(((st[..., 0] - ref[..., 0]).abs() / bm).max()), float(((st[..., 1] - ref[..., 1]).abs() / b2).max()))
        print(f"strip statistics random {_eng(bf16)} M={M} K={K}: error / bound {r:.3e}")
        _worst(f"stats_out<{_eng(bf16)}>", r)
        assert r <= 1.0
        # consumer: PRO_LNS on the producer's own rows and statistics, both still on the device
        _, gamma, beta = SC.ln_inputs(1, K, 730 + M)
        if not SC.lns_fits(M, K, bf16):  # the plan (pro_gemm) keeps rows_prep + PRO_COPY where the M rows do not fit in LDS: the harness declines too
            gb, bb = gamma.to(DEV), beta.to(DEV)
            out = Guarded(M * 72, torch.float32)
            a = SH.ShGemm()
            pk = pack(H, bf16, SC.ints((64, K), 1))
            a.W, a.x, a.x_ld, a.gamma, a.beta, a.lnstat = pk.data_ptr(), p.out.ptr(), K + 8, gb.data_ptr(), bb.data_ptr(), p.stats_out.ptr()
            a.out, a.out_ld, a.M, a.N, a.K, a.x_row_mul, a.decode = out.ptr(), 72, M, 64, K, 1, 1
            assert H.gemm(bf16, PRO_LNS, EPI_STORE, a, _stream()) == SH.PTTS_E_INVALID
            continue
        y_lns = SM.lns_layer_norm64(h, st, gamma, beta)
        y64 = SM.layer_norm64(h, gamma, beta)
        bar, _ = SM.ln_tolerance_fp32(h, gamma, beta, y64)

        def launch_with(pk, N, out, out_ld):
            a = SH.ShGemm()
            gb, bb = gamma.to(DEV), beta.to(DEV)
            launch_with.keep = (gb, bb)
            a.W, a.x, a.x_ld, a.gamma, a.beta, a.lnstat = pk.data_ptr(), p.out.ptr(), K + 8, gb.data_ptr(), bb.data_ptr(), p.stats_out.ptr()
            a.out, a.out_ld, a.M, a.N, a.K, a.x_row_mul, a.decode = out.ptr(), out_ld, M, N, K, 1, 1
            return H.gemm(bf16, PRO_LNS, EPI_STORE, a, _stream())
        y = expose_rows(H, bf16, M, K, 740 + M, launch_with)
        check_ln_rows(f"{fam} M={M} against lns_layer_norm64", fam, y, y_lns, bar, bf16)
        check_ln_rows(f"{fam} M={M} against layer_norm64", fam + " (plain)", y, y64, bar, bf16)
        # (a) through both epilogues of the consumer
        for epi in (EPI_STORE, EPI_GELU_WT):
            for out_fo in ((0, 1) if epi == EPI_GELU_WT else (0,)):
                Strip(H, bf16, PRO_LNS, epi, M, 64, K, 750 + M, out_fo=out_fo).run().check(f"gemm_strip<LNS, {SH.EPI_NAMES[epi]}> {_eng(bf16)} M={M} K={K} out_fo={out_fo}")
    if bf16:
        check_flips(fam)
        check_flips(fam + " (plain)")


# ---- lnproj_fused_kernel -----------------------------------------------------------------------------------------------------------------------
def lnproj_args(M, N, K, x, gamma, beta, packed, out, out_ld, out_fo=0):
    xb = nanpad(x, K + 8, torch.float32)
    gb, bb = gamma.to(DEV), beta.to(DEV)
    a = SH.ShLnProj()
    a.W, a.x, a.gamma, a.beta, a.out = packed.data_ptr(), xb.data_ptr(), gb.data_ptr(), bb.data_ptr(), out.ptr()
    a.M, a.N, a.K, a.x_ld, a.out_ld, a.out_fo = M, N, K, K + 8, out_ld, out_fo
    a.keep = (xb, gb, bb, packed)
    return a


@pytest.mark.parametrize("bf16", SC.ENGINES, ids=_eng)
@pytest.mark.parametrize("K", SC.WIDTHS_FULL)
def test_lnproj_fused(H, K, bf16):
    fam = f"lnproj_fused<{_eng(bf16)}> K={K}"
    dt = _edt(bf16)
    for g, Ms in SC.LNPROJ_ROWS.items():
        for M in Ms:
            # (a) GEMM-exact through both epilogues
            x, gamma, beta = SC.exact_ln_inputs(M, K, 800 + M)
            rows = beta.to(F64)[None, :].expand(M, K)
            for N in SC.N_COLS:
                W = SC.ints((N, K), 810 + M + N)
                out = Guarded(M * (N + 8), torch.float32)
                a = lnproj_args(M, N, K, x, gamma, beta, pack(H, bf16, W), out, N + 8)
                twice(H, fam, lambda: H.lnproj(bf16, EPI_STORE, g, a, _stream()), [out])
                check_epilogue(f"{fam} STORE g={g} M={M} N={N}", out, M, N, N + 8, 0, EPI_STORE, bf16, rows @ W.t())
                Ws, acc = SC.scale_into_gelu_range(W, rows @ W.t())
                for out_fo in (0, 1):
                    ld = N if out_fo else N + 8
                    out = Guarded(act_size(M, N, ld, out_fo), dt)
                    a = lnproj_args(M, N, K, x, gamma, beta, pack(H, bf16, Ws), out, ld, out_fo)
                    twice(H, fam, lambda: H.lnproj(bf16, EPI_GELU_WT, g, a, _stream()), [out])
                    check_epilogue(f"{fam} GELU_WT g={g} M={M} N={N} out_fo={out_fo}", out, M, N, ld, out_fo, EPI_GELU_WT, bf16, acc)
            # (b) the rows the node staged: against float64, and bit for bit against rows_prep_kernel<PRO_LN> on the same x
            x, gamma, beta, y64, bar, _ = ln_ref(M, K, 100 + M if M in SC.ROWS_COPY_FO else 820 + M)

            def launch_with(p, N, out, out_ld):
                launch_with.a = lnproj_args(M, N, K, x, gamma, beta, p, out, out_ld)
                return H.lnproj(bf16, EPI_STORE, g, launch_with.a, _stream())
            y = expose_rows(H, bf16, M, K, 830 + M, launch_with)
            check_ln_rows(f"{fam} g={g} M={M}", fam, y, y64, bar, bf16)
            _, prep, _ = prep_ln(H, bf16, M, K, x, gamma, beta, 0)
            same = torch.equal(y, prep.double().cpu())
            log_parity(f"[ln rows] {fam} g={g} M={M}: rows {'equal' if same else 'DIFFER from'} rows_prep_kernel<PRO_LN>'s bit for bit", LOG)
            assert same, f"{fam} g={g} M={M}: {int((y != prep.double().cpu()).sum())} staged elements differ from rows_prep_kernel<PRO_LN>'s"
            # (c) Gaussian weights on those rows
            Wg = torch.randn(64, K, generator=SC.gen(840 + M)).to(dt).to(F64)
            out = Guarded(M * 72, torch.float32)
            a = lnproj_args(M, 64, K, x, gamma, beta, pack(H, bf16, Wg), out, 72)
            twice(H, fam, lambda: H.lnproj(bf16, EPI_STORE, g, a, _stream()), [out], exact=False)
            r = float(((out.t.view(M, 72)[:, :64].double().cpu() - y @ Wg.t()).abs() / SM.gemm_bound(Wg, y)).max())
            print(f"{fam} random g={g} M={M}: error / bound {r:.3e}")
            _worst(fam, r)
            assert r <= 1.0
    # EPI_STORE with the cache append at a prefill shape: B = 3 utterances x Q = 11 rows, K / V columns behind kv_H = 64 query columns, one K/V head
    B, Q, cap, kvH, nkv = SC.LNPROJ_PREFILL["B"], SC.LNPROJ_PREFILL["Q"], 16, 64, 1
    M, N = B * Q, kvH + 2 * 64 * nkv
    x, gamma, beta = SC.exact_ln_inputs(M, K, 850)
    W = SC.ints((N, K), 851)
    acc = beta.to(F64)[None, :].expand(M, K) @ W.t()
    out, kc, vc = Guarded(M * (N + 8), torch.float32), Guarded(B * nkv * cap * 64, dt), Guarded(B * nkv * cap * 64, dt)
    a = lnproj_args(M, N, K, x, gamma, beta, pack(H, bf16, W), out, N + 8)
    a.kcache, a.vcache, a.kv_Q, a.kv_cap, a.kv_heads, a.kv_H = kc.ptr(), vc.ptr(), Q, cap, nkv, kvH
    twice(H, fam, lambda: H.lnproj(bf16, EPI_STORE, 8, a, _stream()), [out, kc, vc])
    check_epilogue(f"{fam} STORE + cache append", out, M, N, N + 8, 0, EPI_STORE, bf16, acc)
    for cache, c0, nm in ((kc, kvH, "K"), (vc, kvH + 64 * nkv, "V")):
        vals = acc[:, c0:c0 + 64 * nkv].float().to(dt)  # the fp32 result rounded to nearest even, as kv_append_kernel rounds it

        def fill(v, vals=vals):
            v.view(B, nkv, cap, 64)[:, :, :Q] = vals.view(B, Q, nkv, 64).permute(0, 2, 1, 3).to(DEV)
        assert_bits(cache.bits(), cache.expected(fill), f"{fam}: {nm} cache rows")
    if bf16:
        check_flips(fam)


# ---- the e4m3 strips ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", SC.WIDTHS_FULL)
def test_e4m3_strips(H, K):
    for table, w8 in ((SC.W8_CASES, 1), (SC.W8_FALLBACK, 2)):
        for (pro, epi, mtp), (M, fo) in table.items():
            assert SC.mtp_of(pro, M, fo) == mtp
            for N in (64,) if pro != PRO_COPY else (64, 256):
                tag = f"gemm_strip<{'e4m3' if w8 == 1 else 'bf16 fallback'}, {SH.PRO_NAMES[pro]}, {SH.EPI_NAMES[epi]}, {mtp}> M={M} N={N} K={K}"
                Strip(H, True, pro, epi, M, N, K, 900 + M + N, x_fo=fo, w8=w8).run().check(tag)


# ---- GELU_WT outputs of the fp32 engine at one fp32 ulp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", SC.WIDTHS_FULL)
def test_gelu_wt_of_the_fp32_engine_within_one_ulp(H, K):
    """The regression case of gelu_erf_wt<float>. With gelu_erf - 0.5 x (1 + erff(x / sqrt 2)) in fp32, which cancels in 1 + erf for x < 0 - the
    fp32 engine's EPI_GELU_WT outputs were 39 .. 90 fp32 ulps of the float64 value away on these launches (measured on an MI355X, K = 1024 / 1536:
    gemm_strip<fp32, COPY, GELU_WT> 79.85 / 39.82, gemm_strip<fp32, LNS, GELU_WT> 90.01 / 73.77, lnproj_fused_kernel<fp32, ..., GELU_WT>
    39.22 / 61.02, on exact accumulators); the bf16 engine's were within 0.50 bf16 ulp. Now 0.5 x erfc(-x / sqrt 2) in double, rounded once.
    A named regression case: its bar is the one-ulp bar every EPI_GELU_WT check of the family tests above applies."""
    Strip(H, False, PRO_COPY, EPI_GELU_WT, 9, 64, K, 609, x_fo=1).run().check(f"gemm_strip<fp32, COPY, GELU_WT> M=9 K={K}, one ulp")
    Strip(H, False, PRO_LNS, EPI_GELU_WT, 9, 64, K, 759).run().check(f"gemm_strip<fp32, LNS, GELU_WT> M=9 K={K}, one ulp")
    M, N = 9, 64
    x, gamma, beta = SC.exact_ln_inputs(M, K, 800 + M)
    W = SC.ints((N, K), 810 + M + N)
    Ws, acc = SC.scale_into_gelu_range(W, beta.to(F64)[None, :].expand(M, K) @ W.t())
    out = Guarded(M * (N + 8), torch.float32)
    a = lnproj_args(M, N, K, x, gamma, beta, pack(H, False, Ws), out, N + 8)
    twice(H, f"lnproj_fused<fp32> K={K}", lambda: H.lnproj(False, EPI_GELU_WT, 8, a, _stream()), [out])
    check_epilogue(f"lnproj_fused<fp32, GELU_WT> M=9 K={K}, one ulp", out, M, N, N + 8, 0, EPI_GELU_WT, False, acc)


# ---- xattn_fused_kernel ----------------------------------------------------------------------------------------------------------------------------
class XRig:
    """Operands of one xattn_fused_kernel launch: B utterances, description of N tokens in an arena of cap positions."""

    def __init__(self, H, bf16, K, B, gsz, N, n_rep, seed, rope=False, out_fo=0):
        self.H, self.bf16, self.K, self.B, self.gsz, self.N, self.n_rep, self.out_fo = H, bf16, K, B, gsz, N, n_rep, out_fo
        self.nh, self.cap, self.P = K // 64, SC.XATTN_CAP, 3
        self.nkv = self.nh // n_rep
        self.g = SC.gen(seed)
        self.scale = 0.125
        self.cos = self.sin = None
        self.cur_len = torch.randint(1, 20, (B,), generator=self.g).int()
        if rope:
            self.cos, self.sin = SC.rope_tables(self.P + 20)
        # distinct masks per utterance; at least one visible key unless a test says otherwise
        self.mask = (torch.rand(B, self.cap, generator=self.g) < 0.7).int()
        self.mask[torch.arange(B), torch.randint(0, N, (B,), generator=self.g)] = 1

    def launch(self, x, gamma, beta, Wq, Kc, Vc, exact, fam):
        """Kc, Vc [B, nkv, cap, 64] float64 (NaN allowed); returns the output rows [B, K] as float64 on the CPU."""
        dt = _edt(self.bf16)
        B, K = self.B, self.K
        xb = nanpad(x, K + 8, torch.float32)
        dims = SH.DevDims(P=self.P, N=self.N, max_length=64)
        dd = torch.frombuffer(bytearray(bytes(dims)), dtype=torch.uint8).to(DEV)
        dev = [t.to(DEV) if t is not None else None for t in (gamma, beta, Kc.to(dt), Vc.to(dt), self.cur_len, self.mask, self.cos, self.sin)]
        out = Guarded(act_size(B, K, K, self.out_fo), dt)
        a = SH.ShXAttn()
        pk = pack(self.H, self.bf16, Wq)
        self.keep = (xb, dd, dev, pk)
        a.W, a.x, a.gamma, a.beta, a.kcache, a.vcache = pk.data_ptr(), xb.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr()
        a.cur_len, a.dims, a.mask, a.out = dev[4].data_ptr(), dd.data_ptr(), dev[5].data_ptr(), out.ptr()
        if self.cos is not None:
            a.cos, a.sin = dev[6].data_ptr(), dev[7].data_ptr()
        a.B, a.K, a.x_ld, a.x_row_mul, a.cap, a.mask_ld, a.nheads, a.kv_heads, a.n_rep, a.out_fo, a.scale = B, K, K + 8, 1, self.cap, self.cap, self.nh, self.nkv, self.n_rep, self.out_fo, self.scale
        twice(self.H, fam, lambda: self.H.xattn(self.bf16, self.gsz, a, _stream()), [out], exact=exact)
        rows, idx = act_rows(out, B, K, K, self.out_fo, self.bf16)
        out.untouched_outside(idx, fam)
        self.out = out
        return rows.double().cpu()

    def visible(self):
        """[B, cap] bool: the keys utterance b may look at."""
        return (torch.arange(self.cap)[None, :] < self.N) & (self.mask != 0)


def xattn_shapes(K):
    """(gsz, B, N, out_fo) of one width: every group size x its utterance counts; the description lengths and the two output orders cycle over them.
    GQA (n_rep 1 / 2) and RoPE (off / on) are CROSSED with every one of these shapes by the tests."""
    out = []
    groups = SC.XATTN_ROWS if K != SC.WIDTH_GENERIC else {8: SC.XATTN_ROWS[8]}
    i = 0
    for gsz, Bs in groups.items():
        for B in Bs:
            out.append((gsz, B, SC.XATTN_DESC[i % 4], 1 if B > 8 and i % 3 else 0))
            i += 1
    return out


@pytest.mark.parametrize("bf16", SC.ENGINES, ids=_eng)
@pytest.mark.parametrize("K", (SC.WIDTH_GENERIC,) + SC.WIDTHS_FULL)
def test_xattn_fused_exact(H, K, bf16):
    fam = f"xattn_fused<{_eng(bf16)}> K={K}"
    nan = float("nan")
    for gsz, B, N, out_fo in xattn_shapes(K):
        for n_rep in (1, 2):
            tag = f"{fam} g={gsz} B={B} N={N} n_rep={n_rep} out_fo={out_fo}"
            # -- uniform: gamma = beta = 0 -> q = 0 -> the exact mean of the visible V rows (a power-of-two count of them, integer V)
            rig = XRig(H, bf16, K, B, gsz, N, n_rep, 1000 + B + N, rope=n_rep == 2, out_fo=out_fo)
            g = rig.g
            cnt = 1 << int(math.log2(N))
            for b in range(B):  # exactly 2^j visible keys among the first N, different ones per utterance
                rig.mask[b] = 0
                rig.mask[b, torch.randperm(N, generator=g)[:max(1, cnt >> (b % 3))]] = 1
            vis = rig.visible()
            x, _, _ = SC.ln_inputs(B, K, 1010 + B)
            Wq = SC.ints((K, K), 1011)
            Kc = torch.randint(-8, 9, (B, rig.nkv, rig.cap, 64), generator=g).to(F64)
            Vc = torch.randint(-8, 9, (B, rig.nkv, rig.cap, 64), generator=g).to(F64)
            hide = ~vis[:, None, :, None].expand_as(Kc)
            Kn, Vn = torch.where(hide, torch.full((), nan, dtype=F64), Kc), torch.where(hide, torch.full((), nan, dtype=F64), Vc)  # NaN wherever no query may look
            got = rig.launch(x, torch.zeros(K), torch.zeros(K), Wq, Kn, Vn, True, fam)
            mean = (Vc * vis[:, None, :, None]).sum(dim=2) / vis.sum(dim=1)[:, None, None].to(F64)             # [B, nkv, 64]
            ref = SM.round_engine(mean.repeat_interleave(n_rep, dim=1).reshape(B, K), bf16)
            assert torch.equal(got, ref), f"{tag} uniform: {int((got != ref).sum())} elements differ from the exact mean of the visible V rows"
            # -- one-hot: gamma = 0, integer beta and Wq -> exact integer q, the same for every utterance BEFORE the rotation. With RoPE the tables turn
            # q by (pos mod 4) quarter turns (exact), so utterance b looks with rot^(P + cur_len[b] - 1)(q): a kernel that rotates at another position,
            # or not at all, looks with another vector and loses the tiers. The two query heads of a K/V head look with q and -2 q: key t of
            # (utterance, K/V head) is a_t * sign(q'), and the positive head's hottest key is a = +6, the negative head's a = -6 - two different V rows,
            # so a head swap inside a group shows. Other visible keys: a in {-4, -2, 0, 2, 4}; hotter decoys a = +-8 sit on masked positions and just
            # past N; NaN on the rest of what no query may look at.
            for rope in (False, True):
                rig = XRig(H, bf16, K, B, gsz, N, n_rep, 1020 + B + N + int(rope), rope=False, out_fo=out_fo)
                if rope:
                    rig.cos, rig.sin = SC.quarter_turn_tables(rig.P + 20)
                g = rig.g
                beta = torch.zeros(K)
                beta[torch.randperm(K, generator=g)[:32]] = torch.where(torch.rand(32, generator=g) < 0.5, -1.0, 1.0)
                base = SC.ints((rig.nkv * 64, K), 1021)
                f = torch.tensor([1.0, -2.0], dtype=F64)[torch.arange(rig.nh) % n_rep]                         # query heads of a K/V head: q, -2 q
                Wq = (base.view(rig.nkv, 1, 64, K) * f.view(rig.nkv, n_rep, 1, 1)).reshape(K, K)
                q = (Wq @ beta.to(F64)).view(1, rig.nh, 64).expand(B, rig.nh, 64)
                pos = rig.P + rig.cur_len.long() - 1
                qr = SM.rope(q, rig.cos, rig.sin, pos[:, None].expand(B, rig.nh)) if rope else q.clone()      # [B, heads, 64], exact integers
                assert torch.equal(qr, qr.round())
                sgn = torch.where(qr.view(B, rig.nkv, n_rep, 64)[:, :, 0] >= 0, 1.0, -1.0).to(F64)             # [B, nkv, 64]: of the positive head
                l1 = qr.abs().sum(dim=2)
                assert float(l1.min()) * rig.scale * 2 * math.log2(math.e) >= 200, "score tiers at least 200 log2-units apart"
                assert float(l1.max()) * 8 < 2 ** 24
                vis = rig.visible()
                tier = torch.randint(-2, 3, (B, rig.nkv, rig.cap), generator=g) * 2                            # -4 .. 4
                hotp = torch.zeros(B, rig.nkv, dtype=torch.int64)
                hotn = torch.zeros(B, rig.nkv, dtype=torch.int64)
                for b in range(B):
                    cand = vis[b].nonzero().flatten()
                    for kh in range(rig.nkv):
                        pick = cand[torch.randperm(len(cand), generator=g)[:2]]
                        hotp[b, kh], hotn[b, kh] = pick[0], pick[-1]
                        if len(pick) == 2:
                            tier[b, kh, pick[1]] = -6
                        tier[b, kh, pick[0]] = 6
                decoy = torch.where(torch.arange(rig.cap) % 4 == 0, 8, -8)[None, None, :].expand_as(tier)
                tier = torch.where(vis[:, None, :].expand_as(tier), tier, decoy)                               # decoys where no query may look ...
                Kc = tier[..., None].to(F64) * sgn[:, :, None, :]
                Vc = torch.randint(-8, 9, (B, rig.nkv, rig.cap, 64), generator=g).to(F64)
                far = (torch.arange(rig.cap) > N)[None, None, :, None].expand_as(Kc) | ((~vis[:, None, :, None]) & (torch.arange(rig.cap) % 2 == 1)[None, None, :, None]).expand_as(Kc)
                Kc, Vc2 = torch.where(far, torch.full((), nan, dtype=F64), Kc), torch.where(far, torch.full((), nan, dtype=F64), Vc)  # ... and NaN on the rest
                x, _, _ = SC.ln_inputs(B, K, 1030 + B)
                got = rig.launch(x, torch.zeros(K), beta, Wq, Kc, Vc2, True, fam)
                kh = torch.arange(rig.nkv)
                vp = torch.stack([Vc[b, kh, hotp[b]] for b in range(B)])                                       # [B, nkv, 64]
                vn = torch.stack([Vc[b, kh, hotn[b]] for b in range(B)])
                ref = (torch.stack((vp, vn), dim=2) if n_rep == 2 else vp[:, :, None]).reshape(B, K)          # head order: (K/V head, head of the group)
                assert torch.equal(got, ref), f"{tag} rope={int(rope)} one-hot: {int((got != ref).sum())} elements differ from the hottest visible key's V row"
                # -- a row without a visible key yields 0
                if B >= 3 and not rope:
                    rig.mask[1] = 0
                    got = rig.launch(x, torch.zeros(K), beta, Wq, Kc, Vc2, True, fam)
                    ref[1] = 0
                    assert torch.equal(got, ref), f"{tag}: an utterance without a visible key must yield 0"


@pytest.mark.parametrize("bf16", SC.ENGINES, ids=_eng)
@pytest.mark.parametrize("K", (SC.WIDTH_GENERIC,) + SC.WIDTHS_FULL)
def test_xattn_fused_random(H, K, bf16):
    """Gaussian data, real RoPE tables, LN2 on rows that differ per utterance - against the float64 cross block evaluated on the rows the kernel's own
    LayerNorm stages (rows_prep_kernel<PRO_LN> on the same x: the same ln_row_sums / ln_mean_rstd / ln_norm), so no LayerNorm term widens the bound
    (step_model.xattn_tolerance; tests/test_step_model_cpu.py shows a wrong position, no rotation, a neighbour's x and a zero output all exceed it)."""
    fam = f"xattn_fused<{_eng(bf16)}> K={K}"
    for i, (gsz, B, N, out_fo) in enumerate(xattn_shapes(K)):
        n_rep = 1 + i % 2
        rig = XRig(H, bf16, K, B, gsz, N, n_rep, 1100 + B + N, rope=True, out_fo=out_fo)
        x, gamma, beta, Wq, Kc, Vc, rig.cur_len, rig.mask = SC.xattn_random_inputs(K, B, n_rep, bf16, 1110 + B)
        got = rig.launch(x, gamma, beta, Wq, Kc, Vc, False, fam)
        _, y, _ = prep_ln(H, bf16, B, K, x, gamma, beta, 0)
        m = SM.cross_block64(x, gamma, beta, Wq, Kc, Vc, n_rep=n_rep, N=N, P=rig.P, cur_len=rig.cur_len, mask=rig.mask, scale=rig.scale,
                             cos=rig.cos, sin=rig.sin, bf16=bf16, y=y.double().cpu())
        tol = SM.xattn_tolerance(m, Wq, Kc, N=N, n_rep=n_rep, scale=rig.scale, bf16=bf16)
        r = float(((got - m["out"]).abs() / tol).max())
        print(f"{fam} random g={gsz} B={B} N={N} n_rep={n_rep} out_fo={out_fo}: error / bound {r:.3e}, median bound {float(tol.median()):.2e}")
        _worst(fam, r)
        assert r <= 1.0
