"""The DAC codec's kernels called directly (tests/native/dac_harness.hip) against the float64 restatement tests/dac_kernel_model.py.

Data are dyadic: inputs are integers in [-2, 2] times 2^-2, weights integers in [-3, 3] times 2^-m with m chosen per layer so that the
pre-activations have a standard deviation near 1 (|v| <= 8, asserted) on a grid of 2^-(2 + m) >= 2^-8. Every product and partial sum is then exact
in fp32 in any order, integers are exact in bf16, and one data set serves both operand modes: every RAW output must equal the model bit for bit.
The Snake's alphas are random fp32 values in [0.2, 0.39], so |alpha v| <= pi (asserted) and the Snake sits in its curved range; they are NOT dyadic:
with a dyadic alpha the leading terms v + alpha v^2 of a small dyadic v land exactly on bf16 rounding ties, and several per cent of the activations
would be undecided below.

Every launch: outputs filled with NaN-payload sentinels with guard regions before and after, input rows beyond each utterance's valid length
poisoned with NaN bits, run twice with bitwise equal results, rows beyond a ragged length keep their sentinels. Batch 2; lengths equal and ragged,
0 and 1 included.

Bars (all derived; only the Snake probe's own accuracy is measured, helpers.DAC_SNAKE_S32_TOL):
  S32 = the dh_snake probe (snake_f<true>) on the model's exact pre-activations.
  bf16 activations: an element is DECIDED if bf16(S32 -/+ 4 fp32 ulps of max(|v|, |y|)) is one value (three roundings - the product inside sin, the
    square, the final multiply-add - may differ between inlinings through fma contraction); decided elements match bitwise, the others are one of
    the two neighbouring values; the undecided share is <= 1 % (expected ~2^-11), checked on the model before the launch.
  fp32 activations of the fast path: within those 4 fp32 ulps of S32. Exact-sinf mode (snake_f<false>): within 8 * 2^-24 * (|v| + (s^2 + 2|s|) / alpha)
    of float64, s = sin(alpha v): four roundings and a 2-ulp sinf, doubled.
  k1 on bf16 activations and the fused unit, per element: |out - model| <= C * 2^-24 * sum|W1||y| + sum over the frame's undecided y of
    ulp_bf16(y) |W1| + 2 fp32 ulps of the result.
  final convolution: the pre-tanh accumulator is exact; tanhf within 4 fp32 ulps of float64 tanh (a 2-ulp tanhf, doubled)."""
import math

import pytest
import torch

import dac_harness as DH
import dac_kernel_model as M
from helpers import DAC_SNAKE_S32_TOL, log_parity

pytestmark = pytest.mark.gpu

LOG = "dac_kernels_parity.txt"
DEV = "cuda"
SENT32, SENT16 = 0x7FBADBAD, 0x7FBB  # NaN payloads no kernel produces
NAN32, NAN16 = 0x7FC0DEAD, 0x7FC1    # the poison of input rows beyond an utterance
F64 = torch.float64
ALPHA_LO, ALPHA_HI = 0.2, 0.39
B = 2


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return DH.Harness(DH.build(str(tmp_path_factory.mktemp("dac_harness"))))


def _stream():
    return torch.cuda.current_stream().cuda_stream


class G:
    """An output tensor inside a flat buffer of sentinels: `guard` elements before and after it."""

    def __init__(self, shape, bf16=False, guard=2048):
        self.shape, self.bf16, self.guard = tuple(shape), bf16, guard
        self.n = math.prod(shape)
        self.sent = SENT16 if bf16 else SENT32
        self.buf = torch.full((2 * guard + self.n,), self.sent, dtype=torch.int16 if bf16 else torch.int32, device=DEV)
        self.t = self.buf[guard:guard + self.n].view(shape)

    def reset(self):
        self.buf.fill_(self.sent)

    def ptr(self):
        return self.t.data_ptr()

    def put(self, values, rows):
        """values [B][T][C] (cpu) into the rows of the boolean mask [B][T]; everything else stays sentinel."""
        v = values.to(torch.bfloat16 if self.bf16 else torch.float32).to(DEV).view(self.buf.dtype)
        m = rows.to(DEV)
        self.t[m] = v[m]

    def values(self):
        return self.t.view(torch.bfloat16 if self.bf16 else torch.float32).float().cpu()

    def check_untouched(self, written, what):
        """guards intact; rows outside the boolean mask `written` (leading dims of the shape) still sentinels."""
        g = self.guard
        assert bool((self.buf[:g] == self.sent).all()) and bool((self.buf[g + self.n:] == self.sent).all()), f"{what}: guard region overwritten"
        keep = ~written.to(DEV)
        assert bool((self.t[keep] == self.sent).all()), f"{what}: rows beyond the written range overwritten"
        assert not bool((self.t[written.to(DEV)] == self.sent).any()), f"{what}: rows inside the written range left unwritten"


def _twice(prep, launch, outs, H, what):
    snaps = []
    for _ in range(2):
        prep()
        rc = launch()
        assert rc == DH.PTTS_OK, (what, rc, H.error())
        torch.cuda.synchronize()
        snaps.append([o.buf.clone() for o in outs])
    for a, b in zip(*snaps):
        assert torch.equal(a, b), f"{what}: two runs differ"


def _ints(g, shape, lo, hi, scale):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64) * scale


def _wexp(K):
    """weights are integers in [-3, 3] (sigma 2) times 2^-m, inputs integers in [-2, 2] times 2^-2 (sigma 0.354): sigma of a K-term sum = sqrt(K) * 0.707 * 2^-m <= 1.01"""
    m = max(0, math.ceil(math.log2(math.sqrt(K) * 0.7)))
    assert 2 + m <= 8
    return m


def _alpha(g, Cn):
    return (ALPHA_LO + (ALPHA_HI - ALPHA_LO) * torch.rand(Cn, generator=g)).to(torch.float32)


def _dev_in(x, Tv, bf16):
    """x [B][T][C] (cpu float64, exactly representable) on the device, rows beyond Tv[b] poisoned with NaN bits."""
    t = x.to(torch.bfloat16 if bf16 else torch.float32).to(DEV).contiguous()
    bits = t.view(torch.int16 if bf16 else torch.int32)
    for b, n in enumerate(Tv):
        bits[b, n:] = NAN16 if bf16 else NAN32
    return t


def _f32(t):
    return t.to(torch.float32).to(DEV).contiguous()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _lens(i, T, mul):
    n = (T + mul - 1) // mul
    return [None, [n, n], [n, 1], [0, n], [max(n - 1, 0), n + 3], [1, n]][i % 6]


def _ulp32(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().to(F64).clamp(min=2.0 ** -126))) - 23)


def _ulp_bf16(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().to(F64).clamp(min=2.0 ** -126))) - 7)


def _exact32(v):
    assert torch.equal(v.to(torch.float32).to(F64), v), "the model's raw result is not exact in fp32: the data are not dyadic enough"
    return v.to(torch.float32)


class Snake:
    """S32: the dh_snake probe on given fp32 values, and the decided / undecided analysis built on it."""

    def __init__(self, H):
        self.H = H

    def s32(self, v32, alpha, fast=True):
        v = v32.to(torch.float32).to(DEV).contiguous()
        Cn = alpha.numel()
        al = torch.cat([alpha.to(torch.float32), torch.zeros(Cn)]).to(DEV)
        out = torch.empty_like(v)
        assert self.H.lib.dh_snake(int(fast), v.data_ptr(), al.data_ptr(), out.data_ptr(), v.numel(), Cn, _stream()) == DH.PTTS_OK, self.H.error()
        torch.cuda.synchronize()
        assert torch.equal(al[Cn:].cpu(), M.inv_alpha(alpha)), "inv_alpha_kernel is not the correctly rounded fp32 1 / (alpha + 1e-9)"
        return out.cpu()

    def __call__(self, v32, alpha):
        return self.s32(v32, alpha)

    def window(self, v32, alpha):
        """(S32, lo, hi, decided): bf16 of S32 -/+ 4 fp32 ulps of max(|v|, |y|)."""
        S = self.s32(v32, alpha)
        tol = 4 * _ulp32(torch.maximum(v32.abs(), S.abs()))
        lo, hi = M.rb((S.to(F64) - tol).to(torch.float32)), M.rb((S.to(F64) + tol).to(torch.float32))
        return S, tol, lo, hi, lo == hi

    def check_bf16(self, got, v32, alpha, rows, what, pre=None):
        S, tol, lo, hi, dec = pre if pre is not None else self.window(v32, alpha)
        g, l, h, d = got[rows], lo[rows], hi[rows], dec[rows]
        assert torch.equal(g[d], l[d]), f"{what}: {int((g[d] != l[d]).sum())} decided bf16 activations differ, max |d| {float((g[d] - l[d]).abs().max()):.3e}"
        assert bool(((g == l) | (g == h))[~d].all()), f"{what}: an undecided activation is neither neighbour"

    def check_f32_fast(self, got, v32, alpha, rows, what):
        S, tol, _, _, _ = self.window(v32, alpha)
        d = (got.to(F64) - S.to(F64)).abs()[rows]
        assert bool((d <= tol[rows]).all()), f"{what}: fp32 activation off S32 by {float((d / tol[rows]).max()) * 4:.2f} fp32 ulps (bar 4)"

    @staticmethod
    def check_f32_exact(got, v32, alpha, rows, what):
        a = alpha.to(F64)
        s = torch.sin(a * v32.to(F64))
        bar = 8 * 2.0 ** -24 * (v32.to(F64).abs() + (s * s + 2 * s.abs()) / a)
        d = (got.to(F64) - M.snake64(v32, alpha)).abs()
        assert bool((d <= bar)[rows].all()), f"{what}: exact-sinf activation off float64 by {float((d / bar.clamp(min=1e-300))[rows].max()):.2f} x its bar"


@pytest.fixture(scope="module")
def SN(H):
    return Snake(H)


def _precond(v, alpha, what):
    assert float(v.abs().max()) <= 8.0, (what, "|v| max", float(v.abs().max()))
    assert float((v.abs() * alpha.to(F64)).max()) <= math.pi, (what, "|alpha v| max")


# ---- the Snake probe's own accuracy: the one measured figure ---------------------------------------------------------------------------------
def test_snake_probe_accuracy_sets_the_bar(H, SN):
    """S32 (v_sin_f32 on alpha x / 2 pi) against the float64 Snake over every multiple of 2^-8 in [-8, 8] and alphas across the range the tests use, relative to
    |v| + 1 / alpha. The bar in helpers is 4 x the measured maximum and must itself stay below 2^-9: a formula error (a wrong inv, sin for sin^2, a
    dropped term) is orders of magnitude above it."""
    v = (torch.arange(-2048, 2049).to(F64) * 2.0 ** -8).to(torch.float32)
    worst = 0.0
    alphas = [float(a) for a in _alpha(torch.Generator().manual_seed(1), 13)] + [ALPHA_LO, 0.25, 0.3125, 0.375, ALPHA_HI]
    for a in alphas:
        alpha = torch.tensor([a], dtype=torch.float32)
        a = float(alpha[0])
        S = SN.s32(v, alpha)
        rel = ((S.to(F64) - M.snake64(v, alpha)).abs() / (v.to(F64).abs() + 1.0 / a))
        inr = (v.abs() * a) <= math.pi
        worst = max(worst, float(rel[inr].max()))
        ex = SN.s32(v, alpha, fast=False)
        Snake.check_f32_exact(ex, v, alpha, inr, f"probe alpha={a}")
    log_parity(f"[dac snake probe] max |S32 - float64 Snake| / (|v| + 1/alpha) over |alpha v| <= pi, {len(alphas)} alphas in [{ALPHA_LO}, {ALPHA_HI}]: {worst:.3e}; "
               f"bar DAC_SNAKE_S32_TOL = {DAC_SNAKE_S32_TOL:.3e}", LOG)
    assert DAC_SNAKE_S32_TOL < 2.0 ** -9
    assert worst <= DAC_SNAKE_S32_TOL, (worst, DAC_SNAKE_S32_TOL)


# ---- convolutions ----------------------------------------------------------------------------------------------------------------------------
EPIS = [dict(skip=0, raw=1, act=0), dict(skip=0, raw=0, act=1), dict(skip=0, raw=1, act=1), dict(skip=1, raw=1, act=1), dict(skip=1, raw=1, act=1, alias=1),
        dict(skip=1, raw=0, act=2), dict(skip=0, raw=1, act=2), dict(skip=1, raw=1, act=0), dict(skip=0, raw=0, act=2), dict(skip=1, raw=0, act=1),
        dict(skip=1, raw=1, act=2), dict(skip=1, raw=1, act=0, alias=1)]


def _share_ok(cases, what):
    """the undecided share of the bf16 activations of a test's launches, on the model, before any of them runs: <= 1 % (expected ~2^-11)"""
    n, und = sum(c["n"] for c in cases), sum(c["und"] for c in cases)
    assert n == 0 or und <= 1e-2 * n, (what, "undecided share before the launches", und, n)


def _conv_case(H, SN, shape, T, lens, mul, epi, forced=None, seed=0, what=""):
    c = _conv_prepare(H, SN, shape, T, lens, mul, epi, forced, seed, what)
    _share_ok([c], what)
    return c["run"]()


def _conv_prepare(H, SN, shape, T, lens, mul, epi, forced=None, seed=0, what=""):
    """One convolution launch checked against the model, in two steps: the model and the undecided count now, the launch in run(). act: 0 none, 1 the
    mode's own format (bf16 with bf16 operands, fp32 otherwise), 2 act_f32 (bf16 operands only; same as 1 otherwise).
    -> dict(n, und, run); run() -> dict(raw=G or None, act=G or None, plan)."""
    g = torch.Generator().manual_seed(seed)
    bf = bool(shape.bf16)
    Cin, Cout, k = shape.Cin, shape.Cout, shape.ksize
    ntaps = 2 if shape.transposed else k
    m = _wexp(ntaps * Cin)
    x = _ints(g, (B, T, Cin), -2, 2, 0.25)
    w = _ints(g, (Cin, Cout, k) if shape.transposed else (Cout, Cin, k), -3, 3, 2.0 ** -m)
    bias = _ints(g, (Cout,), -8, 8, 0.125)
    alpha = _alpha(g, Cout)
    raw64, written = M.conv(x, w, bias, k, dil=shape.dil, stride=shape.stride, transposed=bool(shape.transposed), pad=shape.pad, lens=lens, len_mul=mul)
    Tout = raw64.shape[1]
    skip = _ints(g, (B, Tout, Cout), -16, 16, 0.0625) if epi["skip"] else None
    if skip is not None:
        raw64 = raw64 + skip
    v32 = _exact32(raw64)
    _precond(raw64[written], alpha.expand(B, Tout, Cout)[written], what)
    act_bf16 = bf and epi["act"] == 1
    pre = SN.window(v32, alpha) if act_bf16 else None
    n_act, n_und = (int(written.sum()) * Cout, int((~pre[4][written]).sum())) if pre is not None else (0, 0)
    return dict(n=n_act, und=n_und, run=lambda: _conv_run(H, SN, shape, T, lens, mul, epi, forced, what, x, w, bias, alpha, skip, v32, written, pre))


def _conv_run(H, SN, shape, T, lens, mul, epi, forced, what, x, w, bias, alpha, skip, v32, written, pre):
    bf, Cout, act_bf16 = bool(shape.bf16), shape.Cout, pre is not None
    Bn, Tout = v32.shape[0], v32.shape[1]
    assert Bn == B
    Tv = M.valid_rows(T, lens, mul, B)
    xd, wd, bd = _dev_in(x, Tv, bf), _f32(w), _f32(bias)
    ald = torch.cat([alpha, torch.zeros(Cout)]).to(DEV)
    Wp = torch.zeros(w.numel() + 64, dtype=torch.float32, device=DEV)
    ktap = torch.zeros(64, dtype=torch.int32, device=DEV)
    lens_d = _i32(lens) if lens is not None else None
    alias = bool(epi.get("alias"))
    o_raw = G((B, Tout, Cout)) if epi["raw"] else None
    o_act = G((B, Tout, Cout), bf16=act_bf16) if epi["act"] else None
    skip_d = None if skip is None or alias else _f32(skip)
    a = DH.DhConv(x=xd.data_ptr(), w=wd.data_ptr(), bias=bd.data_ptr(), skip=(o_raw.ptr() if alias else skip_d.data_ptr()) if skip is not None else None,
                  out_raw=o_raw.ptr() if o_raw else None, out_act=o_act.ptr() if o_act else None, alpha=ald.data_ptr(), lens=lens_d.data_ptr() if lens is not None else None,
                  Wp=Wp.data_ptr(), ktap=ktap.data_ptr(), shape=shape, B=B, Tin=T, len_mul=mul, act_f32=int(epi["act"] == 2), forced=int(forced is not None))
    if forced is not None:
        a.plan.kernel = forced[0]
        a.plan.p[:] = (tuple(forced[1:]) + (0,) * 5)[:5]

    def prep():
        for o in (o_raw, o_act):
            if o:
                o.reset()
        if alias:
            o_raw.put(skip, written)  # the residual lives in the output buffer; rows beyond the utterance hold sentinels and are never read

    _twice(prep, lambda: H.conv(a, _stream()), [o for o in (o_raw, o_act) if o], H, what)
    if forced is not None:
        assert a.plan.instance()[:len(forced)] == tuple(forced), (what, a.plan.instance())
    for o, name in ((o_raw, "raw"), (o_act, "act")):
        if o:
            o.check_untouched(written, f"{what} {name}")
    if o_raw:
        got = o_raw.values()
        assert torch.equal(got[written], v32[written]), f"{what}: raw differs from the exact result in {int((got[written] != v32[written]).sum())} elements, " \
                                                       f"max |d| {float((got[written] - v32[written]).abs().max()):.3e}"
    if o_act:
        got = o_act.values()
        if act_bf16:
            SN.check_bf16(got, v32, alpha, written, what, pre)
        elif bf:
            SN.check_f32_fast(got, v32, alpha, written, what)
        else:
            Snake.check_f32_exact(got, v32, alpha, written, what)
    return dict(raw=o_raw, act=o_act, plan=a.plan)


MFMA_KINDS = [("k1", dict(k=1)), ("k7d1", dict(k=7)), ("k7d9", dict(k=7, dil=9)), ("up2", dict(k=4, stride=2, tr=1)), ("up4", dict(k=8, stride=4, tr=1)),
              ("up8", dict(k=16, stride=8, tr=1)), ("down2", dict(k=4, stride=2, pad=1)), ("down8", dict(k=16, stride=8, pad=4))]


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("bf", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cs", [1, 2, 4, 6, 8])
def test_conv_mfma_kernel(H, SN, cs, bf, waves):
    """conv_mfma_kernel<CS, BF> forced onto 1, 2 and 4 waves: k1, k7 (dil 1, 9), transposed (stride 2, 4, 8), strided fp32 ((2, 4) and the 16-tap (8, 16));
    Tn in {1, 31, 33, 129}; every epilogue combination in turn, skip aliasing out_raw included; ragged lengths in turn."""
    Cout, i, cases = 16 * cs, 0, []
    for name, kd in MFMA_KINDS:
        strided = "pad" in kd
        if strided and bf:
            continue  # the down-sampling convs belong to the encoder: fp32 only
        for Tn in (1, 31, 33, 129):
            shape = DH.ConvShape(32, Cout, kd["k"], kd.get("dil", 1), kd.get("stride", 1), kd.get("tr", 0), bf, kd.get("pad", -1))
            T = Tn * shape.stride if strided else Tn
            mul = 2 if i % 5 == 3 and not strided else 1
            lens = None if strided else _lens(i, T, mul)
            epi = EPIS[i % len(EPIS)]
            cases.append(_conv_prepare(H, SN, shape, T, lens, mul, epi, forced=(DH.CONV_MFMA, cs, bf, waves), seed=1000 * cs + 10 * i + bf,
                                       what=f"conv_mfma<{cs},{bf}> x{waves} {name} Tn={Tn} lens={lens} mul={mul} {epi}"))
            i += 1
    _share_ok(cases, f"conv_mfma<{cs},{bf}>")
    for c in cases:
        c["run"]()


LDS_T = (1, 40, 64, 65, 128, 129, 183)


@pytest.mark.parametrize("inst", [(3, 4, 1, 54, 4), (3, 4, 1, 54, 8), (3, 2, 1, 54, 8), (3, 4, 3, 2, 4), (3, 4, 3, 2, 8), (3, 2, 1, 2, 8)], ids=lambda t: "-".join(map(str, t)))
def test_conv_lds_kernel(H, SN, inst):
    """Every conv_lds_kernel instance, forced: the MAXHALO = 54 instances on k7 with dil 1, 3, 9; the MAXHALO = 2 ones on transposed stride 2 and 8 and
    on k1 (the 32 768-row rule's instance at 129 rows); Cin 96 and 192; T through the tile seams; every epilogue combination the kernel branches on."""
    _, nw, ks, maxhalo, ft = inst
    Cout = 48 * nw
    kinds = [dict(k=7, dil=1), dict(k=7, dil=3), dict(k=7, dil=9)] if maxhalo == 54 else [dict(k=4, stride=2, tr=1), dict(k=16, stride=8, tr=1), dict(k=1)]
    i, cases = 0, []
    for kd in kinds:
        for Cin in (96, 192):
            for T in LDS_T if kd["k"] != 1 else (129,):
                shape = DH.ConvShape(Cin, Cout, kd["k"], kd.get("dil", 1), kd.get("stride", 1), kd.get("tr", 0), 1, -1)
                mul = 2 if i % 5 == 3 else 1
                lens, epi = _lens(i, T, mul), EPIS[i % len(EPIS)]
                cases.append(_conv_prepare(H, SN, shape, T, lens, mul, epi, forced=(DH.CONV_LDS,) + inst, seed=7000 + 100 * sum(inst) + i,
                                           what=f"conv_lds<{inst}> {kd} Cin={Cin} T={T} lens={lens} mul={mul} {epi}"))
                i += 1
    _share_ok(cases, f"conv_lds<{inst}>")
    for c in cases:
        c["run"]()


@pytest.mark.parametrize("kd", [dict(k=7, dil=3), dict(k=16, stride=8, tr=1), dict(k=1)], ids=["k7", "up8", "k1"])
def test_conv_lds_ft4_and_ft8_agree_bitwise(H, SN, kd):
    ks, mh = (1, 54) if kd["k"] == 7 else (3, 2)
    for T, lens in ((65, None), (183, [183, 70]), (129, [1, 129])):
        shape = DH.ConvShape(192, 192, kd["k"], kd.get("dil", 1), kd.get("stride", 1), kd.get("tr", 0), 1, -1)
        epi = dict(skip=1, raw=1, act=1)
        r = [_conv_case(H, SN, shape, T, lens, 1, epi, forced=(DH.CONV_LDS, 3, 4, ks, mh, ft), seed=31, what=f"FT={ft} {kd} T={T}") for ft in (4, 8)]
        assert torch.equal(r[0]["raw"].buf, r[1]["raw"].buf) and torch.equal(r[0]["act"].buf, r[1]["act"].buf), (kd, T)


def test_planned_dispatch_runs_what_the_plan_says(H, SN):
    """dh_conv as planned: the instance run_conv would pick (small launches: the one-wave direct kernel, the FT = 4 tiles)."""
    r = _conv_case(H, SN, DH.ConvShape(96, 192, 7, 3, 1, 0, 1, -1), 65, [65, 9], 1, dict(skip=0, raw=1, act=1), seed=5, what="planned k7")
    assert r["plan"].instance() == (DH.CONV_LDS, 3, 4, 1, 54, 4)
    r = _conv_case(H, SN, DH.ConvShape(96, 96, 1, 1, 1, 0, 1, -1), 65, None, 1, dict(skip=1, raw=1, act=2), seed=6, what="planned k1")
    assert r["plan"].instance() == (DH.CONV_MFMA, 6, 1, 1, 0, 0)
    r = _conv_case(H, SN, DH.ConvShape(32, 64, 16, 1, 8, 0, 0, 4), 264, None, 1, dict(skip=0, raw=1, act=1), seed=7, what="planned down8")
    assert r["plan"].instance() == (DH.CONV_MFMA, 4, 0, 1, 0, 0)


# ---- the fused residual unit -----------------------------------------------------------------------------------------------------------------
def _k1_bound(y, und, w1, result):
    """per element: C * 2^-24 * sum|W1||y| + sum over undecided y of ulp_bf16(y) |W1| + 2 fp32 ulps of the result"""
    Cn = y.shape[-1]
    aw = w1.to(F64)[:, :, 0].abs()
    b = Cn * 2.0 ** -24 * torch.einsum("btc,oc->bto", y.to(F64).abs(), aw) + 2 * _ulp32(result)
    if und is not None:
        b = b + torch.einsum("btc,oc->bto", und.to(F64) * _ulp_bf16(y), aw)
    return b


def _res_launch(H, Cn, dil, T, lens, mul, x_d, xin, w, skip_d, raw, act, act_f32, written, what):
    """one dh_resunit launch, twice; x_d: the device input (bf16 activation, or the fp32 stream when xin) -> (raw G, act G, plan)"""
    o_raw = G((B, T, Cn)) if raw else None
    o_act = G((B, T, Cn), bf16=not act_f32) if act else None
    Wp7 = torch.zeros(7 * Cn * Cn + 64, dtype=torch.float32, device=DEV)
    Wp1 = torch.zeros(Cn * Cn + 64, dtype=torch.float32, device=DEV)
    ktap = torch.zeros(64, dtype=torch.int32, device=DEV)
    al = {k: torch.cat([w[k], torch.zeros(Cn)]).to(DEV) for k in ("alpha7", "alpha1", "alpha_in")}
    lens_d = _i32(lens) if lens is not None else None
    a = DH.DhRes(x=x_d.data_ptr(), w7=w["w7d"].data_ptr(), b7=w["b7d"].data_ptr(), alpha7=al["alpha7"].data_ptr(), w1=w["w1d"].data_ptr(), b1=w["b1d"].data_ptr(),
                 alpha1=al["alpha1"].data_ptr(), skip=skip_d.data_ptr(), out_raw=o_raw.ptr() if o_raw else None, out_act=o_act.ptr() if o_act else None,
                 alpha_in=al["alpha_in"].data_ptr() if xin else None, lens=lens_d.data_ptr() if lens is not None else None, Wp7=Wp7.data_ptr(), Wp1=Wp1.data_ptr(),
                 ktap=ktap.data_ptr(), C=Cn, dil=dil, B=B, T=T, len_mul=mul, act_f32=int(act_f32))
    outs = [o for o in (o_raw, o_act) if o]
    _twice(lambda: [o.reset() for o in outs], lambda: H.resunit(a, _stream()), outs, H, what)
    for o in outs:
        o.check_untouched(written, what)
    return o_raw, o_act, a.plan


RES_T = (1, 63, 64, 65, 128, 129, 183)


@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("Cn", [96, 192, 384])
def test_resunit_lds_kernel(H, SN, Cn, dil):
    """resunit_lds_kernel at every width: the plain unit on dyadic input against the model (inner activation rounded to bf16) and against the
    two-launch pair; the XIN unit (input = the fp32 stream a product conv wrote, Snake evaluated on the way into LDS) bitwise against the plain unit
    on the bf16 activation the same conv wrote, in all three output combinations; fp32 activations at C = 96."""
    cases = []
    for i, T in enumerate(RES_T):  # the model of every launch first: the undecided share of the inner activations, before any launch
        cases.append(_res_prepare(SN, Cn, dil, i, T))
    _share_ok(cases, f"resunit C={Cn} dil={dil}")
    worst = max(_res_run(H, SN, Cn, dil, c) for c in cases)
    log_parity(f"[dac resunit C={Cn} dil={dil}] T in {RES_T}: undecided inner activations {sum(c['und'] for c in cases)} of {sum(c['n'] for c in cases)}; "
               f"fused unit against the model: worst element at {worst:.3f} x its bound", LOG)


def _res_prepare(SN, Cn, dil, i, T):
    if True:
        g = torch.Generator().manual_seed(100 * Cn + 10 * dil + i)
        mul = 2 if i % 3 == 2 else 1
        lens = _lens(i + dil, T, mul)
        Tv = M.valid_rows(T, lens, mul, B)
        what = f"resunit C={Cn} dil={dil} T={T} lens={lens} mul={mul}"
        w = dict(w7=_ints(g, (Cn, Cn, 7), -3, 3, 2.0 ** -_wexp(7 * Cn)), b7=_ints(g, (Cn,), -8, 8, 0.125), w1=_ints(g, (Cn, Cn, 1), -3, 3, 2.0 ** -(_wexp(Cn) + 3)),
                 b1=_ints(g, (Cn,), -8, 8, 0.125), alpha7=_alpha(g, Cn), alpha1=_alpha(g, Cn), alpha_in=_alpha(g, Cn))
        w.update({k + "d": _f32(w[k]) for k in ("w7", "b7", "w1", "b1")})
        x, skip = _ints(g, (B, T, Cn), -2, 2, 0.25), _ints(g, (B, T, Cn), -16, 16, 0.0625)
        act_f32 = Cn == 96 and i % 2 == 1
        # ---- the model, with S32 for the inner Snake; undecided share checked before any launch
        y_pre, written = M.conv(x, w["w7"], w["b7"], 7, dil=dil, lens=lens, len_mul=mul)
        y32 = _exact32(y_pre)
        _precond(y_pre[written], w["alpha7"].expand(B, T, Cn)[written], what)
        S32, _, ylo, yhi, ydec = SN.window(y32, w["alpha7"])
        y_s = M.rb(S32)
        und = ~ydec
        model_raw = torch.einsum("btc,oc->bto", y_s.to(F64), w["w1"][:, :, 0]) + w["b1"] + skip
        return dict(n=int(written.sum()) * Cn, und=int(und[written].sum()), loc=dict(locals()))


def _res_run(H, SN, Cn, dil, c):
    S = DH.ConvShape
    L = c["loc"]
    i, T, g, mul, lens, Tv, what, w, x, skip, act_f32, written, y32, und, y_s, model_raw = (L[k] for k in (
        "i", "T", "g", "mul", "lens", "Tv", "what", "w", "x", "skip", "act_f32", "written", "y32", "und", "y_s", "model_raw"))
    if True:
        # ---- (a) the plain unit on dyadic input
        x_d, skip_d = _dev_in(x, Tv, True), _dev_in(skip, Tv, False)
        o_raw, o_act, plan = _res_launch(H, Cn, dil, T, lens, mul, x_d, False, w, skip_d, True, True, act_f32, written, what + " plain")
        assert plan.instance() == (Cn // 48, 3, 1, int(act_f32), 0, 1)
        got = o_raw.values()
        bound = _k1_bound(y_s, und, w["w1"], model_raw)
        d = (got.to(F64) - model_raw).abs()
        assert bool((d <= bound)[written].all()), f"{what}: fused unit off the model by {float((d / bound)[written].max()):.2f} x its per-element bound"
        worst = float((d / bound)[written].max())
        # its activation: the Snake of the stream it wrote itself
        _precond(got.to(F64)[written], w["alpha1"].expand(B, T, Cn)[written], what + " out")
        if act_f32:
            SN.check_f32_fast(o_act.values(), got, w["alpha1"], written, what + " act")
        else:
            SN.check_bf16(o_act.values(), got, w["alpha1"], written, what + " act")
        # without the stream output: the same activation bits
        _, o_act2, plan = _res_launch(H, Cn, dil, T, lens, mul, x_d, False, w, skip_d, False, True, act_f32, written, what + " plain, no raw")
        assert plan.instance() == (Cn // 48, 3, 0, int(act_f32), 0, 1) and torch.equal(o_act2.buf, o_act.buf), what
        # ---- (b) the two-launch pair: k7 with a bf16 activation output, then k1 + skip on it
        if i % 2 == 0 or T == 183:
            ald = torch.cat([w["alpha7"], torch.zeros(Cn)]).to(DEV)
            Wp = torch.zeros(7 * Cn * Cn + 64, dtype=torch.float32, device=DEV)
            ktap = torch.zeros(64, dtype=torch.int32, device=DEV)
            lens_d = _i32(lens) if lens is not None else None
            o_y = G((B, T, Cn), bf16=True)
            a7 = DH.DhConv(x=x_d.data_ptr(), w=w["w7d"].data_ptr(), bias=w["b7d"].data_ptr(), out_act=o_y.ptr(), alpha=ald.data_ptr(),
                           lens=lens_d.data_ptr() if lens is not None else None, Wp=Wp.data_ptr(), ktap=ktap.data_ptr(), shape=S(Cn, Cn, 7, dil, 1, 0, 1, -1), B=B, Tin=T,
                           len_mul=mul)
            _twice(o_y.reset, lambda: H.conv(a7, _stream()), [o_y], H, what + " pair k7")
            o_y.check_untouched(written, what + " pair y")
            y_pair = o_y.values()
            SN.check_bf16(y_pair, y32, w["alpha7"], written, what + " pair y")
            y_in = torch.where(written[:, :, None], y_pair, torch.zeros(()))
            al1 = torch.cat([w["alpha1"], torch.zeros(Cn)]).to(DEV)
            o_r2 = G((B, T, Cn))
            y_d = _dev_in(y_in.to(F64), Tv, True)
            a1 = DH.DhConv(x=y_d.data_ptr(), w=w["w1d"].data_ptr(), bias=w["b1d"].data_ptr(), skip=skip_d.data_ptr(), out_raw=o_r2.ptr(),
                           alpha=al1.data_ptr(), lens=lens_d.data_ptr() if lens is not None else None, Wp=Wp.data_ptr(), ktap=ktap.data_ptr(),
                           shape=S(Cn, Cn, 1, 1, 1, 0, 1, -1), B=B, Tin=T, len_mul=mul)
            _twice(o_r2.reset, lambda: H.conv(a1, _stream()), [o_r2], H, what + " pair k1")
            o_r2.check_untouched(written, what + " pair raw")
            pair64 = torch.einsum("btc,oc->bto", y_in.to(F64), w["w1"][:, :, 0]) + w["b1"] + skip
            d = (o_r2.values().to(F64) - pair64).abs()
            bk = _k1_bound(y_in, None, w["w1"], pair64)
            assert bool((d <= bk)[written].all()), f"{what}: k1 on bf16 activations off float64 by {float((d / bk)[written].max()):.2f} x its bound"
            d = (got.to(F64) - pair64).abs()
            bf_ = _k1_bound(y_in, und, w["w1"], pair64)
            assert bool((d <= bf_)[written].all()), f"{what}: fused unit off the two-launch pair by {float((d / bf_)[written].max()):.2f} x the bound"
        # ---- (c) XIN: a product conv writes the fp32 stream and its bf16 activation; the XIN unit reads the stream, the plain unit the activation
        m0 = _wexp(Cn)
        x0, w0, b0 = _ints(g, (B, T, Cn), -2, 2, 0.25), _ints(g, (Cn, Cn, 1), -3, 3, 2.0 ** -m0), _ints(g, (Cn,), -8, 8, 0.125)
        stream64, _ = M.conv(x0, w0, b0, 1, lens=lens, len_mul=mul)
        _precond(stream64[written], w["alpha_in"].expand(B, T, Cn)[written], what + " stream")
        al_in = torch.cat([w["alpha_in"], torch.zeros(Cn)]).to(DEV)
        Wp0 = torch.zeros(Cn * Cn + 64, dtype=torch.float32, device=DEV)
        ktap = torch.zeros(64, dtype=torch.int32, device=DEV)
        lens_d = _i32(lens) if lens is not None else None
        w0d, b0d, x0d = _f32(w0), _f32(b0), _dev_in(x0, Tv, True)
        o_s, o_a = G((B, T, Cn)), G((B, T, Cn), bf16=True)
        ap = DH.DhConv(x=x0d.data_ptr(), w=w0d.data_ptr(), bias=b0d.data_ptr(), out_raw=o_s.ptr(), out_act=o_a.ptr(), alpha=al_in.data_ptr(),
                       lens=lens_d.data_ptr() if lens is not None else None, Wp=Wp0.data_ptr(), ktap=ktap.data_ptr(), shape=S(Cn, Cn, 1, 1, 1, 0, 1, -1), B=B, Tin=T, len_mul=mul)
        assert H.conv(ap, _stream()) == DH.PTTS_OK, H.error()
        torch.cuda.synchronize()
        assert torch.equal(o_s.values()[written], _exact32(stream64)[written]), what + " stream"
        # rows beyond the utterance of both buffers hold sentinels (NaN payloads): the poison of the units' inputs
        stream_d, act_d = o_s.t.view(torch.float32), o_a.t.view(torch.bfloat16)
        pr, pa, _ = _res_launch(H, Cn, dil, T, lens, mul, act_d, False, w, stream_d, True, True, act_f32, written, what + " plain on the conv's activation")
        combos = [(True, True), (True, False), (False, True)]
        for raw, act in combos if i % 2 == 0 or T == 183 else [combos[i % 3]]:
            xr, xa, plan = _res_launch(H, Cn, dil, T, lens, mul, stream_d, True, w, stream_d, raw, act, act_f32 and act, written, what + f" XIN raw={raw} act={act}")
            assert plan.instance() == (Cn // 48, 1 if Cn == 96 else 3, int(raw), int(act_f32 and act), 1, int(act)), plan.instance()
            if raw:
                assert torch.equal(xr.buf, pr.buf), f"{what}: XIN unit (raw={raw}, act={act}) and plain unit differ in the stream"
            if act:
                assert torch.equal(xa.buf, pa.buf), f"{what}: XIN unit (raw={raw}, act={act}) and plain unit differ in the activation"
        return worst


# ---- the final convolution -------------------------------------------------------------------------------------------------------------------
def _out_launch(H, x_d, w_d, b_d, T, Cn, skip, tend, rows, lens, mul, direct, out_ld, what):
    o = G((B, out_ld))
    wt = torch.zeros(7 * Cn, dtype=torch.float32, device=DEV)
    sk_d, te_d = (_i32(skip), _i32(tend)) if rows else (None, None)
    lens_d = _i32(lens) if lens is not None else None
    a = DH.DhOut(x=x_d.data_ptr(), w=w_d.data_ptr(), bias=b_d.data_ptr(), wt=wt.data_ptr(), out=o.ptr(), skip_of=sk_d.data_ptr() if rows else None,
                 t_end_of=te_d.data_ptr() if rows else None, lens=lens_d.data_ptr() if lens is not None else None, out_ld=out_ld, B=B, T=T, C=Cn,
                 skip=0 if rows else skip, t_end=0 if rows else tend, len_mul=mul, rows=int(rows), force_direct=int(direct))
    _twice(o.reset, lambda: H.conv_out(a, _stream()), [o], H, what)
    return o


@pytest.mark.parametrize("rows", [0, 1], ids=["range", "ROWS"])
@pytest.mark.parametrize("kernel", ["lds96", "direct96", "direct32"])
def test_final_conv_tanh(H, kernel, rows):
    """conv_out_tanh_lds_kernel (C = 96) and conv_out_tanh_kernel (C = 96 forced, C = 32): emit ranges that start inside a tile and end before the ragged
    length, out_ld larger than what is emitted with sentinels between; the pre-tanh accumulator is exact, so the result is tanhf of a known fp32."""
    Cn, direct = (96, kernel != "lds96") if kernel != "direct32" else (32, False)
    assert H.conv_out_plan(Cn, B, 64, direct).lds_kernel == int(kernel == "lds96")
    for i, T in enumerate((1, 3, 63, 64, 65, 130)):
        g = torch.Generator().manual_seed(40 + i)
        x, w, b = _ints(g, (B, T, Cn), -2, 2, 0.25), _ints(g, (1, Cn, 7), -3, 3, 2.0 ** -_wexp(7 * Cn)), _ints(g, (1,), -8, 8, 0.125)
        mul = 2 if i % 2 else 1
        lens = _lens(i + 1, T, mul)
        Tv = M.valid_rows(T, lens, mul, B)
        if rows:
            skip, tend = [T // 3, 0], [max(T - 2, 0), T + 7]
        else:
            skip, tend = (T * 7) // 13, max(T - 1, 1)  # T = 130: the first 64-sample tile is skipped whole, the range starts inside the second
        acc, wav, emitted = M.conv_out(x, w, b, skip, tend, lens=lens, len_mul=mul)
        acc32 = _exact32(acc)
        sk = skip if rows else [skip] * B
        out_ld = T + 9
        what = f"conv_out {kernel} rows={rows} T={T} lens={lens} mul={mul} emit=[{skip}, {tend})"
        o = _out_launch(H, _dev_in(x, Tv, False), _f32(w), _f32(b), T, Cn, skip, tend, rows, lens, mul, direct, out_ld, what)
        wr = torch.zeros(B, out_ld, dtype=torch.bool)
        exp = torch.zeros(B, out_ld, dtype=F64)
        for bb in range(B):
            n = int(emitted[bb].sum())
            wr[bb, :n] = True
            exp[bb, :n] = torch.tanh(acc32[bb].to(F64))[emitted[bb]]
        o.check_untouched(wr, what)
        d = (o.values().to(F64) - exp).abs()
        assert bool((d <= 4 * 2.0 ** -24 * exp.abs())[wr].all()), f"{what}: tanh off by {float((d / (2.0 ** -24 * exp.abs()).clamp(min=1e-300))[wr].max()):.2f} x 2^-24 relative"


def test_final_conv_kernels_agree_bitwise_on_random_data(H):
    """the LDS-tiled and the direct kernel accumulate in the same order (bias, tap 0..6 x channel 0..95): bit-identical on any data"""
    g = torch.Generator().manual_seed(77)
    for T, lens, rows in ((130, None, 0), (197, [197, 60], 1), (65, [3, 65], 0)):
        x, w, b = torch.randn(B, T, 96, generator=g).to(F64), 0.05 * torch.randn(1, 96, 7, generator=g).to(F64), torch.randn(1, generator=g).to(F64)
        Tv = M.valid_rows(T, lens, 1, B)
        skip, tend = ([7, 0], [T - 3, T]) if rows else (5, T - 2)
        o = [_out_launch(H, _dev_in(x, Tv, False), _f32(w), _f32(b), T, 96, skip, tend, rows, lens, 1, direct, T + 4, f"random T={T} direct={direct}") for direct in (0, 1)]
        assert torch.equal(o[0].buf, o[1].buf), (T, lens, rows)
        x32, w32, b32 = x.to(torch.float32), w.to(torch.float32), b.to(torch.float32)
        acc, wav, emitted = M.conv_out(x32, w32, b32, skip, tend, lens=lens)
        mag = M.conv_out(x32.abs(), w32.abs(), b32.abs(), skip, tend, lens=lens)[0]  # sum |w||x|: a chain of 7 * 96 + 1 fmas, then tanh (slope <= 1)
        got = o[0].values()
        for bb in range(B):
            n, e = int(emitted[bb].sum()), emitted[bb]
            assert n == 0 or bool(((got[bb, :n].to(F64) - wav[bb][e]).abs() <= 673 * 2.0 ** -24 * mag[bb][e] + 4 * 2.0 ** -24).all())


# ---- the encoder's first convolution ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [16, 64])
def test_conv_in_kernel(H, Cn):
    for L in (1, 7, 33):
        g = torch.Generator().manual_seed(Cn + L)
        wave, w, b, alpha = _ints(g, (B, L), -8, 8, 0.125), _ints(g, (Cn, 1, 7), -3, 3, 0.25), _ints(g, (Cn,), -8, 8, 0.125), _alpha(g, Cn)
        raw64, act64 = M.conv_in(wave, w, b, alpha)
        _precond(raw64, alpha.expand(B, L, Cn), f"conv_in C={Cn} L={L}")
        o_raw, o_act = G((B, L, Cn)), G((B, L, Cn))
        wd, wwd, bd, ald = _f32(wave), _f32(w), _f32(b), torch.cat([alpha, torch.zeros(Cn)]).to(DEV)
        _twice(lambda: (o_raw.reset(), o_act.reset()),
               lambda: H.lib.dh_conv_in(wd.data_ptr(), wwd.data_ptr(), bd.data_ptr(), ald.data_ptr(), o_raw.ptr(), o_act.ptr(), B, L, Cn, _stream()), [o_raw, o_act], H, "conv_in")
        allrows = torch.ones(B, L, dtype=torch.bool)
        o_raw.check_untouched(allrows, "conv_in raw")
        o_act.check_untouched(allrows, "conv_in act")
        assert torch.equal(o_raw.values(), _exact32(raw64)), f"conv_in C={Cn} L={L}: raw differs"
        Snake.check_f32_exact(o_act.values(), _exact32(raw64), alpha, allrows, f"conv_in C={Cn} L={L}")


# ---- RVQ: table, gather, normalise, encode ---------------------------------------------------------------------------------------------------
def test_rvq_table_and_gather_are_exact(H):
    K, ncodes, cdim, latent, T = 9, 64, 8, 96, 11
    g = torch.Generator().manual_seed(3)
    cb, w, bias = _ints(g, (K, ncodes, cdim), -4, 4, 0.25), _ints(g, (K, latent, cdim), -3, 3, 0.125), _ints(g, (K, latent), -8, 8, 2.0 ** -9)
    table64 = torch.stack([M.rvq_table(cb[i], w[i], bias[i]) for i in range(K)])
    tab = G((K, ncodes, latent))
    cbd, wd, bd = _f32(cb), _f32(w), _f32(bias)

    def launch():
        for i in range(K):
            rc = H.lib.dh_rvq_table(cbd[i].data_ptr(), wd[i].data_ptr(), bd[i].data_ptr(), tab.ptr() + 4 * i * ncodes * latent, ncodes, cdim, latent, _stream())
            if rc:
                return rc
        return 0

    _twice(tab.reset, launch, [tab], H, "rvq_table")
    tab.check_untouched(torch.ones(K, ncodes, dtype=torch.bool), "rvq_table")
    assert torch.equal(tab.values(), _exact32(table64))
    table_d = tab.t.view(torch.float32)
    codes = torch.randint(0, ncodes, (B, K, T + 5), generator=g)
    codes[0, 0, 2], codes[1, 3, 4], codes[0, 8, 6], codes[1, 1, 9] = -1, ncodes, -2 ** 40, 2 ** 40  # clamp to 0 / ncodes - 1
    codes_d = codes.to(DEV)
    for bf16 in (0, 1):
        for lens in (None, [T, 4], [0, 1]):
            z64, written = M.rvq_gather(codes[:, :, 2:2 + T], table64, ncodes, lens, bool(bf16))
            if bf16:  # the bf16 value must be a genuine rounding somewhere, and a tie somewhere is welcome; RNE either way
                assert not torch.equal(z64, M.rvq_gather(codes[:, :, 2:2 + T], table64, ncodes, lens, False)[0])
            o = G((B, T, latent), bf16=bool(bf16))
            lens_d = _i32(lens) if lens is not None else None
            a = DH.DhGather(codes=codes_d.data_ptr(), table=table_d.data_ptr(), z=o.ptr(), lens=lens_d.data_ptr() if lens is not None else None, ld=T + 5, K=K, T=T, B=B,
                            ncodes=ncodes, latent=latent, z_bf16=bf16, t0=2, stream=0)
            _twice(o.reset, lambda: H.rvq_gather(a, _stream()), [o], H, f"rvq_gather bf16={bf16} lens={lens}")
            o.check_untouched(written, "rvq_gather")
            assert torch.equal(o.values().to(F64)[written], z64[written]), (bf16, lens)
    # STREAM: row b reads tab[slot[b]][k][start[b] + t], t < lens[b]
    slots, cap = 5, 23
    stab = torch.randint(0, ncodes, (slots, K, cap), generator=g)
    stab[3, 2, 9], stab[1, 0, 4] = -7, ncodes + 3
    slot, start, lens = [3, 1], [6, 2], [T, 5]
    z64, written = M.rvq_gather_stream(stab, slot, start, lens, cap, table64, ncodes, T, True)
    o = G((B, T, latent), bf16=True)
    stab_d, slot_d, start_d, lens_d = stab.to(torch.int32).to(DEV), _i32(slot), _i32(start), _i32(lens)
    a = DH.DhGather(tab=stab_d.data_ptr(), p_lens=lens_d.data_ptr(), start=start_d.data_ptr(), slot=slot_d.data_ptr(), table=table_d.data_ptr(), z=o.ptr(),
                    lens=lens_d.data_ptr(), ld=0, cap=cap, K=K, T=T, B=B, ncodes=ncodes, latent=latent, z_bf16=1, t0=0, stream=1)
    _twice(o.reset, lambda: H.rvq_gather(a, _stream()), [o], H, "rvq_gather STREAM")
    o.check_untouched(written, "rvq_gather STREAM")
    assert torch.equal(o.values().to(F64)[written], z64[written])


DUPS = ((10, 1), (70, 64), (200, 256), (500, 300))  # (c, c + 1) two lanes of a wave, (c, c + 64) two waves, (c, c + 256) one lane's next iteration, (c, c + 300) another wave's


def _encode_case(latent, T, seed):
    """Weights, duplicate codebook rows in stage 0 and stage 4, and B x T latent frames whose every stage has a top-2 gap >= 1e-2 in the float64 model
    (an exact tie between duplicate rows counts as one code: the gap to the third then). The first frames project onto the duplicated codes."""
    K, cdim, ncodes = 9, 8, 1024
    g = torch.Generator().manual_seed(seed)
    in_w = torch.randn(K, cdim, latent, generator=g) / math.sqrt(latent)
    in_b = 0.01 * torch.randn(K, cdim, generator=g)
    cb = torch.randn(K, ncodes, cdim, generator=g)
    out_w = torch.randn(K, latent, cdim, generator=g) / math.sqrt(cdim)
    out_b = 0.01 * torch.randn(K, latent, generator=g)
    for st in (0, 4):
        for c, off in DUPS:
            cb[st, c + off] = cb[st, c]
    in_w, in_b, cb, out_w, out_b = (t.to(torch.float32) for t in (in_w, in_b, cb, out_w, out_b))

    def gaps_ok(z):
        """per frame: every stage's gap >= 1e-2, ties between identical rows skipped"""
        res = z.to(F64).clone()
        ok = torch.ones(z.shape[0], dtype=torch.bool)
        for i in range(K):
            p = res @ in_w[i].to(F64).t() + in_b[i].to(F64)
            e = p / p.norm(dim=1, keepdim=True)
            cbn, sq = M.cb_normalize(cb[i])
            score = -(((e * e).sum(1, keepdim=True) - 2.0 * (e @ cbn.t())) + sq)
            top = score.topk(3, dim=1)
            same = (cb[i][top.indices[:, 0]] == cb[i][top.indices[:, 1]]).all(1)
            gap = torch.where(same, top.values[:, 0] - top.values[:, 2], top.values[:, 0] - top.values[:, 1])
            ok &= gap >= 1e-2
            idx = torch.minimum(top.indices[:, 0], torch.where(same, top.indices[:, 1], top.indices[:, 0]))
            q = p + (cb[i].to(F64)[idx] - p)
            res = res - (q @ out_w[i].to(F64).t() + out_b[i].to(F64))
        return ok

    frames = []
    pinv = torch.linalg.pinv(in_w[0].to(F64))
    for c, _ in DUPS[:min(len(DUPS), B * T)]:  # frames whose stage-0 projection is the duplicated code (plus noise), later stages by rejection
        cand = ((cb[0, c].to(F64) - in_b[0].to(F64)) @ pinv.t())[None] + 0.02 * torch.randn(400, latent, generator=g).to(F64)
        cand = cand.to(torch.float32)
        good = cand[gaps_ok(cand)]
        assert len(good), "no candidate frame with clear gaps"
        frames.append(good[0])
    while len(frames) < B * T:
        cand = torch.randn(64, latent, generator=g)
        good = cand[gaps_ok(cand)]
        frames.extend(good[:B * T - len(frames)])
    z = torch.stack(frames[:B * T]).reshape(B, T, latent)
    return z, in_w, in_b, cb, out_w, out_b


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("latent", [64, 1024])
def test_rvq_encode_kernel(H, latent, T):
    """(latent, cdim, codes, stages) = (latent, 8, 1024, 9): every code equals the float64 model's, no exemptions (top-2 gaps >= 1e-2 by construction);
    duplicate codebook rows at (c, c + 1), (c, c + 64), (c, c + 256), (c, c + 300): the lowest index wins; nq = 4 is a prefix of nq = 9."""
    K, cdim, ncodes = 9, 8, 1024
    z, in_w, in_b, cb, out_w, out_b = _encode_case(latent, T, 900 + latent + T)
    ref, _ = M.rvq_encode(z, in_w, in_b, cb, out_w, out_b, K)
    won = {int(v) for v in ref[:, 0].flatten()}
    assert {c for c, _ in DUPS[:B * T]} <= won, "the duplicated codes do not win their frames in the model"
    zd, iwd, ibd, cbd, owd, obd = (_f32(t) for t in (z, in_w, in_b, cb, out_w, out_b))
    cbn, sq = G((K, ncodes, cdim)), G((K, ncodes))

    def norm():
        for i in range(K):
            rc = H.lib.dh_cb_normalize(cbd[i].data_ptr(), cbn.ptr() + 4 * i * ncodes * cdim, sq.ptr() + 4 * i * ncodes, ncodes, cdim, _stream())
            if rc:
                return rc
        return 0

    _twice(lambda: (cbn.reset(), sq.reset()), norm, [cbn, sq], H, "cb_normalize")
    cbn.check_untouched(torch.ones(K, ncodes, dtype=torch.bool), "cbn")
    sq.check_untouched(torch.ones(K, dtype=torch.bool), "cbn_sq")
    n64 = torch.stack([M.cb_normalize(cb[i])[0] for i in range(K)])
    # fp32: the squared norm is 8 products + 8 sequential adds (<= 9 roundings), halved by the square root, + sqrt, division and product: <= 6 * 2^-24
    # relative per element; the squared norm of the result twice that + 9 more: <= 21 * 2^-24. Bars: the next powers of two.
    assert bool(((cbn.values().to(F64) - n64).abs() <= 8 * 2.0 ** -24 * n64.abs()).all()) and float((sq.values().to(F64) - 1.0).abs().max()) <= 32 * 2.0 ** -24
    outs = {}
    for nq in (9, 4):
        o = torch.full((2 * 64 + B * nq * T,), -77, dtype=torch.int64, device=DEV)
        a = DH.DhEncode(z=zd.data_ptr(), in_w=iwd.data_ptr(), in_b=ibd.data_ptr(), cb=cbd.data_ptr(), cbn=cbn.ptr(), cbn_sq=sq.ptr(), out_w=owd.data_ptr(), out_b=obd.data_ptr(),
                        codes=o.data_ptr() + 8 * 64, B=B, T=T, latent=latent, cdim=cdim, ncodes=ncodes, nq=nq)
        snaps = []
        for _ in range(2):
            o.fill_(-77)
            assert H.rvq_encode(a, _stream()) == DH.PTTS_OK, H.error()
            torch.cuda.synchronize()
            snaps.append(o.clone())
        assert torch.equal(snaps[0], snaps[1])
        assert bool((o[:64] == -77).all()) and bool((o[64 + B * nq * T:] == -77).all())
        outs[nq] = o[64:64 + B * nq * T].view(B, nq, T).cpu()
    assert torch.equal(outs[9], ref), f"codes differ from the model at {(outs[9] != ref).nonzero().tolist()}"
    assert torch.equal(outs[4], outs[9][:, :4])
