"""The prefill-sized GEMM kernels called directly (tests/native/gemm_harness.hip) against exact results.

Exact mode: W and x hold small integers (|v| <= 8), so every product and partial sum of K <= 4096 terms is an integer below 2^24 and fp32
accumulation is exact in any order - the kernel must equal the float64 product bit for bit (fp32 outputs, integer residuals), or its
round-to-nearest-even bf16 value (KV caches). The GELU epilogues get weight rows scaled by powers of two (still exact) so that their
accumulators sit in the curved range of the nonlinearity, where the result must be within one bf16 ulp of the float64 function.
Every output is surrounded by sentinels (guard rows before and after, the columns between the row width and out_ld, cache positions past
the utterance) that must survive, and every launch runs twice with bitwise equal results.
Random data: gemm_glds_kernel, gemm_tile_kernel and gemm_block_kernel accumulate in the same order and must agree bitwise (ptts_gemm_glds.h),
within K 2^-24 (|W| |x|) of float64; the two entry points of each 128-row strip instance agree bitwise."""
import math

import pytest
import torch

import gemm_harness as GH
from gemm_harness import EPI_GATE_WT, EPI_GELU_WT, EPI_KV, EPI_RESID, EPI_STORE, PTTS_E_UNSUPPORTED, PTTS_OK
from helpers import log_parity

pytestmark = pytest.mark.gpu

LOG = "gemm_kernels.txt"
DEV = "cuda"
SENT32, SENT16 = 0x7FBADBAD, 0x7FBB  # NaN payloads no kernel produces
GLDS = {}  # (EPI, BNS, BMT, WN, WM, NST, RP) -> instance, filled from the harness


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    h = GH.Harness(GH.build(str(tmp_path_factory.mktemp("gemm_harness"))))
    for t in h.glds_instances():
        GLDS[t] = t
    return h


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inst(epi, bns, bmt):
    (t,) = [t for t in GLDS if t[0] == epi and t[1] == bns and t[2] == bmt]
    return t


def _name(t):
    return f"glds<{GH.EPI_NAMES[t[0]]},{','.join(str(v) for v in t[1:])}>"


class Guarded:
    """A [rows][cols] tensor inside a flat buffer of sentinels: `pre` elements before it, `post` after it."""

    def __init__(self, rows, cols, dtype, pre=4096, post=4096):
        self.rows, self.cols, self.dtype, self.pre = rows, cols, dtype, pre
        self.sent = SENT16 if dtype == torch.bfloat16 else SENT32
        self.buf = torch.full((pre + rows * cols + post,), self.sent, dtype=torch.int16 if dtype == torch.bfloat16 else torch.int32, device=DEV).view(dtype)
        self.t = self.buf[pre:pre + rows * cols].view(rows, cols)

    def reset(self):
        self.bits().fill_(self.sent)

    def ptr(self):
        return self.t.data_ptr()

    def bits(self):
        return self.buf.view(torch.int16 if self.dtype == torch.bfloat16 else torch.int32)

    def expected_bits(self, fill):
        """The whole buffer as it must be: sentinels everywhere except where `fill(view)` writes."""
        e = torch.full_like(self.bits(), self.sent).view(self.dtype)
        fill(e[self.pre:self.pre + self.rows * self.cols].view(self.rows, self.cols))
        return e.view(self.bits().dtype)


def _ints(shape, gen, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=DEV, dtype=torch.int32).double()


def _ulp_bf16(v):
    a = v.abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def _gelu_erf(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def _gelu_new(u):
    return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))


class Problem:
    """One GEMM out[m][n] = sum_k W[n][k] x[m][k] with its operands on the device, packed weights and the float64 reference."""

    def __init__(self, H, bf16, epi, M, N, K, x_ld=None, seed=0, layers=0, kv=None, kv_col0=0, gaussian=False):
        self.H, self.bf16, self.epi, self.M, self.N, self.K = H, bf16, epi, M, N, K
        self.x_ld = x_ld or K
        self.dt = torch.bfloat16 if bf16 else torch.float32
        self.layers, self.kv, self.kv_col0 = layers, kv, kv_col0
        if kv is not None:  # the cache extents the kernels address: heads x 64 columns per K / V half, positions < kv_cap
            assert (N == 2 * kv[0] * 64) if epi == EPI_KV else (kv_col0 > 0 and kv_col0 + 2 * kv[0] * 64 == N), (N, kv, kv_col0)
            assert kv[1] <= kv[2]
        g = torch.Generator(device=DEV).manual_seed(seed)
        nW = max(layers, 1)
        if gaussian:
            self.Ws = [torch.randn(N, K, generator=g, device=DEV).to(self.dt).double() for _ in range(nW)]
            x = torch.randn(M, K, generator=g, device=DEV).to(self.dt).double()
        else:
            self.Ws = [_ints((N, K), g) for _ in range(nW)]
            x = _ints((M, K), g)
        self.x = x
        self.acc = [x @ W.t() for W in self.Ws]  # exact for integer data (float64)
        if not gaussian and epi in (EPI_GELU_WT, EPI_GATE_WT):  # scale rows by powers of two: accumulators into (-3, 3], still exact
            for W, acc in zip(self.Ws, self.acc):
                rows = torch.arange(N, device=DEV)
                sel = rows % 2 == 0 if epi == EPI_GATE_WT else torch.ones(N, dtype=torch.bool, device=DEV)
                mx = acc.abs().amax(0).clamp(min=1.0)
                e = torch.clamp(torch.ceil(torch.log2(mx / 3.0)), min=0.0)
                s = torch.where(sel, torch.exp2(-e), torch.ones_like(e))
                W.mul_(s[:, None])
                acc.mul_(s[None, :])
        # activations with row stride x_ld: the columns past K hold NaN, which any read of them would spread into the results
        self.xbuf = torch.full((M, self.x_ld), float("nan"), device=DEV, dtype=self.dt)
        self.xbuf[:, :K] = x.to(self.dt)
        KT = 32 if bf16 else 16
        self.packed = []
        for W in self.Ws:
            p = torch.empty(N * K, device=DEV, dtype=self.dt)
            Wf = W.float().contiguous()
            assert H.pack(bf16, Wf.data_ptr(), p.data_ptr(), N, K, _stream()) == PTTS_OK, H.error()
            self.packed.append(p)
        torch.cuda.synchronize()
        self.KT = KT
        self.resid = None
        self.kv_table = None
        if layers:
            self.caches = [self._caches() for _ in range(layers)]
            self.kv_table = torch.tensor([[p.data_ptr(), kc.ptr(), vc.ptr()] for p, (kc, vc) in zip(self.packed, self.caches)],
                                         dtype=torch.int64, device=DEV)
        elif kv is not None:
            self.caches = [self._caches()]

    def _caches(self):
        nh, rpb, cap = self.kv
        nb = (self.M + rpb - 1) // rpb
        return Guarded(nb * nh * cap, 64, self.dt), Guarded(nb * nh * cap, 64, self.dt)

    def out_cols(self):
        return self.N // 2 if self.epi == EPI_GATE_WT else self.N

    def fresh(self, out_ld):
        """Output buffers for one launch (sentinels; EPI_RESID: an integer residual in the output rows) and the argument struct."""
        od = self.dt if self.epi in (EPI_GELU_WT, EPI_GATE_WT) else torch.float32
        self.out_ld = out_ld
        self.out = Guarded(self.M, out_ld, od, pre=2 * out_ld + 64, post=3 * out_ld + 64)
        if self.epi == EPI_RESID:
            if self.resid is None:
                self.resid = _ints((self.M, self.N), torch.Generator(device=DEV).manual_seed(99), -1000, 1000)
            self.out.t[:, :self.N] = self.resid.float()
        if self.kv is not None:
            for kc, vc in self.caches:
                kc.reset()
                vc.reset()
        a = GH.GhArgs()
        a.W, a.x, a.out = self.packed[0].data_ptr(), self.xbuf.data_ptr(), self.out.ptr()
        a.M, a.N, a.K, a.x_ld, a.out_ld, a.xcd_swz = self.M, self.N, self.K, self.x_ld, out_ld, 1
        if self.kv is not None:
            a.nheads, a.kv_rows_per_b, a.kv_cap = self.kv
            a.kcache, a.vcache = self.caches[0][0].ptr(), self.caches[0][1].ptr()
            a.kv_col0 = self.kv_col0
        if self.layers:
            a.kv_layers, a.kv_nlayers = self.kv_table.data_ptr(), self.layers
        return a

    def run(self, launch, out_ld=None):
        """launch(args) twice on fresh buffers; returns the status and the buffers' bits of both runs (bitwise equal is asserted)."""
        res = []
        for _ in range(2):
            a = self.fresh(out_ld or self.out_cols() + 8)
            rc = launch(a)
            torch.cuda.synchronize()
            if rc != PTTS_OK:
                return rc, None
            snap = [self.out.bits().clone()] + [c.bits().clone() for kv in (self.caches if self.kv is not None else []) for c in kv]
            res.append(snap)
        for s0, s1 in zip(*res):
            assert torch.equal(s0, s1), "two launches of the same GEMM differ"
        return PTTS_OK, res[0]

    def check_exact(self, tag):
        """Compare the last launch's buffers with the exact result; returns a log string. Nonlinear epilogues: one bf16 ulp."""
        acc = self.acc[0]
        N, M = self.N, self.M
        od = self.out.dtype
        msg = "exact"
        if self.epi == EPI_KV:
            assert_bits(self.out.bits(), self.out.expected_bits(lambda v: None), self.out_ld, f"{tag}: output (unused by EPI_KV)")
        elif self.epi in (EPI_STORE, EPI_RESID):
            ref = acc + (self.resid if self.epi == EPI_RESID else 0)
            exp = self.out.expected_bits(lambda v: v[:, :N].copy_(ref.float()))
            assert_bits(self.out.bits(), exp, self.out_ld, f"{tag}: output")
        elif self.epi in (EPI_GELU_WT, EPI_GATE_WT):
            ref = _gelu_erf(acc) if self.epi == EPI_GELU_WT else _gelu_new(acc[:, 0::2]) * acc[:, 1::2]
            nc = ref.shape[1]
            got = self.out.t[:, :nc].double()
            # outside the written columns: sentinels only
            exp = self.out.expected_bits(lambda v: v[:, :nc].copy_(self.out.t[:, :nc]))
            assert torch.equal(self.out.bits(), exp), f"{tag}: writes outside the output"
            err = (got - ref).abs()
            # fp32 outputs: the fp32 nonlinearity's own error, a few ulp of its tanh / erf scaled by |u| (|v|)
            mag = acc.abs() if self.epi == EPI_GELU_WT else acc[:, 0::2].abs() * acc[:, 1::2].abs()
            tol = _ulp_bf16(ref) if od == torch.bfloat16 else 2.0 ** -18 * (ref.abs() + mag)
            bound = "1 bf16 ulp" if od == torch.bfloat16 else "2^-18 (|ref| + |u| |v|)"
            worst = float(torch.where(tol > 0, err / tol, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))).max())
            assert worst <= 1.0, f"{tag}: {int((err > tol).sum())} outputs beyond {bound}, worst {worst:.2f} x"
            same = float((got == ref.to(od).double()).double().mean())
            msg = f"within {bound} (worst {worst:.2f} x), {same * 100:.2f} % equal to the rounded float64 value"
        if self.kv is not None:
            self._check_caches(tag)
        return msg

    def _check_caches(self, tag):
        nh, rpb, cap = self.kv
        m = torch.arange(self.M, device=DEV)
        b, t = m // rpb, m % rpb
        for li, (kc, vc) in enumerate(self.caches):
            acc = self.acc[li]
            if self.epi == EPI_KV:
                Hc, c0 = self.N // 2, 0
            else:
                Hc, c0 = nh * 64, self.kv_col0
            for which, cache in ((0, kc), (1, vc)):
                vals = acc[:, c0 + which * Hc:c0 + (which + 1) * Hc].to(self.dt)  # float64 -> engine dtype, round to nearest even

                def fill(v, vals=vals):
                    v4 = v.view(-1, nh, cap, 64)
                    v4[b, :, t, :] = vals.view(self.M, nh, 64)
                assert_bits(cache.bits(), cache.expected_bits(fill), 64, f"{tag}: layer {li} {'V' if which else 'K'} cache")


def assert_bits(got, exp, ld, what):
    if torch.equal(got, exp):
        return
    d = (got != exp).nonzero().flatten()
    first = int(d[0])
    raise AssertionError(f"{what}: {d.numel()} elements differ, first at flat {first} (row/col {first // ld}/{first % ld} from the buffer start)")


def _exact(H, bf16, epi, M, N, K, launch, tag, **kw):
    p = Problem(H, bf16, epi, M, N, K, **kw)
    rc, _ = p.run(launch)
    assert rc == PTTS_OK, f"{tag}: status {rc} {H.error()}"
    msg = p.check_exact(tag)
    log_parity(f"[gemm exact] {tag} M={M} N={N} K={K} x_ld={p.x_ld}: {msg}", LOG)
    return p


# ---- gemm_glds_kernel, every instance, directly ----------------------------------------------------------------------------------------
# (EPI, BNS, BMT) -> shapes (M, N, K, x_ld extra) - the product's own shapes first, then ragged last row tiles of the 64- / 128- / 256-row
# tiles, short K (the ring's prologue and vmcnt drain: nstage < NST), N % 128 != 0 above 1024 columns, x_ld > K
GLDS_CASES = {
    (EPI_STORE, 12, 8): [(2048, 3072, 1024, 0), (2049, 3072, 1024, 8), (300, 3072, 64, 0), (1600, 1536, 192, 64)],
    (EPI_STORE, 4, 4): [(1056, 1024, 1024, 0), (257, 1088, 64, 0), (4097, 1024, 128, 8), (300, 1088, 4096, 0)],
    (EPI_STORE, 8, 8): [(2048, 5632, 1024, 0), (1920, 2048, 128, 0), (2049, 1024, 1536, 64)],
    (EPI_STORE, 8, 4): [(1056, 3072, 1024, 0), (1056, 4096, 1024, 0), (300, 2048, 192, 8), (1600, 1024, 64, 0)],
    (EPI_RESID, 4, 4): [(2048, 1024, 2816, 0), (1056, 1024, 4096, 0), (257, 1088, 64, 8)],
    (EPI_RESID, 8, 8): [(2049, 1536, 1024, 0), (1600, 1024, 128, 64)],
    (EPI_RESID, 8, 4): [(300, 2048, 1024, 0), (1056, 1024, 192, 8)],
    (EPI_GELU_WT, 4, 4): [(1056, 1088, 1024, 0), (300, 1024, 64, 8)],
    (EPI_GELU_WT, 8, 8): [(1056, 6144, 1536, 0), (2049, 1024, 128, 0)],
    (EPI_GELU_WT, 8, 4): [(1056, 4096, 1024, 0), (257, 2048, 192, 64)],
    (EPI_GATE_WT, 11, 16): [(2048, 5632, 1024, 0), (1920, 5632, 1024, 0), (300, 5632, 64, 8), (4097, 1408, 128, 0), (1600, 2816, 192, 0)],
    (EPI_GATE_WT, 4, 4): [(1056, 1024, 1024, 0), (257, 1088, 128, 8)],
    (EPI_GATE_WT, 8, 8): [(2048, 2048, 1024, 0), (2049, 1024, 64, 0)],
    (EPI_GATE_WT, 8, 4): [(300, 2048, 1024, 64), (1600, 1024, 192, 0)],
}


@pytest.mark.parametrize("key", list(GLDS_CASES), ids=lambda k: f"{GH.EPI_NAMES[k[0]]}-{k[1]}x{k[2]}")
def test_glds_instance_exact(H, key):
    inst = _inst(*key)
    for i, (M, N, K, pad) in enumerate(GLDS_CASES[key]):
        _exact(H, True, key[0], M, N, K, lambda a: H.glds(inst, a, _stream()), _name(inst), x_ld=K + pad, seed=i)


def test_every_glds_instance_has_exact_cases(H):
    """Together with test_gemm_harness_cpu.py (harness instances == the product's): no instance without an exact case."""
    covered = {_inst(*k) for k in GLDS_CASES} | {_inst(EPI_KV, b, m) for b, m in ((4, 4), (8, 8), (8, 4))}
    assert covered == set(GLDS), set(GLDS) ^ covered


# cross K/V (EPI_KV): N = 2 x 64 heads; kv_rows_per_b = 37 or 33 does not divide any tile; with the layer table (blockIdx.z) and without
@pytest.mark.parametrize("bns,bmt,M,rpb,layers", [(4, 4, 333, 37, 0), (4, 4, 2049, 33, 3), (8, 8, 1665, 37, 3), (8, 8, 300, 100, 0),
                                                  (8, 4, 2048, 64, 0), (8, 4, 1056, 33, 2)])
def test_glds_kv_exact(H, bns, bmt, M, rpb, layers):
    inst = _inst(EPI_KV, bns, bmt)
    nh = 16
    kv = (nh, rpb, rpb + 3)
    _exact(H, True, EPI_KV, M, 2 * nh * 64, 1024, lambda a: H.glds(inst, a, _stream()), f"{_name(inst)} rows/b {rpb} layers {layers}",
           kv=kv, layers=layers, seed=M)


# QKV with the K / V columns into the self-attention cache (EPI_STORE + kv_col0), every EPI_STORE policy
@pytest.mark.parametrize("bns,bmt", [(12, 8), (4, 4), (8, 8), (8, 4)])
def test_glds_qkv_cache_columns_exact(H, bns, bmt):
    inst = _inst(EPI_STORE, bns, bmt)
    nkv = 16
    _exact(H, True, EPI_STORE, 1056, 1024 + 2 * nkv * 64, 1024, lambda a: H.glds(inst, a, _stream()), f"{_name(inst)} kv_col0 1024",
           kv=(nkv, 33, 40), kv_col0=1024, seed=bns)


# ---- the fallbacks and the dispatcher, bf16 and fp32 ----------------------------------------------------------------------------------
FALLBACK_CASES = [(EPI_STORE, 300, 1024, 1024), (EPI_RESID, 1056, 1088, 192), (EPI_GELU_WT, 257, 2048, 128), (EPI_GATE_WT, 2049, 1024, 64)]


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_tile_and_block_exact(H, bf16):
    for epi, M, N, K in FALLBACK_CASES:
        _exact(H, bf16, epi, M, N, K, lambda a: H.tile(bf16, epi, a, _stream()), f"tile<{'bf16' if bf16 else 'fp32'},{GH.EPI_NAMES[epi]}>", seed=M)
        for ns in (2, 4):
            _exact(H, bf16, epi, M, N, K, lambda a: H.block(bf16, epi, ns, a, _stream()), f"block<{'bf16' if bf16 else 'fp32'},{GH.EPI_NAMES[epi]},{ns}>",
                   x_ld=K + 8, seed=M + ns)
    kv = (8, 37, 40)
    _exact(H, bf16, EPI_STORE, 333, 2048, 256, lambda a: H.tile(bf16, EPI_STORE, a, _stream()), "tile kv_col0", kv=kv, kv_col0=1024)
    _exact(H, bf16, EPI_KV, 333, 1024, 256, lambda a: H.block(bf16, EPI_KV, 4, a, _stream()), "block<KV,4>", kv=kv)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_dispatcher_exact(H, bf16):
    """launch_gemm<WT, PRO_COPY, EPI>: the strips up to 256 rows (1 / 2 / 4 / 8 row tiles), the > 256-row kernels above."""
    d = "bf16" if bf16 else "fp32"
    for epi in GH.EPIS:
        N = 2048 if epi == EPI_KV else 1024
        kv = (16, 17, 20) if epi == EPI_KV else None
        for M in (1, 16, 17, 33, 128, 129, 255, 256, 257, 1056):
            for K in ((1024, 2816) if M in (33, 255) else (1024,)):
                _exact(H, bf16, epi, M, N, K, lambda a: H.gemm(bf16, epi, a, _stream()), f"launch_gemm<{d},{GH.EPI_NAMES[epi]}>", kv=kv, seed=M + K)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_strip128_entry_points_exact(H, bf16):
    d = "bf16" if bf16 else "fp32"
    for epi in GH.EPIS:
        kv = (8, 37, 40) if epi == EPI_KV else None
        N = 1024
        for M, K in ((128, 1024), (129, 2816), (255, 192), (256, 1024)):
            for bv in (False, True):
                _exact(H, bf16, epi, M, N, K, lambda a: H.strip(bf16, epi, bv, a, _stream()),
                       f"strip<{d},{GH.EPI_NAMES[epi]},8,{'by value' if bv else 'preloaded'}>", kv=kv, seed=M)


# ---- random data: the kernels' agreement and the float64 bound ---------------------------------------------------------------------------
def _bound_ratio(p, got):
    ref = p.acc[0]
    bound = p.K * 2.0 ** -24 * (p.x.abs() @ p.Ws[0].abs().t())
    r = float(((got.double() - ref).abs() / bound.clamp(min=1e-300)).max())
    assert r <= 1.0, f"error {r:.3f} x the bound K 2^-24 (|W| |x|)"
    return r


@pytest.mark.parametrize("M,N,K", [(2048, 3072, 1024), (1056, 1024, 2816), (300, 5632, 1024), (2049, 1088, 192)])
def test_glds_tile_block_agree_bitwise_on_random_data(H, M, N, K):
    p = Problem(H, True, EPI_STORE, M, N, K, gaussian=True, seed=7)
    outs = {}
    for name, fn in [("glds", lambda a: H.glds_dispatch(EPI_STORE, a, _stream())), ("tile", lambda a: H.tile(True, EPI_STORE, a, _stream())),
                     ("block2", lambda a: H.block(True, EPI_STORE, 2, a, _stream())), ("block4", lambda a: H.block(True, EPI_STORE, 4, a, _stream()))]:
        if name == "block4" and (N // 16) % 4:
            continue
        rc, _ = p.run(fn)
        assert rc == PTTS_OK, (name, H.error())
        outs[name] = p.out.t[:, :N].clone()
    for name, o in outs.items():
        assert torch.equal(o.view(torch.int32), outs["glds"].view(torch.int32)), f"{name} differs from glds bitwise"
    r = _bound_ratio(p, outs["glds"])
    log_parity(f"[gemm random bf16] glds = tile = block bitwise, M={M} N={N} K={K}: error / bound {r:.2e}", LOG)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_random_data_strips_and_fp32_paths(H, bf16):
    d = "bf16" if bf16 else "fp32"
    for M, N, K in ((255, 1024, 2816), (129, 2048, 1024)):
        p = Problem(H, bf16, EPI_STORE, M, N, K, gaussian=True, seed=M)
        outs = {}
        for bv in (False, True):
            rc, _ = p.run(lambda a: H.strip(bf16, EPI_STORE, bv, a, _stream()))
            assert rc == PTTS_OK, H.error()
            outs[bv] = p.out.t[:, :N].clone()
        assert torch.equal(outs[False].view(torch.int32), outs[True].view(torch.int32)), "preloaded and by-value strip entries differ"
        r = _bound_ratio(p, outs[False])
        log_parity(f"[gemm random {d}] strip<8> preloaded = by value bitwise, M={M} N={N} K={K}: error / bound {r:.2e}", LOG)
    if not bf16:  # the fp32 engine's > 256-row kernels
        p = Problem(H, False, EPI_STORE, 1056, 1024, 1024, gaussian=True, seed=3)
        outs = {}
        for name, fn in (("tile", lambda a: H.tile(False, EPI_STORE, a, _stream())), ("block2", lambda a: H.block(False, EPI_STORE, 2, a, _stream())),
                         ("block4", lambda a: H.block(False, EPI_STORE, 4, a, _stream()))):
            rc, _ = p.run(fn)
            assert rc == PTTS_OK, H.error()
            outs[name] = p.out.t[:, :1024].clone()
            log_parity(f"[gemm random fp32] {name} M=1056 N=1024 K=1024: error / bound {_bound_ratio(p, outs[name]):.2e}", LOG)
        assert torch.equal(outs["tile"].view(torch.int32), outs["block2"].view(torch.int32)) and torch.equal(outs["tile"], outs["block4"])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,pad", [(300, 1024, 96, 0), (300, 1040, 1024, 0), (300, 1024, 1024, 4)], ids=["K%64", "N%64", "x_ld%8"])
def test_glds_declines_and_the_fallback_is_exact(H, M, N, K, pad):
    p = Problem(H, True, EPI_STORE, M, N, K, x_ld=K + pad, seed=1)
    a = p.fresh(N + 8)
    assert H.glds_dispatch(EPI_STORE, a, _stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(p.out.bits(), p.out.expected_bits(lambda v: None)), "a declined launch wrote"
    _exact(H, True, EPI_STORE, M, N, K, lambda a: H.gemm(True, EPI_STORE, a, _stream()), "launch_gemm fallback", x_ld=K + pad, seed=1)


def test_glds_grid_field_limits(H):
    inst = _inst(EPI_STORE, 4, 4)
    _exact(H, True, EPI_STORE, 65, 2047 * 64, 64, lambda a: H.glds(inst, a, _stream()), f"{_name(inst)} 2047 column tiles")
    p = Problem(H, True, EPI_STORE, 65, 64, 64)
    a = p.fresh(72)
    for N, M in ((2049 * 64, 65), (64, 64 * 0x100000 + 1)):  # 11-bit / 20-bit grid fields: refused before any launch
        a.N, a.M = N, M
        assert H.glds(inst, a, _stream()) == PTTS_E_UNSUPPORTED, (N, M)
        assert "grid extents" in H.error()
    torch.cuda.synchronize()
    assert torch.equal(p.out.bits(), p.out.expected_bits(lambda v: None))
    log_parity(f"[gemm refusal] {_name(inst)}: N = 2047 x 64 exact, 2049 x 64 columns / 2^20 + 1 row tiles PTTS_E_UNSUPPORTED", LOG)


# ---- negative control: one packed weight off by one ------------------------------------------------------------------------------------
def test_negative_control_one_packed_weight(H):
    inst = _inst(EPI_STORE, 4, 4)
    M, N, K = 300, 1024, 1024
    p = Problem(H, True, EPI_STORE, M, N, K, seed=5)
    n0, k0 = 517, 777
    # A-fragment order: strip n0 / 16, fragment k0 / 32, lane (n0 % 16) + 16 ((k0 % 32) / 8), element k0 % 8
    idx = (((n0 // 16) * (K // 32) + k0 // 32) * 64 + (n0 % 16) + 16 * ((k0 % 32) // 8)) * 8 + k0 % 8
    assert float(p.packed[0][idx]) == float(p.Ws[0][n0, k0])
    p.packed[0][idx] += 1
    rc, _ = p.run(lambda a: H.glds(inst, a, _stream()))
    assert rc == PTTS_OK
    with pytest.raises(AssertionError):
        p.check_exact("negative control")
    diff = (p.out.t[:, :N].double() - p.acc[0]) != 0
    cols = diff.any(0).nonzero().flatten().tolist()
    rows = diff[:, n0].nonzero().flatten()
    assert cols == [n0], cols
    assert torch.equal(rows, (p.x[:, k0] != 0).nonzero().flatten())
    assert torch.equal(p.out.t[:, n0].double() - p.acc[0][:, n0], p.x[:, k0])
    log_parity(f"[gemm negative control] {_name(inst)}: W[{n0}][{k0}] + 1 fails the exact check on column {n0} only ({rows.numel()} rows)", LOG)


# ---- the folded T5 RMSNorm (rs_part / nx_out) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_folded_norm_is_refused_where_no_kernel_serves_it(H, bf16):
    """Above 256 rows only the strips carry the folded RMSNorm fields: the dispatcher used to fall back to the tile / block kernels, which
    ignore them (no rstd scaling, no nx_out / ss_out) and report success. Now PTTS_E_UNSUPPORTED, nothing written; <= 64 rows per pass: served."""
    N, K = 1024, 1024
    rs_n = K // 16
    for epi, M in ((EPI_STORE, 300), (EPI_GATE_WT, 1056), (EPI_RESID, 2048), (EPI_STORE, 200)):
        p = Problem(H, bf16, epi, M, N, K, seed=M)
        rs = torch.rand(M, rs_n, device=DEV) + 0.5
        nx = torch.empty(M, N, device=DEV, dtype=p.dt)
        ss = torch.empty(M, N // 16, device=DEV)
        gam = torch.ones(N, device=DEV)
        a = p.fresh(p.out_cols() + 8)
        if epi == EPI_RESID:
            a.nx_out, a.nx_gamma, a.ss_out = nx.data_ptr(), gam.data_ptr(), ss.data_ptr()
        else:
            a.rs_part, a.rs_n, a.rs_invD, a.rms_eps = rs.data_ptr(), rs_n, 1.0 / K, 1e-6
        rc = H.gemm(bf16, epi, a, _stream())
        torch.cuda.synchronize()
        assert rc == PTTS_E_UNSUPPORTED, f"{GH.EPI_NAMES[epi]} M={M}: status {rc}"
        keep = (lambda v: v[:, :N].copy_(p.resid.float())) if epi == EPI_RESID else (lambda v: None)
        assert torch.equal(p.out.bits(), p.out.expected_bits(keep)), "a refused GEMM wrote"
    # served: 64 rows, rstd scaling of the consumer
    M = 64
    p = Problem(H, bf16, EPI_STORE, M, N, K, seed=11)
    rs = torch.rand(M, rs_n, device=DEV) + 0.5
    a = p.fresh(N + 8)
    a.rs_part, a.rs_n, a.rs_invD, a.rms_eps = rs.data_ptr(), rs_n, 1.0 / K, 1e-6
    assert H.gemm(bf16, EPI_STORE, a, _stream()) == PTTS_OK, H.error()
    torch.cuda.synchronize()
    rstd = 1.0 / torch.sqrt(rs.double().sum(1) / K + 1e-6)
    ref = p.acc[0] * rstd[:, None]
    rel = float(((p.out.t[:, :N].double() - ref).abs() / ref.abs().amax()).max())
    assert rel <= 1e-6, rel
    log_parity(f"[gemm folded norm {'bf16' if bf16 else 'fp32'}] > 256 rows and 128-row passes: PTTS_E_UNSUPPORTED; 64 rows served, rel err {rel:.1e}", LOG)
