"""Helpers shared by the tests that call decode-step kernels directly (tests/test_step_kernels_gpu.py, tests/test_gemv_kernels_gpu.py): buffers
between sentinels, bitwise comparison, the launch-twice rule with its stop on a faulted device, NaN-padded rows, and the check of an epilogue's
output against exact accumulators."""
import collections
import math

import pytest
import torch

import step_model as SM
from step_harness import EPI_GELU_WT, EPI_RESID, EPI_STORE, PTTS_OK

DEV = "cuda"
F64 = torch.float64
SENT32, SENT16 = 0x7FBADBAD, 0x7FBB  # NaN payloads no kernel produces
EXACT = collections.Counter()        # kernel family -> exact launches (each run twice and compared whole)


def _edt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


class Guarded:
    """n elements inside a flat buffer of sentinels: `pre` elements before, `post` after. `init(flat view)` (optional) writes what the launch
    finds in them (a residual); everything it leaves alone is a sentinel."""

    def __init__(self, n, dtype, init=None, pre=1024, post=1024):
        self.n, self.dtype, self.pre = n, dtype, pre
        self.idt = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self.sent = SENT16 if dtype == torch.bfloat16 else SENT32
        self.buf = torch.full((pre + n + post,), self.sent, dtype=self.idt, device=DEV)
        self.t = self.buf.view(dtype)[pre:pre + n]
        self.init = init
        self.reset()

    def reset(self):
        self.buf.fill_(self.sent)
        if self.init is not None:
            self.init(self.t)

    def ptr(self):
        return self.t.data_ptr()

    def bits(self):
        return self.buf

    def expected(self, fill):
        """The whole buffer as it must be: sentinels (or init) everywhere except where `fill(flat view of the n elements)` writes."""
        e = torch.full_like(self.buf, self.sent)
        v = e.view(self.dtype)[self.pre:self.pre + self.n]
        if self.init is not None:
            self.init(v)
        fill(v)
        return e

    def untouched_outside(self, idx, what):
        """Every element except the flat positions idx still holds its sentinel."""
        got = self.buf.clone()
        got[self.pre + idx.reshape(-1).to(DEV)] = self.sent
        exp = torch.full_like(self.buf, self.sent)
        assert_bits(got, exp, f"{what}: writes outside the real rows")


def assert_bits(got, exp, what):
    if torch.equal(got, exp):
        return
    d = (got != exp).nonzero().flatten()
    raise AssertionError(f"{what}: {d.numel()} elements differ, first at flat {int(d[0])} of the guarded buffer")


def twice(H, fam, launch, outs, exact=True):
    """launch() twice on reset buffers; bitwise equal results; the buffers hold the second run."""
    snaps = []
    for _ in range(2):
        for o in outs:
            o.reset()
        rc = launch()
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:  # a faulted device: nothing more is launched on it
            pytest.exit(f"{fam}: the device reported an error after the launch: {e}", returncode=3)
        assert rc == PTTS_OK, f"{fam}: status {rc}: {H.error()}"
        snaps.append([o.bits().clone() for o in outs])
    for a, b in zip(*snaps):
        assert torch.equal(a, b), f"{fam}: two launches of the same node differ"
    if exact:
        EXACT[fam] += 1


def nanpad(x, ld, dtype):
    """[M, K] -> device [M, ld] of dtype whose columns past K hold NaN (any read of them would spread into the results)."""
    M, K = x.shape
    b = torch.full((M, ld), float("nan"), device=DEV, dtype=dtype)
    b[:, :K] = x.to(device=DEV, dtype=dtype)
    return b


def act_rows(g, M, K, ld, fo, bf16):
    """(rows [M, K] of a Guarded activation buffer, flat positions of the rows' elements): row-major with stride ld, or fragment order."""
    idx = SM.fo_elem_index(M, K, bf16) if fo else (torch.arange(M)[:, None] * ld + torch.arange(K)[None, :])
    return g.t[idx.to(DEV)], idx


def check_epilogue(tag, g, M, N, ld, fo, epi, bf16, acc, resid=None):
    """The output buffer g of one launch against the exact accumulators acc [M, N] (float64, CPU)."""
    wt = epi == EPI_GELU_WT
    od = _edt(bf16) if wt else torch.float32
    if epi in (EPI_STORE, EPI_RESID):
        ref = acc + (resid if resid is not None else 0)
        assert float(ref.abs().max()) < 2 ** 24
        assert_bits(g.bits(), g.expected(lambda v: v.view(M, ld)[:, :N].copy_(ref.to(od))), f"{tag}: output")
        return "exact"
    got, idx = act_rows(g, M, N, ld, fo, bf16 and wt)
    g.untouched_outside(idx, tag)
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{tag}: NaN / inf in a real row"
    ref = SM.gelu_erf64(acc)
    # EPI_GELU_WT: one ulp of the engine dtype of float64's value, in both engines (gelu_erf_wt). EPI_GELU (an fp32 intermediate of either engine,
    # up to 8 rows): the bound of an fp32 evaluation of 0.5 x (1 + erf(x / sqrt 2)) (step_model.gelu_bound_fp32)
    one_ulp = wt
    tol = SM.ulp(ref, od == torch.bfloat16) if one_ulp else SM.gelu_bound_fp32(acc)
    err = (got - ref).abs()
    r = float(torch.where(tol > 0, err / tol, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err))).max())  # gelu(0) = 0 exactly
    print(f"{tag}: gelu error / {'one ulp of ' + str(od) if one_ulp else 'fp32 evaluation bound'} {r:.2f}")
    assert r <= 1.0, f"{tag}: {int(((got - ref).abs() > tol).sum())} outputs beyond {'one ulp of ' + str(od) if one_ulp else 'the fp32 evaluation bound'}, worst {r:.2f} x"
    return f"within the bound (worst {r:.2f})"
