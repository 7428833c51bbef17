"""GPU: score_heads_kernel (final LayerNorm + LM heads + cross-entropy, parler_tts_amd/csrc/ptts_score_kernels.h) launched directly through
score_launch - the function the engine calls - behind tests/native/score_harness.hip, on guarded buffers.

Checks, per case: `counted` is exact; an uncounted `nll` is exactly 0; with logits stored, `nll` agrees with the float64 cross-entropy of the
kernel's OWN stored logits within score_model.kernel_bound -
    V * 2^-24  (the fp32 sum of V terms in (0, 1])  +  8 ulp32(|lse|)  (base-2 scaling, v_exp / v_log, the multiplication by ln 2)
    +  4 ulp32(|label logit|)  (the final subtraction);
the stored logits equal the existing PRO_LN / EPI_STORE projection on the same rows (another kernel: rows_prep + strip / tile GEMM) within the fp32
summation-order band 2e-5 * scale, scale = max(1, max |logit|) (an fp32 accumulation error grows with the magnitude of what is accumulated), and
within the project's existing bf16 band, a flat 1e-2 whatever the magnitude (both kernels round the same LayerNorm output to bf16 and differ
only in fp32 accumulation order); the no-store instance gives `nll` bit-equal to the store instance; every
guard band around nll / counted / logits is intact.
Shapes: H = 128 and 1024; (K, V) = (9, 1088) and (4, 2048); rows M in {1, 15, 16, 17, 65} (every row-tile count 1 / 2 / 4 with a ragged last
tile, one workgroup and two); two utterances with Q > T (row selection with an offset; logits for all Q rows); labels at column 0, V - 1, the
EOS id, -100 and BOS, an input EOS, one codebook without a counted position; and one case whose logits span more than +-100 (gamma scaled: an
implementation that skips the max subtraction overflows exp there)."""
import numpy as np
import pytest
import torch

import score_harness as SH
import score_model as SM
from helpers import log_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT32 = 0x7FA5C3D2


class Guarded:
    """A tensor of `shape` inside a flat buffer of 32-bit sentinels: `pad` words before it and after it."""

    def __init__(self, shape, dtype, pad=1024):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
        self.pad, self.n = pad, n
        self.buf = torch.full((pad + n + pad,), SENT32, dtype=torch.int32, device=DEV)
        self.t = self.buf[pad:pad + n].view(dtype).view(*shape)

    def guards_intact(self):
        return bool((self.buf[:self.pad] == SENT32).all()) and bool((self.buf[self.pad + self.n:] == SENT32).all())


@pytest.fixture(scope="module")
def harness():
    return SH.Harness(SH.build(SH.default_dir()))


_W = {}


def weights(harness, bf16, H, K, V, gain=1.0):
    key = (bf16, H, K, V, gain)
    if key not in _W:
        g = torch.Generator().manual_seed(H + V)
        w = (torch.randn(K * V, H, generator=g) * (0.3 / H ** 0.5)).to(DEV)
        gamma = ((1.0 + 0.1 * torch.randn(H, generator=g)) * gain).to(DEV)
        beta = (0.1 * torch.randn(H, generator=g)).to(DEV)
        _W[key] = (harness.pack(bf16, w), gamma, beta)
    return _W[key]


def run_case(harness, bf16, H, K, V, B, Q, T, seed, gain=1.0):
    eos, bos = V - 64, V - 63
    packed, gamma, beta = weights(harness, bf16, H, K, V, gain)
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B * Q, H, generator=g) * (1.0 + torch.arange(B * Q)[:, None] % 5)).to(DEV)
    ids = torch.randint(0, V - 64, (B * K, T), generator=g)
    labels = torch.randint(0, V, (B, T, K), generator=g)
    labels[:, :, K - 1] = -100                      # a codebook without a counted position
    labels[0, 0, 0], labels[0, T - 1, 1] = 0, V - 1  # first and last column of the vocabulary
    labels[0, T // 2, 2] = eos
    labels[B - 1, T - 1, 0] = -100
    labels[B - 1, 0, 1] = bos
    ids[2, T // 3] = eos                            # an input EOS under a real label
    want_counted = SM.counted_mask(ids, labels, bos, eos, V)
    assert not bool(want_counted[..., K - 1].any()) and (T < 2 or not bool(want_counted[0, T // 3, 2]))
    ids_d, labels_d = ids.to(DEV), labels.to(DEV)

    def launch(Qs, store):
        nll, counted = Guarded((B, T, K), torch.float32), Guarded((B, T, K), torch.int32)
        logits = Guarded((B * K, Qs, V), torch.float32) if store else None
        a = SH.ShArgs(x=x.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), W=packed.data_ptr(), ids=ids_d.data_ptr(), labels=labels_d.data_ptr(),
                      nll=nll.t.data_ptr(), counted=counted.t.data_ptr(), logits=logits.t.data_ptr() if store else None, x_ld=H, H=H, K=K, V=V, B=B, Q=Q,
                      Qs=Qs, T=T, bos=bos, eos=eos)
        harness.check(harness.score(bf16, a))
        torch.cuda.synchronize()
        assert nll.guards_intact() and counted.guards_intact() and (logits is None or logits.guards_intact())
        return nll.t.cpu(), counted.t.cpu(), logits.t.cpu() if store else None

    nll, counted, logits = launch(Q, True)
    nll0, counted0, _ = launch(T, False)
    assert torch.equal(counted.bool(), want_counted) and torch.equal(counted0, counted) and set(counted.unique().tolist()) <= {0, 1}
    assert torch.equal(nll0, nll), "no-store instance: the same bits"
    assert bool((nll[~want_counted] == 0).all()) and bool(torch.isfinite(nll).all())
    own, lse, picked = SM.token_nll(logits, labels, want_counted)
    d = (nll.double() - own).abs()
    log_parity(f"score kernel {'bf16' if bf16 else 'fp32'} H={H} K={K} V={V} B={B} Q={Q} T={T} gain={gain}: max |logit| {float(logits.abs().max()):.2f} "
          f"max |d nll| vs float64 of own logits {float(d.max()):.3e} (bound >= {float(SM.kernel_bound(lse, picked, V).min()):.3e}; {int(want_counted.sum())} counted)", "score_kernel.txt")
    assert bool((d <= SM.kernel_bound(lse, picked, V)).all())
    # the existing projection on the same rows
    M = B * Q
    out = Guarded((M, K * V), torch.float32)
    xw = torch.empty(M * H * 4, dtype=torch.uint8, device=DEV)
    p = SH.ShArgs(x=x.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), W=packed.data_ptr(), xw=xw.data_ptr(), out=out.t.data_ptr(), x_ld=H, H=H, K=K,
                  V=V, M=M)
    harness.check(harness.project(bf16, p))
    torch.cuda.synchronize()
    assert out.guards_intact()
    proj = out.t.cpu().view(B, Q, K, V).permute(0, 2, 1, 3).reshape(B * K, Q, V)
    band = 1e-2 if bf16 else 2e-5 * max(1.0, float(proj.abs().max()))
    dp = float((logits - proj).abs().max())
    log_parity(f"   stored logits vs PRO_LN / EPI_STORE projection: max |d| {dp:.3e} (band {band:.3e})", "score_kernel.txt")
    assert dp <= band
    return logits


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [128, 1024])
@pytest.mark.parametrize("KV", [(9, 1088), (4, 2048)], ids=["9x1088", "4x2048"])
def test_row_counts_and_row_selection(harness, bf16, H, KV):
    K, V = KV
    for M in (1, 15, 16, 17, 65):
        run_case(harness, bf16, H, K, V, B=1, Q=M, T=M, seed=M)
    run_case(harness, bf16, H, K, V, B=2, Q=23, T=19, seed=99)  # rows [4, 23) of each utterance carry labels; logits for all 46 rows


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_logits_spanning_more_than_a_hundred_either_way(harness, bf16):
    logits = run_case(harness, bf16, 1024, 9, 1088, B=2, Q=20, T=17, seed=7, gain=120.0)
    assert float(logits.max()) > 100 and float(logits.min()) < -100
