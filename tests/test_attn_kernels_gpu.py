"""The attention kernels called directly (tests/native/attn_harness.hip -> launch_attn / launch_prefill_attn / kv_append_kernel / the T5 attention
kernels) against their float64 restatement (tests/attn_model.py) on the inputs of tests/attn_cases.py.

A. Exact modes, bit for bit: uniform (q = 0: the output is the exact mean of the visible V rows) and one-hot (score tiers at least 200 log2-units
   apart: the output is the hottest visible key's V row), with exact RoPE tables, NaN where no query may look, a hotter decoy just beyond the
   context and on masked positions.
B. At the lengths where each path of each instance begins and ends (attn_cases.attn_lengths, PREFILL_Q, PREFILL_N, CROSS_N, T5_SHAPES).
C. Random data (Gaussian q / K / V, real RoPE tables, the e4m3 quantiser) against float64 inside the bound attn_model.tolerance derives from
   float64-side quantities only.

Every buffer a kernel writes - direct_out, part, stats, both caches, both scale arrays - sits between sentinel guards and is compared WHOLE; every
launch runs twice from the same state with bitwise equal results.

Random decode cases with the fused append: the row the launch appends is first checked against the float64 rotation within the rounding of the
engine dtype (one e4m3 step for the quantised cache); the model then attends over that row as the cache holds it after the launch - the contract
("every position, the newest included, is seen as the cache holds it") - so that a last-bit difference of the fp32 rotation does not turn into a
whole bf16 / e4m3 step of a key."""
import math

import numpy as np
import pytest
import torch

import attn_cases as AC
import attn_harness as AH
import attn_model as AM
from helpers import log_parity
from oracle import fp8_oracle as FO

pytestmark = pytest.mark.gpu

LOG = "attn_kernels_parity.txt"
DEV = "cuda"
SENT32 = 0x7FBADBAD  # as a float: a NaN payload no kernel produces
F32, F64 = torch.float32, torch.float64
NH, HH = AC.NH, AC.H
WORST = {}   # kernel family -> largest error / bound of part C
COUNT = {"exact launches": 0, "random launches": 0}


@pytest.fixture(scope="module")
def Hn(tmp_path_factory):
    h = AH.Harness(AH.build(str(tmp_path_factory.mktemp("attn_harness"))))
    yield h
    log_parity(f"[attn kernels] {COUNT['exact launches']} exact launches (each run twice, compared whole and bit for bit), "
               f"{COUNT['random launches']} random launches inside the derived bound", LOG)
    for fam in sorted(WORST):
        log_parity(f"[attn kernels] {fam}: largest error / bound {WORST[fam]:.3e}", LOG)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_bytes(struct):
    return torch.frombuffer(bytearray(bytes(struct)), dtype=torch.uint8).to(DEV)


def _ibits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Guarded:
    """A tensor of `shape` inside a flat buffer of 32-bit sentinels: `pad` words before it and after it (the tensor itself starts as sentinels)."""

    def __init__(self, shape, dtype, pad=1024):
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        n = (nbytes + 3) // 4
        self.pad, self.n, self.nbytes = pad, n, nbytes
        self.buf = torch.full((pad + n + pad,), SENT32, dtype=torch.int32, device=DEV)
        self.t = self.buf[pad:pad + n].view(torch.uint8)[:nbytes].view(dtype).view(*shape)
        self.init = None

    def set(self, cpu):
        """Initial contents (kept: restore() before every launch)."""
        self.init = cpu.contiguous().to(DEV)
        self.t.copy_(self.init)
        return self

    def restore(self):
        self.buf.fill_(SENT32)
        if self.init is not None:
            self.t.copy_(self.init)

    def ptr(self):
        return self.t.data_ptr()

    def snapshot(self):
        return self.buf.clone()

    def guards_intact(self):
        return bool((self.buf[:self.pad] == SENT32).all()) and bool((self.buf[self.pad + self.n:] == SENT32).all())


def sentinels(shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full(((n + 3) // 4,), SENT32, dtype=torch.int32).view(torch.uint8)[:n].view(dtype).view(*shape).clone()


def same(got, exp):
    """Elementwise: equal bits, or equal values (+0 = -0); a sentinel / NaN only equals its own bits."""
    got, exp = got.cpu(), exp.cpu()
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    ok = _ibits(got) == _ibits(exp)
    if got.dtype in (torch.float32, torch.bfloat16):
        ok |= got.float() == exp.float()
    return ok


def assert_same(got, exp, what):
    ok = same(got, exp)
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(int(x) for x in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} elements differ, first at {i}: got {got.cpu()[i].item()!r}, expected {exp.cpu()[i].item()!r}")


def _cache_tensors(c, K):
    """A float64 cache as the engine stores it: (rows tensor in the cache dtype, scales or None); NaN rows stay NaN (e4m3: byte 0x7f, scale NaN)."""
    if c.kv8:
        nan = torch.isnan(K)
        b, s = AM.kv8_quantize(torch.nan_to_num(K).to(F32))
        assert torch.equal(AM.kv8_dequantize(b, s)[~nan], K[~nan]), "the case's cache rows are not e4m3 x power-of-two values"
        b[nan] = 0x7F
        s = s[..., 0].clone()
        s[nan.any(dim=-1)] = float("nan")
        return b, s
    t = K.to(F32).to(torch.bfloat16 if c.bf16 else F32)
    nan = torch.isnan(K)
    assert torch.equal(t.to(F64)[~nan], K[~nan]), "the case's cache rows are not engine-dtype values"
    return t, None


class DecRig:
    """The device side of one DecCase: inputs as plain tensors, everything a kernel writes in guarded buffers."""

    def __init__(self, Hn, c, S=1, out_fo=0):
        self.Hn, self.c, self.S, self.out_fo = Hn, c, S, out_fo
        rows = c.B * c.Q
        self.rows = rows
        self.odt = torch.bfloat16 if (c.bf16 or c.kv8) else F32
        self.q = c.q.to(DEV)
        self.knew = c.knew.to(DEV) if c.knew is not None else None
        self.vnew = c.vnew.to(DEV) if c.vnew is not None else None
        kt, ks = _cache_tensors(c, c.K)
        vt, vs = _cache_tensors(c, c.V)
        self.K = Guarded(kt.shape, kt.dtype).set(kt)
        self.V = Guarded(vt.shape, vt.dtype).set(vt)
        self.Ks = Guarded(ks.shape, F32).set(ks) if c.kv8 else None
        self.Vs = Guarded(vs.shape, F32).set(vs) if c.kv8 else None
        self.dims = _dev_bytes(AH.DevDims(P=c.P, N=c.N))
        self.cur_len = torch.tensor(c.cur_len, dtype=torch.int32, device=DEV) if c.cur_len is not None else None
        self.mask = c.mask.to(DEV) if c.mask is not None else None
        self.cos = c.cos.contiguous().to(DEV) if c.cos is not None else None
        self.sin = c.sin.contiguous().to(DEV) if c.sin is not None else None
        self.out_rows = (rows + 15) // 16 * 16 if out_fo else rows
        self.out = Guarded((self.out_rows, HH), self.odt)
        self.part = Guarded((rows, S, HH), F32)
        self.stats = Guarded((rows, S, NH, 2), F32)
        self.written = [g for g in (self.out, self.part, self.stats, self.K, self.V, self.Ks, self.Vs) if g is not None]

    def args(self, kv_bound=None, waves=4, mode=1, hostP=None, mask_ld=None):
        c = self.c
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        a = AH.AhArgs()
        a.q, a.knew, a.vnew, a.kcache, a.vcache = p(self.q), p(self.knew), p(self.vnew), self.K.ptr(), self.V.ptr()
        a.cur_len, a.dims, a.mask, a.cos, a.sin = p(self.cur_len), p(self.dims), p(self.mask), p(self.cos), p(self.sin)
        a.part, a.stats = self.part.ptr(), self.stats.ptr()
        a.direct_out = self.out.ptr() if self.S == 1 else None
        a.kscale, a.vscale = (self.Ks.ptr(), self.Vs.ptr()) if c.kv8 else (None, None)
        a.q_ld, a.kv_ld, a.cap, a.kv_bound = c.q_ld, c.kv_ld, c.cap, c.cap if kv_bound is None else kv_bound
        a.mask_ld = c.mask_ld if mask_ld is None else mask_ld
        a.S, a.Q, a.nheads, a.H, a.kv_heads, a.n_rep = self.S, c.Q, NH, HH, c.kv_heads, NH // c.kv_heads
        a.cross, a.fused_append, a.out_fo = c.cross, c.fused_append, self.out_fo
        a.hostP, a.hostN = c.P if hostP is None else hostP, c.N
        a.B, a.bf16, a.waves, a.mode, a.scale = c.B, int(c.bf16 or c.kv8), waves, mode, c.scale
        # what the host cannot see in the harness: every length the kernels take from device memory stays inside the buffers
        assert 0 < a.kv_bound <= c.cap and max(c.lens) <= c.cap and (c.mask is None or (c.N if c.cross else c.P) <= c.mask_ld)
        return a

    def run_twice(self, fn, a):
        """Launch from the initial state twice; returns the snapshots of the first run (the second must equal them bit for bit)."""
        snaps = []
        for _ in range(2):
            for g in self.written:
                g.restore()
            rc = fn(a, _stream())
            assert rc == AH.PTTS_OK, self.Hn.error()
            torch.cuda.synchronize()
            snaps.append([g.snapshot() for g in self.written])
        for g, s0, s1 in zip(self.written, *snaps):
            assert torch.equal(s0, s1), "two launches from the same state differ"
            assert g.guards_intact(), "a sentinel guard was overwritten"
        return snaps[0]

    # ---- expectations -----------------------------------------------------------------------------------------------------------------------
    def place_out(self, o):
        """[rows, H] in the output dtype -> the whole output buffer as it must be (sentinels where nothing is written)."""
        e = sentinels((self.out_rows, HH), self.odt)
        if self.out_fo:
            e.view(-1)[AM.fo_elem_index(self.rows, HH, self.odt == torch.bfloat16).reshape(-1)] = o.reshape(-1)
        else:
            e[:self.rows] = o
        return e

    def expected_caches(self):
        """[(guarded, expected tensor)] for K, V and the scales: the initial contents with the appended rows in place."""
        c = self.c
        out = [[self.K, self.K.init.cpu().clone()], [self.V, self.V.init.cpu().clone()]]
        if c.kv8:
            out += [[self.Ks, self.Ks.init.cpu().clone()], [self.Vs, self.Vs.init.cpu().clone()]]
        if c.fused_append:
            nr = c.new_rows()
            for b in range(c.B):
                pos = c.P + c.cur_len[b] - 1
                if c.kv8:
                    out[0][1][b, :, pos], out[1][1][b, :, pos] = nr["kbytes"][b], nr["vbytes"][b]
                    out[2][1][b, :, pos], out[3][1][b, :, pos] = nr["kscale"][b], nr["vscale"][b]
                else:
                    out[0][1][b, :, pos], out[1][1][b, :, pos] = nr["k"][b].to(self.odt), nr["v"][b].to(self.odt)
        return out

    def check_exact(self, m, what):
        """The buffers of the last launch against the model `m` (exact modes): whole and bit for bit."""
        c = self.c
        AC.assert_tiers(m)
        if self.S == 1:
            assert_same(self.out.t, self.place_out(AC.exact_out(m["num"], m["den"], self.odt == torch.bfloat16)), what + ": direct_out")
            assert_same(self.part.t, sentinels(self.part.t.shape, F32), what + ": part (unsplit: untouched)")
            assert_same(self.stats.t, sentinels(self.stats.t.shape, F32), what + ": stats (unsplit: untouched)")
        else:
            assert_same(self.out.t, sentinels(self.out.t.shape, self.odt), what + ": direct_out (split: untouched)")
            assert_same(self.part.t, m["part"].to(F32), what + ": part")
            assert_same(self.stats.t, m["stats"].to(F32), what + ": stats")
        for g, e in self.expected_caches():
            assert_same(g.t, e, what + ": cache / scales")
        COUNT["exact launches"] += 1


def _launcher(Hn, kind):
    return Hn.attn if kind == "attn" else Hn.prefill_attn


def _cfg_id(cfg):
    bf16, kv8, S, NW = cfg
    return f"{'bf16' if bf16 else 'fp32'}{'-e4m3' if kv8 else ''}-S{S}-NW{NW}"


# ---- A + B: attn_kernel, decode self-attention with the fused append -------------------------------------------------------------------------------
@pytest.mark.parametrize("li", range(9))
@pytest.mark.parametrize("cfg", AC.ATTN_CONFIGS, ids=_cfg_id)
def test_attn_decode_self_exact(Hn, cfg, li):
    bf16, kv8, S, NW = cfg
    big = AC.is_big(S, NW, bf16)
    L = AC.attn_lengths(S, NW, bf16)[li]
    kv_heads = 2 if big else (4, 2, 1)[(li + S) % 3]
    Ls = AC.ragged(L, big)
    rounds = AC.hot_rounds(Ls, kv_heads, S, NW, bf16)  # every utterance gets every one of its candidates as the hot key of some K/V head
    variants = [("uniform", None, "nan", 0)] + [("onehot", "exact" if r % 2 == 0 else None, "nan" if r % 2 else "hot", r) for r in range(rounds)]
    if rounds > 1:  # every candidate also with the other RoPE / decoy pairing where the rounds alternate them: shift the walk by one
        variants += [("onehot", None if r % 2 == 0 else "exact", "hot" if r % 2 else "nan", r) for r in range(min(rounds, 2))]
    c64 = (L + 63) // 64 * 64
    for vi, (mode, rope, decoy, r) in enumerate(variants):
        bound_kind = (li + vi) % 3  # kv_bound: the capacity, the longest context rounded up to 64 (below the capacity), exactly the longest context
        cap = c64 + 64 if bound_kind == 1 else None
        c = AC.dec_case(mode=mode, bf16=bf16, kv8=kv8, Ls=Ls, kv_heads=kv_heads, rope=rope, decoy=decoy, hot_round=r, S=S, NW=NW, cap=cap, seed=li)
        rig = DecRig(Hn, c, S=S, out_fo=(li + vi) % 2 if S == 1 else 0)
        kv_bound = (c.cap, c64, L)[bound_kind]
        rig.run_twice(Hn.attn, rig.args(kv_bound=kv_bound, waves=NW))
        rig.check_exact(c.model(S=S, NW=NW), f"{_cfg_id(cfg)} L={L} {mode} rope={rope} decoy={decoy} round={r} kv_heads={kv_heads} kv_bound={kv_bound}")


# ---- attn_kernel, decode cross-attention: 1 / 2 / 4 waves, a fully masked utterance yields 0 ---------------------------------------------------------
@pytest.mark.parametrize("N", AC.CROSS_N)
@pytest.mark.parametrize("NW", [1, 2, 4])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_attn_decode_cross_exact(Hn, bf16, NW, N):
    kv_heads = (4, 2, 1)[(N + NW) % 3]
    rounds = AC.hot_rounds([N, N, N], kv_heads, 1, NW, bf16)
    variants = [("uniform", "exact", "nan", 0)] + [("onehot", "exact" if r % 2 == 0 else None, "nan" if r % 2 else "hot", r) for r in range(rounds)]
    for vi, (mode, rope, decoy, r) in enumerate(variants):
        c = AC.dec_case(mode=mode, bf16=bf16, cross=True, Ls=[0, 0, 0], N=N, kv_heads=kv_heads, rope=rope, decoy=decoy, hot_round=r, NW=NW, seed=N)
        rig = DecRig(Hn, c, out_fo=vi % 2)
        rig.run_twice(Hn.attn, rig.args(waves=NW))
        m = c.model(NW=NW)
        rig.check_exact(m, f"cross {'bf16' if bf16 else 'fp32'} NW={NW} N={N} {mode} rope={rope} decoy={decoy}")
        assert int(m["count"][1].max()) == 0 and float(AC.exact_out(m["num"], m["den"], bf16)[1].float().abs().max()) == 0.0  # the fully masked utterance: 0


# ---- attn_kernel on prefill rows (cur_len null, Q = 5): position = row index -----------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_attn_prefill_rows_exact(Hn, bf16, cross, S):
    for vi, (mode, rope, decoy, P) in enumerate([("uniform", None, "nan", 3), ("onehot", "exact", "hot", 3), ("onehot", "exact", "nan", 0), ("onehot", None, "hot", 4)]):
        c = AC.dec_case(mode=mode, bf16=bf16, decode=False, cross=cross, Ls=[0, 0, 0], Q=5, N=33, P=P, kv_heads=(4, 2, 1)[vi % 3], rope=rope, decoy=decoy,
                        hot_round=vi, S=S, seed=vi)
        rig = DecRig(Hn, c, S=S, out_fo=vi % 2 if S == 1 else 0)
        rig.run_twice(Hn.attn, rig.args(waves=4))
        rig.check_exact(c.model(S=S, NW=4), f"attn_kernel prefill rows {'bf16' if bf16 else 'fp32'} cross={cross} S={S} {mode} P={P}")


# ---- launch_prefill_attn: the VALU kernel (mode 1) and the MFMA kernel (mode 2) on the same inputs ---------------------------------------------------
def _prefill_variants(Q):
    return [("uniform", None, "nan", 0), ("onehot", "exact", "hot", 1), ("onehot", None, "nan", 2)]


# the e4m3 cache runs on the VALU kernel only: a few sizes (one tile, the tile edge, several workgroups, two key tiles)
PREFILL_SELF = [(dt, Q) for dt in ("bf16", "fp32") for Q in AC.PREFILL_Q] + [("e4m3", Q) for Q in (1, 9, 17, 65)]


@pytest.mark.parametrize("dt,Q", PREFILL_SELF, ids=[f"{d}-Q{q}" for d, q in PREFILL_SELF])
def test_prefill_attn_self_exact(Hn, dt, Q):
    # P = 0, 3 and Q - 1 (every query but the last sees prompt positions only), each with its own mode
    for vi, (mode, rope, decoy, P) in enumerate([("uniform", None, "nan", min(3, Q)), ("onehot", "exact", "hot", 0), ("onehot", None, "nan", Q - 1),
                                                 ("onehot", "exact", "nan", min(3, Q))]):
        c = AC.dec_case(mode=mode, bf16=dt != "fp32", kv8=dt == "e4m3", decode=False, Ls=[0, 0, 0], Q=Q, P=P, kv_heads=(4, 2, 1)[(Q + vi) % 3], rope=rope,
                        decoy=decoy, hot_round=vi + Q, prefill_kernel=True, seed=Q)
        m = c.model()
        for kmode in (1,) if dt == "e4m3" else (1, 2):
            rig = DecRig(Hn, c, out_fo=(vi + kmode) % 2)
            rig.run_twice(Hn.prefill_attn, rig.args(mode=kmode))
            rig.check_exact(m, f"prefill self {dt} Q={Q} P={P} mode={kmode} {mode} rope={rope}")


@pytest.mark.parametrize("N", AC.PREFILL_N)
@pytest.mark.parametrize("dt", ["bf16", "fp32", "e4m3"])
def test_prefill_attn_cross_exact(Hn, dt, N):
    for Q in (1, 17, 65) if dt != "e4m3" else (9,):
        for vi, (mode, rope, decoy, r) in enumerate(_prefill_variants(Q)):
            c = AC.dec_case(mode=mode, bf16=dt != "fp32", kv8=dt == "e4m3", decode=False, cross=True, Ls=[0, 0, 0], Q=Q, N=N, kv_heads=(4, 2, 1)[(N + vi) % 3],
                            rope=rope, decoy=decoy, hot_round=r + Q, prefill_kernel=True, seed=N)
            m = c.model()
            for kmode in (1,) if dt == "e4m3" else (1, 2):
                rig = DecRig(Hn, c, out_fo=(vi + kmode) % 2)
                rig.run_twice(Hn.prefill_attn, rig.args(mode=kmode))
                rig.check_exact(m, f"prefill cross {dt} Q={Q} N={N} mode={kmode} {mode} rope={rope}")


@pytest.mark.parametrize("B", [31, 32])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_prefill_attn_mode3_both_sides_of_128_pairs(Hn, bf16, B):
    """mode 3 picks the MFMA kernel from B * heads = 128 (utterance, head) pairs up, the VALU kernel below: both must give the exact result."""
    c = AC.dec_case(mode="onehot", bf16=bf16, decode=False, Ls=[0] * B, Q=3, P=2, kv_heads=2, rope="exact", decoy="hot", prefill_kernel=True, seed=B)
    rig = DecRig(Hn, c)
    rig.run_twice(Hn.prefill_attn, rig.args(mode=3))
    rig.check_exact(c.model(), f"prefill mode 3 B={B}")


def test_prefill_attn_refuses_what_its_16_bit_fields_cannot_hold(Hn):
    c = AC.dec_case(mode="uniform", bf16=True, decode=False, Ls=[0, 0], Q=3, P=2, kv_heads=2, prefill_kernel=True)
    rig = DecRig(Hn, c)
    for kw in (dict(hostP=65536), dict(mask_ld=65536)):  # refused on the host: nothing is launched, the mask is never read
        for g in rig.written:
            g.restore()
        before = [g.snapshot() for g in rig.written]
        a = rig.args()
        for k, v in kw.items():
            setattr(a, k, v)
        assert Hn.prefill_attn(a, _stream()) == AH.PTTS_E_UNSUPPORTED, kw
        assert "16-bit" in Hn.error()
        torch.cuda.synchronize()
        assert all(torch.equal(b, g.snapshot()) for b, g in zip(before, rig.written)), "a refused launch wrote something"


# ---- kv_append_kernel ---------------------------------------------------------------------------------------------------------------------------------
def _append_rig(Hn, c, knew, vnew, Q):
    """A DecRig whose knew / vnew are [B*Q, kv_ld] rows for kv_append_kernel (positions 0 .. Q - 1)."""
    rig = DecRig(Hn, c)
    rig.knew, rig.vnew = knew.to(DEV), vnew.to(DEV)
    return rig


@pytest.mark.parametrize("rope", [None, "exact"], ids=["norope", "rope"])
@pytest.mark.parametrize("Q", [1, 5])
@pytest.mark.parametrize("dt", ["bf16", "fp32", "e4m3"])
def test_kv_append_exact(Hn, dt, Q, rope):
    """Rows 0 .. Q - 1 of every (utterance, K/V head) are written - K rotated at its row index - and nothing else: positions >= Q, the guards."""
    B, kvh = 3, 2
    c = AC.dec_case(mode="uniform", bf16=dt != "fp32", kv8=dt == "e4m3", decode=False, Ls=[0] * B, Q=Q, P=0, kv_heads=kvh, rope=rope, cap=Q + 3, masked=False)
    g = torch.Generator().manual_seed(Q)
    knew = torch.full((B * Q, c.kv_ld), float("nan"), dtype=F32)
    vnew = knew.clone()
    ky, vy = AC._ints(g, B * Q, kvh, 64), AC._ints(g, B * Q, kvh, 64)
    pos = (torch.arange(B * Q) % Q)[:, None].expand(B * Q, kvh)
    knew[:, :kvh * 64] = AC.unrope(ky, c.cos, c.sin, pos).to(F32).reshape(B * Q, -1)
    vnew[:, :kvh * 64] = vy.to(F32).reshape(B * Q, -1)
    rig = _append_rig(Hn, c, knew, vnew, Q)
    a = rig.args()
    rig.run_twice(Hn.kv_append, a)
    nr = AM.append_rows(knew[:, :kvh * 64].reshape(B, Q, kvh, 64), vnew[:, :kvh * 64].reshape(B, Q, kvh, 64), c.cos, c.sin, pos.reshape(B, Q, kvh), c.bf16, c.kv8)
    assert torch.equal(nr["k"], ky.reshape(B, Q, kvh, 64)), "exact RoPE: the rotation of the raw rows is the wanted integer rows"
    ek, ev = rig.K.init.cpu().clone(), rig.V.init.cpu().clone()
    if c.kv8:
        ek[:, :, :Q], ev[:, :, :Q] = nr["kbytes"].transpose(1, 2), nr["vbytes"].transpose(1, 2)
        eks, evs = rig.Ks.init.cpu().clone(), rig.Vs.init.cpu().clone()
        eks[:, :, :Q], evs[:, :, :Q] = nr["kscale"].transpose(1, 2), nr["vscale"].transpose(1, 2)
        assert_same(rig.Ks.t, eks, "kscale")
        assert_same(rig.Vs.t, evs, "vscale")
    else:
        ek[:, :, :Q], ev[:, :, :Q] = nr["k"].transpose(1, 2).to(rig.odt), nr["v"].transpose(1, 2).to(rig.odt)
    assert_same(rig.K.t, ek, "kcache")
    assert_same(rig.V.t, ev, "vcache")
    for g_ in (rig.out, rig.part, rig.stats):
        assert_same(g_.t, sentinels(g_.t.shape, g_.t.dtype), "an attention output (untouched by the append)")
    COUNT["exact launches"] += 1


def test_kv8_quantiser_edges_append_kernel_fused_append_and_oracle_agree(Hn):
    """The edge rows of the e4m3 quantiser: bytes and scales of kv_append_kernel<bf16, KV8> equal oracle/fp8_oracle.quantize_kv_rows bit for bit,
    and equal what attn_kernel<bf16, 4, KV8>'s fused append writes for the same row."""
    x = AC.kv8_edge_rows()
    n = x.shape[0]
    # kv_append_kernel: one utterance, one K/V head, row i at position i
    c = AC.dec_case(mode="uniform", bf16=True, kv8=True, decode=False, Ls=[0], Q=n, P=0, kv_heads=1, cap=n + 2, masked=False)
    knew = torch.full((n, c.kv_ld), float("nan"), dtype=F32)
    knew[:, :64] = x
    vnew = knew.clone()
    vnew[:, :64] = x.flip(0)
    rig = _append_rig(Hn, c, knew, vnew, n)
    rig.run_twice(Hn.kv_append, rig.args())
    kb, ks = rig.K.t[0, 0, :n].cpu(), rig.Ks.t[0, 0, :n].cpu()
    vb, vs = rig.V.t[0, 0, :n].cpu(), rig.Vs.t[0, 0, :n].cpu()
    mb, ms = AM.kv8_quantize(x)
    assert torch.equal(kb, mb) and torch.equal(ks, ms[:, 0]) and torch.equal(vb, mb.flip(0)) and torch.equal(vs, ms[:, 0].flip(0))
    deq = kb.view(torch.float8_e4m3fn).float() * ks[:, None]  # bytes read back through torch.float8_e4m3fn
    assert torch.equal(deq, FO.quantize_kv_rows(x))
    # attn_kernel's fused append: n utterances of one position each (P = 0, cur_len = 1), the same rows
    d = AC.dec_case(mode="uniform", bf16=True, kv8=True, Ls=[1] * n, kv_heads=1, masked=False)
    d.knew[:, :64], d.vnew[:, :64] = x, x.flip(0)
    rig2 = DecRig(Hn, d)
    rig2.run_twice(Hn.attn, rig2.args(waves=4))
    assert torch.equal(rig2.K.t[:, 0, 0].cpu(), kb) and torch.equal(rig2.Ks.t[:, 0, 0].cpu(), ks)
    assert torch.equal(rig2.V.t[:, 0, 0].cpu(), vb) and torch.equal(rig2.Vs.t[:, 0, 0].cpu(), vs)
    # and the one visible key is the appended row: the output is its dequantised V row, rounded to bf16
    exp = (vb.view(torch.float8_e4m3fn).float() * vs[:, None]).bfloat16()
    assert_same(rig2.out.t.view(n, NH, 64)[:, 0], exp, "attention over the appended row alone")
    COUNT["exact launches"] += 2


# ---- T5 ------------------------------------------------------------------------------------------------------------------------------------------------
class T5Rig:
    def __init__(self, Hn, c, bf16, out_fo):
        self.Hn, self.c, self.bf16, self.out_fo = Hn, c, bf16, out_fo
        self.rows = c.B * c.N
        self.odt = torch.bfloat16 if bf16 else F32
        self.qkv, self.bias = c.qkv.to(DEV), c.bias.contiguous().to(DEV)
        self.mask = c.mask.contiguous().to(DEV) if c.mask is not None else None
        self.out_rows = (self.rows + 15) // 16 * 16 if out_fo else self.rows
        self.out = Guarded((self.out_rows, HH), self.odt)

    def run_twice(self, mfma):
        c = self.c
        a = AH.AhT5Args()
        a.qkv, a.bias, a.mask, a.out = self.qkv.data_ptr(), self.bias.data_ptr(), self.mask.data_ptr() if self.mask is not None else None, self.out.ptr()
        a.ld, a.inner, a.bias_ld, a.bias_zero, a.N, a.out_fo, a.B, a.nheads, a.bf16, a.mfma = c.ld, HH, c.bias_ld, c.bias_zero, c.N, self.out_fo, c.B, NH, int(self.bf16), mfma
        snaps = []
        for _ in range(2):
            self.out.restore()
            assert self.Hn.t5_attn(a, _stream()) == AH.PTTS_OK, self.Hn.error()
            torch.cuda.synchronize()
            snaps.append(self.out.snapshot())
        assert torch.equal(*snaps) and self.out.guards_intact()

    place_out = DecRig.place_out


@pytest.mark.parametrize("mask_kind", [None, "right", "left", "row"])
@pytest.mark.parametrize("shape", AC.T5_SHAPES, ids=lambda s: f"B{s[0]}-N{s[1]}")
def test_t5_attn_exact(Hn, shape, mask_kind):
    B, N = shape
    for vi, (mode, r) in enumerate([("uniform", 0), ("onehot", 0), ("onehot", 1), ("onehot", 2)]):
        c = AC.t5_case(mode=mode, B=B, N=N, mask_kind=mask_kind, offset_round=r + N, seed=N + vi)
        m = AC.t5_model(c)
        for b in range(B):  # tiers: 0, T5_HOT, -FLT_MAX
            u = torch.unique(m["scores"][b])
            assert u.numel() == 1 or float((u[1:] - u[:-1]).min()) >= AC.TIER_GAP * math.log(2.0)
        if mask_kind == "row" and mode == "uniform":  # a fully masked row is uniform over ALL N keys
            v = c.qkv[(B - 1) * N:B * N, 2 * HH:3 * HH].double()
            assert torch.equal(m["num"][B - 1, 0], v.sum(dim=0)) and float(m["den"][B - 1, 0, 0]) == N
        for bf16 in (True, False):
            exp = AC.exact_out(m["num"].reshape(B * N, HH), m["den"].reshape(B * N, NH), bf16)
            for mfma in (0, 1):
                rig = T5Rig(Hn, c, bf16, out_fo=(vi + mfma) % 2)
                rig.run_twice(mfma)
                assert_same(rig.out.t, rig.place_out(exp), f"t5 {'mfma' if mfma else 'valu'} {'bf16' if bf16 else 'fp32'} B={B} N={N} mask={mask_kind} {mode} round={r}")
                COUNT["exact launches"] += 1


# ---- C: random data against float64 --------------------------------------------------------------------------------------------------------------------
def _ratio(got, ref, tol):
    return float(((got.double().cpu() - ref).abs() / tol.clamp_min(1e-300)).max())


def _worst(fam, r):
    WORST[fam] = max(WORST.get(fam, 0.0), r)


RANDOM_DEC = AC.random_dec_cases()


def _check_appended_rows(rig):
    """Random decode self-attention: the appended rows within the engine dtype's rounding of the float64 rotation; returns them as the cache holds them."""
    c = rig.c
    u = 2.0 ** -23
    kvh = c.kv_heads
    pos = torch.tensor([c.P + x - 1 for x in c.cur_len])
    kraw = c.knew[:, :kvh * 64].reshape(c.B, kvh, 64).double()
    y = AM.rope(kraw, c.cos, c.sin, pos[:, None].expand(c.B, kvh))
    e = u * (kraw.abs() * c.cos.double()[pos][:, None].abs() + AM.rotate_half(kraw).abs() * c.sin.double()[pos][:, None].abs())
    v = c.vnew[:, :kvh * 64].reshape(c.B, kvh, 64).double()
    bi = torch.arange(c.B)
    if c.kv8:
        ks, vs = rig.Ks.t.cpu()[bi, :, pos].double(), rig.Vs.t.cpu()[bi, :, pos].double()
        nr = c.new_rows()
        assert torch.equal(ks.float(), nr["kscale"]) and torch.equal(vs.float(), nr["vscale"]), "e4m3 row scales"
        k = rig.K.t.cpu()[bi, :, pos].view(torch.float8_e4m3fn).double() * ks[..., None]
        vv = rig.V.t.cpu()[bi, :, pos].view(torch.float8_e4m3fn).double() * vs[..., None]
        assert bool(((k - y).abs() <= 2.0 ** -4 * (y.abs() + 2 * e) + ks[..., None] * 2.0 ** -10 + 2 * e).all()), "appended e4m3 K row"
        assert torch.equal(vv, nr["v"]), "appended e4m3 V row"
    else:
        k, vv = rig.K.t.cpu()[bi, :, pos].double(), rig.V.t.cpu()[bi, :, pos].double()
        rel = 2.0 ** -8 if c.bf16 else 0.0  # bf16: half an ulp of a value in [2^e, 2^(e+1)) is 2^(e-8)
        assert bool(((k - y).abs() <= rel * (y.abs() + 2 * e) + 2 * e).all()), "appended K row"
        assert torch.equal(vv, AM.round_engine(v, c.bf16)), "appended V row"
    return k, vv


@pytest.mark.parametrize("ci", range(len(RANDOM_DEC)), ids=[x[0].replace(" ", "_") for x in RANDOM_DEC])
def test_attention_random_inside_the_derived_bound(Hn, ci):
    name, kind, c, S, NW = RANDOM_DEC[ci]
    bf16_out = c.bf16 or c.kv8
    outs = {}
    for kmode in ((1, 2) if kind == "prefill" and not c.kv8 else (1,)):
        rig = DecRig(Hn, c, S=S)
        rig.run_twice(_launcher(Hn, kind), rig.args(waves=NW, mode=kmode))
        nk = nv = None
        if c.fused_append:
            nk, nv = _check_appended_rows(rig)
            for (g, e), what in zip(rig.expected_caches(), ("kcache", "vcache", "kscale", "vscale")):  # everything but the appended rows: untouched
                ok = same(g.t, e)
                for b in range(c.B):
                    ok[b, :, c.P + c.cur_len[b] - 1] = True
                assert bool(ok.all()), what
        else:
            for g in (rig.K, rig.V, rig.Ks, rig.Vs):
                assert g is None or torch.equal(_ibits(g.t), _ibits(g.init)), "a cache the launch must not write"
        m = AM.decoder_attention(c.heads_q(), c.K, c.V, Q=c.Q, n_rep=NH // c.kv_heads, P=c.P, N=c.N, cur_len=c.cur_len, cross=c.cross, mask=c.mask,
                                 scale=c.scale, cos=c.cos, sin=c.sin, bf16=bf16_out, S=S, NW=NW, new_k=nk, new_v=nv)
        tol = AC.dec_tolerance(c, m, S, NW, bf16_out)
        got = rig.out.t if S == 1 else AM.combine_splits(rig.part.t.cpu(), rig.stats.t.cpu())
        r = _ratio(got, m["out"], tol)
        fam = "attn_kernel" if kind == "attn" else ("prefill_attn_kernel" if kmode == 1 else "prefill_attn_mfma_kernel")
        print(f"{name} [{fam}]: error / bound {r:.3e}")
        _worst(fam + (" e4m3" if c.kv8 else " bf16" if c.bf16 else " fp32"), r)
        assert r <= 1.0, (name, fam, r)
        outs[kmode] = got.double().cpu()
        COUNT["random launches"] += 1
    if len(outs) == 2:
        d = float((outs[1] - outs[2]).abs().max())
        log_parity(f"[attn kernels] {name}: VALU against MFMA prefill, largest |difference| {d:.3e}", LOG)


RANDOM_T5 = AC.random_t5_cases()


@pytest.mark.parametrize("ci", range(len(RANDOM_T5)), ids=[x[0].replace(" ", "_") for x in RANDOM_T5])
def test_t5_attention_random_inside_the_derived_bound(Hn, ci):
    name, c = RANDOM_T5[ci]
    m = AC.t5_model(c)
    for bf16 in (True, False):
        tol = AC.t5_tolerance(c, m, bf16).reshape(c.B * c.N, HH)
        outs = []
        for mfma in (0, 1):
            rig = T5Rig(Hn, c, bf16, out_fo=0)
            rig.run_twice(mfma)
            r = _ratio(rig.out.t, m["out"].reshape(c.B * c.N, HH), tol)
            fam = ("t5_attn_mfma_kernel" if mfma else "t5_attn_kernel") + (" bf16" if bf16 else " fp32")
            print(f"{name} [{fam}]: error / bound {r:.3e}")
            _worst(fam, r)
            assert r <= 1.0, (name, fam, r)
            outs.append(rig.out.t.double().cpu())
            COUNT["random launches"] += 1
        log_parity(f"[attn kernels] {name} {'bf16' if bf16 else 'fp32'}: VALU against MFMA T5, largest |difference| {float((outs[0] - outs[1]).abs().max()):.3e}", LOG)
