"""The WARP instances of the sampler tail called directly (tests/native/warp_tail_harness.hip -> tail_launch -> tail_warp_kernel<NV, SESSION>)
against the host model of their stages (tests/warper_model.py on top of sampler_model.TailModel), token for token, after every step: the
whole sampler state (ids, cur_len, unfinished, has_eos, first_unf) must equal the model's. A draw the model calls ambiguous (a decision inside
a rounding band, or a target on a cumulative boundary) is settled as TailModel.step settles one: the device's token must come from the accepted
neighbourhood. Shapes: V = 300 / 1088 / 2048 (NV 8 / 18 / 32), K = 9 and K = 18 (more codebooks than waves: the loop reloads its logits),
static with 3 utterances under three different records, and a 3-slot session (one idle, one on the session's record, one with its own
sampler record and its own warper record). With the neutral record the WARP instance draws what the instance without the feature draws."""
import numpy as np
import pytest
import torch

import sampler_cases as SC
import sampler_model as SM
import warp_tail_harness as WH
import warper_cases as WC
import warper_model as WM
from helpers import log_parity
from tail_harness import DevDims, DevGen

pytestmark = pytest.mark.gpu

LOG = "warp_tail.txt"
DEV = "cuda"
FILL = -777
STEPS = 12
SHAPES = [(300, 9), (1088, 9), (2048, 9), (300, 18), (1088, 18), (2048, 18)]
F32 = np.float32


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return WH.Harness(WH.build(str(tmp_path_factory.mktemp("warp_tail_harness"))))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_bytes(struct):
    return torch.frombuffer(bytearray(bytes(struct)), dtype=torch.uint8).to(DEV)


def _dev_gen(gp, seed):
    return DevGen(gp.max_length, gp.min_new_tokens, int(gp.do_sample), gp.top_k, int(gp.use_eos_gate), gp.temperature, gp.top_p, seed)


class Rig:
    """The device side of one case: TailModel's state in device tensors (ids inside guard columns), DevGen / DevDims, the records."""

    def __init__(self, H, m, gp, seed):
        self.H, self.m = H, m
        B, K, V = m.B, m.K, m.V
        self.ids = torch.full((B * K + 2, m.ld), FILL, dtype=torch.int64, device=DEV)  # a guard row on either side
        self.cur_len, self.first_unf = (torch.zeros(B, dtype=torch.int32, device=DEV) for _ in range(2))
        self.unfinished, self.has_eos = (torch.zeros(B * K, dtype=torch.int32, device=DEV) for _ in range(2))
        self.row_maxlen = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.logits = torch.zeros(B, K, V, dtype=torch.float32, device=DEV)
        self.warp = torch.zeros(B, 4, dtype=torch.float32, device=DEV)
        self.slot_gen = torch.zeros(B, WH.C.sizeof(WH.SlotGen), dtype=torch.uint8, device=DEV)
        self.set_gen(gp, seed)
        self.dims = _dev_bytes(DevDims(m.P, 0, gp.max_length, 0, None, 0))
        self.upload()

    def set_gen(self, gp, seed):
        self.gen = _dev_bytes(_dev_gen(gp, seed))

    def upload(self):
        m = self.m
        self.ids[1:-1].copy_(torch.from_numpy(m.ids))
        for t, v in ((self.cur_len, m.cur_len), (self.first_unf, m.first_unf), (self.unfinished, m.unfinished), (self.has_eos, m.has_eos)):
            t.copy_(torch.from_numpy(v))
        if m.session:
            self.row_maxlen.copy_(torch.from_numpy(m.row_maxlen))

    def set_records(self, recs):
        for b, wp in enumerate(recs):
            assert self.H.set_warp(self.warp.data_ptr(), b, 1, tuple(wp), _stream()) == WH.PTTS_OK, self.H.error()
        torch.cuda.synchronize()
        assert np.array_equal(self.warp.cpu().numpy(), np.asarray(recs, dtype=F32))  # set_warp_kernel wrote what it was given, nothing else

    def launch(self, lg, warp=True, grid=None, row0=0):
        m = self.m
        self.logits.copy_(torch.from_numpy(lg))
        a = WH.WhArgs()
        a.logits, a.ids, a.cur_len, a.unfinished = self.logits.data_ptr(), self.ids[1:].data_ptr(), self.cur_len.data_ptr(), self.unfinished.data_ptr()
        a.has_eos, a.first_unf, a.gen, a.dims = self.has_eos.data_ptr(), self.first_unf.data_ptr(), self.gen.data_ptr(), self.dims.data_ptr()
        a.row_maxlen, a.slot_gen = self.row_maxlen.data_ptr(), self.slot_gen.data_ptr()
        a.warp = self.warp.data_ptr() if warp else None
        a.ids_ld, a.B, a.K, a.V, a.eos, a.pad = m.ld, m.B, m.K, m.V, m.eos, m.pad
        a.session, a.row0, a.grid = int(m.session), row0, m.B if grid is None else grid
        assert self.H.tail(a, _stream()) == WH.PTTS_OK, self.H.error()
        torch.cuda.synchronize()

    def dev_ids(self):
        return self.ids[1:-1].cpu().numpy()

    def chooser(self, what, m=None, row0=0):
        """Settles an ambiguous draw of model ``m`` (default the rig's; a one-slot model: its rows start at device row ``row0``)."""
        m = m or self.m
        dev = self.dev_ids()

        def choose(row, accepted):
            tok = int(dev[row0 + row, int(m.cur_len[row // m.K])])
            assert tok in accepted, (what, row0 + row, tok, sorted(accepted))
            return tok

        return choose

    def assert_equals_model(self, what):
        m = self.m
        assert bool((self.ids[0] == FILL).all()) and bool((self.ids[-1] == FILL).all()), f"{what}: a guard row was overwritten"
        got = self.dev_ids()
        assert np.array_equal(got, m.ids), (what, np.argwhere(got != m.ids)[:8])
        for name, t, v in (("cur_len", self.cur_len, m.cur_len), ("first_unf", self.first_unf, m.first_unf), ("unfinished", self.unfinished, m.unfinished),
                           ("has_eos", self.has_eos, m.has_eos)):
            assert np.array_equal(t.cpu().numpy(), v), (what, name)


def _static_model(V, K, B, gp):
    eos, pad, bos = SC.ids_of(V)
    return SM.TailModel(B, K, V, eos, pad, bos, ld=gp.max_length + 2, P=2, max_length=gp.max_length, fill=FILL)


def _rows(V, K, B, seed):
    return WC.random_rows(V, B * K, seed).reshape(B, K, V)


# ---- static ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", SHAPES)
def test_static_tokens_equal_the_model_under_three_records_per_launch(H, V, K):
    B, seed = 3, 4321
    draws = ambiguous = 0
    n = len(WC.CONFIGS)
    for cfg, (name, wp, T, top_k, top_p) in enumerate(WC.CONFIGS):
        gp = WC.gen(T, top_k, top_p, max_length=STEPS + 2, min_new_tokens=STEPS + 2 if cfg % 2 else 0)
        recs = [wp, WC.CONFIGS[(cfg + 3) % n][1], WM.NEUTRAL]  # utterance b reads record b
        lg = _rows(V, K, B, 100 + cfg)
        rig = Rig(H, _static_model(V, K, B, gp), gp, seed)
        rig.set_records(recs)
        for s in range(STEPS):
            what = f"V={V} K={K} {name} step {s}"
            rig.launch(lg)
            WM.step_with_records(rig.m, lg, gp, recs, seed=seed, choose=rig.chooser(what))
            rig.assert_equals_model(what)
        draws, ambiguous = draws + rig.m.stats["draws"], ambiguous + rig.m.stats["ambiguous"]
    log_parity(f"static NV={SM.nv_of(V)} V={V} K={K} B={B}: {n} configurations x {STEPS} steps, {draws} draws, {draws - ambiguous} exact, "
               f"ambiguous {ambiguous} ({100 * ambiguous / draws:.2f} %), state equal after every step", LOG)
    assert draws >= n * STEPS * K and ambiguous / draws <= SC.AMBIGUOUS_CAP, (draws, ambiguous)


@pytest.mark.parametrize("V,K", [(300, 9), (1088, 18), (2048, 9)])
def test_crafted_rows(H, V, K):
    """Ties at every threshold, only the arg-max left, near one-hot, uniform, -inf entries: in the first and the last codebook of utterances
    0 and 1, random rows around them. Rows the model calls ambiguous go one way or the other as a whole (the accepted set)."""
    B, seed = 2, 77
    for name, row, wp, (T, top_k, top_p), _ in WC.crafted(V):
        gp = WC.gen(T, top_k, top_p, max_length=6, min_new_tokens=0)  # EOS is free in codebook 0 (the gate blocks it above first_unf only)
        lg = _rows(V, K, B, 7)
        lg[0, 0] = lg[1, K - 1] = row
        rig = Rig(H, _static_model(V, K, B, gp), gp, seed)
        rig.set_records([wp, wp])
        for s in range(4):
            what = f"crafted V={V} K={K} {name} step {s}"
            rig.launch(lg)
            WM.step_with_records(rig.m, lg, gp, [wp, wp], seed=seed, choose=rig.chooser(what))
            rig.assert_equals_model(what)
        kept = WM.warp_kept(row, gp, wp, False, V - 8)
        assert all(kept.mask[t] or kept.ambiguous for t in rig.m.ids[0, 1:5]), name
    log_parity(f"crafted NV={SM.nv_of(V)} V={V} K={K}: {len(WC.crafted(V))} rows x 4 steps, state equal after every step", LOG)


@pytest.mark.parametrize("V,K", [(300, 9), (1088, 18), (2048, 9)])
def test_a_greedy_row_ignores_a_non_neutral_record(H, V, K):
    B = 3
    gp = WC.gen(max_length=STEPS + 2, min_new_tokens=0, do_sample=False)
    recs = [WM.Warp(min_p=0.9), WC.ALL, WM.Warp(typical_p=0.2, eta_cutoff=0.5)]
    rig = Rig(H, _static_model(V, K, B, gp), gp, 5)
    rig.set_records(recs)
    for s in range(4):
        lg = _rows(V, K, B, 300 + s)
        lg[:, :, V - 8] = -20.0  # no EOS: the rows stay live
        rig.launch(lg)
        WM.step_with_records(rig.m, lg, gp, recs, seed=5)
        rig.assert_equals_model(f"greedy V={V} K={K} step {s}")
        assert np.array_equal(rig.m.ids[:, s + 1].reshape(B, K), lg.argmax(-1))


# ---- the neutral record ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("session", [False, True])
@pytest.mark.parametrize("V,K", [(300, 9), (1088, 9), (2048, 18)])
def test_with_the_neutral_record_the_tokens_are_those_of_the_instance_without_the_feature(H, V, K, session):
    B, seed = 3, 99
    out = {}
    for warp in (False, True):
        cols = []
        for name, T, top_k, top_p in (("plain", 1.0, 0, 1.0), ("top-k top-p", 0.8, 40, 0.9)):
            gp = WC.gen(T, top_k, top_p, max_length=STEPS + 2, min_new_tokens=STEPS + 2)  # EOS blocked: every row stays live
            eos, pad, bos = SC.ids_of(V)
            if session:
                m = SM.TailModel(B, K, V, eos, pad, bos, ld=STEPS + 4, session=True, P=2, fill=FILL)
                for b in range(B):
                    m.reset_row(b, 1, STEPS + 2)
            else:
                m = _static_model(V, K, B, gp)
            rig = Rig(H, m, gp, seed)
            rig.set_records([WM.NEUTRAL] * B)
            lg = _rows(V, K, B, 500)
            for s in range(STEPS):
                rig.launch(lg, warp=warp)
            cols.append(rig.dev_ids().copy())
            assert (rig.cur_len.cpu().numpy() == STEPS + 1).all()
        out[warp] = cols
    for a, b in zip(out[False], out[True]):
        assert np.array_equal(a, b), np.argwhere(a != b)[:8]
    assert len({c.tobytes() for c in out[True]}) == 2  # the two settings do draw differently


# ---- session --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", SHAPES)
def test_session_slots_idle_default_and_own_records(H, V, K):
    """Slot 0 stays idle, slot 1 runs on the session's sampler and warper records, slot 2 on its own SlotGen (its own seed: the hash sees the
    codebook index alone) and its own warper record. Admission launches are grid 1 at row0 = the slot, steps grid 3."""
    B, L = 3, STEPS + 4
    eos, pad, bos = SC.ids_of(V)
    sgp, sseed, swp = WC.gen(1.0, 0, 0.95, max_length=3, min_new_tokens=2), 7, WC.ALL
    ogp, oseed, owp = WC.gen(0.8, 60, 1.0, max_length=L, min_new_tokens=L), 0x5EEDA0000001, WM.Warp(min_p=0.2, typical_p=0.5)
    full = SM.TailModel(B, K, V, eos, pad, bos, ld=L + 2, session=True, P=2, fill=FILL)
    sub = SM.TailModel(1, K, V, eos, pad, bos, ld=L + 2, session=True, P=2, fill=FILL)
    for b in range(B):
        full.reset_row(b, 0, L)
    rig = Rig(H, full, sgp, sseed)
    rig.set_records([swp, swp, swp])
    lg = _rows(V, K, B, 900)
    lg[:, :, eos] = -30.0  # no EOS: both requests stay live through the steps

    def pull():
        full.ids[2 * K:] = sub.ids
        full.unfinished[2 * K:], full.has_eos[2 * K:] = sub.unfinished, sub.has_eos
        full.cur_len[2], full.first_unf[2], full.row_maxlen[2] = sub.cur_len[0], sub.first_unf[0], sub.row_maxlen[0]

    def step(what, slots, **launch):
        rig.launch(lg, **launch)
        live = WM.step_with_records(full, lg, sgp, [swp] * B, slots=[b for b in slots if b != 2], seed=sseed, choose=rig.chooser(what))
        if 2 in slots:
            live += [2] * bool(WM.step_with_records(sub, lg[2:3], ogp, [owp], seed=oseed, choose=rig.chooser(what, sub, 2 * K)))
            pull()
        rig.assert_equals_model(what)
        return sorted(live)

    # admissions: slot 1 plainly, slot 2 with both records (written while the slot is idle, as the engine does)
    full.reset_row(1, 1, L)
    rig.upload()
    assert step("admit slot 1", [1], grid=1, row0=1) == [1]
    full.reset_row(2, 1, L)
    sub.reset_row(0, 1, L)
    rig.upload()
    assert H.set_slot_gen(rig.slot_gen.data_ptr(), 2, _dev_gen(ogp, oseed), _stream()) == WH.PTTS_OK, H.error()
    assert H.set_warp(rig.warp.data_ptr(), 2, 1, tuple(owp), _stream()) == WH.PTTS_OK, H.error()
    assert step("admit slot 2", [2], grid=1, row0=2) == [2]
    for s in range(STEPS):
        assert step(f"session V={V} K={K} step {s}", [0, 1, 2]) == [1, 2]
    assert full.cur_len[0] == 1 and (full.ids[:K, 1:] == FILL).all()  # the idle slot was never written
    st = {k: full.stats[k] + sub.stats[k] for k in full.stats}
    log_parity(f"session NV={SM.nv_of(V)} V={V} K={K}: 2 admissions + {STEPS} steps, {st['draws']} draws, ambiguous {st['ambiguous']} "
               f"({100 * st['ambiguous'] / st['draws']:.2f} %), state equal after every launch", LOG)
    assert st["ambiguous"] / st["draws"] <= SC.AMBIGUOUS_CAP, st
