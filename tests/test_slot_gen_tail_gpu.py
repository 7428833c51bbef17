"""The session tail with per-slot sampler records, called directly (tests/native/slot_gen_harness.hip -> tail_launch with the record pointer
-> tail_kernel<NV, true>; records written by the product's set_slot_gen_kernel) against the host restatement (tests/slot_gen_cases.py:
one sampler_model.TailModel per slot that has a record, row index = the codebook index; the B-slot model on the session's seed and rows
b * K + k for the others), on the three NV instances.

After EVERY launch the whole state - ids, cur_len, unfinished, has_eos, first_unf, row_maxlen, the records and the embedding h of the next
column - must equal the model's bit for bit, the guards around them must survive, the logits must be untouched, and every launch runs twice
from the same state with bitwise equal results (Rig.twice of tests/test_sampler_tail_gpu.py). Draws whose target lies within the fp32 rounding
band of a cumulative boundary (sampler_model.band) are settled from the accepted neighbourhood, at most 4 % per configuration."""
import numpy as np
import pytest
import torch

import sampler_cases as SC
import sampler_model as SM
import slot_gen_cases as GC
import slot_gen_harness as SG
import tail_harness as TH
from helpers import log_parity
from test_sampler_tail_gpu import Guarded, Rig, _stream

pytestmark = pytest.mark.gpu

LOG = "slot_gen_tail.txt"


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return TH.Harness(TH.build(str(tmp_path_factory.mktemp("tail_harness"))))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return SG.Harness(SG.build(str(tmp_path_factory.mktemp("slot_gen_harness"))))


class SlotRig(Rig):
    """Rig of tests/test_sampler_tail_gpu.py over SlotSession.full, plus the B records in a guarded buffer (snapshot / restore / twice and the
    guard checks cover it) and launches through the harness that passes the record pointer."""

    def __init__(self, H, S, session, hidden):
        self.S, self.session = S, session
        super().__init__(H, session.full, session.gp, session.seed, hidden=hidden, dims_max_length=3)
        self.recs = Guarded((session.B, SG.WORDS), torch.int32)
        self.guarded.append(self.recs)

    def assert_equals_model(self, what):
        super().assert_equals_model(what)
        got, want = self.recs.t.cpu().numpy().copy(), self.session.recs.copy()
        got[:, SG.PAD_WORD] = want[:, SG.PAD_WORD] = 0
        assert np.array_equal(got, want), (what, "records", got, want)

    def set_slots(self, row0, nrows, gen):
        def launch():
            assert self.S.set_slots(self.recs.ptr(), self.m.B, row0, nrows, gen, _stream()) == TH.PTTS_OK, self.S.error()

        self.twice(launch)

    def reset(self, b, live, L, rec, what):
        """What ptts_admit_row_gen / ptts_admit_row / ptts_retire_row enqueue for one slot: session_reset_rows_kernel, then its record."""
        a = self.args()

        def launch():
            assert self.H.reset_rows(a, self.row_maxlen.data_ptr(), b, 1, live, L, _stream()) == TH.PTTS_OK, self.H.error()

        self.twice(launch)
        self.set_slots(b, 1, None if rec is None else GC.dev_gen(rec[0], L, rec[1]))
        self.session.reset(b, live, L, rec)
        self.assert_equals_model(what)

    def tail(self, lg, what, grid=None, row0=0, slots=None):
        """One tail launch with the records (twice), the same step on the model, the whole-state comparison. Returns the live slots."""
        m = self.m
        self.logits.copy_(torch.from_numpy(lg))
        kept = self.logits.clone()
        a = self.args(grid, row0)

        def launch():
            assert self.S.tail(a, self.recs.ptr(), _stream()) == TH.PTTS_OK, self.S.error()

        self.twice(launch)
        assert torch.equal(self.logits.view(torch.int32), kept.view(torch.int32)), f"{what}: the logits changed"
        dev_ids = self.ids.t.cpu().numpy()
        cols = m.cur_len.copy()  # the column each slot writes in this launch

        def choose(row, accepted):  # an ambiguous draw: the device's token, which must come from the neighbourhood of the boundary
            tok = int(dev_ids[row, int(cols[row // m.K])])
            assert tok in accepted, (what, row, tok, sorted(accepted))
            return tok

        live = self.session.step(lg, slots=slots, choose=choose, tables=self.tables_host, pos_table=self.pos_host, h=self.model_h)
        self.assert_equals_model(what)
        return live

    def play(self, events, what, watch=None):
        """Runs the events; returns, per launch that covered slot `watch`, (its ids rows so far, its h row) as the DEVICE holds them."""
        seen = []
        K = self.m.K
        for ev in events:
            if ev[0] == "clear":
                self.recs.t.fill_(0x5A5A5A5A)  # whatever the allocation held
                self.set_slots(0, self.m.B, None)
                self.assert_equals_model(f"{what} clear")
            elif ev[0] == "reset":
                self.reset(*ev[1:], f"{what} reset slot {ev[1]} live {ev[2]}")
            else:
                if ev[0] == "admit":
                    live = self.tail(ev[2], f"{what} admit slot {ev[1]}", grid=1, row0=ev[1], slots=[ev[1]])
                    assert live == [ev[1]]
                else:
                    live = self.tail(ev[2], f"{what} step {ev[1]}")
                if watch is not None and watch in live:
                    n = int(self.m.cur_len[watch])
                    seen.append((self.ids.t[watch * K:(watch + 1) * K, :n].cpu().clone(), self.h.t[watch].view(torch.int32).cpu().clone()))
        return seen


def _rig(H, S, V, K):
    return SlotRig(H, S, GC.SlotSession(GC.SLOTS, K, V, GC.MAXLEN + 3, GC.session_gen(), GC.SESSION_SEED), GC.HIDDEN)


@pytest.mark.parametrize("V,K", GC.SHAPES)
def test_mixed_slots_in_one_launch(H, S, V, K):
    """Greedy, two sampled records admitted at different steps, a slot on the session's DevGen, a slot with its own min_new_tokens and an idle
    slot decode side by side; state, records and the next-column embedding are bit-exact after every launch."""
    rig = _rig(H, S, V, K)
    rig.play(GC.mixed_events(V, K), f"mixed V={V} K={K}")
    m, ses = rig.m, rig.session
    assert (m.unfinished[5 * K:] == 0).all() and m.cur_len[5] == 1  # the idle slot
    assert sorted(ses.own) == [0, 1, 2, 4] and [int(m.cur_len[b]) for b in range(4)] == [14, 12, 9, 14] and m.cur_len[4] >= GC.MIN_NEW_4 + 2
    GC.assert_slot4_waits_for_its_own_bound(ses, K, V)
    st = ses.stats
    share = st["ambiguous"] / st["draws"]
    log_parity(f"mixed slots NV={SM.nv_of(V)} V={V} K={K}: state, records and h bit-exact after every launch; {st['draws']} draws, ambiguous "
               f"{st['ambiguous']} ({100 * share:.2f} %)", LOG)
    assert st["draws"] >= 30 * K and share <= SC.AMBIGUOUS_CAP, st


@pytest.mark.parametrize("V,K", GC.SHAPES)
def test_tokens_of_a_record_do_not_depend_on_the_slot_nor_on_the_admission_step(H, S, V, K):
    """The same logits and the same record in slot 0 from step 0 and in slot 4 from step 3, other live slots beside it: tokens and embedding
    rows are identical. Without the record (retired, then a plain admission) the same placements draw from (7, t, b * K + k), which differ
    between the slots as the model predicts."""
    seen = {}
    for rec in (True, False):
        for slot, at in ((0, 0), (4, 3)):
            rig = _rig(H, S, V, K)
            seen[rec, slot] = rig.play(GC.placement_events(V, K, slot, at, rec), f"placement V={V} K={K} slot {slot} record {rec}", watch=slot)
            assert len(seen[rec, slot]) == 1 + GC.PLACE_STEPS
            model_ids = rig.m.ids[slot * K:(slot + 1) * K, :2 + GC.PLACE_STEPS]
            assert np.array_equal(seen[rec, slot][-1][0].numpy(), model_ids)
            assert (slot in rig.session.own) == rec
    for (ids_a, h_a), (ids_b, h_b) in zip(seen[True, 0], seen[True, 4]):
        assert torch.equal(ids_a, ids_b) and torch.equal(h_a, h_b)
    # the session's draw stream sees the slot: the model's own prediction differs between slot 0 and slot 4, and the device matched it above
    assert not torch.equal(seen[False, 0][-1][0], seen[False, 4][-1][0])
    log_parity(f"placement NV={SM.nv_of(V)} V={V} K={K}: record (seed A) in slot 0 @ step 0 == slot 4 @ step 3 over {1 + GC.PLACE_STEPS} launches (ids and h "
               f"bitwise); cleared record: session draws differ between the slots as predicted", LOG)
