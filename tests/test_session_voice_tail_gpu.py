"""The session tail with per-slot voice-prompt lengths, called directly (tests/native/session_voice_harness.hip -> tail_launch with the
seventh argument -> tail_kernel<NV, true>; the id columns, the lengths and the clock written by the product's kernels a voice admission
runs) against the host restatement (tests/session_voice_model.py::VoiceTailModel, itself checked against ``sample_loop(decoder_input_ids=)``
in tests/test_session_voice_cpu.py), on the three NV instances.

Slots have T in {0, 3} and their own max_length (with and without a delay pattern), are admitted at different steps, and a slot is reused by
a request of the other kind. After EVERY launch the whole state - ids, cur_len, unfinished, has_eos, first_unf, row_maxlen, the prefix
lengths and the embedding h of the next column - must equal the model's bit for bit, the guards around them must survive, every launch runs
twice from the same state with bitwise equal results (Rig of tests/test_sampler_tail_gpu.py), and embed_kernel<float, true> with the same
lengths must reproduce h."""
import numpy as np
import pytest
import torch

import sampler_cases as SC
import sampler_model as SM
import session_voice_harness as SV
import session_voice_model as VM
import tail_harness as TH
from helpers import log_parity
from test_sampler_tail_gpu import DEV, FILL, SENT32, Guarded, Rig, _stream

pytestmark = pytest.mark.gpu

LOG = "session_voice_tail.txt"
SLOTS, HIDDEN, P, SESSION_L, T = 4, 32, 2, 24, 3
SHAPES = [(64, 4), (1088, 9), (2048, 9)]  # the three NV instances
HOT = SC.SESSION_HOT


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return TH.Harness(TH.build(str(tmp_path_factory.mktemp("tail_harness"))))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    return SV.Harness(SV.build(str(tmp_path_factory.mktemp("session_voice_harness"))))


class VoiceRig(Rig):
    def __init__(self, H, S, model, gp):
        self.S, self.gp = S, gp
        super().__init__(H, model, gp, 0, hidden=HIDDEN, prefix=model.prefix, dims_max_length=3)
        self.slot_T = Guarded((model.B,), torch.int32)
        self.slot_T.t.zero_()
        self.guarded.append(self.slot_T)

    def assert_equals_model(self, what):
        super().assert_equals_model(what)
        assert np.array_equal(self.slot_T.t.cpu().numpy(), self.m.slot_T), (what, "prefix lengths")

    def admit(self, b, L, prefix, what):
        m, a = self.m, self.args()
        n = 0 if prefix is None else prefix.shape[1]
        if n:
            self.prefix[b * m.K:(b + 1) * m.K, :n] = torch.from_numpy(prefix).to(DEV)

        def launch():
            assert self.H.reset_rows(a, self.row_maxlen.data_ptr(), b, 1, 1, L, _stream()) == TH.PTTS_OK, self.H.error()
            assert self.S.set_prefix(a, self.prefix.data_ptr(), m.ld, self.slot_T.ptr(), b, n, L, _stream()) == TH.PTTS_OK, self.S.error()

        self.twice(launch)
        m.admit(b, L, prefix)
        self.assert_equals_model(what)

    def retire(self, b, what):
        a = self.args()

        def launch():
            assert self.H.reset_rows(a, self.row_maxlen.data_ptr(), b, 1, 0, SESSION_L, _stream()) == TH.PTTS_OK, self.H.error()
            assert self.S.set_prefix(a, None, 0, self.slot_T.ptr(), b, 0, SESSION_L, _stream()) == TH.PTTS_OK, self.S.error()

        self.twice(launch)
        self.m.retire(b, SESSION_L)
        self.assert_equals_model(what)

    def tail(self, lg, what, grid=None, row0=0, slots=None):
        m = self.m
        self.logits.copy_(torch.from_numpy(lg))
        kept = self.logits.clone()
        a = self.args(grid, row0)

        def launch():
            assert self.S.tail(a, None, self.slot_T.ptr(), _stream()) == TH.PTTS_OK, self.S.error()

        self.twice(launch)
        assert torch.equal(self.logits.view(torch.int32), kept.view(torch.int32)), f"{what}: the logits changed"
        live = m.step(lg, self.gp, slots=slots, tables=self.tables_host, pos_table=self.pos_host, h=self.model_h)
        self.assert_equals_model(what)
        # the manual path's embedding of the column just written, under the same per-slot lengths
        self.h2.buf.fill_(SENT32)
        assert self.S.embed(self.args(h=self.h2), self.slot_T.ptr(), _stream()) == TH.PTTS_OK, self.S.error()
        x, y = self.h.t.view(torch.int32).cpu(), self.h2.t.view(torch.int32).cpu()
        for s in live:
            assert torch.equal(x[s], y[s]), (what, "embed_kernel<float, true>", s)
        assert self.h2.guards_intact()
        return live


def _logits(V, K, step, eos):
    rng = np.random.default_rng(1000 * V + 10 * K + step)
    lg = (2.0 * rng.standard_normal((SLOTS, K, V))).astype(np.float32)
    for b in range(SLOTS):
        if (step + b) % 5 == 4:
            lg[b, :, eos] += HOT  # EOS wins wherever min_new_tokens and the gate allow it
    return lg


@pytest.mark.parametrize("V,K", SHAPES)
def test_slots_with_and_without_a_prefix_in_one_launch(H, S, V, K):
    eos, pad, bos = SC.ids_of(V)
    gp = SC.Gen(max_length=SESSION_L, min_new_tokens=2)
    m = VM.VoiceTailModel(SLOTS, K, V, eos, pad, bos, ld=SESSION_L + 3, P=P, fill=FILL)
    rig = VoiceRig(H, S, m, gp)
    rng = np.random.default_rng(V + K)
    pre = lambda: rng.integers(0, V - 8, size=(K, T)).astype(np.int64)
    short = 2 * K - 3  # below 2K - 1: no pattern, the prefix un-shifted; >= T + 2
    assert short >= T + 2 and SESSION_L >= T + K
    launches, seen_T = 0, set()
    # what session begin leaves: every slot idle with BOS in column 0, the session's max_length and no prefix. The model starts with ids the
    # device never holds (FILL) and embed_kernel<float, true> looks up the table row of EVERY slot's last column, idle ones included
    for b in range(SLOTS):
        rig.retire(b, f"V={V} K={K}: session begin, slot {b}")

    def admit(b, L, prefix, step):
        rig.admit(b, L, prefix, f"V={V} K={K} step {step}: admit slot {b}")
        live = rig.tail(_logits(V, K, 100 + step, eos), f"V={V} K={K} step {step}: first token of slot {b}", grid=1, row0=b, slots=[b])
        assert live == [b] and m.cur_len[b] == 2 + (0 if prefix is None else T)

    for step in range(22):
        if step == 0:
            admit(0, SESSION_L, pre(), step)      # a pattern behind the prefix
        if step == 2:
            admit(1, 19, None, step)
        if step == 3:
            admit(2, short, pre(), step)          # no pattern: raw prefix columns
        if step == 9:                             # a request without a prompt behind a voice request in slot 2 (finished, or cancelled here) ...
            rig.retire(2, f"V={V} K={K} step {step}: retire slot 2")
            admit(2, 19, None, step)
        if step == 11:                            # ... and a voice request behind a cancelled plain one in slot 1
            rig.retire(1, f"V={V} K={K} step {step}: retire slot 1")
            admit(1, SESSION_L, pre(), step)
        live = rig.tail(_logits(V, K, step, eos), f"V={V} K={K} step {step}")
        launches += 1
        seen_T |= {int(m.slot_T[b]) for b in live}
        assert 3 not in live
    assert m.cur_len[3] == 1 and seen_T == {0, T}
    assert m.slot_T.tolist() == [T, T, 0, 0]
    log_parity(f"session tail with per-slot prefix lengths NV={SM.nv_of(V)} V={V} K={K}: state, lengths and h bit-exact after {launches} step launches and "
               f"5 admissions, embed_kernel<float, true> reproduces h", LOG)
