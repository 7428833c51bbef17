"""The logit-edit node called directly (tests/native/logit_edit_harness.hip -> logit_edit_launch -> logit_edit_kernel) against its host model
(tests/logit_edit_model.py, pinned against transformers' processors on the CPU by tests/test_logit_edit_model_cpu.py): equality of the bits,
no tolerance. V in {33, 1088, 2048}, K in {1, 9}, 3 utterances under three different records, one of them neutral, at the clocks around the
given columns and around each decay's start, and a late one.

The logits sit between sentinel guards that must survive; the clocks and the records must be untouched; an utterance under the neutral record
is compared with an untouched copy."""
import ctypes as C

import numpy as np
import pytest
import torch

import logit_edit_harness as LH
import logit_edit_model as LM

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT32 = 0x7FBADBAD
LD_T = 1024  # entries of a decay table: more than the late clock's idx
CASES = LM.cases()


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return LH.Harness(LH.build(str(tmp_path_factory.mktemp("logit_edit_harness"))))


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Rig:
    def __init__(self, H, c, pad=4096, extra_records=0):
        self.H, self.c, self.pad = H, c, pad
        n = c.B * c.K * c.V
        self.buf = torch.full((pad + n + pad,), SENT32, dtype=torch.int32, device=DEV)
        self.logits = self.buf[pad:pad + n].view(torch.float32).view(c.B, c.K, c.V)
        self.src = torch.from_numpy(c.logits).to(DEV)
        hdr, bias, decay, flags, self.ld_v = LM.pack(c, LD_T, extra_records)
        self.host = (hdr, bias, decay, flags)
        self.hdr, self.bias, self.decay, self.flags = (torch.from_numpy(x).to(DEV) for x in self.host)
        self.t_prefix = torch.tensor(c.t_prefix, dtype=torch.int32, device=DEV)
        self.cur_len = torch.zeros(c.B, dtype=torch.int32, device=DEV)

    def args(self, row0, nb, stride=1):
        c = self.c
        return LH.LhArgs(self.logits.data_ptr(), self.cur_len.data_ptr(), self.t_prefix.data_ptr(), self.hdr.data_ptr(), self.bias.data_ptr(),
                         self.decay.data_ptr(), self.flags.data_ptr(), self.ld_v, LD_T, stride, c.B, c.K, c.V, c.eos, row0, nb)

    def run(self, cur_len, row0=0, nb=None, stride=1):
        """Fresh logits, one launch; returns the logits as numpy."""
        self.logits.copy_(self.src)
        self.cur_len.copy_(torch.tensor(cur_len, dtype=torch.int32))
        assert self.H.logit_edit(self.args(row0, self.c.B if nb is None else nb, stride), _stream()) == LH.PTTS_OK, self.H.error()
        torch.cuda.synchronize()
        assert self.cur_len.tolist() == list(cur_len)
        return self.logits.cpu().numpy()

    def intact(self):
        n = self.c.B * self.c.K * self.c.V
        guards = bool((self.buf[:self.pad] == SENT32).all()) and bool((self.buf[self.pad + n:] == SENT32).all())
        recs = all(np.array_equal(d.cpu().numpy(), h) for d, h in zip((self.hdr, self.bias, self.decay, self.flags), self.host))
        return guards and recs and self.t_prefix.tolist() == self.c.t_prefix


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _diff(got, want, what):
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} logits differ, first (b, k, v) = {bad[0].tolist()}: " \
                              f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_kernel_equals_the_host_model_at_every_clock(H, case):
    rig = Rig(H, case)
    for cur_len in case.clocks:
        got = rig.run(cur_len)
        _diff(got, LM.apply(case, cur_len), f"{case.name} at clocks {cur_len}")
        for b, rec in enumerate(case.records):
            if rec.neutral:
                _diff(got[b], case.logits[b], "the neutral record must leave the row's bits alone")
    assert rig.intact()


@pytest.mark.parametrize("name", ["V1088_K9_B3", "V33_K1_B3"])
def test_sub_ranges_touch_their_utterances_only(H, name):
    """grid (K, nb) with row0: (slot, 1) is what an admission launches."""
    case = next(c for c in CASES if c.name == name)
    rig = Rig(H, case)
    cur_len = case.clocks[6]  # every decay active
    want = LM.apply(case, cur_len)
    for row0, nb in ((0, 1), (2, 1), (1, 2), (0, 2)):
        got = rig.run(cur_len, row0, nb)
        for b in range(case.B):
            _diff(got[b], want[b] if row0 <= b < row0 + nb else case.logits[b], f"utterance {b} of launch ({row0}, {nb})")
    assert rig.intact()


def test_one_prefix_length_for_the_whole_batch(H):
    """stride 0: the static call's single T_prefix; every utterance counts from the same given columns."""
    case = next(c for c in CASES if c.name == "V33_K9_B3")
    rig = Rig(H, case)
    rig.t_prefix[0] = 5
    same = case._replace(t_prefix=[5, 5, 5])
    for j in (1, 6):
        cur_len = [case.clocks[j][1]] * 3
        _diff(rig.run(cur_len, stride=0), LM.apply(same, cur_len), f"clocks {cur_len}")


def test_copying_the_default_record_restores_a_slot(H):
    """copy_logit_edit_kernel: what session begin, ptts_retire_row and a NULL slot record launch."""
    case = next(c for c in CASES if c.name == "V1088_K1_B3")
    rig = Rig(H, case, extra_records=1)  # record 3: zeroed, the neutral default
    cur_len = case.clocks[6]
    assert H.copy_records(rig.args(0, 3), 3, 0, 1, _stream()) == LH.PTTS_OK, H.error()   # slot 0 <- neutral
    assert H.copy_records(rig.args(0, 3), 2, 1, 1, _stream()) == LH.PTTS_OK, H.error()   # slot 1 <- record 2
    got = rig.run(cur_len)
    moved = case._replace(records=[LM.Record(), case.records[2], case.records[2]], t_prefix=case.t_prefix)
    _diff(got, LM.apply(moved, cur_len), "records after the copies")
    assert np.array_equal(rig.hdr.cpu().numpy()[2], rig.host[0][2]) and np.array_equal(rig.decay.cpu().numpy()[1], rig.host[2][2])


def test_launch_helper_refuses_what_the_kernel_does_not_serve(H):
    case = CASES[0]
    rig = Rig(H, case)
    rig.logits.copy_(rig.src)
    a = rig.args(0, case.B)
    a.V = H.max_vocab + 1  # 2049: refused without a launch
    assert H.max_vocab == 2048 and H.logit_edit(a, _stream()) == LH.PTTS_E_UNSUPPORTED
    a = rig.args(0, case.B)
    a.V = rig.ld_v + 4  # wider than a record's rows
    assert H.logit_edit(a, _stream()) == LH.PTTS_E_UNSUPPORTED
    a = rig.args(1, case.B)
    assert H.logit_edit(a, _stream()) == LH.PTTS_E_INVALID
    torch.cuda.synchronize()
    _diff(rig.logits.cpu().numpy(), case.logits, "refused launches")
    assert rig.intact()
