"""The history-penalty node called directly (tests/native/penalty_harness.hip -> penalty_launch -> history_penalty_kernel) against the installed
transformers' RepetitionPenaltyLogitsProcessor + NoRepeatNGramLogitsProcessor applied on the CPU to the same logits and ids: torch.equal on
the bits, no tolerance. Cases: tests/penalty_model.py (pinned against the same oracle on the CPU by tests/test_penalty_model_cpu.py).

The logits sit between sentinel guards that must survive; the ids and cur_len must be untouched; columns at and past cur_len hold a token that
would change the result if it were read; an utterance under the neutral record keeps the bits of its logits."""
import ctypes as C

import pytest
import torch

import penalty_harness as PH
import penalty_model as PM

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT32 = 0x7FBADBAD
CASES = PM.cases()


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return PH.Harness(PH.build(str(tmp_path_factory.mktemp("penalty_harness"))))


@pytest.fixture(scope="module")
def oracle():
    """transformers' result of every case, computed once on the CPU."""
    return {c.name: PM.transformers_apply(c.logits, c.ids, c.cur_len, c.records) for c in CASES}


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Rig:
    def __init__(self, H, c, pad=4096):
        self.H, self.c, self.pad = H, c, pad
        n = c.B * c.K * c.V
        self.buf = torch.full((pad + n + pad,), SENT32, dtype=torch.int32, device=DEV)
        self.logits = self.buf[pad:pad + n].view(torch.float32).view(c.B, c.K, c.V)
        self.logits.copy_(c.logits)
        self.ids = c.ids.to(DEV).contiguous()
        self.cur_len = torch.tensor(c.cur_len, dtype=torch.int32, device=DEV)
        self.pen = torch.zeros(c.B * C.sizeof(PH.HistoryPenalty), dtype=torch.uint8, device=DEV)
        for b, (p, n_) in enumerate(c.records):
            assert H.set_records(self.pen.data_ptr(), b, 1, p, n_, _stream()) == PH.PTTS_OK, H.error()

    def args(self, row0, nb):
        c = self.c
        return PH.PhArgs(self.logits.data_ptr(), self.ids.data_ptr(), self.cur_len.data_ptr(), self.pen.data_ptr(), c.ld, c.B, c.K, c.V, row0, nb)

    def guards_intact(self):
        n = self.c.B * self.c.K * self.c.V
        return bool((self.buf[:self.pad] == SENT32).all()) and bool((self.buf[self.pad + n:] == SENT32).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_kernel_equals_transformers_processors(H, oracle, case):
    rig = Rig(H, case)
    assert H.penalty(rig.args(0, case.B), _stream()) == PH.PTTS_OK, H.error()
    torch.cuda.synchronize()
    got, want = rig.logits.cpu(), oracle[case.name]
    assert rig.guards_intact()
    assert torch.equal(rig.ids.cpu(), case.ids) and rig.cur_len.tolist() == case.cur_len
    bad = (_bits(got) != _bits(want)).nonzero()
    assert bad.numel() == 0, f"{case.name}: {bad.shape[0]} logits differ, first (b, k, v) = {bad[0].tolist()}: " \
                             f"{got[tuple(bad[0])].item()!r} != {want[tuple(bad[0])].item()!r}"
    for b, (p, n) in enumerate(case.records):
        if p == 1.0 and n == 0:
            assert torch.equal(_bits(got[b]), _bits(case.logits[b])), "the neutral record must leave the row's bits alone"


def test_one_slot_launch_touches_that_slot_only(H, oracle):
    """grid (K, 1) with row0 = the slot: what finish_admission launches."""
    case = next(c for c in CASES if c.name == "V1088_K9_B3")
    rig = Rig(H, case)
    assert H.penalty(rig.args(2, 1), _stream()) == PH.PTTS_OK, H.error()
    torch.cuda.synchronize()
    got = rig.logits.cpu()
    assert torch.equal(_bits(got[2]), _bits(oracle[case.name][2])) and torch.equal(_bits(got[:2]), _bits(case.logits[:2]))
    assert rig.guards_intact()


def test_launch_helper_refuses_what_the_kernel_does_not_serve(H):
    case = CASES[0]
    rig = Rig(H, case)
    a = rig.args(0, case.B)
    a.V = H.max_vocab + 1
    assert H.penalty(a, _stream()) == PH.PTTS_E_UNSUPPORTED
    a = rig.args(1, case.B)
    assert H.penalty(a, _stream()) == PH.PTTS_E_INVALID
    torch.cuda.synchronize()
    assert torch.equal(_bits(rig.logits.cpu()), _bits(case.logits))
