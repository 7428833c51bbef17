"""CPU: the host restatement of the history-penalty node (tests/penalty_model.py) against the installed transformers'
RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor, bit for bit, on the cases the GPU test of the kernel runs
(tests/test_history_penalty_kernel_gpu.py). The model forms its products and quotients in float64 and rounds once, so the equality also shows
that the oracle's float32 multiply and divide on the CPU are the correctly rounded IEEE operations the kernel is written to."""
import pytest
import torch

import penalty_model as PM

CASES = PM.cases()


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    names = {c.name for c in CASES}
    assert len(names) == len(CASES)
    assert {(c.V, c.K, c.B) for c in CASES} >= {(V, K, B) for V in (40, 1088, 2048) for K in (1, 9) for B in (1, 3)}
    assert any(1 in c.cur_len and 2611 in c.cur_len for c in CASES)
    assert {n for c in CASES for _, n in c.records} >= {0, 1, 2, 3, 5}
    assert all(c.ld > max(c.cur_len) for c in CASES)
    assert any(c.B > 1 and c.records[1] == (1.0, 0) for c in CASES)
    for c in CASES:  # the sentinel behind every history is a token no history holds
        for b in range(c.B):
            rows = c.ids[b * c.K:(b + 1) * c.K]
            assert bool((rows[:, c.cur_len[b]:] == PM.SENTINEL).all()) and not bool((rows[:, : c.cur_len[b]] == PM.SENTINEL).any()), c.name


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_model_equals_transformers_processors(case):
    want = PM.transformers_apply(case.logits, case.ids, case.cur_len, case.records)
    got = PM.apply(case.logits, case.ids, case.cur_len, case.records)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), case.name  # bits: -0.0 and +0.0 differ
    for b, (p, n) in enumerate(case.records):
        if p == 1.0 and n == 0:
            assert torch.equal(got[b].view(torch.int32), case.logits[b].view(torch.int32))


def test_reading_the_sentinel_column_would_change_the_result():
    """The guard columns are live: a history one column longer gives another output in every case with an active record."""
    c = next(c for c in CASES if c.name == "V1088_K9_B1")
    longer = PM.apply(c.logits, c.ids, [t + 1 for t in c.cur_len], c.records)
    assert not torch.equal(longer, PM.apply(c.logits, c.ids, c.cur_len, c.records))


def test_duplicates_do_not_compound():
    c = next(c for c in CASES if c.name == "constant50")
    out = PM.apply(c.logits, c.ids, c.cur_len, c.records)
    assert torch.equal(out[0, :, 5], c.logits[0, :, 5] / torch.tensor(1.4))
    assert torch.equal(out[0, :, :5], c.logits[0, :, :5]) and torch.equal(out[0, :, 6:], c.logits[0, :, 6:])
