"""CPU: the host restatement of the logit-edit node (tests/logit_edit_model.py) against the installed transformers' SequenceBiasLogitsProcessor,
NoBadWordsLogitsProcessor, ExponentialDecayLengthPenalty, SuppressTokensLogitsProcessor and SuppressTokensAtBeginLogitsProcessor, as
``generation_extras.build_processors`` chains them, bit for bit (int32 views; NaN positions included), on the cases the GPU test of the kernel
runs (tests/test_logit_edit_kernel_gpu.py)."""
import numpy as np
import pytest

import logit_edit_model as LM

CASES = LM.cases()


def _same_bits(got, want):
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(np.where(gn, np.float32(0), got).view(np.int32), np.where(wn, np.float32(0), want).view(np.int32))


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    assert len({c.name for c in CASES}) == len(CASES)
    assert {(c.V, c.K, c.B) for c in CASES} >= {(V, K, 3) for V in (33, 1088, 2048) for K in (1, 9)}
    for c in CASES:
        assert {1 + T for T in c.t_prefix} == {1, 6}  # given of 1 and of 1 + 5
        eos_col = c.logits[:, :, c.eos]
        assert np.isfinite(eos_col).all()  # no +-inf EOS logit enters the decay: the excluded case
        rest = np.delete(c.logits, c.eos, axis=2)
        assert np.isneginf(rest).any() and (np.signbit(rest) & (rest == 0)).any()  # -inf and -0.0 at tokens that are not EOS
        for b, rec in enumerate(c.records):
            g = 1 + c.t_prefix[b]
            ts = {cl[b] for cl in c.clocks}
            assert ts >= {g - 1, g, g + 1, g + 2}
            if rec.exponential_decay_length_penalty is not None:
                s = rec.exponential_decay_length_penalty[0]
                assert ts >= {s + g + d for d in (-1, 0, 1, 2, 3)} and s + g + LM.LATE in ts
    big = [c for c in CASES if c.B == 3]
    assert all(c.records[1].neutral and all(v is not None for v in c.records[0]) for c in big)
    assert any([c.eos] in (r.bad_words_ids or []) for c in CASES for r in c.records)                    # a bad word equal to [eos]
    assert any(any(v >= c.V for v in (r.suppress_tokens or [])) for c in CASES for r in c.records)      # a suppress token at or above V
    singles = [r for c in CASES if c.B == 2 for r in c.records]
    for name in LM.Record._fields:  # each option alone
        assert any(getattr(r, name) is not None and sum(v is not None for v in r) == 1 for r in singles), name
    assert any(r.exponential_decay_length_penalty == (2, 1.01) for c in CASES for r in c.records)       # the late clock at factor 1.01


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_model_equals_transformers_chain(case):
    for cur_len in case.clocks:
        got, want = LM.apply(case, cur_len), LM.transformers_apply(case, cur_len)
        assert got.dtype == np.float32 and _same_bits(got, want), (case.name, cur_len, np.argwhere(got.view(np.int32) != want.view(np.int32))[:3])
        for b, rec in enumerate(case.records):
            if rec.neutral:
                assert np.array_equal(got[b].view(np.int32), case.logits[b].view(np.int32))
    changed = [not np.array_equal(LM.apply(case, cl).view(np.int32), case.logits.view(np.int32)) for cl in case.clocks]
    inert = all(r.neutral or (r.suppress_tokens is not None and min(r.suppress_tokens) >= case.V) for r in case.records)  # nothing inside the vocabulary
    assert any(changed) != inert


def test_whole_row_adds_turn_minus_zero_into_plus_zero_and_selects_keep_it():
    c = next(c for c in CASES if c.name.startswith("alone0"))  # sequence_bias alone
    out = LM.apply(c, c.clocks[1])
    neg0 = np.signbit(c.logits) & (c.logits == 0)
    assert neg0.any() and not (np.signbit(out) & (out == 0))[neg0].any()
    c = next(c for c in CASES if c.name.startswith("alone5"))  # suppress_tokens alone
    out = LM.apply(c, c.clocks[1])
    keep = np.ones(c.V, bool)
    keep[[1, 2]] = False
    assert np.array_equal(out[:, :, keep].view(np.int32), c.logits[:, :, keep].view(np.int32)) and np.isneginf(out[:, :, [1, 2]]).all()


def test_the_decay_is_two_roundings_not_a_fused_multiply_add():
    """On random values the correctly rounded fused form differs from torch in a good share of them; the model's two-step form in none."""
    rng = np.random.default_rng(5)
    l = (rng.standard_normal(20000) * 4).astype(np.float32)
    m = LM.decay_m(1.07, 9)
    two = l + np.abs(l) * m
    fused = (l.astype(np.float64) + np.abs(l).astype(np.float64) * np.float64(m)).astype(np.float32)  # exact product, one rounding
    import torch

    t = torch.from_numpy(l)
    want = (t + torch.abs(t) * (pow(1.07, 9) - 1)).numpy()
    assert np.array_equal(two.view(np.int32), want.view(np.int32))
    assert (fused.view(np.int32) != want.view(np.int32)).mean() > 0.05


def test_why_the_decay_inside_the_min_new_tokens_block_is_excluded():
    """transformers runs MinNewTokensLength in front of the decay: the -inf it writes at EOS becomes |-inf| * m + -inf = NaN. The device tail blocks
    EOS behind the node instead, so a request with min_new_tokens > start + 1 is not eligible (it keeps the host loop)."""
    c = next(c for c in CASES if c.name.startswith("alone3"))  # decay (3, 1.08) alone
    g = [1 + T for T in c.t_prefix]
    cur_len = [x + 3 + 2 for x in g]  # idx = 2: the decay is active, 5 new tokens so far
    blocked = LM.transformers_apply(c, cur_len, min_new_tokens=8)  # 8 > start + 1: EOS still blocked
    assert np.isnan(blocked[:, :, c.eos]).all()
    free = LM.transformers_apply(c, cur_len, min_new_tokens=4)     # 4 <= start + 1: never both
    assert _same_bits(free, LM.apply(c, cur_len)) and np.isfinite(free[:, :, c.eos]).all()
