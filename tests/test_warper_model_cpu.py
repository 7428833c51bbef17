"""CPU: the host model of the four warper stages (tests/warper_model.py) against transformers' own chain, as
``generation_extras.build_processors`` assembles it: the kept sets are equal on every row the model does not call ambiguous, the random rows
are ambiguous in at most 1 % of the cases, and every crafted row is ambiguous exactly where it says."""
import numpy as np
import pytest
import torch
from transformers import GenerationConfig

import sampler_model as SM
import warper_cases as WC
import warper_model as WM
from parler_tts_amd.generation_extras import build_processors

F32 = np.float32
V = 1088
ROWS = 80  # per configuration


def hf_kept(row, wp, T, top_k, top_p):
    """The entries transformers' warpers leave finite: temperature -> top-k -> top-p -> MinP -> Typical -> Epsilon -> Eta."""
    gc = GenerationConfig(do_sample=True, temperature=T, top_k=top_k or None, top_p=top_p,
                          min_p=wp.min_p if wp.min_p > 0 else None, typical_p=wp.typical_p,
                          epsilon_cutoff=wp.epsilon_cutoff, eta_cutoff=wp.eta_cutoff)
    procs = build_processors(gc, 1, None, [], "cpu", 0)
    names = [type(p).__name__ for p in procs]
    want = [n for n, on in (("MinPLogitsWarper", wp.min_p > 0), ("TypicalLogitsWarper", wp.typical_p < 1), ("EpsilonLogitsWarper", wp.epsilon_cutoff > 0),
                            ("EtaLogitsWarper", wp.eta_cutoff > 0)) if on]
    assert [n for n in names if n in ("MinPLogitsWarper", "TypicalLogitsWarper", "EpsilonLogitsWarper", "EtaLogitsWarper")] == want, names
    s = procs(None, torch.from_numpy(row)[None].clone())
    return torch.isfinite(s[0]).numpy()


def _compare(row, wp, T, top_k, top_p, blocked, eos):
    ks = WM.warp_kept(row, WC.gen(T, top_k, top_p), wp, blocked, eos)
    ref = row.copy()
    if blocked:
        ref[eos] = -np.inf  # the processors run before the warpers
    return ks, hf_kept(ref, wp, T, min(top_k, row.shape[0]), top_p)


def test_kept_sets_equal_transformers_chain_on_random_rows():
    """Every configuration of warper_cases.CONFIGS (each warper alone, all four, top-k / top-p in front, temperature != 1), every second row
    with EOS blocked, every fourth with -inf entries. The 1 % cap holds over the random rows of the file (typical_p alone on a flat 1088-entry
    row is the costliest case: its boundary falls between cumulative masses about 1e-3 apart, against a band of 3e-6 and the order band)."""
    eos = V - 8
    total = 0
    for cfg, (name, wp, T, top_k, top_p) in enumerate(WC.CONFIGS):
        ambiguous = 0
        for i, row in enumerate(WC.random_rows(V, ROWS, cfg)):
            blocked = i % 2 == 1
            ks, want = _compare(row, wp, T, top_k, top_p, blocked, eos)
            top = int(np.argmax(np.where(np.arange(V) == eos, -np.inf, row) if blocked else row))
            assert ks.mask.any() and (ks.mask[top] or wp.typical_p < 1)  # typical_p may drop the arg-max (it keeps what is near the entropy)
            assert not blocked or not ks.mask[eos]
            if ks.ambiguous:
                ambiguous += 1
                continue
            assert np.array_equal(ks.mask, want), (name, i, np.nonzero(ks.mask != want)[0])
        print(f"{name}: {ROWS} rows, {ambiguous} ambiguous")
        total += ambiguous
    assert total <= 0.01 * ROWS * len(WC.CONFIGS), total


def test_at_most_one_percent_of_the_random_rows_is_ambiguous_at_the_stated_values():
    """V = 1088, logits N(0, sigma^2) with sigma in {1.5, 3, 5}, all four warpers at (0.05, 0.9, 3e-4, 2e-3)."""
    rng = np.random.default_rng(2024)
    n, ambiguous = 600, 0
    gp = WC.gen()
    for i in range(n):
        row = (rng.standard_normal(V) * WC.SIGMAS[i % 3]).astype(F32)
        ks = WM.warp_kept(row, gp, WC.ALL, False, V - 8)
        ambiguous += ks.ambiguous
        if not ks.ambiguous and i % 4 == 0:
            assert np.array_equal(ks.mask, hf_kept(row, WC.ALL, 1.0, 0, 1.0)), i
    print(f"{ambiguous} of {n} rows ambiguous")
    assert ambiguous <= 0.01 * n, ambiguous


@pytest.mark.parametrize("Vc", [300, 1088, 2048])
def test_crafted_rows_are_ambiguous_where_they_say_and_equal_transformers_elsewhere(Vc):
    eos = Vc - 8
    for name, row, wp, (T, top_k, top_p), expect in WC.crafted(Vc):
        ks, want = _compare(row, wp, T, top_k, top_p, False, eos)
        if expect is not None:
            assert ks.ambiguous == expect, (name, ks.ambiguous)
        if not ks.ambiguous:
            assert np.array_equal(ks.mask, want), (name, np.nonzero(ks.mask != want)[0])
        else:  # the doubtful groups dropped / kept bracket transformers' answer
            lo = np.logical_and.reduce([w > 0 for w in ks.variants])
            hi = np.logical_or.reduce([w > 0 for w in ks.variants])
            assert not (lo & ~want).any() and not (want & ~hi).any(), name


def test_what_the_crafted_rows_keep():
    rows = {c[0]: c for c in WC.crafted(1088)}
    kept = lambda name: WM.warp_kept(rows[name][1], WC.gen(*rows[name][3]), rows[name][2], False, 1080)  # noqa: E731
    assert sorted(np.nonzero(kept("only the arg-max survives").mask)[0]) == [17]
    assert sorted(np.nonzero(kept("near one-hot").mask)[0]) == [64]
    assert kept("uniform: every s equal, typical_p keeps all").mask.all()
    assert sorted(np.nonzero(kept("typical_p boundary inside a tie").mask)[0]) == [9, 40, 41, 42]
    assert kept("epsilon = p at the maximum").mask.sum() == 256
    ks = kept("typical_p drops the arg-max, epsilon spares the rest")
    assert not ks.mask[33] and ks.mask.sum() == 1087
    ks = kept("min_p = 1 keeps the tied maxima only")
    assert ks.mask[[5, 130]].all() and all((w > 0)[[5, 130]].all() and (w > 0).sum() <= 3 for w in ks.variants)
    ks = kept("min_p tie at the threshold")
    assert {tuple(np.nonzero(w > 0)[0]) for w in ks.variants} == {(3,), (3, 70, 71, 200)}  # all of the tie goes one way


def test_a_neutral_record_is_the_plain_kept_set_and_the_cache_serves_tail_model():
    row = WC.random_rows(V, 1, 99)[0]
    gp = WC.gen(0.8, 40, 0.9)
    a, b = SM.kept_set(row, gp, True, V - 8), WM.warp_kept(row, gp, WM.NEUTRAL, True, V - 8)
    assert np.array_equal(a.mask, b.mask) and np.array_equal(a.weights, b.weights) and a.ambiguous == b.ambiguous
    # step_with_records: utterance 1 under min_p = 1 draws its arg-max whatever the seed, utterance 0 (neutral) draws what TailModel draws
    K, B = 2, 2
    lg = WC.random_rows(V, B * K, 5).reshape(B, K, V)
    plain = SM.TailModel(B, K, V, V - 8, V - 8, V, ld=8, max_length=8)
    warped = SM.TailModel(B, K, V, V - 8, V - 8, V, ld=8, max_length=8)
    g = WC.gen(max_length=8, min_new_tokens=8)
    pick = lambda row, acc: min(acc)  # noqa: E731
    for _ in range(4):
        plain.step(lg, g, seed=11, choose=pick)
        assert WM.step_with_records(warped, lg, g, [WM.NEUTRAL, WM.Warp(min_p=1.0)], seed=11, choose=pick) == [0, 1]
    assert np.array_equal(warped.ids[:K], plain.ids[:K])
    masked = lg[1].copy()
    masked[:, V - 8] = -np.inf
    assert (warped.ids[K:, 1:5] == masked.argmax(-1)[:, None]).all()
