"""CPU: the restatement of the sampler tail (tests/sampler_model.py) is itself right - its kept set against transformers' own warpers,
its state machine against oracle.decoder_oracle.sample_loop, its uniform against a KS bound - and the inputs of the GPU file
(tests/sampler_cases.py) keep the share of draws excluded as ambiguous under the cap, measured on the reference alone."""
import math

import numpy as np
import pytest
import torch

import sampler_cases as SC
import sampler_model as SM
from oracle import decoder_oracle as DO

F32 = np.float32


# ---- warpers against transformers ------------------------------------------------------------------------------------------------
def _hf_kept(row, T, top_k, top_p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    s = torch.from_numpy(row)[None].clone()
    if T != 1.0:
        s = TemperatureLogitsWarper(T)(None, s)
    if top_k:
        s = TopKLogitsWarper(top_k)(None, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p)(None, s)
    return torch.isfinite(s[0]).numpy()


GRID = [(0.7, 0, 1.0), (3.0, 0, 1.0), (1.0, 1, 1.0), (1.0, 7, 1.0), (1.0, 50, 1.0), (1.0, 10 ** 6, 1.0), (1.0, 0, 0.1), (1.0, 0, 0.9),
        (1.0, 0, 0.999), (0.7, 50, 0.9), (1.3, 20, 0.5), (0.05, 0, 0.9)]


@pytest.mark.parametrize("V", [64, 1088, 2048])
def test_kept_set_equals_transformers_warpers(V):
    eos = V - 8
    rng = np.random.default_rng(V)
    compared = ambiguous = 0
    for T, top_k, top_p in GRID:
        gp = SC.Gen(max_length=8, do_sample=True, temperature=T, top_k=min(top_k, 10 ** 6), top_p=top_p)
        for i in range(12):
            row = (rng.standard_normal(V) * 2).astype(F32)
            if i % 3 == 1:
                row[rng.random(V) < 0.3] = -np.inf
            blocked = i % 2 == 1
            ks = SM.kept_set(row, gp, blocked, eos)
            if ks.ambiguous:
                ambiguous += 1
                continue
            ref = row.copy()
            if blocked:
                ref[eos] = -np.inf  # the processors run before the warpers
            want = _hf_kept(ref, T, min(top_k, V) if top_k else 0, top_p)
            assert np.array_equal(ks.mask, want), (V, T, top_k, top_p, i, np.nonzero(ks.mask != want)[0])
            assert blocked is False or not ks.mask[eos]
            compared += 1
    print(f"V={V}: {compared} rows compared, {ambiguous} ambiguous")
    assert compared >= 0.75 * 12 * len(GRID), (compared, ambiguous)  # the comparison must not be hollowed out by exclusions


def test_tie_at_the_kth_value_keeps_every_tied_entry_as_transformers_does():
    V = 128
    row = np.linspace(-3, 0, V).astype(F32)
    row[[5, 70, 71, 100]] = [2.0, 1.0, 1.0, 1.0]  # top_k = 2: the 2nd value is a tie of 3
    gp = SC.Gen(max_length=8, do_sample=True, top_k=2)
    ks = SM.kept_set(row, gp, False, V - 8)
    assert sorted(np.nonzero(ks.mask)[0]) == [5, 70, 71, 100]
    assert np.array_equal(ks.mask, _hf_kept(row, 1.0, 2, 1.0))


def test_tie_at_the_top_p_boundary_keeps_every_tied_entry_where_transformers_keeps_some():
    V = 64
    mass = np.full(V, 0.2 / (V - 4))
    mass[[3, 10, 11, 40]] = [0.5, 0.1, 0.1, 0.1]  # top_p = 0.65: mass 0.5 above the tie, 0.8 below it
    row = np.log(mass).astype(F32)
    gp = SC.Gen(max_length=8, do_sample=True, top_p=0.65)
    ks = SM.kept_set(row, gp, False, V - 8)
    assert not ks.ambiguous
    assert sorted(np.nonzero(ks.mask)[0]) == [3, 10, 11, 40]  # the contract: all of the tie
    hf = _hf_kept(row, 1.0, 0, 0.65)
    assert hf[3] and not (hf & ~ks.mask).any()  # transformers keeps a subset ...
    assert set(np.nonzero(ks.mask & ~hf)[0]) <= {10, 11, 40}  # ... that differs by tied entries only
    assert 1 <= hf[[10, 11, 40]].sum() <= 3


def test_draw_walks_lane_major_and_falls_back_to_the_last_kept_entry():
    V = 192
    w = np.zeros(V)
    w[[130, 2, 66, 1]] = [1.0, 1.0, 1.0, 1.0]  # draw order: 1, 65.., 129.. | 2, 66, 130
    kept = w > 0
    assert list(SM.draw_order(V)[:4]) == [0, 64, 128, 1]
    assert SM.draw(kept, w, F32(0.1)) == 1
    assert SM.draw(kept, w, F32(0.3)) == 2
    assert SM.draw(kept, w, F32(0.6)) == 66
    assert SM.draw(kept, w, F32(0.9)) == 130
    assert SM.draw(kept, w, F32(1.0)) == 130  # u == 1.0f: the last boundary, reached or not
    assert SM.draw(kept, w, F32(2.0 ** -25)) == 1
    assert SM.draw(kept, w, F32(0.5)) is None  # on a boundary: ambiguous
    assert SM.accept_set(w, F32(0.5), V) == {2, 66}


# ---- the uniform ----------------------------------------------------------------------------------------------------------------
def test_draw_u_is_uniform_over_a_seed_column_row_grid():
    seed, t, row = np.meshgrid(np.arange(10, dtype=np.uint64) * np.uint64(0x123456789) + np.uint64(7), np.arange(1, 101, dtype=np.uint64),
                               np.arange(100, dtype=np.uint64), indexing="ij")
    u = np.sort(SM.draw_u(seed.ravel(), t.ravel(), row.ravel()).astype(np.float64))
    n = u.size
    assert n == 100_000
    i = np.arange(1, n + 1)
    ks = max((i / n - u).max(), (u - (i - 1) / n).max())
    assert ks < 1.63 / math.sqrt(n), ks  # the 1 % point of the Kolmogorov distribution
    assert u.min() >= 2.0 ** -25 and u.max() <= 1.0


def find_special_seeds(t=SC.SPECIAL_T, row=SC.SPECIAL_ROW, chunk=1 << 22, limit=1 << 32):
    """The one-off search behind SC.SEED_U_ONE / SC.SEED_U_MIN: the smallest seeds whose hash at (t, row) has its top 24 bits all ones / all
    zeros (about 2^24 candidates each). Not run by the suite; the test below asserts the two properties of the committed constants."""
    inner = SM.splitmix64((np.uint64(t) << np.uint64(32)) ^ np.uint64(row))[0]
    one = low = None
    for s0 in range(0, limit, chunk):
        seeds = np.arange(s0, s0 + chunk, dtype=np.uint64)
        top = SM.splitmix64(seeds ^ inner) >> np.uint64(40)
        if one is None and (top == 0xFFFFFF).any():
            one = int(seeds[np.argmax(top == 0xFFFFFF)])
        if low is None and (top == 0).any():
            low = int(seeds[np.argmax(top == 0)])
        if one is not None and low is not None:
            return one, low
    raise AssertionError("not found")


def test_special_seeds_give_u_one_and_the_smallest_u():
    assert SM.draw_u(SC.SEED_U_ONE, SC.SPECIAL_T, SC.SPECIAL_ROW) == F32(1.0)  # "(0, 1)" is (0, 1]: the top 24 bits all ones round up
    assert SM.draw_u(SC.SEED_U_MIN, SC.SPECIAL_T, SC.SPECIAL_ROW) == F32(2.0 ** -25)
    assert int(SM.draw_hash(SC.SEED_U_MIN, SC.SPECIAL_T, SC.SPECIAL_ROW)[0] >> np.uint64(40)) == 0


# ---- TailModel against the restated _sample loop ----------------------------------------------------------------------------------
class ScriptedModel:
    """Duck-typed stand-in for DecoderOracle in sample_loop: forward() returns the scripted logits of the step, whatever it is fed."""

    def __init__(self, spec, script):
        self.spec, self.script, self.step = spec, script, 0

    def reset(self):
        self.step = 0

    def forward(self, ids, *a, **kw):
        lg = torch.from_numpy(self.script(self.step)).reshape(-1, self.spec.vocab_size)
        self.step += 1
        return lg[:, None, :].expand(-1, ids.shape[-1], -1)


def _model_sequences(V, K, B, gp, script, pad, prefix=None):
    eos, _, bos = SC.ids_of(V)
    m = SM.TailModel(B, K, V, eos, pad, bos, ld=gp.max_length + 2, prefix=prefix, max_length=gp.max_length)
    s = 0
    while m.step(script(s), gp):
        s += 1
        assert s <= gp.max_length
    assert not m.step(script(s), gp)  # the no-op step changes nothing
    L = int(m.cur_len[0])
    assert (m.cur_len == L).all()
    return m.ids[:, :L], m


@pytest.mark.parametrize("V,K,B,max_length,min_new,pad_is_eos,T_prefix", [
    (64, 4, 3, 11, 2, True, 0), (64, 4, 3, 11, 2, False, 0), (512, 9, 2, 21, 2, True, 0), (16, 1, 1, 5, 2, True, 0),
    (64, 4, 2, 5, 0, True, 0),      # max_length < 2K - 1: no pattern
    (528, 10, 2, 30, 6, False, 3),  # voice prompt: MinNewTokens counts from 1 + T_prefix
])
def test_greedy_tail_model_equals_sample_loop(V, K, B, max_length, min_new, pad_is_eos, T_prefix):
    eos, _, bos = SC.ids_of(V)
    pad = eos if pad_is_eos else V - 7
    spec = DO.DecoderSpec(num_codebooks=K, vocab_size=V, pad_token_id=pad, eos_token_id=eos, bos_token_id=bos)
    gp = DO.GenParams(max_length=max_length, min_new_tokens=min_new)
    script = lambda s: SC.greedy_logits(V, K, B, s, eos)  # noqa: E731
    prefix = torch.randint(0, V - 16, (B * K, T_prefix), generator=torch.Generator().manual_seed(1)) if T_prefix else None
    ref = DO.sample_loop(ScriptedModel(spec, script), torch.zeros(B, 1, 8), None, None, None, gp, decoder_input_ids=prefix)
    seq, m = _model_sequences(V, K, B, gp, script, pad, prefix=None if prefix is None else prefix.numpy())
    assert np.array_equal(seq, ref.sequences.numpy()), (seq, ref.sequences)
    assert (ref.sequences == eos).any()
    if B > 1 and max_length >= 2 * K - 1:
        stamps = -m.unfinished.reshape(B, K)
        assert len(set(stamps.max(axis=1))) > 1, "rows should finish at different steps"


# ---- the exclusion cap, on the reference alone -----------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", SC.SAMPLED_SHAPES)
def test_ambiguous_share_of_every_gpu_configuration_is_under_the_cap(V, K):
    eos, pad, bos = SC.ids_of(V)
    B = SC.sampled_batch(K)
    for name, T, top_k, top_p in SC.sampled_configs(V):
        gp = SC.Gen(max_length=SC.SAMPLED_STEPS + 2, min_new_tokens=SC.SAMPLED_STEPS + 2, do_sample=True, temperature=T, top_k=top_k, top_p=top_p)
        lg = SC.sampled_logits(V, K, B, gp, eos)
        m = SM.TailModel(B, K, V, eos, pad, bos, ld=gp.max_length + 1, max_length=gp.max_length)
        for _ in range(SC.SAMPLED_STEPS):
            m.step(lg, gp, seed=1234, choose=lambda row, acc: min(acc))
        assert m.stats["draws"] >= 500, (name, m.stats)
        share = m.stats["ambiguous"] / m.stats["draws"]
        print(f"V={V} K={K} {name}: {m.stats['draws']} draws, ambiguous {100 * share:.2f} %")
        assert share <= SC.AMBIGUOUS_CAP, (name, m.stats)


@pytest.mark.parametrize("V,K,B", SC.GATE_SHAPES)
def test_ambiguous_share_of_the_gpu_gate_cases_is_under_the_cap(V, K, B):
    eos, pad, bos = SC.ids_of(V)
    gp = SC.gate_gen(K)
    m = SM.TailModel(B, K, V, eos, pad, bos, ld=gp.max_length + 3, max_length=gp.max_length)
    for s in range(SC.gate_steps(K)):
        m.step(SC.gate_logits(V, K, B, s, gp, eos), gp, seed=99, choose=lambda row, acc: min(acc))
    print(f"gate V={V} K={K}: {m.stats}")
    assert m.stats["draws"] > 0 and m.stats["ambiguous"] / m.stats["draws"] <= SC.AMBIGUOUS_CAP, m.stats


@pytest.mark.parametrize("V,K,B", [c[:3] for c in SC.SESSION_CASES if c[3]])
def test_ambiguous_share_of_the_gpu_session_cases_is_under_the_cap(V, K, B):
    eos, pad, bos = SC.ids_of(V)
    gp = SC.session_gen(True)
    m = SM.TailModel(B, K, V, eos, pad, bos, ld=SC.session_steps(K) + 8, session=True, P=2)
    for ev in SC.session_events(V, K, B, True):
        if ev[0] == "reset":
            m.reset_row(*ev[1:])
        else:
            m.step(ev[2], gp, slots=[ev[1]] if ev[0] == "admit" else None, seed=7, choose=lambda row, acc: min(acc))
    print(f"session V={V} K={K} slots={B}: {m.stats}")
    assert m.stats["draws"] > 0 and m.stats["ambiguous"] / m.stats["draws"] <= SC.AMBIGUOUS_CAP, m.stats


def test_signed_zeros_tie_at_the_kth_value_the_contract_is_the_float_comparison():
    """The contract is transformers': `scores < kth` removes, and -0.0 < +0.0 is false, so a -0.0 tied with +0.0 at the k-th value stays.
    kept_set states that side. (The kernel's radix keys order the bit patterns and put -0.0 below +0.0: a known deviation)"""
    V = 64
    row = np.linspace(-3, -1, V).astype(F32)
    row[[4, 9, 30]] = [2.0, 0.0, -0.0]
    assert np.signbit(row[30]) and not np.signbit(row[9])
    gp = SC.Gen(max_length=8, do_sample=True, top_k=2)
    ks = SM.kept_set(row, gp, False, V - 8)
    assert sorted(np.nonzero(ks.mask)[0]) == [4, 9, 30]
    assert np.array_equal(ks.mask, _hf_kept(row, 1.0, 2, 1.0))
