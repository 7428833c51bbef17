"""CPU: the host model of one recorded row (tests/step_record_model.py) against transformers' own processors in their order -
MinNewTokensLengthLogitsProcessor, ParlerTTSLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, then MinP, Typical,
Epsilon, Eta - on the row kinds of sampler_cases.ROW_KINDS: bit for bit outside the entries the model calls doubtful and outside an exact tie at
the top-p boundary (the device keeps all of the tie, transformers' sort some of it: the exception tests/test_sampler_model_cpu.py makes). And,
on the model alone, the inputs of the GPU file keep the share of rows with any doubtful entry at or below sampler_cases.AMBIGUOUS_CAP."""
import numpy as np
import pytest
import torch

import parler_tts_amd as P
import sampler_cases as SC
import step_record_cases as RC
import step_record_model as RM
import warper_cases as WC
import warper_model as WM

F32 = np.float32
K = 5  # one row of every kind


def _hf_scores(rows, gp, wp, min_new, eos):
    """[K][V] -> what transformers appends to `scores` at the first generated column (input_ids = the BOS column)."""
    from transformers.generation.logits_process import (EpsilonLogitsWarper, EtaLogitsWarper, LogitsProcessorList, MinNewTokensLengthLogitsProcessor,
                                                         MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper,
                                                         TypicalLogitsWarper)

    V = rows.shape[1]
    procs = LogitsProcessorList()
    if min_new > 0:
        procs.append(MinNewTokensLengthLogitsProcessor(1, min_new, eos, device="cpu"))
    procs.append(P.ParlerTTSLogitsProcessor(eos, rows.shape[0], 1, "cpu"))
    if gp.do_sample:
        if gp.temperature != 1.0:
            procs.append(TemperatureLogitsWarper(gp.temperature))
        if gp.top_k:
            procs.append(TopKLogitsWarper(min(gp.top_k, V)))
        if gp.top_p < 1.0:
            procs.append(TopPLogitsWarper(gp.top_p))
        if wp.min_p > 0:
            procs.append(MinPLogitsWarper(wp.min_p))
        if wp.typical_p < 1:
            procs.append(TypicalLogitsWarper(wp.typical_p))
        if wp.epsilon_cutoff > 0:
            procs.append(EpsilonLogitsWarper(wp.epsilon_cutoff))
        if wp.eta_cutoff > 0:
            procs.append(EtaLogitsWarper(wp.eta_cutoff, device="cpu"))
    ids = torch.full((rows.shape[0], 1), V, dtype=torch.long)
    return procs(ids, torch.from_numpy(rows).clone()).numpy()


def _rows(V, top_p, seed):
    return np.stack([SC._row(kind, V, top_p, np.random.default_rng([seed, V, i])) for i, kind in enumerate(SC.ROW_KINDS)])


def _check(rows, gp, wp, min_new, eos, what):
    want = _hf_scores(rows, gp, wp, min_new, eos)
    doubtful = 0
    for k in range(rows.shape[0]):
        blocked = min_new > 0 or k > 0  # the first generated column: first_unf = 0, the gate blocks every codebook above it
        assert want[k, eos] == -np.inf if blocked else True
        got, maybe = RM.recorded_row(rows[k], gp, wp, blocked, eos)
        doubtful += bool(maybe.any())
        diff = got.view(np.uint32) != want[k].view(np.uint32)
        allowed = maybe.copy()
        if gp.do_sample and gp.top_p < 1.0 and np.isfinite(got).any():  # an exact tie at the top-p boundary: the lowest kept value, more than once
            low = got[np.isfinite(got)].min()
            if (got == low).sum() > 1:
                allowed |= got == low
        assert not (diff & ~allowed).any(), (what, k, SC.ROW_KINDS[k % 5], np.nonzero(diff & ~allowed)[0][:8])
    return doubtful


@pytest.mark.parametrize("V", [64, 1088, 2048])
def test_recorded_rows_equal_transformers_chain_without_warpers(V):
    eos = SC.ids_of(V)[0]
    doubtful = rows_n = 0
    for name, gp in RC.plain_cases(V):
        for min_new in (0, 3):
            rows = _rows(V, gp.top_p, 11)
            doubtful += _check(rows, gp, WM.NEUTRAL, min_new, eos, f"V={V} {name} min_new={min_new}")
            rows_n += K
    print(f"V={V}: {rows_n} rows, {doubtful} with a doubtful entry")
    assert doubtful <= 0.1 * rows_n  # the comparison must not be hollowed out (these rows are not screened as the GPU inputs are)


@pytest.mark.parametrize("V", [1088, 300])
def test_recorded_rows_equal_transformers_chain_with_warpers(V):
    eos = SC.ids_of(V)[0]
    doubtful = rows_n = 0
    for i, (name, wp, T, top_k, top_p) in enumerate(WC.CONFIGS):
        gp = SC.Gen(max_length=8, do_sample=True, temperature=T, top_k=top_k, top_p=top_p)
        for min_new, rows in ((0, _rows(V, top_p, 20 + i)), (3, WC.random_rows(V, K, 60 + i))):
            doubtful += _check(rows, gp, wp, min_new, eos, f"V={V} {name} min_new={min_new}")
            rows_n += K
    print(f"V={V}: {rows_n} rows, {doubtful} with a doubtful entry")
    assert doubtful <= 0.1 * rows_n


def test_underflowed_entries_stay_finite_under_top_p_one_and_leave_with_any_stage():
    V, eos = 1088, 1080
    lg = RC.far_below_logits(V, 2, 1)[0]
    gp = SC.Gen(max_length=8, do_sample=True, temperature=1.0)
    for row in lg:
        far = row < row.max() - 105.0
        assert far.sum() >= V // 5
        got, maybe = RM.recorded_row(row, gp, WM.NEUTRAL, False, eos)
        assert np.isfinite(got).all() and not maybe.any() and RM.same_bits(got, row)
        want = _hf_scores(row[None], gp, WM.NEUTRAL, 0, eos)[0]
        assert RM.same_bits(got, want)
        for wp in (WM.Warp(min_p=0.05), WM.Warp(epsilon_cutoff=3e-4), WM.Warp(eta_cutoff=2e-3), WM.Warp(typical_p=0.9)):
            got, maybe = RM.recorded_row(row, gp, wp, False, eos)
            want = _hf_scores(row[None], gp, wp, 0, eos)[0]
            assert not np.isfinite(got[far]).any() and not np.isfinite(want[far]).any()
            assert not ((got.view(np.uint32) != want.view(np.uint32)) & ~maybe).any(), wp
        got, _ = RM.recorded_row(row, SC.Gen(max_length=8, do_sample=True, top_p=0.9), WM.NEUTRAL, False, eos)
        assert not np.isfinite(got[far]).any()


def test_greedy_rows_keep_their_bits_and_block_eos():
    V, eos = 64, 56
    row = np.random.default_rng(1).standard_normal(V).astype(F32)
    row[3] = -0.0
    gp = SC.Gen(max_length=8, do_sample=False, temperature=0.5, top_k=3, top_p=0.5)  # sampler settings are ignored by a greedy row
    got, maybe = RM.recorded_row(row, gp, WM.Warp(min_p=0.9), False, eos)
    assert RM.same_bits(got, row) and not maybe.any()
    got, _ = RM.recorded_row(row, gp, None, True, eos)
    assert got[eos] == -np.inf and RM.same_bits(np.delete(got, eos), np.delete(row, eos))


@pytest.mark.parametrize("V,Kc,B", RC.SHAPES)
def test_the_inputs_of_the_gpu_file_stay_under_the_ambiguous_cap(V, Kc, B):
    """Counted on the model alone, over every row of every case the GPU file runs, with EOS blocked and free: the GPU comparison excludes the
    doubtful entries of such rows and must not be able to hide a failure behind them."""
    eos = SC.ids_of(V)[0]
    rows_n = doubtful = 0
    cases = [(gp, [WM.NEUTRAL] * B, RC.plain_logits(V, Kc, B, gp)) for _, gp in RC.plain_cases(V)]
    cases += [(gp, recs, RC.warp_logits(V, Kc, B, i)) for i, (_, gp, recs) in enumerate(RC.warp_cases(V))]
    gp1 = SC.Gen(max_length=8, do_sample=True)
    cases.append((gp1, [WM.NEUTRAL] * B, RC.far_below_logits(V, Kc, B)))
    for wp in RC.FAR_BELOW_WARPS:
        cases.append((gp1, [wp] * B, RC.far_below_logits(V, Kc, B)))
    for warp in (False, True):  # the session test's sampled inputs (5 slots)
        gp, wps, lg = RC.session_case(V, Kc, 5, 12, True, warp)
        cases.append((gp, wps or [WM.NEUTRAL] * 5, lg))
    for gp, recs, lg in cases:
        for b in range(lg.shape[0]):
            for k in range(Kc):
                for blocked in (False, True):
                    _, maybe = RM.recorded_row(lg[b, k], gp, recs[b], blocked, eos)
                    rows_n += 1
                    doubtful += bool(maybe.any())
    print(f"V={V} K={Kc} B={B}: {rows_n} rows, {doubtful} with a doubtful entry ({100 * doubtful / rows_n:.2f} %)")
    assert doubtful / rows_n <= SC.AMBIGUOUS_CAP, (doubtful, rows_n)
