"""GPU, fp32 engine: scoring ties to generation. A greedy ``generate_ids`` run, then ``score`` on the ids the model SAW - the raw ids under the
delay pattern (``apply_delay_pattern_mask``), all columns but the last - with logits for all positions: at EVERY generated position and EVERY
codebook row the arg-max of the scoring logits is the id generation chose. It is the one place where the raw-column embedding and the
all-position heads meet the generation path (delayed_token embedding, last-row heads, sampler tail).

The cases are cases.batch_case(3) and cases.gqa_case(3): seeds scanned on the CPU oracle (tools/scan_margin_seeds.py) for a top-2 margin of at
least cases.MARGIN = 1e-4 at every step - asserted below on the oracle - against <= 4e-6 of fp32 engine-vs-oracle logit noise. They generate under
``min_new_tokens = max_length - 1``: no row finishes before the last column (every row is unfinished at every position: none is left out) and
the EOS column is barred throughout, so the arg-max is taken over the other columns, as the sampler tail did."""
import pytest
import torch

import cases as C
from helpers import make_engine
from oracle import decoder_oracle as DO

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["batch", "gqa"])
def test_argmax_of_scoring_logits_is_what_greedy_generation_chose(case):
    spec, sd, enc, enc_mask, prompt, prompt_mask, gp = C.batch_case(3) if case == "batch" else C.gqa_case(3)
    assert gp.min_new_tokens == gp.max_length - 1
    ref = DO.sample_loop(DO.DecoderOracle(spec, sd), enc, enc_mask, prompt, prompt_mask, gp)
    assert ref.min_margin >= C.MARGIN, f"top-2 margin {ref.min_margin:.1e} below {C.MARGIN}"
    K, L, P = spec.num_codebooks, gp.max_length, prompt.shape[1]
    eng = make_engine(spec, sd, max_batch=3, max_ctx=64, max_enc=32, max_prompt=P + L)
    eng.set_gen_params(max_length=L, min_new_tokens=gp.min_new_tokens)
    ids = eng.generate_ids(enc, enc_mask, prompt, prompt_mask).cpu()
    assert torch.equal(ids, ref.sequences) and ids.shape == (3 * K, L)
    _, pattern = DO.build_delay_pattern_mask(ids[:, :1], spec.bos_token_id, spec.pad_token_id, L, K)
    seen = DO.apply_delay_pattern_mask(ids, pattern)[:, : L - 1]  # column j is the input of the step that chose column j + 1
    _, _, logits = eng.score(enc, enc_mask, prompt, prompt_mask, seen, None, return_logits=True)
    lg = logits.cpu()[:, P:]
    assert lg.shape == (3 * K, L - 1, spec.vocab_size)
    lg[:, :, spec.eos_token_id] = -float("inf")
    assert torch.equal(lg.argmax(-1), ids[:, 1:])
    # and generation after the scoring pass is the same run
    assert torch.equal(eng.generate_ids(enc, enc_mask, prompt, prompt_mask).cpu(), ids)


def test_argmax_tie_where_a_row_finishes_early():
    """cases.voice_lm_case(100) without its voice prompt (scanned margin 4.1e-4, asserted): the EOS logit is amplified, ``min_new_tokens = 6``,
    and codebook row 0 reaches EOS at column 10 of 36 while the EOS gate holds the other rows back. The generation's processors are replayed over
    the scoring logits - EOS barred for the first ``min_new_tokens`` steps, then the EOS gate on the ids so far - and at every position every row
    that was unfinished there chose the arg-max; a finished row holds the pad id."""
    spec, sd, enc, prompt, _, gp = C.voice_lm_case(100)
    ref = DO.sample_loop(DO.DecoderOracle(spec, sd), enc, None, prompt, None, gp)
    assert ref.min_margin >= C.MARGIN, f"top-2 margin {ref.min_margin:.1e} below {C.MARGIN}"
    K, P, eos = spec.num_codebooks, prompt.shape[1], spec.eos_token_id
    eng = make_engine(spec, sd, max_batch=1, max_ctx=64, max_enc=32, max_prompt=P + gp.max_length)
    eng.set_gen_params(max_length=gp.max_length, min_new_tokens=gp.min_new_tokens)
    ids = eng.generate_ids(enc, None, prompt, None).cpu()
    assert torch.equal(ids, ref.sequences)
    L = ids.shape[1]
    _, pattern = DO.build_delay_pattern_mask(ids[:, :1], spec.bos_token_id, spec.pad_token_id, gp.max_length, K)
    seen = DO.apply_delay_pattern_mask(ids, pattern)[:, : L - 1]
    lg = eng.score(enc, None, prompt, None, seen, None, return_logits=True)[2].cpu()[:, P:]
    gate, unfinished, finished_early = DO.EosGate(eos, K, 1), torch.ones(K, dtype=torch.bool), 0
    for j in range(L - 1):  # the step that chose column j + 1 from the columns up to j
        scores = lg[:, j].clone()
        if j < gp.min_new_tokens:
            scores[:, eos] = -float("inf")
        scores = gate(ids[:, : j + 1], scores)
        assert torch.equal(scores.argmax(-1)[unfinished], ids[unfinished, j + 1]), j
        assert bool((ids[~unfinished, j + 1] == spec.pad_token_id).all()), j
        unfinished = unfinished & ~((ids[:, j + 1] == eos) | (j + 2 >= gp.max_length))
        finished_early = max(finished_early, int((~unfinished).sum()) if j + 2 < gp.max_length else 0)
    assert finished_early >= 1, "no row finished before the last column: the case does not exercise the clause"
