"""GPU: ``ptts_score`` (include/ptts_score.h) at the engine level - one teacher-forced forward over raw decoder columns ending in the fused final
LayerNorm + LM heads + cross-entropy kernel - against ``DecoderOracle.forward`` (logits at all positions) and the float64 cross-entropy of
tests/score_model.py, the state the call leaves behind, and its refusals.

Bounds. Log-sum-exp is 1-Lipschitz in the sup norm and the label logit moves by at most the logit band, so with the project's logit bands
(tests/test_lm_gpu.py: fp32 engine 2e-5, bf16 engine against ``precision="bf16"`` 1e-2):
  fp32: |d nll| <= 2 * 2e-5 + score_model.kernel_bound (the kernel's own fp32 log-sum-exp, derived there);   logits within 2e-5
  bf16: |d nll| <= 2 * 1e-2;                                                                                logits within 1e-2
The largest differences observed on MI355X are recorded in profiles/score_forward.txt."""
import pytest
import torch

import cases as C
import score_model as SM
from helpers import log_parity, make_engine
from oracle import decoder_oracle as DO

pytestmark = pytest.mark.gpu

VARIANTS = {
    "sinusoidal": {},
    "rope": {"rope_embeddings": True},
    "grouped_query": {"rope_embeddings": True, "num_key_value_heads": 1, "num_cross_attention_key_value_heads": 1},
}


def make_case(spec, B, N, P, T, seed):
    """Ragged description / prompt masks; columns that start with BOS, one input EOS; labels = the next column, -100 tails of different lengths,
    one label equal to BOS, ids up to V - 1."""
    g = torch.Generator().manual_seed(seed)
    K, V = spec.num_codebooks, spec.vocab_size
    enc = torch.randn(B, N, spec.hidden_size, generator=g)
    prompt = torch.randn(B, P, spec.hidden_size, generator=g) * 0.5
    enc_mask, prompt_mask = C.ragged_masks(B, N, P)
    enc_mask[-1, N - 2:] = 0
    prompt_mask[-1, :1] = 0
    enc = enc * enc_mask[..., None]
    ids = torch.randint(0, 1024, (B * K, T), generator=g)
    ids[:, 0] = spec.bos_token_id
    labels = torch.randint(0, V, (B, T, K), generator=g)
    labels[:, :-1] = ids.view(B, K, T)[:, :, 1:].transpose(1, 2)
    for b in range(B):
        for k in range(K):
            tail = (b * 3 + k) % min(T, 7)
            if tail:
                labels[b, T - tail:, k] = -100
    if T > 4:
        ids[1, 3] = spec.eos_token_id       # input EOS: (b 0, codebook 1, t 3) does not count
        labels[0, 2, 1] = spec.eos_token_id  # "one single EOS at the end": a label EOS counts
        labels[0, 1, 2] = spec.bos_token_id  # label BOS does not count
        labels[0, 0, 0] = 0
        labels[0, 1, 0] = V - 1
    return enc, enc_mask, prompt, prompt_mask, ids, labels


def oracle_logits(spec, sd, case, precision="fp32"):
    enc, enc_mask, prompt, prompt_mask, ids, _ = case
    return DO.DecoderOracle(spec, sd, precision=precision).forward(ids, enc, enc_mask, prompt, prompt_mask)


def check_against_oracle(eng, spec, sd, case, bf16, tag):
    enc, enc_mask, prompt, prompt_mask, ids, labels = case
    V = spec.vocab_size
    ref = oracle_logits(spec, sd, case, "bf16" if bf16 else "fp32")
    cm = SM.counted_mask(ids, labels, spec.bos_token_id, spec.eos_token_id, V)
    ref_nll, _, _ = SM.token_nll(ref, labels, cm)
    nll, counted, logits = eng.score(enc, enc_mask, prompt, prompt_mask, ids, labels, return_logits=True)
    nll0, counted0, none = eng.score(enc, enc_mask, prompt, prompt_mask, ids, labels)
    assert none is None
    nll, counted, logits, nll0, counted0 = nll.cpu(), counted.cpu(), logits.cpu(), nll0.cpu(), counted0.cpu()
    assert torch.equal(counted.bool(), cm) and torch.equal(counted0, counted)
    assert torch.equal(nll0, nll), "the no-store path computes the same bits"
    assert bool((nll[~cm] == 0).all())
    own_nll, lse, picked = SM.token_nll(logits, labels, cm)
    d_own = (nll.double() - own_nll).abs()
    # rows of padded prompt positions are left out: such a query sees no key at all, where the engine's attention yields 0 and the reference's
    # additive mask a softmax over nothing but masked keys - padding either way, which no later row attends to
    P, K = (prompt.shape[1] if prompt is not None else 0), spec.num_codebooks
    real = torch.ones(logits.shape[:2], dtype=torch.bool)
    if prompt_mask is not None:
        real[:, :P] = prompt_mask.bool().repeat_interleave(K, 0)
    d_log = float((logits - ref)[real].abs().max())
    d_nll = float((nll.double() - ref_nll).abs().max())
    log_parity(f"{tag}: max |d logits| {d_log:.3e}  max |d nll| vs oracle {d_nll:.3e}  max |d nll| vs float64 of own logits {float(d_own.max()):.3e}",
               name="score_forward.txt")
    assert bool((d_own <= SM.kernel_bound(lse, picked, V)).all())
    if bf16:
        assert d_log <= 1e-2 and d_nll <= 2 * 1e-2
    else:
        assert d_log <= 2e-5
        assert bool(((nll.double() - ref_nll).abs() <= 2 * 2e-5 + SM.kernel_bound(lse, picked, V)).all())


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_engine_score_against_oracle(variant, bf16):
    spec = DO.DecoderSpec(**{**DO.TINY.__dict__, **VARIANTS[variant]})
    sd = DO.make_decoder_weights(spec, seed=31)
    case = make_case(spec, B=2, N=7, P=3, T=37, seed=7)
    eng = make_engine(spec, sd, dtype=torch.bfloat16 if bf16 else torch.float32, max_batch=2, max_ctx=64, max_enc=8, max_prompt=40)
    check_against_oracle(eng, spec, sd, case, bf16, f"TINY {variant} {'bf16' if bf16 else 'fp32'} B=2 N=7 P=3 T=37")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_engine_score_150_columns_cross_key_blocks_and_row_tiles(bf16):
    spec = DO.TINY
    sd = DO.make_decoder_weights(spec, seed=32)
    case = make_case(spec, B=2, N=7, P=3, T=150, seed=8)
    eng = make_engine(spec, sd, dtype=torch.bfloat16 if bf16 else torch.float32, max_batch=2, max_ctx=160, max_enc=8, max_prompt=153)
    check_against_oracle(eng, spec, sd, case, bf16, f"TINY sinusoidal {'bf16' if bf16 else 'fp32'} B=2 N=7 P=3 T=150")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_engine_score_mini_width_nine_utterances(bf16):
    spec = DO.DecoderSpec(num_hidden_layers=2, max_position_embeddings=64)
    sd = DO.make_decoder_weights(spec, seed=33)
    case = make_case(spec, B=9, N=7, P=3, T=6, seed=9)
    eng = make_engine(spec, sd, dtype=torch.bfloat16 if bf16 else torch.float32, max_batch=9, max_ctx=32, max_enc=8, max_prompt=9)
    check_against_oracle(eng, spec, sd, case, bf16, f"Mini-v1 width 2 layers {'bf16' if bf16 else 'fp32'} B=9 N=7 P=3 T=6")


def test_logits_only_and_no_prompt():
    spec = DO.TINY
    sd = DO.make_decoder_weights(spec, seed=34)
    enc, enc_mask, _, _, ids, labels = make_case(spec, B=2, N=7, P=3, T=19, seed=10)
    eng = make_engine(spec, sd, max_batch=2, max_ctx=32, max_enc=8, max_prompt=20)
    nll, counted, logits = eng.score(enc, enc_mask, None, None, ids, None, return_logits=True)
    assert nll is None and counted is None and tuple(logits.shape) == (18, 19, spec.vocab_size)
    ref = DO.DecoderOracle(spec, sd).forward(ids, enc, enc_mask, None, None)
    assert float((logits.cpu() - ref).abs().max()) <= 2e-5
    with pytest.raises(ValueError):
        eng.score(enc, enc_mask, None, None, ids, None, return_logits=False)
    bad = labels.clone()
    bad[1, 0, 0] = spec.vocab_size  # a counted label that is no class
    with pytest.raises(ValueError):
        eng.score(enc, enc_mask, None, None, ids, bad)


def test_state_after_score_and_refusals():
    spec, sd, enc, enc_mask, prompt, prompt_mask, gp = C.batch_case(3)
    ref = DO.sample_loop(DO.DecoderOracle(spec, sd), enc, enc_mask, prompt, prompt_mask, gp)
    assert ref.min_margin >= C.MARGIN
    g = torch.Generator().manual_seed(3)
    T = 11
    ids = torch.randint(0, 1024, (3 * spec.num_codebooks, T), generator=g)
    labels = torch.randint(0, 1024, (3, T, spec.num_codebooks), generator=g)

    fresh = make_engine(spec, sd, max_batch=3, max_prompt=16)
    fresh.set_gen_params(max_length=gp.max_length, min_new_tokens=gp.min_new_tokens)
    want = fresh.generate_ids(enc, enc_mask, prompt, prompt_mask).cpu()
    assert torch.equal(want, ref.sequences)
    nodes = fresh.graph_nodes()

    eng = make_engine(spec, sd, max_batch=3, max_prompt=16)
    eng.set_gen_params(max_length=gp.max_length, min_new_tokens=gp.min_new_tokens)
    nll, _, _ = eng.score(enc, enc_mask, prompt, prompt_mask, ids, labels)
    with pytest.raises(ValueError):  # the engine counts as never prefilled
        eng.decode_steps(1)
    assert torch.equal(eng.generate_ids(enc, enc_mask, prompt, prompt_mask).cpu(), want) and eng.graph_nodes() == nodes
    nll2, _, _ = eng.score(enc, enc_mask, prompt, prompt_mask, ids, labels)  # and after a generation
    assert torch.equal(nll2, nll)

    # above capacity: P + T rows, batch
    with pytest.raises(ValueError):
        eng.score(enc, enc_mask, prompt, prompt_mask, torch.zeros(27, 13, dtype=torch.long), None, return_logits=True)  # 4 + 13 > max_prompt 16
    with pytest.raises(ValueError):
        eng.score(torch.cat([enc, enc[:1]]), None, None, None, torch.zeros(36, 4, dtype=torch.long), None, return_logits=True)
    # a pending voice prompt
    eng.set_audio_prefix(torch.randint(0, 1024, (27, 3), generator=g))
    with pytest.raises(NotImplementedError):
        eng.score(enc, enc_mask, prompt, prompt_mask, ids, labels)
    eng.set_audio_prefix(None)
    assert torch.equal(eng.generate_ids(enc, enc_mask, prompt, prompt_mask).cpu(), want)

    # inside a live session: refused, and the session goes on unharmed
    ses, ctl = make_engine(spec, sd, max_batch=3, max_prompt=16), make_engine(spec, sd, max_batch=3, max_prompt=16)
    for e in (ses, ctl):
        e.set_gen_params(max_length=gp.max_length, min_new_tokens=gp.min_new_tokens)
        e.begin_session(3, enc.shape[1], prompt.shape[1])
        e.admit_row(1, enc[1], enc_mask[1], prompt[1], prompt_mask[1])
        e.decode_steps(4)
    with pytest.raises(ValueError):
        ses.score(enc, enc_mask, prompt, prompt_mask, ids, labels)
    for e in (ses, ctl):
        e.decode_steps(gp.max_length - 5)
    assert torch.equal(ses.row_ids(1, gp.max_length), ctl.row_ids(1, gp.max_length))
    ses.retire_row(1)
    nll3, _, _ = ses.score(enc, enc_mask, prompt, prompt_mask, ids, labels)  # every slot idle: allowed, ends the session
    assert torch.equal(nll3, nll)


def test_kv_fp8_engine_refuses_and_keeps_generating():
    spec = DO.DecoderSpec(num_hidden_layers=2, max_position_embeddings=64)  # the e4m3 cache exists on the wide bf16 engine above 8 utterances
    sd = DO.make_decoder_weights(spec, seed=35)
    g = torch.Generator().manual_seed(12)
    enc, prompt = torch.randn(9, 7, spec.hidden_size, generator=g), torch.randn(9, 3, spec.hidden_size, generator=g) * 0.5
    eng = make_engine(spec, sd, dtype=torch.bfloat16, max_batch=12, max_ctx=32, max_enc=8, max_prompt=9, kv_fp8=True)
    eng.set_gen_params(max_length=8, min_new_tokens=7)
    before = eng.generate_ids(enc, None, prompt, None).cpu()
    with pytest.raises(NotImplementedError):
        eng.score(enc, None, prompt, None, torch.zeros(9 * spec.num_codebooks, 5, dtype=torch.long), None, return_logits=True)
    assert torch.equal(eng.generate_ids(enc, None, prompt, None).cpu(), before)
