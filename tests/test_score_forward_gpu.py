"""GPU, end to end: ``ParlerTTSForConditionalGeneration.forward`` on the tiny model - native T5 description encoder, prompt embeddings, the HIP
decoder pass and its fused LM-heads + cross-entropy kernel - against tests/score_model.py on the oracle's logits for the same conditioning.
fp32 model: the loss is a mean (or sum) of per-token values that each sit within 2 * 2e-5 + the kernel's own bound of the oracle's
(tests/test_score_engine_gpu.py; score_model.kernel_bound = 1088 * 2^-24 = 6.5e-5 plus 12 ulps at |lse| <= 8, 1.2e-5): 1.2e-4 per position, so
a mean is held to TOL = 1.2e-4 and a sum to TOL per counted position."""
import pytest
import torch

import cases as C
import score_model as SM
from oracle import decoder_oracle as DO

pytestmark = pytest.mark.gpu

T = 21
TOL = 1.2e-4


def _inputs(spec, seed=3):
    g = torch.Generator().manual_seed(seed)
    K = spec.num_codebooks
    desc, desc_mask, prompt_ids, prompt_mask, _ = C.gen_eos_inputs(seed)
    labels = torch.randint(0, 1024, (2, T, K), generator=g)
    for b in range(2):
        for k in range(K):
            tail = (b + 2 * k) % 6
            if tail:
                labels[b, T - tail:, k] = -100
    labels[0, 4, 2] = spec.bos_token_id
    labels[1, 7, 5] = spec.eos_token_id
    return desc, desc_mask, prompt_ids, prompt_mask, labels


def _oracle_loss(m, spec, sd, out, cols, labels, prompt_ids, prompt_mask, enc_mask, red, weights=None, cross=False):
    enc = out.encoder_last_hidden_state.float().cpu()
    ph = m.embed_prompts(prompt_ids.cuda()).float().cpu()
    if cross:  # encoder_last_hidden_state is the joined context, as in the reference (:2806-2813): description states, then prompt + positions
        ph = ph + m.embed_positions.weights[: ph.shape[1]].float().cpu()[None]
        assert enc.shape[1] == enc_mask.shape[1] + ph.shape[1] and float((enc[:, enc_mask.shape[1]:] - ph).abs().max()) < 1e-6
        enc_mask, ph, prompt_mask = torch.cat([enc_mask, prompt_mask], 1), None, None
    logits = DO.DecoderOracle(spec, sd).forward(cols.cpu(), enc, enc_mask, ph, prompt_mask)
    return SM.loss_from_logits(logits, cols.cpu(), labels, spec.bos_token_id, spec.eos_token_id, red, weights), logits


@pytest.mark.parametrize("cross", [False, True], ids=["prompt_prepended", "prompt_cross_attention"])
def test_forward_loss_against_the_oracle(cross):
    m, spec, sd, _ = C.tiny_model(seed=5, eos_gain=6.0, prompt_cross_attention=cross)
    m = m.to("cuda")
    desc, desc_mask, prompt_ids, prompt_mask, labels = _inputs(spec)
    kw = dict(input_ids=desc.cuda(), attention_mask=desc_mask.cuda(), prompt_input_ids=prompt_ids.cuda(), prompt_attention_mask=prompt_mask.cuda(),
              labels=labels.cuda())
    cols = m.prepare_decoder_input_ids_from_labels(labels).reshape(2 * spec.num_codebooks, T)
    n_counted = int(SM.counted_mask(cols, labels, spec.bos_token_id, spec.eos_token_id).sum())
    weights = [3.0, 2.0, 1.0, 1.0, 1.0, 1.0, 0.5, 0.5, 0.25]
    for red, w in (("mean", None), ("sum", None), ("mean", weights)):
        m.config.decoder.codebook_weights = w
        out = m(**kw, loss_reduction=red)
        (loss, per), logits = _oracle_loss(m, spec, sd, out, cols, labels, prompt_ids, prompt_mask, desc_mask, red, w, cross)
        tol = TOL * (n_counted if red == "sum" else 1)
        print(f"forward {'cross' if cross else 'prepended'} {red} weights={w is not None}: loss {float(out.loss):.6f} oracle {float(loss):.6f}")
        assert abs(float(out.loss) - float(loss)) <= tol
        assert (torch.stack(out.per_codebook_losses).double().cpu() - per).abs().max() <= tol
        assert tuple(out.logits.shape) == tuple(logits.shape) and out.logits.dtype == torch.float32
        quiet = m(**kw, loss_reduction=red, output_logits=False)
        assert quiet.logits is None and torch.equal(quiet.loss, out.loss)
        assert all(torch.equal(a, b) for a, b in zip(quiet.per_codebook_losses, out.per_codebook_losses))
    # generation afterwards runs as on a fresh model
    m.config.decoder.codebook_weights = None
    gen_kw = dict(input_ids=desc.cuda(), attention_mask=desc_mask.cuda(), prompt_input_ids=prompt_ids.cuda(), prompt_attention_mask=prompt_mask.cuda(),
                  do_sample=False, max_new_tokens=12, min_new_tokens=4)
    after = m.generate(**gen_kw)
    fresh, *_ = C.tiny_model(seed=5, eos_gain=6.0, prompt_cross_attention=cross)
    assert torch.equal(after, fresh.to("cuda").generate(**gen_kw))


def test_input_values_alone_score_the_codes_of_the_models_codec():
    m, spec, sd, _ = C.tiny_model(seed=5)
    m = m.to("cuda")
    desc, prompt_ids, voice, _, _ = C.gen_voice_inputs(4)
    kw = dict(input_ids=desc.cuda(), prompt_input_ids=prompt_ids.cuda())
    a = m(**kw, input_values=voice.cuda())
    codes = m._voice_prompt_codes(voice.cuda())
    assert codes.shape == (spec.num_codebooks, 6)
    b = m(**kw, decoder_input_ids=codes)
    assert a.loss is None and tuple(a.logits.shape) == (spec.num_codebooks, prompt_ids.shape[1] + 6, spec.vocab_size) and torch.equal(a.logits, b.logits)
    with pytest.raises(NotImplementedError, match="generate"):
        m(**kw)
