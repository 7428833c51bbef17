"""Writes tests/golden/score_ref.npz from the reference's own classes (run where the reference tree is importable):
ParlerTTSForCausalLM.forward with labels on a tiny config - B = 2, ragged description and prompt masks, labels with -100 tails of different
lengths, one label equal to BOS, one input column holding EOS - once with codebook_weights and the mean reduction, once without weights and
loss_reduction="sum". Stored: the inputs, loss, per_codebook_losses and logits of both runs. Data only; nothing of the reference's text."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import decoder_oracle as DO  # noqa: E402

SPEC = DO.DecoderSpec(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, ffn_dim=256, max_position_embeddings=64, vocab_size=80,
                      pad_token_id=64, eos_token_id=64, bos_token_id=65)
WEIGHT_SEED = 4242
CODEBOOK_WEIGHTS = [4.0, 2.0, 1.0, 1.0, 1.0, 0.5, 0.5, 0.25, 0.25]
B, N, P, T = 2, 7, 3, 9


def inputs():
    g = torch.Generator().manual_seed(17)
    K = SPEC.num_codebooks
    enc = torch.randn(B, N, SPEC.hidden_size, generator=g)
    prompt = torch.randn(B, P, SPEC.hidden_size, generator=g) * 0.5
    enc_mask, prompt_mask = torch.ones(B, N, dtype=torch.long), torch.ones(B, P, dtype=torch.long)
    enc_mask[1, 5:] = 0
    prompt_mask[1, :1] = 0
    enc = enc * enc_mask[..., None]
    labels = torch.randint(0, 64, (B, T, K), generator=g)
    for b in range(B):
        for k in range(K):
            tail = (2 * b + k) % 5
            if tail:
                labels[b, T - tail:, k] = -100
    labels[1, :, 8] = -100                 # a codebook row without a label; with b = 0 below, codebook 8 keeps some
    labels[0, 2, 1] = SPEC.bos_token_id    # a label equal to BOS
    labels[0, 3, 2] = SPEC.eos_token_id    # the one EOS a row ends with counts
    ids = labels.transpose(1, 2).clone()   # shift right: what prepare_decoder_input_ids_from_labels gives
    ids[..., 1:] = labels.transpose(1, 2)[..., :-1]
    ids[..., 0] = SPEC.bos_token_id
    ids = ids.masked_fill(ids == -100, SPEC.pad_token_id).reshape(B * K, T)  # pad == eos: columns behind a row's end hold EOS
    ids[4, 2] = SPEC.eos_token_id          # an input column holding EOS in the middle of a row
    return enc, enc_mask, prompt, prompt_mask, ids, labels


def reference_results():
    """{run__field: array} of the two runs, computed on the reference's ParlerTTSForCausalLM."""
    from oracle.reference_shims import import_reference
    import oracle.make_golden as mg

    ref = import_reference()
    sd = DO.make_decoder_weights(SPEC, seed=WEIGHT_SEED)
    enc, enc_mask, prompt, prompt_mask, ids, labels = inputs()
    m = mg.build_reference_lm(ref, SPEC, sd)
    out = {}
    for tag, weights, red in (("weighted_mean", CODEBOOK_WEIGHTS, "mean"), ("sum", None, "sum")):
        m.config.codebook_weights = weights
        with torch.no_grad():
            o = m(input_ids=ids.view(B, SPEC.num_codebooks, T), attention_mask=torch.ones(B, T, dtype=torch.long), encoder_hidden_states=enc, encoder_attention_mask=enc_mask,
                  prompt_hidden_states=prompt, prompt_attention_mask=prompt_mask, labels=labels, loss_reduction=red, use_cache=False, return_dict=True)
        out[f"{tag}__loss"] = o.loss.numpy()
        out[f"{tag}__per_codebook_losses"] = torch.stack(list(o.per_codebook_losses)).numpy()
        out[f"{tag}__logits"] = o.logits.numpy()
    return out


def main():
    enc, enc_mask, prompt, prompt_mask, ids, labels = inputs()
    out = reference_results()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "score_ref.npz"), enc=enc.numpy(), enc_mask=enc_mask.numpy(), prompt=prompt.numpy(),
                        prompt_mask=prompt_mask.numpy(), input_ids=ids.numpy(), labels=labels.numpy(), codebook_weights=np.array(CODEBOOK_WEIGHTS),
                        weight_seed=np.array(WEIGHT_SEED), **out)
    print({k: (v.shape, float(np.asarray(v).reshape(-1)[0])) for k, v in out.items()})


if __name__ == "__main__":
    main()
