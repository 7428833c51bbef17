"""Shared test helpers: build native engines from oracle specs + seeded synthetic weights."""
import numpy as np
import torch

from oracle import decoder_oracle as DO
from oracle import dac_oracle as DA


# END-TO-END relative waveform RMS of the bf16-operand DAC engine against DacOracle(precision="bf16"): 2 x the value measured on MI355X at 860
# frames (9.7e-3, profiles/r04_parity_dac_bf16.txt). It cannot be tighter: the oracle evaluated with float64 accumulation is already 9.0e-3 away
# from itself (bf16 rounding flips amplified by ~30 layers, profiles/r04_dac_bf16_sensitivity.txt). The tight pin of the bf16 kernels is per stage,
# on identical inputs: tests/test_dac_stage_parity_gpu.py (4e-4 on each stage's own contribution).
DAC_BF16_TOL = 2e-2
# The dh_snake probe (snake_f<true>: v_sin_f32 on alpha x / 2 pi) against the float64 Snake, relative to |v| + 1 / alpha, over |alpha v| <= pi:
# 4 x the maximum measured on MI355X (1.527e-7, profiles/dac_kernels_parity.txt). tests/test_dac_kernels_gpu.py takes the probe as the reference of
# every fast-path activation and requires this bar to stay below 2^-9, so that an error in the formula cannot hide behind it.
DAC_SNAKE_S32_TOL = 4 * 1.527e-7


def log_parity(msg, name="r04_parity_dac_bf16.txt"):
    """print + append to gpurun_out/<name> (copied into profiles/ as the record of the run)."""
    import os

    print(msg, flush=True)
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", name), "a") as f:
            f.write(msg + "\n")
    except OSError:
        pass


def spec_from_gold(arr, **kw):
    H, L, nh, F, mp, rope = [int(x) for x in arr[:6]]
    if len(arr) > 6:  # grouped-query fixtures also record the K/V head counts
        kw = {"num_key_value_heads": int(arr[6]), "num_cross_attention_key_value_heads": int(arr[7]), **kw}
    return DO.DecoderSpec(hidden_size=H, num_hidden_layers=L, num_attention_heads=nh, ffn_dim=F, max_position_embeddings=mp,
                          rope_embeddings=bool(rope), **kw)


def make_engine(spec, sd, dtype=torch.float32, max_batch=2, max_ctx=128, max_enc=32, max_prompt=16, weights_fp8=False, kv_fp8=False):
    from parler_tts_amd.engine import DecoderEngine

    eng = DecoderEngine(hidden_size=spec.hidden_size, num_layers=spec.num_hidden_layers, num_heads=spec.num_attention_heads,
                        ffn_dim=spec.ffn_dim, num_codebooks=spec.num_codebooks, vocab_size=spec.vocab_size,
                        max_positions=spec.max_position_embeddings, rope=spec.rope_embeddings, rope_theta=spec.rope_theta,
                        pad_token_id=spec.pad_token_id, eos_token_id=spec.eos_token_id, bos_token_id=spec.bos_token_id, dtype=dtype,
                        max_batch=max_batch, max_ctx=max_ctx, max_enc=max_enc, max_prompt=max_prompt,
                        num_kv_heads=spec.kv_heads, num_cross_kv_heads=spec.cross_kv_heads, weights_fp8=weights_fp8, kv_fp8=kv_fp8)
    eng.load_state_dict(sd)
    return eng


def make_dac(spec, sd, max_batch=2, max_frames=64):
    from parler_tts_amd.engine import DacEngine

    d = DacEngine(num_codebooks=spec.num_codebooks, codebook_size=spec.codebook_size, codebook_dim=spec.codebook_dim,
                  latent_dim=spec.latent_dim, decoder_dim=spec.decoder_dim, rates=spec.decoder_rates, max_batch=max_batch,
                  max_frames=max_frames)
    d.load_state_dict(sd)
    return d


def t(x):
    return torch.from_numpy(np.asarray(x))
