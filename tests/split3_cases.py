"""Inputs and runs shared by tests/test_split3_combine_gpu.py and tools/make_split3_combine_golden.py (which records the parent
library's logits): a 2-layer H = 512 bf16 single-utterance engine, description 64, the prompt length sets the context.

Context C of a decode step = self-KV positions including the new one = prompt + 1 (BOS column) + steps so far. The step graph / eager
forward of that step is built for the bucket kv_bound = (C + 1) rounded up to 64, and the fused self-attention node takes the smallest
power of two S with S * 256 >= kv_bound."""
import hashlib

import torch

from helpers import make_engine
from oracle import decoder_oracle as DO

N_DESC = 64
WEIGHT_SEED = 131
# (prompt length, teacher-forced steps, KV splits of each step): contexts 251..256 across the 1 -> 2 edge (bucket 256 | 320), 302..307 on
# 2 splits, 511..516 across the 2 -> 4 edge (bucket 512 | 576), 1032..1033 on 8 splits
WINDOWS = {"edge_256": (249, 6, [1, 1, 1, 1, 1, 2]), "two": (300, 6, [2] * 6), "edge_512": (509, 6, [2, 4, 4, 4, 4, 4]), "eight": (1030, 2, [8, 8])}
MAX_CTX = 1344
# free-running greedy case (prompt 499, 42 columns): the input seed with the largest top-2 margin on the CPU oracle in bf16 precision
# out of seeds 1..60, so that a last-bit difference between two paths cannot turn an arg-max
GREEDY_SEED, GREEDY_MARGIN = 50, 1.7e-3


def spec():
    return DO.DecoderSpec(hidden_size=512, num_attention_heads=8, ffn_dim=1024, num_hidden_layers=2, max_position_embeddings=2048)


def weights():
    return DO.make_decoder_weights(spec(), seed=WEIGHT_SEED)


def inputs(P, seed=7):
    g = torch.Generator().manual_seed(seed * 10007 + P)
    sp = spec()
    enc = torch.randn(1, N_DESC, sp.hidden_size, generator=g)
    prompt = torch.randn(1, P, sp.hidden_size, generator=g) * 0.5
    ids = torch.randint(0, 1024, (8, sp.num_codebooks), generator=g)
    return enc, prompt, ids


def engine(sd):
    """PTTS_NO_FUSE_QA (the two-node path) is read when the engine is created: set it before the call."""
    return make_engine(spec(), sd, torch.bfloat16, max_batch=1, max_ctx=MAX_CTX, max_enc=N_DESC, max_prompt=MAX_CTX - 16)


def step_logits(eng, P, steps):
    """Prefill of P prompt positions, then `steps` teacher-forced decode forwards: their logits (contexts P + 2 .. P + 1 + steps)."""
    enc, prompt, ids = inputs(P)
    eng.set_gen_params(max_length=16)  # < 2K - 1: no delay pattern, the ids are fed as given
    eng.prefill(enc, None, prompt, None, sample=False)
    outs = []
    for s in range(steps):
        eng.push_tokens(ids[s])
        eng.step_forward()
        outs.append(eng.logits().cpu())
    return outs


def digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()
