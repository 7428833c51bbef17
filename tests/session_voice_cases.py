"""Seeded requests of the voice-prompt session tests (tests/test_session_voice_gpu.py, tests/test_session_voice_cpu.py), next to tests/cases.py:
shapes DO.TINY (K = 9: the delay pattern starts at max_length 2K - 1 = 17), N = 9, P = 4. A free-running comparison asserts
``min_margin >= cases.MARGIN`` on seeds scanned on the CPU with ``python tools/scan_margin_seeds.py session_voice`` - the oracle on each
request alone, run BOTH with and without its prefix (the minimum of the two margins is what is recorded)."""
import torch

from oracle import decoder_oracle as DO

N, P = 9, 4
WEIGHT_SEED = 1234
SESSION_MAX_LENGTH = 30

# (voice-prompt frames T, the request's own max_length L, scanned input seed): L on both sides of 17, L == T + 2 (one generated token),
# T + 1 > L - K + 1 with L >= 17 (the pad triangle reaches into the prefix columns), T in {1, 8, 9, 11} and requests without a prompt
# (the reference's own build_delay_pattern_mask needs max_length >= T + K wherever there is a pattern: it writes the shifted prefix of codebook
# K - 1 up to column T + K - 1; so does the oracle. A pad triangle that reaches INTO the prefix columns is therefore a case of the writer's
# restatement on the CPU, against the package's mask, not of a free-running comparison)
FREE_RUNNING = [
    (0, 20, 700), (8, 24, 701), (1, 3, 702), (0, 12, 703), (9, 30, 713), (11, 13, 705),
    (0, 17, 706), (8, 16, 707), (1, 17, 717), (11, 20, 724), (0, 26, 711), (9, 11, 711),
]
# oracle margins (min over the run with and without the prefix), same order:
# 4.1e-4, 5.6e-4, 3.7e-3, 2.5e-4, 2.1e-4, 1.0e-3, 1.7e-4, 5.3e-4, 9.6e-4, 2.1e-4, 4.8e-4, 4.2e-4

# test_min_new_tokens_counts_from_the_given_columns, EOS-favouring weights (eos_gain 6), max_length 36: request(888, T = 4) with min_new_tokens 3,
# request(889, no prompt) with its own record (min_new_tokens 5), and request(890, T = 4) twice with its own records, min_new_tokens 4 and 5.
# On these weights the first codebook's EOS never wins before column 9, so the bound of 3 does not move the first pair's ids; the last pair pins
# the count: the oracle ends codebook 0 at column 9 (= 1 + T + 4) under min_new_tokens 4 and at column 10 under 5. Margins (with and without the
# prefix) >= 1.6e-4.
MIN_NEW_SEED = 888
MIN_NEW_MAX_LENGTH = 36


def request(seed, T, rows_n=N, rows_p=P, spec=DO.TINY):
    """One request at the session's widths: enc [N, H] (masked tail zeroed), enc_mask [N], prompt [P, H], prompt_mask [P], prefix [K, T] or None."""
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(rows_n, spec.hidden_size, generator=g)
    prompt = torch.randn(rows_p, spec.hidden_size, generator=g) * 0.5
    enc_mask = torch.ones(rows_n, dtype=torch.long)
    prompt_mask = torch.ones(rows_p, dtype=torch.long)
    enc_mask[rows_n - seed % 3:] = 0 if seed % 3 else 1
    prompt_mask[: seed % 2] = 0
    enc = enc * enc_mask[:, None]
    pre = torch.randint(0, 1024, (spec.num_codebooks, T), generator=g) if T else None
    return enc, enc_mask, prompt, prompt_mask, pre


def weights(eos_gain=None, spec=DO.TINY, seed=WEIGHT_SEED):
    sd = DO.make_decoder_weights(spec, seed=seed)
    if eos_gain:  # cases.voice_lm_case's gain: EOS wins as soon as it is allowed
        for k in range(spec.num_codebooks):
            sd[f"lm_heads.{k}.weight"][spec.eos_token_id] *= eos_gain
    return sd


def oracle_run(spec, sd, req, L, min_new=0, with_prefix=True, precision="fp32", keep_logits=False):
    """sample_loop on the request alone (greedy): the reference of every comparison."""
    enc, enc_mask, prompt, prompt_mask, pre = req
    with torch.no_grad():
        return DO.sample_loop(DO.DecoderOracle(spec, sd, precision=precision), enc[None], enc_mask[None], prompt[None], prompt_mask[None],
                              DO.GenParams(max_length=L, min_new_tokens=min_new), decoder_input_ids=pre if with_prefix else None, keep_logits=keep_logits)


def margin(T, L, seed, sd=None, min_new=0):
    """What the scan records: the smaller margin of the run with and the run without the prefix (the latter with the same total length)."""
    sd = weights() if sd is None else sd
    req = request(seed, T)
    m = oracle_run(DO.TINY, sd, req, L, min_new).min_margin
    return min(m, oracle_run(DO.TINY, sd, req, L, min_new, with_prefix=False).min_margin) if T else m
