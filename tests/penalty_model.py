"""Host restatement of the history-penalty node (parler_tts_amd/csrc/ptts_penalty_kernels.h) in plain torch, and the cases both the CPU pin
(tests/test_penalty_model_cpu.py: this model == the installed transformers' two processors) and the GPU test of the kernel
(tests/test_history_penalty_kernel_gpu.py: the kernel == transformers' processors) run.

The arithmetic is written without torch's own float32 multiply / divide: the product and the quotient of two float32 values are formed in
float64 (the product is exact there; the quotient carries 53 >= 2 * 24 + 2 bits, so rounding it to float32 is the correctly rounded float32
quotient) and rounded once. That the installed torch gives the same bits on the CPU is what the pin shows."""
import math

import torch

NEG_INF = -math.inf


def apply_row(logits, history, p, n):
    """logits float32 [V] (not modified), history int64 [t] -> the row after the repetition penalty `p` and the n-gram ban `n`."""
    V, t = logits.shape[0], int(history.shape[0])
    out = logits.clone()
    if p == 1.0 and n == 0:
        return out
    hist = history.tolist()
    if p != 1.0:
        p32 = torch.tensor(p, dtype=torch.float32).double()
        for v in sorted({h for h in hist if 0 <= h < V}):  # once per distinct token: duplicates do not compound
            l = logits[v].double()
            out[v] = (l * p32 if bool(logits[v] < 0) else l / p32).float()
    if n >= 1 and t >= n:
        suffix = hist[t - n + 1:]
        for j in range(t - n + 1):
            if hist[j:j + n - 1] == suffix and 0 <= hist[j + n - 1] < V:
                out[hist[j + n - 1]] = NEG_INF  # after the penalty
    return out


def apply(logits, ids, cur_len, records):
    """logits [B, K, V], ids [B * K, ld], cur_len [B], records [(p, n)] * B -> the node's output [B, K, V]."""
    B, K, V = logits.shape
    out = logits.clone()
    for b in range(B):
        p, n = records[b]
        for k in range(K):
            out[b, k] = apply_row(logits[b, k], ids[b * K + k, : cur_len[b]], p, n)
    return out


def transformers_apply(logits, ids, cur_len, records):
    """The oracle: the installed transformers' RepetitionPenaltyLogitsProcessor then NoRepeatNGramLogitsProcessor, on the CPU, per
    utterance (each has its own history length and record), built as generation_extras.build_processors builds them."""
    from transformers.generation import logits_process as LP

    B, K, V = logits.shape
    out = logits.clone()
    for b in range(B):
        p, n = records[b]
        scores, hist = logits[b].clone(), ids[b * K:(b + 1) * K, : cur_len[b]].clone()
        if p != 1.0:
            scores = LP.RepetitionPenaltyLogitsProcessor(penalty=float(p))(hist, scores)
        if n > 0:
            scores = LP.NoRepeatNGramLogitsProcessor(int(n))(hist, scores)
        out[b] = scores
    return out


SENTINEL = 7  # the token columns at and past cur_len hold: a valid id whose logit is never -inf, so reading it would change the result


class Case:
    def __init__(self, name, logits, ids, cur_len, records):
        self.name, self.logits, self.ids, self.cur_len, self.records = name, logits, ids, list(cur_len), list(records)
        self.B, self.K, self.V = logits.shape
        self.ld = ids.shape[1]


def _logits(g, B, K, V):
    """Positive and negative values, +-0, -inf and a subnormal in every row, at places the histories below name."""
    x = torch.randn(B, K, V, generator=g) * 6.0
    x[..., 0] = 0.0
    x[..., 1] = -0.0
    x[..., 2] = NEG_INF
    x[..., 3] = 1e-41
    x[..., 4] = -3.5
    x[..., 5] = 3.5
    x[..., SENTINEL] = 2.25
    return x


def _skip_sentinel(h):
    """No history holds the sentinel: a kernel that read a column at or past t would see a token the oracle never saw."""
    return h + (h >= SENTINEL).long()


def _history(g, rows, t, V, kind):
    if kind == "random":      # a small alphabet: repeats and matching n-grams are frequent
        return _skip_sentinel(torch.randint(0, min(V, 12) - 1, (rows, t), generator=g))
    if kind == "wide":        # the whole vocabulary, the special low ids included
        h = _skip_sentinel(torch.randint(0, V - 1, (rows, t), generator=g))
        h[:, : min(t, 7)] = torch.arange(7)[: min(t, 7)]
        return h
    if kind == "constant":    # one token repeated: catches compounding
        return torch.full((rows, t), 5, dtype=torch.long)
    if kind == "loop":        # a period-3 loop: every third window matches the suffix
        return (torch.arange(t) % 3 + 4).repeat(rows, 1)
    raise ValueError(kind)


def make_case(name, V, K, B, ts, records, kinds, seed, ld=None, special=None):
    """ts / records / kinds: one entry per utterance. `special`: ids written into the first columns of every row (BOS / pad)."""
    g = torch.Generator().manual_seed(seed)
    ld = ld if ld is not None else max(ts) + 5
    ids = torch.full((B * K, ld), SENTINEL, dtype=torch.long)
    for b in range(B):
        h = _history(g, K, ts[b], V, kinds[b])
        if special is not None:
            m = min(len(special), ts[b])
            h[:, :m] = torch.tensor(special[:m])
        ids[b * K:(b + 1) * K, : ts[b]] = h
    return Case(name, _logits(g, B, K, V), ids, ts, records)


def cases():
    out = []
    seed = 100
    # every shape of the issue: V in {40, 1088, 2048} x K in {1, 9} x B in {1, 3}; a different cur_len per utterance; utterance 1 (where
    # there is one) under the neutral record; ids_ld larger than every t
    for V in (40, 1088, 2048):
        for K in (1, 9):
            for B in (1, 3):
                seed += 1
                ts = [37, 300, 1][:B] if B == 3 else [61]
                recs = [(1.4, 2), (1.0, 0), (1.3, 1)][:B] if B == 3 else [(1.4, 2)]
                kinds = ["random", "random", "wide"][:B] if B == 3 else ["random"]
                out.append(make_case(f"V{V}_K{K}_B{B}", V, K, B, ts, recs, kinds, seed))
    # n in {0, 1, 2, 3, 5} at t in {n - 1, n, n + 1} (t >= 1: the BOS column is always there), with and without the penalty
    for n in (0, 1, 2, 3, 5):
        for t in sorted({max(n - 1, 1), max(n, 1), n + 1}):
            for p in (1.0, 1.7):
                seed += 1
                out.append(make_case(f"n{n}_t{t}_p{p}", 1088, 9, 1, [t], [(p, n)], ["constant" if n else "random"], seed))
    # t = 1 (BOS only) and t = 2611, the longest history of the stock generation config, in one batch; loops and one token repeated 50 times
    out.append(make_case("bos_only_and_longest", 1088, 9, 3, [1, 2611, 50], [(1.2, 3), (1.4, 3), (2.0, 2)], ["wide", "loop", "constant"], 901, ld=2620,
                         special=[1025]))
    out.append(make_case("constant50", 1088, 9, 1, [50], [(1.4, 0)], ["constant"], 902))
    out.append(make_case("longest_random_n5", 2048, 9, 1, [2611], [(0.8, 5)], ["random"], 903))
    # BOS / pad ids in the history (1025 / 1024 at V = 1088): they are vocabulary entries of the LM head like any other
    out.append(make_case("bos_pad_history", 1088, 9, 2, [40, 23], [(1.4, 2), (1.1, 1)], ["random", "wide"], 904, special=[1025, 1025, 1024, 1024, 1025]))
    # penalties below one (a reward) and a penalty that overflows a large logit to inf
    big = make_case("overflow", 40, 1, 1, [9], [(3.0e38, 0)], ["wide"], 905)
    big.logits[0, 0, 4] = -3.0e30
    big.logits[0, 0, 5] = 1.0e-30
    out.append(big)
    return out


def greedy_reference(spec, sd, enc, enc_mask, prompt, prompt_mask, max_length, min_new_tokens, records, prefix=None):
    """The greedy loop of oracle.decoder_oracle.sample_loop with transformers' two processors in front of MinNewTokens and the EOS gate (the
    order of generation_extras.build_processors), one (p, n) record per utterance. Returns (raw ids [B * K, columns], the smallest top-2
    margin over live rows): the reference of the engine's device path on requests whose margin is asserted."""
    from oracle import decoder_oracle as DO

    model = DO.DecoderOracle(spec, sd)
    K, bsz = spec.num_codebooks, enc.shape[0]
    eos, pad, bos = spec.eos_token_id, spec.pad_token_id, spec.bos_token_id
    model.reset()
    seq = torch.full((bsz * K, 1), bos, dtype=torch.long)
    if prefix is not None and prefix.shape[-1] > 0:
        seq = torch.cat([seq, prefix.long()], dim=-1)
    seq, pattern = DO.build_delay_pattern_mask(seq, bos, pad, max_length, K)
    given = seq.shape[-1]
    gate = DO.EosGate(eos, K, bsz)
    unfinished = torch.ones(bsz * K, dtype=torch.long)
    margin, step = math.inf, 0
    with torch.no_grad():
        while True:
            fed = DO.apply_delay_pattern_mask(seq, pattern)
            logits = model.forward(fed, enc, enc_mask, prompt, prompt_mask) if step == 0 else model.forward(fed[:, -1:])
            scores = logits[:, -1, :].clone().float().view(bsz, K, -1)
            scores = transformers_apply(scores, seq, [seq.shape[-1]] * bsz, records).view(bsz * K, -1)
            if min_new_tokens > 0 and (seq.shape[-1] - given) < min_new_tokens:
                scores[:, eos] = NEG_INF
            scores = gate(seq, scores)
            top2 = torch.topk(scores, 2, dim=-1)[0]
            m = (top2[:, 0] - top2[:, 1])[unfinished.bool()]
            if m.numel():
                margin = min(margin, float(m.min()))
            nxt = torch.argmax(scores, dim=-1)
            nxt = nxt * unfinished + pad * (1 - unfinished)
            seq = torch.cat([seq, nxt[:, None]], dim=-1)
            unfinished = unfinished & ~((nxt == eos) | (seq.shape[-1] >= max_length)).long()
            step += 1
            if int(unfinished.max()) == 0:
                return seq, margin
