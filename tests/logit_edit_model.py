"""Host model of the logit-edit node (parler_tts_amd/csrc/ptts_logit_edit_kernels.h) in numpy fp32, the cases the tests of the node share, and
the same cases through transformers' own processors (the chain ``generation_extras.build_processors`` builds).

The model restates include/ptts_logit_edit.h: five stages in transformers' order, each an elementwise fp32 operation - numpy rounds every
operation once, so the decay's product and sum are two roundings, as torch's are. tests/test_logit_edit_model_cpu.py pins it against
transformers bit for bit; tests/test_logit_edit_kernel_gpu.py compares the kernel with it."""
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

LE_BIAS, LE_BAD, LE_DECAY, LE_SUPPRESS, LE_BEGIN = 1, 2, 4, 8, 16
LEF_BAD, LEF_SUPPRESS, LEF_BEGIN = 1, 2, 4


class Record(NamedTuple):
    """The options of one utterance as ``GenerationConfig`` takes them; ``None``: absent."""
    sequence_bias: Optional[Dict[Tuple[int], float]] = None
    bad_words_ids: Optional[List[List[int]]] = None
    exponential_decay_length_penalty: Optional[Tuple[int, float]] = None
    suppress_tokens: Optional[List[int]] = None
    begin_suppress_tokens: Optional[List[int]] = None

    @property
    def neutral(self):
        return all(v is None for v in self)


class Case(NamedTuple):
    name: str
    V: int
    K: int
    eos: int
    logits: np.ndarray          # [B][K][V] fp32
    t_prefix: List[int]         # [B] voice-prompt frames: given = 1 + t_prefix
    records: List[Record]       # [B]
    clocks: List[List[int]]     # the launches of the case: each a cur_len [B]

    @property
    def B(self):
        return len(self.records)


def decay_m(factor: float, idx: int) -> np.float32:
    return np.float32(pow(float(factor), idx) - 1.0)  # Python's float pow is the C library's


def apply_row(l: np.ndarray, rec: Record, t: int, given: int, eos: int) -> np.ndarray:
    """One utterance: ``l`` [K][V] fp32 at clock ``t``; returns a new array (the input itself when no stage is active)."""
    V = l.shape[-1]
    ninf = np.float32(-np.inf)
    out = l
    if rec.sequence_bias is not None:
        bias = np.zeros(V, np.float32)
        for (tok,), b in rec.sequence_bias.items():
            bias[tok] = np.float32(b)
        out = out + bias
    if rec.bad_words_ids is not None:  # [eos] is dropped; the add happens whatever is left
        bad = [w[0] for w in rec.bad_words_ids if w != [eos]]
        add = np.zeros(V, np.float32)
        add[bad] = ninf
        out = out + add
    if rec.exponential_decay_length_penalty is not None:
        start, factor = rec.exponential_decay_length_penalty
        idx = t - start - given
        if idx > 0:
            pen = np.zeros_like(out)
            pen[:, eos] = np.abs(out[:, eos]) * decay_m(factor, idx)  # rounded here ...
            out = out + pen                                           # ... and here
    if rec.suppress_tokens is not None:
        toks = [v for v in rec.suppress_tokens if 0 <= v < V]
        out = out.copy()
        out[:, toks] = ninf
    if rec.begin_suppress_tokens is not None and t == given:
        toks = [v for v in rec.begin_suppress_tokens if 0 <= v < V]
        out = out.copy()
        out[:, toks] = ninf
    return out


def apply(case: Case, cur_len: List[int]) -> np.ndarray:
    return np.stack([apply_row(case.logits[b], case.records[b], cur_len[b], 1 + case.t_prefix[b], case.eos) for b in range(case.B)])


def transformers_apply(case: Case, cur_len: List[int], min_new_tokens: Optional[int] = None) -> np.ndarray:
    """The same through the chain generation_extras.build_processors assembles from transformers' classes, utterance by utterance on the CPU."""
    from parler_tts_amd.generation_extras import build_processors

    out = []
    for b in range(case.B):
        gc = SimpleNamespace(do_sample=False, min_new_tokens=min_new_tokens, **case.records[b]._asdict())
        procs = build_processors(gc, 1 + case.t_prefix[b], None, [], "cpu", case.eos)
        ids = torch.zeros((case.K, cur_len[b]), dtype=torch.long)
        out.append(procs(ids, torch.from_numpy(case.logits[b].copy())).numpy())
    return np.stack(out)


def pack(case: Case, ld_t: int, extra_records: int = 0):
    """The records as the device arrays of LogitEditRecs (what the engine's build_logit_edit writes): header int32 [n][4], bias fp32 [n][ld_v],
    decay fp32 [n][ld_t], flags uint8 [n][ld_v]; ``extra_records`` more (zeroed) behind them."""
    n, V = case.B + extra_records, case.V
    ld_v = (V + 3) & ~3
    hdr, bias = np.zeros((n, 4), np.int32), np.zeros((n, ld_v), np.float32)
    decay, flags = np.zeros((n, ld_t), np.float32), np.zeros((n, ld_v), np.uint8)
    for b, rec in enumerate(case.records):
        mask = 0
        if rec.sequence_bias is not None:
            mask |= LE_BIAS
            for (tok,), v in rec.sequence_bias.items():
                bias[b, tok] = np.float32(v)
        for w in rec.bad_words_ids or []:
            mask |= LE_BAD
            if w != [case.eos]:
                flags[b, w[0]] |= LEF_BAD
        if rec.exponential_decay_length_penalty is not None:
            start, factor = rec.exponential_decay_length_penalty
            mask |= LE_DECAY
            decay[b] = [decay_m(factor, i) for i in range(ld_t)]
            hdr[b, 1], hdr[b, 2] = start, ld_t
        if rec.suppress_tokens is not None:
            mask |= LE_SUPPRESS
            for v in rec.suppress_tokens:
                if 0 <= v < V:
                    flags[b, v] |= LEF_SUPPRESS
        if rec.begin_suppress_tokens is not None:
            mask |= LE_BEGIN
            for v in rec.begin_suppress_tokens:
                if 0 <= v < V:
                    flags[b, v] |= LEF_BEGIN
        hdr[b, 0] = mask
    return hdr, bias, decay, flags, ld_v


LATE = 800  # idx of the late decay clock


def _logits(rng, B, K, V, eos):
    """Normal fp32 logits with -0.0, +0.0 and -inf at tokens that are not EOS; the EOS logits finite, of both signs (the decay takes |l|)."""
    l = rng.standard_normal((B, K, V)).astype(np.float32) * np.float32(3.0)
    other = [v for v in range(V) if v != eos]
    for b in range(B):
        for k in range(K):
            pick = rng.choice(other, size=min(6, len(other)), replace=False)
            l[b, k, pick[0:2]] = np.float32(-0.0)
            l[b, k, pick[2]] = np.float32(0.0)
            l[b, k, pick[3:6]] = -np.inf
            l[b, k, eos] = np.float32((-1.0) ** (b + k)) * (np.float32(0.5) + abs(l[b, k, eos]))
    return l


def _clocks(t_prefix, records):
    """given - 1 .. given + 2, and around each decay's start: start + given - 1 .. start + given + 3, then idx = LATE; utterances side by side."""
    per = []
    for T, rec in zip(t_prefix, records):
        g = 1 + T
        start = rec.exponential_decay_length_penalty[0] if rec.exponential_decay_length_penalty is not None else 3
        per.append([g - 1, g, g + 1, g + 2] + [start + g + d for d in (-1, 0, 1, 2, 3)] + [start + g + LATE])
    return [[p[j] for p in per] for j in range(len(per[0]))]


def three_records(V, eos):
    """What the kernel test runs at every shape: all five stages, the neutral record, and a decay with a suppress list."""
    full = Record(sequence_bias={(eos,): 2.5, (3,): -1.25, (V - 1,): 0.75, (4,): 0.0},
                  bad_words_ids=[[5], [eos], [V - 2]],
                  exponential_decay_length_penalty=(4, 1.05),
                  suppress_tokens=[7, V + 5, 0, 3],
                  begin_suppress_tokens=[eos, 9, 2 * V])
    return [full, Record(), Record(exponential_decay_length_penalty=(2, 1.01), suppress_tokens=[V - 1, 1])]


def cases() -> List[Case]:
    out = []
    for V in (33, 1088, 2048):
        for K in (1, 9):
            rng = np.random.default_rng(1000 * V + K)
            eos = V - 9  # as in Parler-TTS: a token near the end of the vocabulary, not the last
            recs = three_records(V, eos)
            T = [0, 5, 5]
            out.append(Case(f"V{V}_K{K}_B3", V, K, eos, _logits(rng, 3, K, V, eos), T, recs, _clocks(T, recs)))
    # each option alone (and a bad word equal to [eos] alone: dropped, the neutral record), given of 1 and of 1 + 5
    V, K, eos = 33, 2, 24
    alone = [Record(sequence_bias={(eos,): -3.0, (2,): 1.5}), Record(bad_words_ids=[[4], [eos]]), Record(bad_words_ids=[[eos]]),
             Record(exponential_decay_length_penalty=(3, 1.08)), Record(exponential_decay_length_penalty=(0, 0.9)),
             Record(suppress_tokens=[1, 2, V, V + 40]), Record(suppress_tokens=[V + 1]), Record(begin_suppress_tokens=[eos, 3, V])]
    for i, rec in enumerate(alone):
        rng = np.random.default_rng(77 + i)
        recs, T = [rec, rec], [0, 5]
        out.append(Case(f"alone{i}_{[n for n, v in rec._asdict().items() if v is not None][0]}", V, K, eos, _logits(rng, 2, K, V, eos), T, recs,
                        _clocks(T, recs)))
    return out


def greedy_reference(spec, sd, enc, enc_mask, prompt, prompt_mask, max_length, min_new_tokens, record: Record, prefix=None):
    """The greedy loop of oracle.decoder_oracle.sample_loop for ONE request under transformers' own chain in transformers' own order
    (generation_extras.build_processors: the record's processors, MinNewTokensLength where it stands, the EOS gate as the custom list). Returns
    (raw ids [K, columns], the smallest top-2 margin over live rows): the reference of the engine's device path - which runs the node in front of
    the tail's min_new_tokens - on requests whose margin is asserted."""
    import math

    from oracle import decoder_oracle as DO
    from parler_tts_amd.generation_extras import build_processors

    model = DO.DecoderOracle(spec, sd)
    K = spec.num_codebooks
    eos, pad, bos = spec.eos_token_id, spec.pad_token_id, spec.bos_token_id
    model.reset()
    seq = torch.full((K, 1), bos, dtype=torch.long)
    if prefix is not None and prefix.shape[-1] > 0:
        seq = torch.cat([seq, prefix.long()], dim=-1)
    seq, pattern = DO.build_delay_pattern_mask(seq, bos, pad, max_length, K)
    given = seq.shape[-1]
    gc = SimpleNamespace(do_sample=False, min_new_tokens=min_new_tokens, **record._asdict())
    procs = build_processors(gc, given, None, [DO.EosGate(eos, K, 1)], "cpu", eos)
    unfinished = torch.ones(K, dtype=torch.long)
    margin, step = math.inf, 0
    with torch.no_grad():
        while True:
            fed = DO.apply_delay_pattern_mask(seq, pattern)
            logits = model.forward(fed, enc, enc_mask, prompt, prompt_mask) if step == 0 else model.forward(fed[:, -1:])
            scores = procs(seq, logits[:, -1, :].clone().float())
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
