"""CPU: the host scheduler of ``parler_tts_amd.ContinuousBatcher`` (padding to the session widths, FIFO admission, poll boundaries, slot
reuse, per-request lengths, un-delay + ragged codec hand-off, errors) driven WITHOUT a GPU by a stand-in that implements the engine's
session interface with the oracle, in the style of ``OracleEngine`` in tests/test_generate_glue_cpu.py (tests may use the oracle; the
product never does). What the HIP session computes is covered by tests/test_continuous_batching_gpu.py."""
import os
import re
import types

import pytest
import torch

from oracle import dac_oracle as DA
from oracle import decoder_oracle as DO

import parler_tts_amd as P
from parler_tts_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SESSION_SYMBOLS = ("ptts_session_begin", "ptts_admit_row", "ptts_row_state", "ptts_retire_row")


class OracleSessionEngine:
    """Session interface of parler_tts_amd.engine.DecoderEngine on the oracle: a slot is idle -> live (admit_row) -> finished -> idle
    (retire_row); decode_steps moves every live slot by one column per step; a slot is never touched while another is admitted."""

    def __init__(self, spec, sd):
        self.spec, self.sd = spec, sd
        self.cfg = types.SimpleNamespace(max_batch=64, max_enc=4096, max_prompt=4096, max_ctx=1 << 20)
        self.log = []  # ("admit" | "retire", slot, step count)
        self.steps = 0
        self.polls = 0

    def set_gen_params(self, **kw):
        self.gp = kw

    def begin_session(self, slots, enc_width, prompt_width):
        self.B, self.N, self.P = slots, enc_width, prompt_width
        self.full = [None] * slots
        self.cur = [1] * slots

    def admit_row(self, row, enc, enc_mask, prompt, prompt_mask, max_length=0, sample=True):
        if not 0 <= row < self.B:
            raise ValueError(f"slot {row} outside the session's {self.B} slots")
        if self.full[row] is not None:
            raise ValueError(f"slot {row} still holds a request (ptts_retire_row first)")
        assert tuple(enc.shape) == (self.N, self.spec.hidden_size) and enc_mask.shape == (self.N,)
        assert (prompt is None) == (self.P == 0) and (prompt is None or tuple(prompt.shape) == (self.P, self.spec.hidden_size))
        L = max_length or self.gp["max_length"]
        gp = DO.GenParams(max_length=L, min_new_tokens=self.gp.get("min_new_tokens", 0))
        with torch.no_grad():
            tr = DO.sample_loop(DO.DecoderOracle(self.spec, self.sd), enc[None].float(), enc_mask[None], None if prompt is None else prompt[None].float(),
                                None if prompt_mask is None else prompt_mask[None], gp)
        self.full[row], self.cur[row] = tr.sequences, 2
        self.log.append(("admit", row, self.steps))

    def decode_steps(self, n):
        assert n >= 1
        self.steps += n
        for s in range(self.B):
            if self.full[s] is not None:
                self.cur[s] = min(self.cur[s] + n, self.full[s].shape[1])

    def row_state(self):
        self.polls += 1
        return list(self.cur), [f is not None and c < f.shape[1] for f, c in zip(self.full, self.cur)]

    def row_ids(self, row, cols):
        return self.full[row][:, :cols].clone()

    def retire_row(self, row):
        self.full[row], self.cur[row] = None, 1
        self.log.append(("retire", row, self.steps))


def _model(eos_gain=None):
    from transformers import T5Config

    torch.manual_seed(0)
    t5 = T5Config(vocab_size=128, d_model=128, d_kv=32, d_ff=256, num_layers=2, num_heads=4, feed_forward_proj="gated-gelu")
    dec = P.ParlerTTSDecoderConfig(vocab_size=1088, max_position_embeddings=256, num_hidden_layers=2, ffn_dim=256, num_attention_heads=2,
                                   hidden_size=128, num_codebooks=9, pad_token_id=1024, eos_token_id=1024, bos_token_id=1025)
    m = P.ParlerTTSForConditionalGeneration(P.ParlerTTSConfig.from_sub_models_config(t5, P.DACConfig(latent_dim=64, decoder_dim=256, decoder_rates=[4, 2, 2, 2]),
                                                                                    dec, vocab_size=128))
    spec, sd = DO.TINY, DO.make_decoder_weights(DO.TINY, seed=1237)
    for k in range(9):
        if eos_gain:
            sd[f"lm_heads.{k}.weight"][1024] *= eos_gain
        else:
            sd[f"lm_heads.{k}.weight"][1024:] = 0.0
    m.decoder.load_state_dict(sd, strict=False)
    eng = OracleSessionEngine(spec, sd)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    dac = DA.DacOracle(DA.DAC_TINY, DA.make_dac_weights(DA.DAC_TINY, seed=4321))
    groups = []

    def decode_filtered(audio_codes):  # ptts_dac_compact_codes + ptts_dac_decode_ragged semantics on the oracle codec
        codes = audio_codes[0].cpu()
        B, _, T = codes.shape
        groups.append(B)
        hop = DA.DAC_TINY.hop_length
        out, frames = torch.zeros(B, 1, hop * T), torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            ok = ((codes[b] >= 1024) | (codes[b] < 0)).sum(dim=0) == 0
            n = int(ok.sum())
            frames[b] = n
            if n:
                out[b, 0, :hop * n] = dac.decode(codes[b:b + 1, :, ok])[0, 0]
        return out, frames

    m.audio_encoder.decode_filtered = decode_filtered
    return m, spec, sd, dac, eng, groups


def _requests(n, seed, N=9, Pw=5):
    g = torch.Generator().manual_seed(seed)
    reqs = []
    for i in range(n):
        nd, npr = N - i % 4, Pw - i % 3  # ragged: shorter descriptions / prompts are padded to the session widths
        reqs.append(dict(input_ids=torch.randint(3, 128, (nd,), generator=g), prompt_input_ids=torch.randint(3, 128, (1, npr), generator=g),
                         max_new_tokens=[10, 24, 13, 19, 30, 16, 11, 27][i % 8]))
    return reqs


def _reference(m, spec, sd, dac, req, N, Pw, min_new):
    """The per-request pipeline: the request as ONE row padded to the session widths -> oracle loop with its own max_length -> un-delay ->
    special-id filter -> oracle codec."""
    ids = torch.zeros(1, N, dtype=torch.long); mask = torch.zeros(1, N, dtype=torch.long)
    d = req["input_ids"].reshape(-1)
    ids[0, : d.shape[0]], mask[0, : d.shape[0]] = d, 1
    pids = torch.zeros(1, Pw, dtype=torch.long); pmask = torch.zeros(1, Pw, dtype=torch.long)
    p = req["prompt_input_ids"].reshape(-1)
    pids[0, : p.shape[0]], pmask[0, : p.shape[0]] = p, 1
    with torch.no_grad():
        enc = m._encode_description(ids, mask).float()
        prompt = m.embed_prompts(pids).float()
        L = req["max_new_tokens"] + 1
        tr = DO.sample_loop(DO.DecoderOracle(spec, sd), enc, mask, prompt, pmask, DO.GenParams(max_length=L, min_new_tokens=min_new))
        codes = DO.valid_frames(DO.undelay(tr.sequences, spec, L)[0])
        return dac.decode(codes[None])[0, 0] if codes.shape[1] else torch.zeros(1)


@pytest.mark.parametrize("eos_gain,min_new", [(None, 0), (6.0, 3)])
def test_results_equal_the_per_request_pipeline_in_submission_order(eos_gain, min_new):
    m, spec, sd, dac, eng, groups = _model(eos_gain)
    reqs = _requests(8, seed=1)
    cb = P.ContinuousBatcher(m, slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, do_sample=False, max_new_tokens=30, min_new_tokens=min_new)
    out = cb.run(reqs)
    assert len(out) == 8
    for r, (wav, n) in zip(reqs, out):
        ref = _reference(m, spec, sd, dac, r, 9, 5, min_new)
        assert wav.dim() == 1 and n == wav.shape[0] == ref.shape[0], (n, wav.shape, ref.shape)
        assert torch.allclose(wav, ref, atol=1e-6)
    if eos_gain is None:  # EOS never wins: request 1 holds 25 columns, of which the delay pattern (>= 2K - 1 = 17 columns) leaves 25 - K frames
        hop = DA.DAC_TINY.hop_length
        assert [n for _, n in out][1] == hop * (25 - 9)


def test_fifo_admission_slot_reuse_after_retirement_and_no_starvation():
    m, spec, sd, dac, eng, groups = _model()
    reqs = _requests(16, seed=2)  # 4 x the slots
    cb = P.ContinuousBatcher(m, slots=4, max_description_tokens=9, max_prompt_tokens=5, poll_steps=16, do_sample=False, max_new_tokens=30, min_new_tokens=30)
    tickets = [cb.submit(**r) for r in reqs]
    assert tickets == list(range(16)) and cb.pending() == 16
    finished = [(t, n) for t, w, n in cb]
    assert sorted(t for t, _ in finished) == tickets and cb.pending() == 0
    admits = [e for e in eng.log if e[0] == "admit"]
    assert len(admits) == 16
    # a slot is admitted into only when idle: per slot the log alternates admit, retire, admit, ...
    for s in range(4):
        kinds = [k for k, slot, _ in eng.log if slot == s]
        assert kinds == ["admit", "retire"] * (len(kinds) // 2) and len(kinds) >= 2
    # FIFO: the i-th admission is the i-th submission (the stand-in computes each request at admission, so its length identifies it)
    L = [r["max_new_tokens"] + 1 for r in reqs]
    by_slot = {}
    order = []
    for kind, slot, step in eng.log:
        if kind == "admit":
            by_slot[slot] = (len(order), step)
            order.append(slot)
        else:
            i, s0 = by_slot.pop(slot)
            # EOS is blocked: request i ends exactly L[i] - 2 steps after its admission, and the scheduler met that end exactly (it is known
            # to the host), so the slot was refilled at once
            assert step - s0 == L[i] - 2, (i, step, s0)
    # no starvation: every request was admitted before any request submitted 2 x slots later finished; here simply: admissions are in ticket order
    # and the first four go in before the first step
    assert [s for k, s, st in eng.log[:4]] == [0, 1, 2, 3] and all(st == 0 for _, _, st in eng.log[:4])
    # requests finish in order of their end step, not of submission: ticket 0 (10 tokens) leaves before ticket 1 (24 tokens)
    assert [t for t, _ in finished].index(0) < [t for t, _ in finished].index(1)


def test_rows_that_finish_at_one_poll_are_decoded_as_one_ragged_batch():
    m, spec, sd, dac, eng, groups = _model()
    g = torch.Generator().manual_seed(3)
    reqs = [dict(input_ids=torch.randint(3, 128, (7,), generator=g), prompt_input_ids=torch.randint(3, 128, (4,), generator=g), max_new_tokens=n)
            for n in (20, 20, 12)]
    cb = P.ContinuousBatcher(m, slots=3, max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_new_tokens=30, min_new_tokens=30)
    out = cb.run(reqs)
    assert groups == [1, 2]  # the short one alone, then the two that end together in one codec pass
    hop = DA.DAC_TINY.hop_length
    assert [n for _, n in out] == [hop * 12, hop * 12, hop * 12]  # 21 columns - K delayed ones; 13 columns < 2K - 1: no delay pattern, all 12 kept


def test_capacity_and_unsupported_arguments():
    m, spec, sd, dac, eng, groups = _model()
    kw = dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_new_tokens=20)
    cb = P.ContinuousBatcher(m, **kw)
    ids, pids = torch.randint(3, 128, (9,)), torch.randint(3, 128, (5,))
    with pytest.raises(ValueError, match="description has 10 tokens"):
        cb.submit(torch.randint(3, 128, (10,)), prompt_input_ids=pids)
    with pytest.raises(ValueError, match="prompt has 6 tokens"):
        cb.submit(ids, prompt_input_ids=torch.randint(3, 128, (6,)))
    with pytest.raises(ValueError, match="exceeds the session's 20"):
        cb.submit(ids, prompt_input_ids=pids, max_new_tokens=21)
    with pytest.raises(ValueError, match="no room"):
        cb.submit(ids, prompt_input_ids=pids, max_new_tokens=0)
    with pytest.raises(ValueError, match="prompt_input_ids` is required"):
        cb.submit(ids)
    with pytest.raises(ValueError, match="one request at a time"):
        cb.submit(torch.randint(3, 128, (2, 9)), prompt_input_ids=pids)
    with pytest.raises(ValueError, match="attention mask of 3 positions"):
        cb.submit(ids, attention_mask=torch.ones(3), prompt_input_ids=pids)
    assert cb.pending() == 0  # nothing was queued by a refused submit
    from transformers import LogitsProcessorList

    for bad in (dict(logits_processor=LogitsProcessorList([P.ParlerTTSLogitsProcessor(1024, 9, 1, "cpu")])), dict(streamer=object()),
                dict(repetition_penalty=1.3), dict(input_values=torch.zeros(1, 1, 64)), dict(decoder_input_ids=torch.zeros(9, 3, dtype=torch.long)),
                dict(output_scores=True)):
        with pytest.raises(NotImplementedError):
            P.ContinuousBatcher(m, **kw, **bad)
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        P.ContinuousBatcher(m, **{**kw, "do_sample": True}, num_return_sequences=2)
    with pytest.raises(ValueError, match="not generation options"):
        P.ContinuousBatcher(m, **kw, no_such_option=1)
    with pytest.raises(ValueError, match="greedy or sampling"):
        P.ContinuousBatcher(m, **kw, num_beams=2)
    with pytest.raises(ValueError):
        P.ContinuousBatcher(m, slots=0, max_description_tokens=9, max_prompt_tokens=5)
    cb0 = P.ContinuousBatcher(m, slots=1, max_description_tokens=9, max_prompt_tokens=0, do_sample=False, max_new_tokens=12, min_new_tokens=12)
    with pytest.raises(ValueError, match="without prompt positions"):
        cb0.submit(ids, prompt_input_ids=pids)
    (wav, n), = cb0.run([dict(input_ids=ids)])
    assert n == wav.shape[0] == DA.DAC_TINY.hop_length * 12


def test_header_symbols_and_ctypes_prototypes_agree_for_the_session_functions():
    hdr = open(os.path.join(ROOT, "include", "ptts.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+PTTS_ABI_VERSION\s+8\b", hdr) and _native.ABI_VERSION == 8  # additive: the version does not move
    ctype_of = {"ptts_engine*": _native.C.c_void_p, "void*": _native.C.c_void_p, "int32_t": _native.C.c_int32, "const float*": _native.C.c_void_p,
                "const int32_t*": _native.C.c_void_p}
    for name in SESSION_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/ptts.h"
        assert name in _native.SYMBOLS, f"{name} missing from _native.SYMBOLS"
        res, args = _native.SYMBOLS[name]
        params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
        assert res is _native.C.c_int and len(args) == len(params), (name, params)
        for p, a in zip(params, args):
            if p == "int32_t*":
                assert a is _native.C.POINTER(_native.C.c_int32), (name, p)
            else:
                assert a is ctype_of[p], (name, p, a)
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read()
    for name in SESSION_SYMBOLS:
        assert re.search(r'extern "C" int ' + name + r"\(", src), f"{name} is not defined in ptts_lm.hip"
