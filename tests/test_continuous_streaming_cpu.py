"""CPU: the streaming mode of ``parler_tts_amd.ContinuousBatcher`` (``stream_chunk_frames`` / ``chunks()`` / ``cancel()``) WITHOUT a GPU. The
decoder engine is the oracle stand-in of tests/test_continuous_scheduler_cpu.py (plus ``ids_buffer``); the codec engine's stream table
(``stream_open / stream_reset / stream_decode``) is tests/stream_model.py - the semantics of include/ptts.h restated on the host - with the
oracle codec behind it, as tests/test_generate_glue_cpu.py does for ``decode_chunk``. What the HIP entry points compute is covered by
tests/test_continuous_streaming_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import dac_oracle as DA
from oracle import decoder_oracle as DO

import parler_tts_amd as P
from parler_tts_amd import _native
from stream_model import StreamTableModel
from test_continuous_scheduler_cpu import OracleSessionEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_SYMBOLS = ("ptts_dac_stream_open", "ptts_dac_stream_reset", "ptts_dac_stream_decode")
K, HOP, HALO = 9, DA.DAC_TINY.hop_length, 26
_TRACES = {}


class StreamSessionEngine(OracleSessionEngine):
    """+ ``ids_buffer``: the stand-in hands out ITSELF as the "pointer"; the codec stand-in reads the slots' raw ids through it."""

    def __init__(self, spec, sd, kind):
        super().__init__(spec, sd)
        self.kind = kind

    def admit_row(self, row, enc, enc_mask, prompt, prompt_mask, max_length=0, sample=True):
        # the oracle loop of a request is the same in the streaming and the non-streaming run of a test: computed once
        key = (self.kind, max_length or self.gp["max_length"], self.gp.get("min_new_tokens", 0), enc.numpy().tobytes(), prompt.numpy().tobytes())
        if key in _TRACES:
            assert self.full[row] is None
            self.full[row], self.cur[row] = _TRACES[key], 2
            self.log.append(("admit", row, self.steps))
            return
        super().admit_row(row, enc, enc_mask, prompt, prompt_mask, max_length, sample)
        _TRACES[key] = self.full[row]

    def ids_buffer(self):
        return self, 0


class OracleStreamCodec:
    """``DACModel.stream_open / stream_reset / stream_decode`` with the semantics of ptts_dac_stream_decode, on the oracle codec."""

    def __init__(self, dac):
        self.dac, self.calls, self.resets = dac, [], []

    def stream_open(self, slots, cap_frames, window_frames):
        self.table, self.cap, self.window = StreamTableModel(slots, K, 1024), cap_frames, window_frames

    def stream_reset(self, slot):
        self.table.reset(slot)
        self.resets.append(slot)

    def stream_decode(self, ids, ids_ld, rows, halo, col0=0, delay=0):
        eng = ids
        self.table.check(rows, self.cap)

        def frames_of(slot, f0, f1):
            assert col0 + f1 - 1 + (K - 1) * delay < eng.cur[slot], "a column the slot has not written yet"
            return np.stack([eng.full[slot][k, col0 + f0 + k * delay: col0 + f1 + k * delay].numpy() for k in range(K)])

        res = self.table.decode(frames_of, rows, halo)
        wave = torch.zeros(len(rows), HOP * max(1, max(e for e, _, _, _ in res)))
        for r, (emit, kept, skip, win) in enumerate(res):
            if emit > 0:
                assert win.shape[1] <= self.window, "a window longer than the codec engine was sized for"
                w = self.dac.decode(torch.from_numpy(win)[None])[0, 0]
                wave[r, : emit * HOP] = w[skip * HOP: (skip + emit) * HOP]
        self.calls.append((eng.steps, list(rows), [e for e, _, _, _ in res]))
        return wave, torch.tensor([[e, k] for e, k, _, _ in res], dtype=torch.int32)


def _model(kind="clean"):
    """clean: the EOS row and the 63 padding-id rows of every head are zero (tests/cases.py::tiny_model). drops: only the EOS row is zero -
    random heads then emit padding ids all the time, and every frame that holds one is dropped (scattered runs). alldrop: those rows x 8 -
    no frame survives. eos: the EOS row x 6, the parametrisation of tests/test_continuous_scheduler_cpu.py (on these inputs all nine codebooks
    rarely get to EOS). eosrow: every head keeps ONE row, the same EOS row, and the final layer norm's bias is shifted a little along it: every
    request ends on EOS, a few columns after min_new_tokens or later, as its own hidden states decide (tests/test_continuous_streaming_gpu.py)."""
    from transformers import T5Config

    torch.manual_seed(0)
    t5 = T5Config(vocab_size=128, d_model=128, d_kv=32, d_ff=256, num_layers=2, num_heads=4, feed_forward_proj="gated-gelu")
    dec = P.ParlerTTSDecoderConfig(vocab_size=1088, max_position_embeddings=256, num_hidden_layers=2, ffn_dim=256, num_attention_heads=2,
                                   hidden_size=128, num_codebooks=9, pad_token_id=1024, eos_token_id=1024, bos_token_id=1025)
    m = P.ParlerTTSForConditionalGeneration(P.ParlerTTSConfig.from_sub_models_config(t5, P.DACConfig(latent_dim=64, decoder_dim=256, decoder_rates=[4, 2, 2, 2]),
                                                                                    dec, vocab_size=128))
    spec, sd = DO.TINY, DO.make_decoder_weights(DO.TINY, seed=1237)
    for k in range(9):
        w = sd[f"lm_heads.{k}.weight"]
        if kind == "eos":
            w[1024] *= 6.0
        elif kind == "eosrow":
            row = sd["lm_heads.0.weight"][1024].clone()
            w.zero_()
            w[1024] = row
        elif kind == "clean":
            w[1024:] = 0.0
        else:
            w[1024] = 0.0
            if kind == "alldrop":
                w[1025:] *= 8.0
    if kind == "eosrow":
        sd["model.decoder.layer_norm.bias"] = sd["model.decoder.layer_norm.bias"] + 0.02 * row / row.pow(2).sum()
    m.decoder.load_state_dict(sd, strict=False)
    eng = StreamSessionEngine(spec, sd, kind)
    m._get_engine = lambda B, N, Pp, L, T=0: eng
    dac = DA.DacOracle(DA.DAC_TINY, DA.make_dac_weights(DA.DAC_TINY, seed=4321))
    kept_of = []

    def decode_filtered(audio_codes):  # ptts_dac_compact_codes + ptts_dac_decode_ragged semantics on the oracle codec
        codes = audio_codes[0].cpu()
        B, _, T = codes.shape
        out, frames = torch.zeros(B, 1, HOP * T), torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            ok = ((codes[b] >= 1024) | (codes[b] < 0)).sum(dim=0) == 0
            n = int(ok.sum())
            frames[b] = n
            kept_of.append((n, int((codes[b, 0] != 1024).sum())))
            if n:
                out[b, 0, :HOP * n] = dac.decode(codes[b:b + 1, :, ok])[0, 0]
        return out, frames

    codec = OracleStreamCodec(dac)
    ae = m.audio_encoder
    ae.decode_filtered, ae.stream_open, ae.stream_reset, ae.stream_decode = decode_filtered, codec.stream_open, codec.stream_reset, codec.stream_decode
    return m, eng, codec, kept_of


def _requests(lengths, seed, N=9, Pw=5):
    g = torch.Generator().manual_seed(seed)
    return [dict(input_ids=torch.randint(3, 128, (N - i % 4,), generator=g), prompt_input_ids=torch.randint(3, 128, (1, Pw - i % 3), generator=g), max_new_tokens=n)
            for i, n in enumerate(lengths)]


KW = dict(max_description_tokens=9, max_prompt_tokens=5, do_sample=False)
LENGTHS = [70, 10, 16, 120, 15, 17, 64, 90]  # 2K - 1 = 17 columns = 16 new tokens: both sides of it, and long ones


def _both(kind, lengths, slots, chunk, first=None, min_new=None, poll_steps=16, seed=1):
    """The same requests through the non-streaming and the streaming batcher on the same stand-ins."""
    mx = max(lengths)
    min_new = mx if min_new is None else min_new
    reqs = _requests(lengths, seed)
    m, eng, codec, kept_of = _model(kind)
    ref = P.ContinuousBatcher(m, slots=slots, poll_steps=poll_steps, max_new_tokens=mx, min_new_tokens=min_new, **KW).run(reqs)
    m, eng, codec, _ = _model(kind)
    cb = P.ContinuousBatcher(m, slots=slots, poll_steps=poll_steps, max_new_tokens=mx, min_new_tokens=min_new, stream_chunk_frames=chunk,
                             stream_first_chunk_frames=first, **KW)
    tickets = [cb.submit(**r) for r in reqs]
    got = [(t, c, last, eng.steps) for t, c, last in cb.chunks()]
    return reqs, ref, tickets, got, eng, codec, kept_of, cb


def _check_stream(ref, tickets, got, chunk, first):
    by = {t: [] for t in tickets}
    closed = set()
    for t, c, last, _ in got:
        assert t not in closed, f"a chunk of ticket {t} after its last one"
        assert c.dim() == 1 and c.dtype == torch.float32
        by[t].append(c)
        if last:
            closed.add(t)
        else:
            assert c.shape[0] >= HOP * (first if len(by[t]) == 1 else chunk), (t, c.shape)  # every non-last chunk holds >= chunk kept frames
            assert c.shape[0] > 0
    assert closed == set(tickets)  # `last` exactly once per ticket
    for t, (wav, n) in zip(tickets, ref):
        w = torch.cat(by[t])
        assert w.shape[0] == n == wav.shape[0], (t, w.shape, n)
        # windowed oracle decodes against one whole decode: the atol of the same comparison in tests/test_generate_glue_cpu.py (streamer chunks
        # vs the full waveform, 1e-5 - torch's CPU convolutions sum in a length-dependent order), and the GPU bar of the entry points
        assert torch.allclose(w, wav, atol=1e-5), (t, float((w - wav).abs().max()))
    return by


@pytest.mark.parametrize("kind,min_new,slots,chunk,first", [("clean", None, 3, 10, 6), ("drops", None, 3, 8, 8), ("eos", 3, 2, 7, 5), ("eosrow", 3, 2, 7, 5), ("clean", None, 1, 30, None)])
def test_chunks_concatenate_to_the_non_streaming_result(kind, min_new, slots, chunk, first):
    reqs, ref, tickets, got, eng, codec, kept_of, cb = _both(kind, LENGTHS, slots, chunk, first, min_new)
    by = _check_stream(ref, tickets, got, chunk, first or chunk)
    assert cb.pending() == 0 and all(f is None for f in eng.full)
    assert sorted(codec.resets) == sorted(s for k, s, _ in eng.log if k == "admit")  # stream_reset goes with every admission
    if kind == "clean":
        assert [n for _, n in ref] == [HOP * (L if L + 1 < 2 * K - 1 else L + 1 - K) for L in LENGTHS]
        assert max(len(by[t]) for t in tickets) >= 3  # a long request came in several pieces
    if kind == "drops":  # a condition on the input: every chunk window holds dropped frames
        long_ = [(n // HOP, L + 1 - K) for (_, n), L in zip(ref, LENGTHS) if L >= 60]
        share = sum(k for k, _ in long_) / sum(f for _, f in long_)
        assert 0.2 <= share <= 0.9, share
        assert any(k < f for k, f in long_)
    finals = sum(1 for _, rows, _ in codec.calls for r in rows if r[2])  # requests flushed out of the stream table; the others took the whole-utterance path
    if kind in ("clean", "drops"):  # EOS blocked: a request of L + 1 >= 2K - 1 columns is flushed out of the table, a shorter one is not
        assert finals == sum(1 for L in LENGTHS if L + 1 >= 2 * K - 1) and 0 < finals < len(LENGTHS)
    if kind == "eosrow":  # every long request ended on EOS, long before its max_length; both paths occur
        admit = [st for k, s, st in eng.log if k == "admit"]
        slot_ticket, took, i = {}, {}, 0
        for k, s, st in eng.log:
            if k == "admit":
                slot_ticket[s], i = i, i + 1
            else:
                took[slot_ticket[s]] = st - admit[slot_ticket[s]]
        assert all(took[t] < L - 1 for t, L in enumerate(LENGTHS) if L >= 60), took
        assert 0 < finals < len(LENGTHS)


def test_a_request_without_any_kept_frame_delivers_the_single_zero_sample_as_its_last_chunk():
    reqs, ref, tickets, got, eng, codec, kept_of, cb = _both("alldrop", [40, 12, 30], 2, 6)
    assert [n for _, n in ref] == [1, 1, 1], "the model is meant to drop every frame"
    assert sorted((t, tuple(c.shape), float(c.abs().sum()), last) for t, c, last, _ in got) == [(t, (1,), 0.0, True) for t in range(3)]


def test_first_chunk_arrives_at_the_step_the_rule_predicts_and_before_the_end():
    """Clean model, EOS blocked: request i is admitted at step a_i with 2 columns and gains one per step. Its first chunk needs
    first_chunk + halo kept frames, i.e. first_chunk + halo + K columns, cut short only by the request's own end at max_length columns (or,
    below 2K - 1 columns, always the end): step a_i + min(first_chunk + halo + K, L_i) - 2 - although poll_steps = 16 divides none of them."""
    first, chunk = 6, 20
    lengths = [70, 10, 120, 45, 30, 90, 41, 64]
    reqs, ref, tickets, got, eng, codec, kept_of, cb = _both("clean", lengths, 3, chunk, first)
    _check_stream(ref, tickets, got, chunk, first)
    admit = [st for k, s, st in eng.log if k == "admit"]  # FIFO: the i-th admission is ticket i
    end = {}
    slot_ticket, i = {}, 0
    for k, s, st in eng.log:
        if k == "admit":
            slot_ticket[s] = i
            i += 1
        else:
            end[slot_ticket[s]] = st
    first_at = {}
    for t, c, last, step in got:
        first_at.setdefault(t, step)
    streamed = 0
    for t, n in enumerate(lengths):
        L = n + 1
        assert end[t] == admit[t] + L - 2
        assert first_at[t] == admit[t] + min(first + HALO + K, L) - 2, (t, first_at[t], admit[t], L)
        if L > first + HALO + K:
            assert first_at[t] < end[t]  # streaming really streams
            streamed += 1
    assert streamed >= 4


def test_slots_due_at_one_poll_share_one_codec_pass():
    reqs, ref, tickets, got, eng, codec, kept_of, cb = _both("clean", [80, 80, 80], 3, 10)
    _check_stream(ref, tickets, got, 10, 10)
    assert all(len(rows) == 3 and sorted(r[0] for r in rows) == [0, 1, 2] for _, rows, _ in codec.calls)  # always together, never one pass per slot
    assert len(codec.calls) <= eng.polls and len({st for st, _, _ in codec.calls}) == len(codec.calls)  # at most one pass per poll
    assert cb.codec_passes == len(codec.calls) and cb.codec_rows == 3 * len(codec.calls)


def test_cancel_of_a_queued_and_of_a_running_ticket():
    lengths = [100, 100, 60, 50]
    m, eng, codec, _ = _model("clean")
    ref = P.ContinuousBatcher(m, slots=2, max_new_tokens=100, min_new_tokens=100, **KW).run(_requests(lengths, 5))
    m, eng, codec, _ = _model("clean")
    cb = P.ContinuousBatcher(m, slots=2, max_new_tokens=100, min_new_tokens=100, stream_chunk_frames=10, **KW)
    tickets = [cb.submit(**r) for r in _requests(lengths, 5)]
    assert cb.cancel(2) and cb.pending() == 3  # queued: dropped before it ever runs
    assert not cb.cancel(17)
    seen, cancelled_at = [], None
    for t, c, last in cb.chunks():
        seen.append((t, c, last))
        if t == 1 and cancelled_at is None:  # ticket 1 is running in slot 1 and has just delivered its first chunk
            assert cb.cancel(1)
            cancelled_at = len(seen)
    assert cancelled_at is not None
    assert all(t != 1 for t, _, _ in seen[cancelled_at:]) and all(t != 2 for t, _, _ in seen)
    assert not any(last for t, _, last in seen if t == 1)
    for t in (0, 3):  # the others are unaffected
        w = torch.cat([c for tt, c, _ in seen if tt == t])
        assert torch.allclose(w, ref[t][0], atol=1e-5) and [last for tt, _, last in seen if tt == t][-1]
    admits = [(s, st) for k, s, st in eng.log if k == "admit"]
    assert [s for s, _ in admits] == [0, 1, 1]  # ticket 3 was admitted into the slot the cancelled ticket left
    retire1 = [st for k, s, st in eng.log if k == "retire" and s == 1][0]
    assert admits[2][1] == retire1 < 99  # ... at once, long before ticket 1 would have ended
    assert not cb.cancel(0)  # finished


def test_mode_errors():
    m, eng, codec, _ = _model("clean")
    cb = P.ContinuousBatcher(m, slots=2, max_new_tokens=20, **KW)
    with pytest.raises(RuntimeError, match="stream_chunk_frames"):
        next(cb.chunks())
    st = P.ContinuousBatcher(m, slots=2, max_new_tokens=20, stream_chunk_frames=5, **KW)
    with pytest.raises(RuntimeError, match=r"chunks\(\)"):
        next(iter(st))
    with pytest.raises(RuntimeError, match=r"chunks\(\)"):
        st.run(_requests([12], 1))
    st.close()
    with pytest.raises(NotImplementedError):
        P.ContinuousBatcher(m, slots=2, max_new_tokens=20, stream_chunk_frames=5, streamer=object(), **KW)
    with pytest.raises(ValueError, match="stream_chunk_frames"):
        P.ContinuousBatcher(m, slots=2, max_new_tokens=20, stream_first_chunk_frames=5, **KW)
    with pytest.raises(ValueError, match=">= 1"):
        P.ContinuousBatcher(m, slots=2, max_new_tokens=20, stream_chunk_frames=0, **KW)


def test_a_replaced_codec_engine_is_noticed():
    """The stream table lives in one codec engine; DACModel._get_engine replaces the engine when a later call needs more capacity. Chosen
    behaviour: stream_reset / stream_decode raise until stream_open is called again (nothing is re-opened or restarted silently)."""
    from parler_tts_amd.dac_wrapper.modeling_dac import DACModel

    class FakeEngine:
        def __init__(self):
            self.opened, self.passes = [], 0

        def stream_open(self, slots, cap):
            self.opened.append((slots, cap))

        def stream_reset(self, slot):
            pass

        def stream_decode(self, ids, ids_ld, rows, halo, col0=0, delay=0):
            self.passes += 1
            return "wave", "out"

    dm = DACModel(P.DACConfig(latent_dim=64, decoder_dim=256, decoder_rates=[4, 2, 2, 2]))
    with pytest.raises(RuntimeError, match="stream_open first"):
        dm.stream_decode(0, 0, [(0, 1, 0, 1)], 26)
    first, second = FakeEngine(), FakeEngine()

    def get_engine(batch, frames, need_encoder=False, whole_batch=False):
        dm._engine = first if not first.opened or frames <= 100 else second
        return dm._engine

    dm._get_engine = get_engine
    dm.stream_open(4, 300, 100)
    assert first.opened == [(4, 300)]
    assert dm.stream_decode(0, 0, [(0, 1, 0, 1)], 26) == ("wave", "out") and first.passes == 1
    dm._get_engine(1, 5000)  # e.g. a long generate() on the same model: the engine is replaced
    with pytest.raises(RuntimeError, match="replaced"):
        dm.stream_decode(0, 0, [(0, 2, 0, 1)], 26)
    with pytest.raises(RuntimeError, match="stream_open first"):
        dm.stream_reset(0)
    dm.stream_open(4, 300, 100)
    dm.stream_reset(0)


def test_header_symbols_ctypes_prototypes_and_definitions_agree_for_the_stream_functions():
    hdr = open(os.path.join(ROOT, "include", "ptts.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+PTTS_ABI_VERSION\s+8\b", hdr) and _native.ABI_VERSION == 8  # additive: the version does not move
    C = _native.C
    ctype_of = {"ptts_dac*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const int64_t*": C.c_void_p, "float*": C.c_void_p,
                "int32_t*": C.c_void_p, "const ptts_dac_stream_row*": C.POINTER(_native.PttsDacStreamRow)}
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_dac.hip")).read()
    for name in STREAM_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/ptts.h"
        assert name in _native.SYMBOLS, f"{name} missing from _native.SYMBOLS"
        res, args = _native.SYMBOLS[name]
        params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
        assert res is C.c_int and len(args) == len(params), (name, params)
        for p, a in zip(params, args):
            assert a is ctype_of[p], (name, p, a)
        d = re.search(r'extern "C" int ' + name + r"\(([^)]*)\)", src)
        assert d, f"{name} is not defined in ptts_dac.hip"
        assert [" ".join(p.split()) for p in d.group(1).split(",")] == [" ".join(p.split()) for p in m.group(1).split(",")], name
    st = re.search(r"typedef struct \{([^}]*)\}\s*ptts_dac_stream_row\s*;", code)
    assert st, "ptts_dac_stream_row is not declared"
    fields = re.findall(r"\bint32_t\s+(\w+)\s*;", st.group(1))
    assert fields == [f for f, _ in _native.PttsDacStreamRow._fields_] and all(t is C.c_int32 for _, t in _native.PttsDacStreamRow._fields_)
    assert ctypes.sizeof(_native.PttsDacStreamRow) == 4 * len(fields) == 16  # sizeof(ptts_dac_stream_row): four int32_t, no padding
