"""CPU: voice prompts per request in a continuous session - the additive C ABI of include/ptts_session_voice.h and its binding table, the
scheduler of ``ContinuousBatcher(max_voice_frames=)`` / ``submit(input_values= | decoder_input_ids=)`` on an oracle-backed session stand-in
with a ``voice`` keyword, and the restatements of tests/session_voice_model.py (the id-column writer against ``build_delay_pattern_mask``,
the per-slot tail against ``sample_loop(decoder_input_ids=)``). What the HIP session computes is covered by tests/test_session_voice_gpu.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import dac_oracle as DA
from oracle import decoder_oracle as DO

import parler_tts_amd as P
from parler_tts_amd import _native
from parler_tts_amd.modeling_parler_tts import apply_delay_pattern_mask, build_delay_pattern_mask

import session_voice_cases as VC
import session_voice_model as VM
import test_batched_admission_cpu as TB
import test_continuous_scheduler_cpu as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptts_session_voice.h")
VOICE_SYMBOLS = ("ptts_admit_row_voice", "ptts_debug_slot_voice")


# ---- the header and the binding -----------------------------------------------------------------------------------------------------------
def test_header_declarations_and_ctypes_prototypes_agree_and_ptts_h_keeps_its_46():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r'^#include "ptts.h"', hdr, flags=re.M)
    assert sorted(set(re.findall(r"\b(ptts_\w+)\s*\(", code))) == sorted(VOICE_SYMBOLS) == sorted(_native.SESSION_VOICE_SYMBOLS)
    assert not set(_native.SESSION_VOICE_SYMBOLS) & (set(_native.SYMBOLS) | set(_native.SESSION_SYMBOLS) | set(_native.SESSION_KV8_SYMBOLS))
    C = _native.C
    ctype_of = {"ptts_engine*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "const float*": C.c_void_p, "const int32_t*": C.c_void_p,
                "const int64_t*": C.c_void_p, "const ptts_gen_params*": C.POINTER(_native.PttsGenParams), "int32_t*": C.POINTER(C.c_int32)}
    for name in VOICE_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/ptts_session_voice.h"
        res, args = _native.SESSION_VOICE_SYMBOLS[name]
        params = [" ".join(re.sub(r"/\*.*?\*/", "", p).split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
        assert res is C.c_int and [ctype_of[p] for p in params] == list(args), (name, params)
    # ptts.h: the 46 declarations of ABI v8, untouched, and it does not know this header (nor does ptts_session.h)
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptts.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(ptts_\w+)\s*\(", base))) == 46 == len(_native.SYMBOLS) and _native.ABI_VERSION == 8
    assert re.search(r"#define\s+PTTS_ABI_VERSION\s+8\b", base)
    for name in ("ptts.h", "ptts_session.h", "ptts_session_kv8.h"):
        assert "ptts_session_voice" not in open(os.path.join(ROOT, "include", name)).read()
    assert '"ptts_session_voice.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()  # a change to it rebuilds the library
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read()
    for name in VOICE_SYMBOLS:
        assert re.search(r'extern "C" int ' + name + r"\(", src), f"{name} is not defined in ptts_lm.hip"


def test_library_exports_the_entry_points_and_a_null_engine_is_a_value_error():
    import __graft_entry__

    __graft_entry__.build()  # incremental; cross-compiles without a GPU
    lib = _native.load_library()
    for name in VOICE_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native.SESSION_VOICE_SYMBOLS[name][1]
    with pytest.raises(ValueError, match="null argument"):
        _native.check(lib.ptts_admit_row_voice(None, 0, None, None, None, None, None, 0, 0, 1, None, None), "ptts_admit_row_voice")
    with pytest.raises(ValueError, match="null argument"):
        _native.check(lib.ptts_debug_slot_voice(None, None, None), "ptts_debug_slot_voice")


# ---- the id-column writer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 9])
def test_the_id_column_writer_is_the_delay_pattern_over_bos_and_prefix(K):
    """K in {4, 9}, T in {1, K - 1, K, K + 2}, max_length in {T + 2, 2K - 2, 2K - 1, T + K, T + 2K + 3}: no pattern (below 2K - 1), the pad
    triangle reaching into the prefix columns (2K - 1 with T >= K - 1), one generated token (T + 2)."""
    bos, pad = 1025, 1024
    g = torch.Generator().manual_seed(K)
    seen = {"none": 0, "pad_in_prefix": 0, "one_token": 0}
    for T in (1, K - 1, K, K + 2):
        for L in (T + 2, 2 * K - 2, 2 * K - 1, T + K, T + 2 * K + 3):
            if L < T + 2:
                continue  # refused: no room for a generated token
            prefix = torch.randint(0, 1024, (K, T), generator=g)
            given = torch.cat([torch.full((K, 1), bos), prefix], dim=-1)
            delayed, pattern = build_delay_pattern_mask(given, bos, pad, L, K)
            want = pattern[:, 1:1 + T] if L >= 2 * K - 1 else prefix  # no pattern: the mask is all -1 and the ids are returned as they are
            got = VM.prefix_id_columns(prefix.numpy(), K, L, bos, pad)
            assert np.array_equal(got, want.numpy()), (K, T, L)
            assert delayed.shape[1] == T + 1 and np.array_equal(got, delayed[:, 1:].numpy()), (K, T, L)  # the columns generate() starts from
            # ... and what the model is fed through them is what it is fed through the reference's pattern
            raw = torch.cat([given[:, :1], torch.from_numpy(got)], dim=-1)
            assert torch.equal(apply_delay_pattern_mask(raw, pattern), apply_delay_pattern_mask(given, pattern)) or L < 2 * K - 1
            assert (got != -1).all()
            seen["none"] += L < 2 * K - 1
            seen["pad_in_prefix"] += L >= 2 * K - 1 and bool((got == pad).any())
            seen["one_token"] += L == T + 2
    assert all(seen.values()), seen


# ---- the per-slot tail restatement against the oracle loop -----------------------------------------------------------------------------------
def test_the_per_slot_tail_restatement_reproduces_sample_loop_with_a_prefix():
    """Slots with T in {0, 3} and their own max_length, admitted at different steps, fed the oracle's own logits: ids, clocks and the columns
    the model is fed equal ``sample_loop(decoder_input_ids=)`` on each request alone."""
    spec, sd = DO.TINY, VC.weights(eos_gain=6.0)
    K, V = spec.num_codebooks, spec.vocab_size
    plan = [(0, 0, 3, 24, 2), (1, 2, 0, 19, 0), (2, 3, 3, 12, 0)]  # slot, admission step, T, max_length, min_new_tokens of the session
    gp = DO.GenParams(max_length=24, min_new_tokens=2)
    reqs = {s: VC.request(900 + s, T) for s, _, T, _, _ in plan}
    refs = {s: VC.oracle_run(spec, sd, reqs[s], L, 2, keep_logits=True) for s, _, _, L, _ in plan}
    m = VM.VoiceTailModel(4, K, V, spec.eos_token_id, spec.pad_token_id, spec.bos_token_id, ld=40, P=VC.P)
    fed = {s: [] for s in reqs}
    nstep = {s: 0 for s in reqs}
    for step in range(40):
        lg = np.zeros((4, K, V), dtype=np.float32)
        for s, at, T, L, _ in plan:
            if step == at:
                m.admit(s, L, None if T == 0 else reqs[s][4].numpy())
        live = [s for s in reqs if (m.unfinished[s * K:(s + 1) * K] > 0).any()]
        for s in live:
            lg[s] = refs[s].step_logits[nstep[s]].numpy()
            nstep[s] += 1
        got = m.step(lg, gp)
        assert sorted(got) == sorted(live)
        for s in live:
            fed[s].append(m.fed_column(s, int(m.cur_len[s]) - 1))
    assert m.cur_len[3] == 1 and not m.unfinished[3 * K:].any()  # the idle slot
    for s, _, T, L, _ in plan:
        ref = refs[s].sequences
        n = int(m.cur_len[s])
        assert n == ref.shape[1] and np.array_equal(m.ids[s * K:(s + 1) * K, :n], ref.numpy()), s
        given = ref[:, :1] if T == 0 else torch.cat([ref[:, :1], reqs[s][4]], dim=-1)  # BOS + the un-delayed prefix
        _, pattern = DO.build_delay_pattern_mask(given, spec.bos_token_id, spec.pad_token_id, L, K)
        want = DO.apply_delay_pattern_mask(ref, pattern)
        for i, col in enumerate(fed[s]):
            assert np.array_equal(col, want[:, 1 + T + i].numpy()), (s, i)
    m.retire(0, 24)
    assert m.slot_T[0] == 0 and m.cur_len[0] == 1


# ---- the scheduler on an oracle-backed stand-in -------------------------------------------------------------------------------------------------
class VoiceSessionEngine(TB.GroupSessionEngine):
    """The stand-in with ``admit_row(..., voice=)``: the oracle loop continues the prefix (``sample_loop(decoder_input_ids=)``), the slot starts
    with 2 + T columns. ``calls`` records (slot, T or None when the keyword was absent, max_length)."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.calls, self.get_engine_args = [], []

    def admit_row(self, row, enc, enc_mask, prompt, prompt_mask, max_length=0, sample=True, **kw):
        assert set(kw) <= {"voice"}, kw
        voice = kw.get("voice")
        self.calls.append((row, None if "voice" not in kw else int(voice.shape[1]), max_length))
        if voice is None:
            return super().admit_row(row, enc, enc_mask, prompt, prompt_mask, max_length=max_length, sample=sample)
        assert voice.dtype == torch.int64 and voice.shape[0] == self.spec.num_codebooks and voice.shape[1] >= 1
        if self.full[row] is not None:
            raise ValueError(f"slot {row} still holds a request (ptts_retire_row first)")
        L = max_length or self.gp["max_length"]
        if voice.shape[1] + 2 > L:
            raise ValueError("voice prompt leaves no room")
        gp = DO.GenParams(max_length=L, min_new_tokens=self.gp.get("min_new_tokens", 0))
        with torch.no_grad():
            tr = DO.sample_loop(DO.DecoderOracle(self.spec, self.sd), enc[None].float(), enc_mask[None], None if prompt is None else prompt[None].float(),
                                None if prompt_mask is None else prompt_mask[None], gp, decoder_input_ids=voice)
        self.full[row], self.cur[row] = tr.sequences, 2 + voice.shape[1]
        self.log.append(("admit", row, self.steps))
        if not getattr(self, "_in_group", False):
            self.singles.append(row)


def _voice_model(eos_gain=None):
    m, spec, sd, dac, _, codec_groups = TS._model(eos_gain)
    eng = VoiceSessionEngine(spec, sd)

    def get_engine(*a):
        eng.get_engine_args.append(a)
        return eng

    m._get_engine = get_engine
    enc_dac = DA.DacOracle(DA.DAC_TINY, DA.make_dac_weights(DA.DAC_TINY, seed=4321, with_encoder=True))
    m.audio_encoder.encode = lambda iv, n_quantizers=None, **kw: types.SimpleNamespace(audio_codes=enc_dac.encode(iv.cpu().float(), n_quantizers)[None])
    return m, spec, sd, dac, eng, enc_dac


def _voice_requests(n, seed, with_wave=(3,)):
    """TS._requests with a voice prompt on every other request: codes [K, T] (one with a leading BOS column), or a waveform."""
    g = torch.Generator().manual_seed(seed)
    reqs = TS._requests(n, seed)
    for i, r in enumerate(reqs):
        if i % 2 == 0:
            continue
        T = [3, 8, 1, 5][(i // 2) % 4]
        if i in with_wave:
            r["input_values"] = 0.3 * torch.randn(1, 1, DA.DAC_TINY.hop_length * T - 5, generator=g)
        else:
            codes = torch.randint(0, 1024, (9, T), generator=g)
            r["decoder_input_ids"] = torch.cat([torch.full((9, 1), 1025), codes], dim=-1) if i % 4 == 1 else codes
    return reqs


def _reference(m, spec, sd, dac, enc_dac, req, N, Pw, min_new, total=None):
    """The per-request pipeline with a voice prompt: sample_loop(decoder_input_ids=) -> undelay(decoder_input_ids=) -> filter -> codec."""
    pre = None
    if "input_values" in req:
        pre = enc_dac.encode(req["input_values"], 9)[0]
    elif "decoder_input_ids" in req:
        pre = req["decoder_input_ids"]
        pre = pre[:, 1:] if bool((pre[:, 0] == 1025).all()) else pre
    if pre is None:
        return TS._reference(m, spec, sd, dac, req, N, Pw, min_new), 0
    ids = torch.zeros(1, N, dtype=torch.long); mask = torch.zeros(1, N, dtype=torch.long)
    d = req["input_ids"].reshape(-1)
    ids[0, : d.shape[0]], mask[0, : d.shape[0]] = d, 1
    pids = torch.zeros(1, Pw, dtype=torch.long); pmask = torch.zeros(1, Pw, dtype=torch.long)
    p = req["prompt_input_ids"].reshape(-1)
    pids[0, : p.shape[0]], pmask[0, : p.shape[0]] = p, 1
    T = pre.shape[1]
    with torch.no_grad():
        enc = m._encode_description(ids, mask).float()
        prompt = m.embed_prompts(pids).float()
        L = total if total is not None else req["max_new_tokens"] + 1 + T
        tr = DO.sample_loop(DO.DecoderOracle(spec, sd), enc, mask, prompt, pmask, DO.GenParams(max_length=L, min_new_tokens=min_new), decoder_input_ids=pre)
        codes = DO.valid_frames(DO.undelay(tr.sequences, spec, L, decoder_input_ids=pre)[0])
        return (dac.decode(codes[None])[0, 0] if codes.shape[1] else torch.zeros(1)), T


@pytest.mark.parametrize("eos_gain,min_new", [(None, 0), (6.0, 3)])
def test_requests_with_and_without_prompts_equal_the_per_request_pipeline(eos_gain, min_new):
    m, spec, sd, dac, eng, enc_dac = _voice_model(eos_gain)
    reqs = _voice_requests(8, seed=1)
    cb = P.ContinuousBatcher(m, slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, do_sample=False, max_new_tokens=30,
                             min_new_tokens=min_new, max_voice_frames=8)
    assert eng.get_engine_args == [(2, 9, 5, 39, 8)] and cb.max_length == 39  # max_new_tokens counts new tokens: the session grows by T_max
    out = cb.run(reqs)
    hop = DA.DAC_TINY.hop_length
    for i, (r, (wav, n)) in enumerate(zip(reqs, out)):
        ref, T = _reference(m, spec, sd, dac, enc_dac, r, 9, 5, min_new)
        assert wav.dim() == 1 and n == wav.shape[0] == ref.shape[0], (i, n, wav.shape, ref.shape)
        assert torch.allclose(wav, ref, atol=1e-6), i
        if eos_gain is None and r["max_new_tokens"] + 1 + T >= 17:  # fixed length: the waveform contains the prompt's frames
            assert n == hop * (r["max_new_tokens"] + 1 + T - 9), (i, n)
    # what reached the engine: no keyword for a request without a prompt, the un-delayed codes (BOS column stripped) and the total length otherwise
    want = [(None if i % 2 == 0 else [3, 8, 1, 5][(i // 2) % 4], r["max_new_tokens"] + 1) for i, r in enumerate(reqs)]
    assert [(T, L) for _, T, L in eng.calls] == [(T, L + (T or 0)) for T, L in want]


def test_a_session_limit_given_as_max_length_stays_the_total():
    m, spec, sd, dac, eng, enc_dac = _voice_model()
    g = torch.Generator().manual_seed(5)
    r = dict(input_ids=torch.randint(3, 128, (9,), generator=g), prompt_input_ids=torch.randint(3, 128, (5,), generator=g))
    codes = torch.randint(0, 1024, (9, 6), generator=g)
    cb = P.ContinuousBatcher(m, slots=1, max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_length=24, min_new_tokens=24, max_voice_frames=8)
    assert eng.get_engine_args == [(1, 9, 5, 24, 8)] and cb.max_length == 24
    (wav, n), (wav0, n0) = cb.run([dict(r, decoder_input_ids=codes), dict(r)])
    assert [(T, L) for _, T, L in eng.calls] == [(6, 24), (None, 24)]
    ref, _ = _reference(m, spec, sd, dac, enc_dac, dict(r, decoder_input_ids=codes), 9, 5, 24, total=24)
    assert n == ref.shape[0] == DA.DAC_TINY.hop_length * (24 - 9) == n0 and torch.allclose(wav, ref, atol=1e-6)


def test_without_max_voice_frames_the_engine_sees_the_calls_it_always_saw():
    """max_voice_frames = 0 (the default, and given as 0): four positional arguments to _get_engine and admit_row without any new keyword - the
    stand-in of tests/test_continuous_scheduler_cpu.py, which has neither, keeps working; the results are those of a batcher built without it."""
    outs = []
    for extra in ({}, {"max_voice_frames": 0}):
        m, spec, sd, dac, eng, groups = TS._model()
        seen = []
        m._get_engine = lambda B, N, Pp, L: (seen.append((B, N, Pp, L)), eng)[1]  # a fifth argument would be a TypeError
        cb = P.ContinuousBatcher(m, slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, do_sample=False, max_new_tokens=30, **extra)
        outs.append(cb.run(TS._requests(5, seed=1)))
        assert seen == [(2, 9, 5, 31)] and cb.max_length == 31
        with pytest.raises(ValueError, match="max_voice_frames"):
            cb.submit(**TS._requests(1, seed=1)[0], decoder_input_ids=torch.zeros(9, 2, dtype=torch.long))
    assert all(n0 == n1 and torch.equal(w0, w1) for (w0, n0), (w1, n1) in zip(*outs))


def test_fifo_order_and_group_splitting_around_a_voice_request():
    """admit_batch = 4 on 10 slots: the pairing of idle slots (ascending) and queued requests (FIFO) is the one without voice prompts; a voice
    request ends the group before it, goes alone through admit_row(voice=), and the next group starts behind it. admit_rows sees none."""
    m, spec, sd, dac, eng, enc_dac = _voice_model()
    reqs = TS._requests(14, seed=2)
    g = torch.Generator().manual_seed(9)
    voiced = {2: 3, 3: 5, 9: 8, 12: 1}
    for i, T in voiced.items():
        reqs[i]["decoder_input_ids"] = torch.randint(0, 1024, (9, T), generator=g)
    cb = P.ContinuousBatcher(m, slots=10, admit_batch=4, poll_steps=16, max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_new_tokens=30,
                             min_new_tokens=40, max_voice_frames=8)
    assert cb.spare == 4 and eng.get_engine_args == [(14, 9, 5, 39, 8)]
    tickets = [cb.submit(**r) for r in reqs]
    finished = [t for t, w, n in cb]
    assert sorted(finished) == tickets
    # first poll, 10 idle slots: [0, 1] | 2 | 3 | [4, 5, 6, 7] | 8 | 9 (9 alone: the voice request); nothing is admitted out of order
    assert eng.groups[:2] == [([0, 1], 0), ([4, 5, 6, 7], 0)]
    first = [(row, T) for row, T, _ in eng.calls[:10]]
    assert first == [(0, None), (1, None), (2, 3), (3, 5), (4, None), (5, None), (6, None), (7, None), (8, None), (9, 8)]
    assert eng.singles[:4] == [2, 3, 8, 9]
    # FIFO over everything: the i-th admission is the i-th submission
    assert [T for _, T, _ in eng.calls] == [voiced.get(i) for i in range(14)]
    assert [L for _, _, L in eng.calls] == [r["max_new_tokens"] + 1 + voiced.get(i, 0) for i, r in enumerate(reqs)]
    # every slot took requests only while idle, and EOS being blocked each ended exactly at its own length (columns 2 + T at admission)
    open_, order = {}, 0
    for kind, slot, step in eng.log:
        if kind == "admit":
            open_[slot] = (order, step)
            order += 1
        else:
            i, s0 = open_.pop(slot)
            assert step - s0 == reqs[i]["max_new_tokens"] - 1, (i, slot, step, s0)


def test_refusals_and_a_refused_submit_draws_no_seed():
    m, spec, sd, dac, eng, enc_dac = _voice_model()
    kw = dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, do_sample=True, max_new_tokens=20)
    ids, pids = torch.randint(3, 128, (9,)), torch.randint(3, 128, (5,))
    with pytest.raises(ValueError, match="max_voice_frames"):
        P.ContinuousBatcher(m, **kw, max_voice_frames=-1)
    for name, val in (("input_values", torch.zeros(1, 1, 64)), ("decoder_input_ids", torch.zeros(9, 3, dtype=torch.long))):
        with pytest.raises(NotImplementedError, match="submit"):  # a voice prompt belongs to a request, not to the session
            P.ContinuousBatcher(m, **kw, max_voice_frames=8, **{name: val})
    cb = P.ContinuousBatcher(m, **kw, max_voice_frames=8)
    cb.submit(ids, prompt_input_ids=pids, temperature=0.7)
    state = torch.random.get_rng_state()
    bad = [
        (dict(decoder_input_ids=torch.zeros(9, 9, dtype=torch.long)), "9 frames, the session was opened for 8"),
        (dict(decoder_input_ids=torch.zeros(8, 4, dtype=torch.long)), "9 codebooks"),
        (dict(decoder_input_ids=torch.zeros(18, 4, dtype=torch.long)), "one request at a time"),
        (dict(decoder_input_ids=torch.zeros(9, dtype=torch.long)), "9 codebooks"),
        (dict(input_values=torch.zeros(1, 1, DA.DAC_TINY.hop_length * 9)), "9 frames, the session was opened for 8"),
        (dict(input_values=torch.zeros(2, 1, DA.DAC_TINY.hop_length * 2)), "one request at a time"),
        (dict(decoder_input_ids=torch.zeros(9, 4, dtype=torch.long), max_new_tokens=0), "no room"),
        (dict(decoder_input_ids=torch.zeros(9, 4, dtype=torch.long), max_new_tokens=21), "exceeds the session's 20"),
        (dict(decoder_input_ids=torch.zeros(9, 4, dtype=torch.long), temperature=0.0), "temperature"),
    ]
    for extra, msg in bad:
        with pytest.raises(ValueError, match=msg):
            cb.submit(ids, prompt_input_ids=pids, seed=None, **{"temperature": 0.9, **extra})
        assert cb.pending() == 1 and len(cb._queue) == 1 and eng.calls == []
        assert torch.equal(state, torch.random.get_rng_state()), msg  # a refused submit draws no seed
    assert cb.submit(ids, prompt_input_ids=pids, decoder_input_ids=torch.zeros(9, 8, dtype=torch.long), max_new_tokens=20) == 1  # and takes no ticket
    # a total limit: T + 2 > max_length leaves no room
    cbt = P.ContinuousBatcher(m, slots=1, max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_length=8, max_voice_frames=8)
    with pytest.raises(ValueError, match="no room for a generated token"):
        cbt.submit(ids, prompt_input_ids=pids, decoder_input_ids=torch.zeros(9, 7, dtype=torch.long))
    assert cbt.submit(ids, prompt_input_ids=pids, decoder_input_ids=torch.zeros(9, 6, dtype=torch.long)) == 0
    # streaming: a voice prompt is refused at submit, a request without one is not
    ms, *_ = _voice_model()
    ms.audio_encoder.stream_open = lambda *a, **k: None
    cbs = P.ContinuousBatcher(ms, slots=2, max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_new_tokens=20, max_voice_frames=8,
                              stream_chunk_frames=4)
    with pytest.raises(NotImplementedError, match="streaming"):
        cbs.submit(ids, prompt_input_ids=pids, decoder_input_ids=torch.zeros(9, 4, dtype=torch.long))
    assert cbs.submit(ids, prompt_input_ids=pids) == 0
