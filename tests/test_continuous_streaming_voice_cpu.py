"""CPU: streaming requests that carry a voice prompt (``ContinuousBatcher(stream_voice_prompts=)``) WITHOUT a GPU - the additive C ABI of
include/ptts_dac_stream_voice.h and its binding table, the host model of tests/stream_voice_model.py, and the scheduler on oracle-backed
stand-ins: the session engine of tests/test_session_voice_cpu.py (``admit_row(voice=)``) plus ``ids_buffer``, and a codec stand-in with the
semantics of ``ptts_dac_stream_open_voice / _reset_voice / _decode_capped`` on the oracle codec. What the HIP entry points compute is covered
by tests/test_continuous_streaming_voice_gpu.py."""
import collections
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import dac_oracle as DA
from oracle import decoder_oracle as DO

import parler_tts_amd as P
from parler_tts_amd import _native
import session_voice_model as VM
from stream_model import StreamTableModel
from stream_voice_model import StreamVoiceTableModel
import test_continuous_scheduler_cpu as TS
import test_continuous_streaming_cpu as TC
import test_session_voice_cpu as TV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptts_dac_stream_voice.h")
VOICE_STREAM_SYMBOLS = ("ptts_dac_stream_open_voice", "ptts_dac_stream_reset_voice", "ptts_dac_stream_decode_capped")
K, HOP, HALO = 9, DA.DAC_TINY.hop_length, 26
_TRACES = {}


# ---- the header and the binding -----------------------------------------------------------------------------------------------------------
def test_header_declarations_ctypes_prototypes_and_definitions_agree():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r'^#include "ptts.h"', hdr, flags=re.M)
    assert sorted(set(re.findall(r"\b(ptts_\w+)\s*\(", code))) == sorted(VOICE_STREAM_SYMBOLS) == sorted(_native.DAC_STREAM_VOICE_SYMBOLS)
    others = set(_native.SYMBOLS) | set(_native.SESSION_SYMBOLS) | set(_native.SESSION_KV8_SYMBOLS) | set(_native.SESSION_VOICE_SYMBOLS)
    assert not set(_native.DAC_STREAM_VOICE_SYMBOLS) & others
    C = _native.C
    ctype_of = {"ptts_dac*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const int64_t*": C.c_void_p, "float*": C.c_void_p,
                "int32_t*": C.c_void_p, "const ptts_dac_stream_row*": C.POINTER(_native.PttsDacStreamRow)}
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_dac.hip")).read()
    for name in VOICE_STREAM_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/ptts_dac_stream_voice.h"
        res, args = _native.DAC_STREAM_VOICE_SYMBOLS[name]
        params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
        assert res is C.c_int and [ctype_of[p] for p in params] == list(args), (name, params)
        d = re.search(r'extern "C" int ' + name + r"\(([^)]*)\)", src)
        assert d, f"{name} is not defined in ptts_dac.hip"
        assert [" ".join(p.split()) for p in d.group(1).split(",")] == [" ".join(p.split()) for p in m.group(1).split(",")], name
    # the capped call is ptts_dac_stream_decode's argument list plus max_emit
    assert _native.DAC_STREAM_VOICE_SYMBOLS["ptts_dac_stream_decode_capped"][1] == _native.SYMBOLS["ptts_dac_stream_decode"][1] + [C.c_int32]
    # ptts.h: the 46 declarations of ABI v8, and it does not know this header
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptts.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(ptts_\w+)\s*\(", base))) == 46 == len(_native.SYMBOLS) and _native.ABI_VERSION == 8
    for name in ("ptts.h", "ptts_session.h", "ptts_session_kv8.h", "ptts_session_voice.h"):
        assert "ptts_dac_stream_voice" not in open(os.path.join(ROOT, "include", name)).read()
    assert '"ptts_dac_stream_voice.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()  # a change to it rebuilds the library


def _built_library():
    import __graft_entry__

    __graft_entry__.build()  # incremental; cross-compiles without a GPU
    return _native.load_library()


def test_library_exports_the_entry_points_and_a_null_engine_is_a_value_error():
    lib = _built_library()
    for name in VOICE_STREAM_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native.DAC_STREAM_VOICE_SYMBOLS[name][1]
    with pytest.raises(ValueError, match="null argument"):
        _native.check(lib.ptts_dac_stream_open_voice(None, 1, 1, 1, None), "ptts_dac_stream_open_voice")
    with pytest.raises(ValueError, match="null argument"):
        _native.check(lib.ptts_dac_stream_reset_voice(None, 0, None, 0, 1, None), "ptts_dac_stream_reset_voice")
    with pytest.raises(ValueError, match="null argument"):
        _native.check(lib.ptts_dac_stream_decode_capped(None, None, 1, 0, 0, None, 1, 0, None, 1, None, None, 1), "ptts_dac_stream_decode_capped")


def test_torch_free_c_client_of_the_header_builds_links_and_is_refused_with_a_message(tmp_path):
    """The header is plain C99 beside ptts.h; a client that knows nothing of torch links against the library and gets the refusals."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no host compiler")
    _built_library()
    inc = os.path.join(ROOT, "include")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    src = tmp_path / "client.c"
    src.write_text('#include <stdio.h>\n#include "ptts.h"\n#include "ptts_dac_stream_voice.h"\n'
                   "int main(void) {\n"
                   "  ptts_dac_stream_row row = {0, 1, 0, 1};\n"
                   "  int a = ptts_dac_stream_open_voice(NULL, 2, 100, 40, NULL);\n"
                   "  int b = ptts_dac_stream_reset_voice(NULL, 0, NULL, 3, 0, NULL);\n"
                   "  int c = ptts_dac_stream_decode_capped(NULL, NULL, 1, 1, 1, &row, 1, 26, NULL, 1, NULL, NULL, 40);\n"
                   '  printf("%d %d %d %s\\n", a != PTTS_OK, b != PTTS_OK, c != PTTS_OK, ptts_last_error());\n'
                   "  return 0;\n}\n")
    exe = str(tmp_path / "client")
    libdir = os.path.dirname(_native.LIB_PATH)
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    r = subprocess.run([gcc, "-std=c99", "-I", inc, str(src), "-o", exe, "-L" + libdir, "-lptts_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link," + torch_lib],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("1 1 1 ") and "null argument" in out.stdout, (out.returncode, out.stdout, out.stderr[-500:])


def test_wrappers_make_todays_calls_by_default_and_the_voice_calls_on_request():
    """DACModel.stream_open / stream_reset / stream_decode pass a new keyword to the engine only when it is given: an engine with the old
    signatures (tests/test_continuous_streaming_cpu.py's FakeEngine) keeps working."""
    from parler_tts_amd.dac_wrapper.modeling_dac import DACModel

    class OldEngine:
        def __init__(self):
            self.calls = []

        def stream_open(self, slots, cap):
            self.calls.append(("open", slots, cap))

        def stream_reset(self, slot):
            self.calls.append(("reset", slot))

        def stream_decode(self, ids, ids_ld, rows, halo, col0=0, delay=0):
            self.calls.append(("decode", col0, delay))
            return "wave", "out"

    class NewEngine(OldEngine):
        def stream_open(self, slots, cap, max_voice_frames=0):
            self.calls.append(("open", slots, cap, max_voice_frames))

        def stream_reset(self, slot, voice=None, emit_prompt=True):
            self.calls.append(("reset", slot, voice, emit_prompt))

        def stream_decode(self, ids, ids_ld, rows, halo, col0=0, delay=0, max_emit=None):
            self.calls.append(("decode", col0, delay, max_emit))
            return "wave", "out"

    for eng, new in ((OldEngine(), False), (NewEngine(), True)):
        dm = DACModel(P.DACConfig(latent_dim=64, decoder_dim=256, decoder_rates=[4, 2, 2, 2]))

        def get_engine(batch, frames, need_encoder=False, whole_batch=False, eng=eng):
            dm._engine = eng
            return eng

        dm._get_engine = get_engine
        if not new:
            dm.stream_open(4, 300, 100)
            dm.stream_reset(2)
            assert dm.stream_decode(0, 0, [(0, 1, 0, 1)], 26, col0=1, delay=1) == ("wave", "out")
            assert eng.calls == [("open", 4, 300), ("reset", 2), ("decode", 1, 1)]
        else:
            dm.stream_open(4, 300, 100, max_voice_frames=70)
            dm.stream_reset(2, voice="codes", emit_prompt=False)
            dm.stream_reset(1)
            dm.stream_decode(0, 0, [(0, 1, 0, 1)], 26, col0=1, delay=1, max_emit=40)
            dm.stream_decode(0, 0, [(0, 1, 0, 1)], 26)
            assert eng.calls == [("open", 4, 300, 70), ("reset", 2, "codes", False), ("reset", 1, None, True), ("decode", 1, 1, 40), ("decode", 0, 0, None)]


# ---- the host model -----------------------------------------------------------------------------------------------------------------------
def test_the_voice_model_without_prompt_and_cap_is_the_plain_model():
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 1100, (3, K, 200))
    frames_of = lambda s, f0, f1: codes[s, :, f0:f1]
    a, b = StreamTableModel(3, K, 1024), StreamVoiceTableModel(3, K, 1024)
    for rows in ([(0, 40, 0, 5), (1, 90, 0, 5)], [(0, 120, 0, 5), (2, 200, 1, 0)], [(0, 200, 1, 0), (1, 200, 1, 0)]):
        ra, rb = a.decode(frames_of, rows, HALO), b.decode(frames_of, rows, HALO)
        assert len(ra) == len(rb)
        for (e0, k0, s0, w0), (e1, k1, s1, w1) in zip(ra, rb):
            assert (e0, k0, s0) == (e1, k1, s1) and (w0 is None) == (w1 is None) and (w0 is None or np.array_equal(w0, w1))


@pytest.mark.parametrize("emit_prompt", [True, False])
def test_the_voice_model_two_sources_lazy_filter_cap_and_repeated_final_passes(emit_prompt):
    rng = np.random.default_rng(1)
    T, n_raw, cap = 50, 120, 30
    prefix = rng.integers(0, 1024, (K, T))
    prefix[3, 0] = 1030                      # the prompt's first frame is dropped
    prefix[5, 45:] = 1024                    # ... and its last five
    raw = rng.integers(0, 1024, (K, n_raw))
    raw[:, :T] = 7                           # the id buffer's cells below T: valid, and never to be read
    raw[2, T:T + 4] = 1025
    asked = []

    def frames_of(s, f0, f1):
        asked.append((f0, f1))
        return raw[:, f0:f1]

    m = StreamVoiceTableModel(1, K, 1024, max_voice_frames=64)
    with pytest.raises(ValueError, match="opened for"):
        m.reset(0, np.zeros((K, 65), dtype=np.int64))
    m.reset(0, prefix, emit_prompt)
    whole = np.concatenate([prefix, raw[:, T:]], axis=1)
    whole = whole[:, ((whole >= 0) & (whole < 1024)).all(axis=0)]
    kept_prompt = 44
    out, first = [], None
    for complete, final in ((30, 0), (60, 0), (n_raw, 0), (n_raw, 1), (n_raw, 1), (n_raw, 1), (n_raw, 1)):
        (emit, kept, skip, win), = m.decode(frames_of, [(0, complete, final, 5)], HALO, max_emit=cap)
        assert emit <= cap
        if emit:
            start = m.emitted[0] - emit
            first = start if first is None else first
            assert np.array_equal(win[:, skip:skip + emit], whole[:, start:start + emit])
            assert win.shape[1] == min(kept, start + emit + HALO) - max(0, start - HALO)  # halo real frames on either side where they exist
            out.append(win[:, skip:skip + emit])
        if final and m.flushed(0):
            break
    assert m.flushed(0) and m.prompt_kept[0] == kept_prompt and m.kept[0].shape[1] == whole.shape[1] == kept_prompt + n_raw - T - 4
    assert all(f0 >= T for f0, _ in asked)  # below T the prompt is the only source
    assert first == (0 if emit_prompt else kept_prompt)
    assert np.array_equal(np.concatenate(out, axis=1), whole[:, first:])
    # a request that ends with complete < T: only that part of the prompt exists
    m.reset(0, prefix, emit_prompt)
    (emit, kept, _, _), = m.decode(frames_of, [(0, 34, 1, 0)], HALO, max_emit=cap)
    assert kept == 33 and emit == (cap if emit_prompt else 0)
    # a plain request in the same slot starts clean
    m.reset(0)
    (emit, kept, _, win), = m.decode(frames_of, [(0, 40, 1, 0)], HALO, max_emit=100)
    assert (emit, kept) == (40, 40) and np.array_equal(win, raw[:, :40])


# ---- the scheduler on oracle-backed stand-ins ---------------------------------------------------------------------------------------------
class VoiceStreamEngine(TV.VoiceSessionEngine):
    """+ ``ids_buffer`` (the stand-in hands out itself as the "pointer") and one oracle loop per distinct request."""

    def admit_row(self, row, enc, enc_mask, prompt, prompt_mask, max_length=0, sample=True, **kw):
        voice = kw.get("voice")
        key = (max_length or self.gp["max_length"], self.gp.get("min_new_tokens", 0), enc.numpy().tobytes(), prompt.numpy().tobytes(),
               None if voice is None else voice.numpy().tobytes())
        if key in _TRACES:
            assert self.full[row] is None and set(kw) <= {"voice"}
            self.calls.append((row, None if "voice" not in kw else int(voice.shape[1]), max_length))
            self.full[row], self.cur[row] = _TRACES[key], 2 + (0 if voice is None else voice.shape[1])
            self.log.append(("admit", row, self.steps))
            return
        L = max_length or self.gp["max_length"]
        if voice is not None and voice.shape[1] + K > L:
            # The oracle's pattern builder, like the reference's, cannot place a prompt whose shifted rows pass max_length. Such a request has
            # max_length - K < T frames, all of them the prompt's: no generated token reaches a final frame, so the stand-in writes the given
            # columns as the engine does (tests/session_voice_model.py) and any valid token behind them.
            assert self.full[row] is None
            T = voice.shape[1]
            given = torch.from_numpy(VM.prefix_id_columns(voice.numpy(), K, L, self.spec.bos_token_id, self.spec.pad_token_id))
            self.calls.append((row, T, max_length))
            self.full[row] = torch.cat([torch.full((K, 1), self.spec.bos_token_id), given, torch.full((K, L - 1 - T), 5)], dim=-1)
            self.cur[row] = 2 + T
            self.log.append(("admit", row, self.steps))
            _TRACES[key] = self.full[row]
            return
        super().admit_row(row, enc, enc_mask, prompt, prompt_mask, max_length=max_length, sample=sample, **kw)
        _TRACES[key] = self.full[row]

    def ids_buffer(self):
        return self, 0


class OracleVoiceStreamCodec:
    """``DACModel.stream_open / stream_reset / stream_decode`` with the voice keywords, on the host model and the oracle codec. ``calls``
    records what the batcher passed, keyword for keyword."""

    def __init__(self, dac):
        self.dac, self.calls, self.resets, self.opens = dac, [], [], []

    def stream_open(self, slots, cap_frames, window_frames, **kw):
        assert set(kw) <= {"max_voice_frames"}
        self.opens.append((slots, cap_frames, window_frames, dict(kw)))
        self.table, self.cap, self.window = StreamVoiceTableModel(slots, K, 1024, kw.get("max_voice_frames", 0)), cap_frames, window_frames

    def stream_reset(self, slot, **kw):
        assert set(kw) <= {"voice", "emit_prompt"}
        voice = kw.get("voice")
        self.table.reset(slot, None if voice is None else voice.numpy(), kw.get("emit_prompt", True))
        self.resets.append((slot, None if voice is None else int(voice.shape[1]), dict((k, v) for k, v in kw.items() if k != "voice")))

    def stream_decode(self, ids, ids_ld, rows, halo, col0=0, delay=0, **kw):
        assert set(kw) <= {"max_emit"}
        eng = ids
        self.table.check(rows, self.cap)

        def frames_of(slot, f0, f1):
            assert col0 + f1 - 1 + (K - 1) * delay < eng.cur[slot], "a column the slot has not written yet"
            return np.stack([eng.full[slot][k, col0 + f0 + k * delay: col0 + f1 + k * delay].numpy() for k in range(K)])

        res = self.table.decode(frames_of, rows, halo, max_emit=kw.get("max_emit"))
        wave = torch.zeros(len(rows), HOP * max(1, max(e for e, _, _, _ in res)))
        for r, (emit, kept, skip, win) in enumerate(res):
            if emit > 0:
                assert win.shape[1] <= self.window, "a window longer than the codec engine was sized for"
                w = self.dac.decode(torch.from_numpy(win)[None])[0, 0]
                wave[r, : emit * HOP] = w[skip * HOP: (skip + emit) * HOP]
        self.calls.append((eng.steps, list(rows), [e for e, _, _, _ in res], dict(kw)))
        return wave, torch.tensor([[e, k] for e, k, _, _ in res], dtype=torch.int32)


def _model():
    m, spec, sd, dac, _, _ = TS._model()
    eng = VoiceStreamEngine(spec, sd)
    m._get_engine = lambda *a: eng
    codec = OracleVoiceStreamCodec(dac)
    ae = m.audio_encoder
    ae.stream_open, ae.stream_reset, ae.stream_decode = codec.stream_open, codec.stream_reset, codec.stream_decode
    return m, eng, codec


NEW, TMAX = 60, 150
# (T, max_new_tokens): the issue's mix - the last of them ends with max_length - K = 34 < T frames, so that only part of its prompt is ever
# final - and two prompts longer than a capped pass, one of which ends at once and is drained by repeated final passes
MIX = [(0, NEW), (1, NEW), (6, NEW), (40, NEW), (70, NEW), (40, 2), (0, 30), (150, NEW), (150, 2), (6, 4)]
KW = dict(max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_new_tokens=NEW, min_new_tokens=NEW, max_voice_frames=TMAX)
STREAM = dict(stream_chunk_frames=8, stream_first_chunk_frames=6, poll_steps=16)


def _requests(mix=MIX, seed=4):
    g = torch.Generator().manual_seed(seed)
    reqs = TC._requests([n for _, n in mix], seed)
    for r, (T, _) in zip(reqs, mix):
        if T:
            codes = torch.randint(0, 1024, (K, T), generator=g)
            if T >= 40:
                codes[int(torch.randint(0, K, (1,), generator=g)), 0] = 1030  # special ids in a prompt: its first frame ...
                codes[4, T - 3:] = 1024                                      # ... and its last three are dropped
            r["decoder_input_ids"] = codes
    return reqs


def _prompt_kept(req, frames):
    """Frames of the request's prompt in its waveform: the valid ones among the first min(T, frames)."""
    v = req.get("decoder_input_ids")
    return 0 if v is None else int(((v[:, :frames] >= 0) & (v[:, :frames] < 1024)).all(dim=0).sum())


def _run_stream(mode, slots, reqs, **extra):
    m, eng, codec = _model()
    cb = P.ContinuousBatcher(m, slots=slots, stream_voice_prompts=mode, **dict(KW, **extra), **STREAM)
    tickets = [cb.submit(**r) for r in reqs]
    by, closed = {t: [] for t in tickets}, set()
    for t, c, last in cb.chunks():
        assert t not in closed, f"a chunk of ticket {t} after its last one"
        assert c.dim() == 1 and c.dtype == torch.float32
        by[t].append(c)
        if last:
            closed.add(t)
    assert closed == set(tickets)  # `last` exactly once per ticket
    assert cb.pending() == 0 and all(f is None for f in eng.full)
    return cb, eng, codec, tickets, by


@pytest.fixture(scope="module")
def reference():
    reqs = _requests()
    m, eng, codec = _model()
    return reqs, P.ContinuousBatcher(m, slots=2, poll_steps=16, **KW).run(reqs)


@pytest.mark.parametrize("mode", ["emit", "skip"])
@pytest.mark.parametrize("slots", [2, 3])
def test_chunks_equal_the_non_streaming_waveform_or_its_tail(reference, mode, slots):
    reqs, ref = reference
    cb, eng, codec, tickets, by = _run_stream(mode, slots, reqs)
    assert cb.max_emit == cb.window_frames - 2 * HALO == 66 and codec.opens == [(slots, NEW + 1 + TMAX, cb.window_frames, {"max_voice_frames": TMAX})]
    for t, r, (T, n_new), (wav, n) in zip(tickets, reqs, MIX, ref):
        # EOS blocked and no generated frame dropped: max_length - K raw frames; below 2K - 1 columns no pattern: every column but BOS
        frames = T + n_new + 1 - K if T + n_new + 1 >= 2 * K - 1 else T + n_new
        assert n == HOP * (frames - (min(T, frames) - _prompt_kept(r, frames))), (t, n)
        w = torch.cat(by[t])
        skip = HOP * _prompt_kept(r, frames) if mode == "skip" else 0
        assert w.shape[0] == n - skip, (t, w.shape, n, skip)
        assert torch.allclose(w, wav[skip:], atol=1e-5), (t, float((w - wav[skip:]).abs().max()))  # the bar of tests/test_continuous_streaming_cpu.py
    # stream_reset follows every admission, with the request's prompt and the mode
    admits = [s for k, s, _ in eng.log if k == "admit"]
    assert [s for s, _, _ in codec.resets] == admits and len(admits) == len(MIX)
    assert [(T, kw) for _, T, kw in codec.resets] == [(T or None, {"emit_prompt": mode == "emit"} if T else {}) for T, _ in MIX]
    # every pass is capped, no window outgrew the engine (asserted in the stand-in), and the long prompts did need the cap
    assert all(kw == {"max_emit": 66} for _, _, _, kw in codec.calls)
    assert cb.whole_requests == 1  # (6, 4) ended below 2K - 1 columns: the whole-utterance path, its prompt dropped on the host in "skip"
    if mode == "emit":
        assert max(e for _, _, emits, _ in codec.calls for e in emits) == 66
        # (150, 2): 143 frames at admission (66 leave at once), one step later it has ended with 77 left: 66 + 11 in two final passes of its
        # slot at the same step, before the slot is reused
        final_passes = collections.Counter((st, r[0]) for st, rows, _, _ in codec.calls for r in rows if r[2])
        assert max(final_passes.values()) == 2
        assert len(by[tickets[8]]) >= 3 and len(by[tickets[7]]) >= 4 and len(by[tickets[4]]) >= 3
    else:  # a skipped prompt that ended before its first generated frame: an empty last chunk
        assert [tuple(c.shape) for c in by[tickets[5]]] == [(0,)] and [tuple(c.shape) for c in by[tickets[8]]] == [(0,)]


def test_a_prompt_that_is_ready_at_admission_leaves_before_any_further_step_and_a_skipped_one_does_not_delay_the_first_chunk():
    reqs = _requests([(70, NEW), (70, NEW)], seed=9)
    for mode in ("emit", "skip"):
        cb, eng, codec, tickets, by = _run_stream(mode, 1, reqs[:1])
        first_pass = codec.calls[0]
        if mode == "emit":  # 70 + 2 - K = 63 frames final at admission, 6 + 26 needed: the pass runs at step 0
            assert first_pass[0] == 0 and first_pass[2][0] > 0
        else:  # the first generated frame is frame 70: first + halo frames behind it, i.e. 70 + 6 + 26 + K columns, 2 + 70 of them given
            assert first_pass[0] == 70 + 6 + HALO + K - 72 and first_pass[2][0] >= 6


def test_a_plain_request_after_a_voice_request_in_the_same_slot_starts_clean_and_keeps_its_chunks():
    """One slot: voice, plain, voice, plain. The plain requests' chunk lengths are those of a streaming session without the option."""
    mix = [(40, 30), (0, NEW), (6, 30), (0, 40)]
    reqs = _requests(mix, seed=6)
    m, eng, codec = _model()
    ref = P.ContinuousBatcher(m, slots=1, poll_steps=16, **KW).run(reqs)
    cb, eng, codec, tickets, by = _run_stream("emit", 1, reqs)
    for t, (wav, n) in zip(tickets, ref):
        w = torch.cat(by[t])
        assert w.shape[0] == n and torch.allclose(w, wav, atol=1e-5)
    assert [T for _, T, _ in codec.resets] == [40, None, 6, None]
    m, eng, codec0 = _model()
    plain = P.ContinuousBatcher(m, slots=1, **KW, **STREAM)
    pt = [plain.submit(**reqs[i]) for i in (1, 3)]
    pby = {t: [] for t in pt}
    for t, c, last in plain.chunks():
        pby[t].append(c.shape[0])
    assert [[c.shape[0] for c in by[tickets[i]]] for i in (1, 3)] == [pby[t] for t in pt]


def test_cancel_of_a_running_voice_request():
    reqs = _requests([(70, NEW), (6, NEW), (0, 30)], seed=7)
    m, eng, codec = _model()
    cb = P.ContinuousBatcher(m, slots=1, stream_voice_prompts="emit", **KW, **STREAM)
    tickets = [cb.submit(**r) for r in reqs]
    seen, cancelled = [], False
    for t, c, last in cb.chunks():
        seen.append((t, last))
        if t == 0 and not cancelled:
            assert cb.cancel(0)
            cancelled = True
    assert [t for t, _ in seen].count(0) == 1 and not any(last for t, last in seen if t == 0)
    assert [t for t, last in seen if last] == [1, 2]
    assert [T for _, T, _ in codec.resets] == [70, 6, None]


def test_the_options_value_errors():
    m, eng, codec = _model()
    with pytest.raises(ValueError, match="stream_chunk_frames"):
        P.ContinuousBatcher(m, slots=2, stream_voice_prompts="emit", **KW)
    with pytest.raises(ValueError, match="max_voice_frames"):
        P.ContinuousBatcher(m, slots=2, stream_voice_prompts="skip", **dict(KW, max_voice_frames=0), **STREAM)
    with pytest.raises(ValueError, match="'emit' or 'skip'"):
        P.ContinuousBatcher(m, slots=2, stream_voice_prompts="drop", **KW, **STREAM)
    cb = P.ContinuousBatcher(m, slots=2, stream_voice_prompts="skip", **KW, **STREAM)
    with pytest.raises(ValueError, match="max_voice_frames"):
        cb.submit(**dict(_requests([(0, 30)])[0], decoder_input_ids=torch.zeros(K, TMAX + 1, dtype=torch.long)))


def test_without_the_option_every_call_is_todays():
    """The stand-ins of tests/test_continuous_streaming_cpu.py have the old signatures: a new keyword or argument would be a TypeError. The
    same requests through a batcher built with the option left out and with ``stream_voice_prompts=None``: the same recorded calls; and a
    voice prompt is still refused with the message that names streaming."""
    recorded = []
    for extra in ({}, {"stream_voice_prompts": None}):
        m, eng, codec, _ = TC._model("clean")
        cb = P.ContinuousBatcher(m, slots=2, max_new_tokens=70, min_new_tokens=70, stream_chunk_frames=8, stream_first_chunk_frames=6, max_voice_frames=8,
                                 **TC.KW, **extra)
        tickets = [cb.submit(**r) for r in TC._requests([70, 10, 40, 16], 3)]
        got = [(t, tuple(c.shape), last) for t, c, last in cb.chunks()]
        recorded.append((codec.calls, codec.resets, eng.log, got))
        with pytest.raises(NotImplementedError, match="streaming"):
            cb.submit(**TC._requests([20], 3)[0], decoder_input_ids=torch.zeros(K, 4, dtype=torch.long))
    assert recorded[0] == recorded[1]
    assert sorted(recorded[0][1]) == sorted(s for k, s, _ in recorded[0][2] if k == "admit")
