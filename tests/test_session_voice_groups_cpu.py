"""CPU: groups of voice-prompt requests in a continuous session - the additive C ABI of include/ptts_session_voice_rows.h and its binding
table (with a torch-free C client of the header), a host model of the ragged move kernels against a plain restatement, and the grouping of
``ContinuousBatcher(admit_voice_groups=True)`` on an oracle-backed session stand-in whose ``admit_rows`` takes ``voices=``. What the HIP
session computes is covered by tests/test_session_voice_groups_gpu.py."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import decoder_oracle as DO

import parler_tts_amd as P
from parler_tts_amd import _native
from parler_tts_amd.engine import DecoderEngine

import test_continuous_scheduler_cpu as TS
import test_session_voice_cpu as TV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptts_session_voice_rows.h")
SYMBOL = "ptts_admit_rows_voice"


# ---- the header and the binding -----------------------------------------------------------------------------------------------------------
def test_header_declaration_and_ctypes_prototype_agree_and_abi_v8_stays():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r'^#include "ptts.h"', hdr, flags=re.M)
    assert sorted(set(re.findall(r"\b(ptts_\w+)\s*\(", code))) == [SYMBOL] == sorted(_native.SESSION_VOICE_ROWS_SYMBOLS)
    others = (set(_native.SYMBOLS) | set(_native.SESSION_SYMBOLS) | set(_native.SESSION_KV8_SYMBOLS) | set(_native.SESSION_VOICE_SYMBOLS))
    assert SYMBOL not in others
    C = _native.C
    ctype_of = {"ptts_engine*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "const float*": C.c_void_p, "const int32_t*": None,
                "const int64_t* const*": C.POINTER(C.c_void_p), "const ptts_gen_params* const*": C.POINTER(C.POINTER(_native.PttsGenParams))}
    m = re.search(r"\bint\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"{SYMBOL} is not declared in include/ptts_session_voice_rows.h"
    res, args = _native.SESSION_VOICE_ROWS_SYMBOLS[SYMBOL]
    params = [" ".join(p.split()[:-1]).replace(" *", "*") for p in m.group(1).split(",")]
    names = [p.split()[-1] for p in m.group(1).split(",")]
    assert names == ["e", "n", "rows", "enc_dev", "enc_mask_dev", "prompt_dev", "prompt_mask_dev", "codes_dev", "Ts", "max_lengths", "sample", "gps", "stream"]
    assert res is C.c_int and len(params) == len(args) == 13
    for name, p, a in zip(names, params, args):
        # host arrays of int32 are bound as typed pointers, device arrays of int32 as addresses
        want = ctype_of[p] if ctype_of[p] is not None else (C.POINTER(C.c_int32) if name in ("rows", "Ts", "max_lengths") else C.c_void_p)
        assert a is want or a == want, (name, p, a)
    # ptts.h: the 46 declarations of ABI v8, untouched; no other header knows this one
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptts.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(ptts_\w+)\s*\(", base))) == 46 == len(_native.SYMBOLS) and _native.ABI_VERSION == 8
    assert re.search(r"#define\s+PTTS_ABI_VERSION\s+8\b", base)
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "ptts_session_voice_rows.h":
            assert "ptts_session_voice_rows" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert '"ptts_session_voice_rows.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()  # a change to it rebuilds the library
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm.hip")).read()
    assert re.search(r'extern "C" int ' + SYMBOL + r"\(", src)


def test_library_exports_the_entry_point_and_a_null_engine_is_a_value_error():
    import __graft_entry__

    __graft_entry__.build()  # incremental; cross-compiles without a GPU
    lib = _native.load_library()
    fn = getattr(lib, SYMBOL)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native.SESSION_VOICE_ROWS_SYMBOLS[SYMBOL][1]
    with pytest.raises(ValueError, match="null engine"):
        _native.check(fn(None, 1, None, None, None, None, None, None, None, None, 1, None, None), SYMBOL)


def test_a_torch_free_c_client_compiles_against_the_header(tmp_path):
    """C99 and C++17, warnings as errors: the header stands on ptts.h alone, and a client that fills the two host arrays the call adds
    (device pointers per request, frames per request) type-checks against the declaration."""
    gcc, gxx = shutil.which("gcc") or shutil.which("cc"), shutil.which("g++") or shutil.which("c++")
    if not gcc or not gxx:
        pytest.skip("no host C / C++ compiler")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER])
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", HEADER])
    src = tmp_path / "client.c"
    src.write_text('#include <stddef.h>\n#include "ptts.h"\n#include "ptts_session_voice_rows.h"\n'
                   "int admit_two(ptts_engine* e, const float* enc, const float* prompt, const int64_t* a, const int64_t* b, void* stream) {\n"
                   "  const int32_t rows[2] = {3, 0}, Ts[2] = {11, 0}, Ls[2] = {24, 0};\n"
                   "  const int64_t* codes[2];\n"
                   "  codes[0] = a; codes[1] = NULL; (void)b;\n"
                   "  return ptts_admit_rows_voice(e, 2, rows, enc, NULL, prompt, NULL, codes, Ts, Ls, 1, NULL, stream);\n"
                   "}\n")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "client.o")])


# ---- the ragged move: a host model of the kernels' index arithmetic against a plain restatement -------------------------------------------------
def _move_model(arena, scales, src0, rows, self_rows, row_u, nkv, cap, threads):
    """admit_move_rows_kernel / admit_move_scales_kernel for the self arena of one layer, in units: arena [slots, nkv, cap * row_u] (K or V; both move
    alike), scales [slots, nkv, cap] or None. Request z of the launch moves self_rows[z] * row_u units per head from slot src0 + z to slot
    rows[z]; the kernels walk a flat unit index `u` with a grid stride, restated here thread for thread."""
    out, out_s = arena.copy(), None if scales is None else scales.copy()
    for z, dst in enumerate(rows):
        src, self_u = src0 + z, self_rows[z] * row_u
        su = nkv * self_u
        for tid in range(threads):
            for u in range(tid, su, threads):
                head = u // self_u
                off = u - head * self_u
                out[dst, head, off] = arena[src, head, off]
        if scales is not None:
            n = self_rows[z]
            for tid in range(256):
                for u in range(tid, nkv * n, 256):
                    head = u // n
                    off = u - head * n
                    out_s[dst, head, off] = scales[src, head, off]
    return out, out_s


@pytest.mark.parametrize("row_u", [4, 8, 16])  # 64-byte e4m3 rows, 128-byte bf16 rows, 256-byte fp32 rows in 16-byte units
def test_the_ragged_move_carries_each_requests_own_rows_and_nothing_of_the_padding(row_u):
    """P = 4, T = (11, 8, 1, 0): 16, 13, 6 and 5 positions (scale counts that are and are not multiples of four) from spare rows 12..15 to
    slots [9, 1, 4, 0], two K/V heads. Against the plain statement: slot rows[z] holds positions [0, P + 1 + T_z) of spare row 12 + z and is
    unchanged behind them; every other slot, the spare rows included, is unchanged."""
    rng = np.random.default_rng(row_u)
    slots, nkv, cap, Pw = 16, 2, 40, 4
    Ts, rows, src0 = [11, 8, 1, 0], [9, 1, 4, 0], 12
    self_rows = [Pw + 1 + t for t in Ts]
    arena = rng.integers(1, 1 << 30, size=(slots, nkv, cap * row_u))
    scales = rng.integers(1, 1 << 30, size=(slots, nkv, cap)) if row_u == 4 else None
    got, got_s = _move_model(arena, scales, src0, rows, self_rows, row_u, nkv, cap, threads=3 * 256)
    want, want_s = arena.copy(), None if scales is None else scales.copy()
    for z, dst in enumerate(rows):
        want[dst, :, : self_rows[z] * row_u] = arena[src0 + z, :, : self_rows[z] * row_u]
        if scales is not None:
            want_s[dst, :, : self_rows[z]] = scales[src0 + z, :, : self_rows[z]]
    assert np.array_equal(got, want) and (scales is None or np.array_equal(got_s, want_s))
    for z, dst in enumerate(rows):  # said once more without the model: nothing behind a request's own positions moved
        assert np.array_equal(got[dst, :, self_rows[z] * row_u:], arena[dst, :, self_rows[z] * row_u:])
        assert not np.array_equal(got[dst, :, : self_rows[z] * row_u], arena[dst, :, : self_rows[z] * row_u])
    untouched = [s for s in range(slots) if s not in rows]
    assert np.array_equal(got[untouched], arena[untouched])
    # the kernels this restates exist and take the lengths by value next to the slot list; an equal-length group runs them too: there is exactly
    # one move kernel and one scale-move kernel, and no ragged twin
    src = open(os.path.join(ROOT, "parler_tts_amd", "csrc", "ptts_lm_kernels.h")).read()
    for name in ("admit_move_rows_kernel", "admit_move_scales_kernel", "admit_voice_slots_kernel", "embed_rows_kernel", "gather_last_rows_kernel"):
        assert re.search(r"__global__ void (__launch_bounds__\(256\) )?" + name + r"\(", src), name
    assert re.search(r"int self_rows\[ADMIT_ROWS_MAX\]", src) and re.search(r"int ns\[ADMIT_ROWS_MAX\]", src)
    assert len(re.findall(r"__global__ void (?:__launch_bounds__\(\d+\) )?admit_move_rows\w*\(", src)) == 1
    assert len(re.findall(r"__global__ void (?:__launch_bounds__\(\d+\) )?admit_move_scales\w*\(", src)) == 1
    assert "_ragged_kernel" not in src


# ---- the batcher's grouping on an oracle-backed stand-in --------------------------------------------------------------------------------------
class VoiceGroupEngine(TV.VoiceSessionEngine):
    """The stand-in whose ``admit_rows`` takes ``voices=``: every request of the group is computed as ``admit_row(voice=)`` computes it.
    ``group_calls`` records (slots, T per request or None where the keyword was absent) per call; ``events`` everything in call order."""

    def __init__(self, spec, sd):
        super().__init__(spec, sd)
        self.group_calls, self.events = [], []

    def admit_row(self, row, *a, **kw):
        if not getattr(self, "_in_group", False):
            self.events.append(("admit_row", row))
        return super().admit_row(row, *a, **kw)

    def admit_rows(self, rows, enc, enc_mask, prompt, prompt_mask, max_lengths=None, sample=True, gens=None, **kw):
        assert set(kw) <= {"voices"}, kw
        rows = list(rows)
        n = len(rows)
        self.events.append(("admit_rows", tuple(rows)))
        if "voices" not in kw:
            self.group_calls.append((rows, None))
            return super().admit_rows(rows, enc, enc_mask, prompt, prompt_mask, max_lengths=max_lengths, sample=sample, gens=gens)
        voices = kw["voices"]
        assert n >= 2 and len(voices) == n and len(set(rows)) == n and all(v is not None and v.dtype == torch.int64 for v in voices)
        self.group_calls.append((rows, [int(v.shape[1]) for v in voices]))
        for r in rows:
            if not 0 <= r < self.B or self.full[r] is not None:
                raise ValueError(f"slot {r} is not an idle slot of the session")
        self._in_group = True
        try:
            for j, r in enumerate(rows):
                self.admit_row(r, enc[j], enc_mask[j], None if prompt is None else prompt[j], None if prompt_mask is None else prompt_mask[j],
                               max_length=max_lengths[j], sample=sample, voice=voices[j])
        finally:
            self._in_group = False
        self.groups.append((rows, self.steps))

    def set_history_penalty(self, *a, **k):
        self.history_penalty = a

    def set_slot_history_penalty(self, slot, *a):
        self.events.append(("pen", slot))


def _model(eos_gain=None):
    m, spec, sd, dac, _, enc_dac = TV._voice_model(eos_gain)
    eng = VoiceGroupEngine(spec, sd)
    m._get_engine = lambda *a: (eng.get_engine_args.append(a), eng)[1]
    return m, spec, sd, dac, eng, enc_dac


VOICED = {0: 3, 1: 8, 2: 1, 5: 5, 6: 8, 7: 2, 8: 4, 9: 8, 12: 1}


def _requests():
    reqs = TS._requests(14, seed=2)
    g = torch.Generator().manual_seed(9)
    for i, T in VOICED.items():
        reqs[i]["decoder_input_ids"] = torch.randint(0, 1024, (9, T), generator=g)
    return reqs


KW = dict(slots=10, admit_batch=4, poll_steps=16, max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_new_tokens=30, min_new_tokens=40,
          max_voice_frames=8)


def test_runs_by_kind_fifo_order_and_group_sizes():
    """14 requests, kinds V V V P P V V V V V | P P V P on 10 slots with 4 spare rows: the first poll pairs slots 0..9 with requests 0..9 and
    cuts [0, 1, 2] | [3, 4] | [5, 6, 7, 8] | [9]: runs of one kind, at most `spare` each, the last one alone through admit_row(voice=). The
    results are those of the per-request pipeline."""
    m, spec, sd, dac, eng, enc_dac = _model()
    reqs = _requests()
    cb = P.ContinuousBatcher(m, **KW, admit_voice_groups=True)
    assert cb.spare == 4 and cb.voice_groups and eng.get_engine_args == [(14, 9, 5, 39, 8)]
    tickets = [cb.submit(**r) for r in reqs]
    got = {t: (w, n) for t, w, n in cb}
    assert sorted(got) == tickets
    assert eng.group_calls[:3] == [([0, 1, 2], [3, 8, 1]), ([3, 4], None), ([5, 6, 7, 8], [5, 8, 2, 4])]
    assert eng.events[:4] == [("admit_rows", (0, 1, 2)), ("admit_rows", (3, 4)), ("admit_rows", (5, 6, 7, 8)), ("admit_row", 9)]
    assert eng.singles[0] == 9 and cb.admission_groups[:3] == [3, 2, 4] and cb.admissions == 14
    # FIFO over everything: the i-th admission is the i-th submission, with its own prompt length and total length
    assert [T for _, T, _ in eng.calls] == [VOICED.get(i) for i in range(14)]
    assert [L for _, _, L in eng.calls] == [r["max_new_tokens"] + 1 + VOICED.get(i, 0) for i, r in enumerate(reqs)]
    for i in (0, 3, 6, 9, 12):
        ref, T = TV._reference(m, spec, sd, dac, enc_dac, reqs[i], 9, 5, 40)
        assert got[i][1] == ref.shape[0] and torch.allclose(got[i][0], ref, atol=1e-6), i


def test_without_the_option_the_grouping_and_the_calls_are_todays():
    """The default: a voice request goes alone and admit_rows sees no `voices` keyword - the stand-in of tests/test_session_voice_cpu.py, whose
    admit_rows has none, keeps working, and the first poll is [0, 1, 2 alone] ... as that file pins it."""
    assert inspect.signature(P.ContinuousBatcher.__init__).parameters["admit_voice_groups"].default is False
    assert "voices" not in inspect.signature(TV.VoiceSessionEngine.admit_rows).parameters
    for extra in ({}, {"admit_voice_groups": False}):
        m, spec, sd, dac, eng, enc_dac = TV._voice_model()
        reqs = TS._requests(14, seed=2)
        g = torch.Generator().manual_seed(9)
        voiced = {2: 3, 3: 5, 9: 8, 12: 1}
        for i, T in voiced.items():
            reqs[i]["decoder_input_ids"] = torch.randint(0, 1024, (9, T), generator=g)
        cb = P.ContinuousBatcher(m, **KW, **extra)
        assert not cb.voice_groups
        for r in reqs:
            cb.submit(**r)
        assert len(list(cb)) == 14
        assert eng.groups[:2] == [([0, 1], 0), ([4, 5, 6, 7], 0)] and eng.singles[:4] == [2, 3, 8, 9]
        assert cb.admission_groups[:2] == [2, 4]


def test_the_option_needs_voice_room_and_spare_rows():
    m, *_ = _model()
    base = dict(slots=10, max_description_tokens=9, max_prompt_tokens=5, do_sample=False, max_new_tokens=30)
    for bad in (dict(admit_batch=4), dict(max_voice_frames=8), dict(admit_batch=1, max_voice_frames=8), dict(admit_batch=4, max_voice_frames=0)):
        with pytest.raises(ValueError, match="admit_voice_groups"):
            P.ContinuousBatcher(m, **base, **bad, admit_voice_groups=True)
    P.ContinuousBatcher(m, **base, admit_batch=2, max_voice_frames=1, admit_voice_groups=True)


def test_slot_records_come_before_the_group_and_stream_resets_behind_it():
    """Streaming with stream_voice_prompts="emit" on a model with device penalties: for the group [0, 1, 2] the requests' own penalty records
    are set first, then ONE admit_rows(voices=), then every slot's stream table is reset with its own prompt - as a lone admission does."""
    m, spec, sd, dac, eng, enc_dac = _model()
    m.device_penalties = True
    ae = m.audio_encoder
    ae.stream_open = lambda *a, **k: None
    ae.stream_reset = lambda s, **k: eng.events.append(("reset", s, None if "voice" not in k else int(k["voice"].shape[1]), k.get("emit_prompt")))
    reqs = _requests()[:5]
    reqs[1]["repetition_penalty"] = 1.3
    reqs[2]["no_repeat_ngram_size"] = 3
    reqs[4]["repetition_penalty"] = 1.1
    cb = P.ContinuousBatcher(m, **KW, admit_voice_groups=True, stream_chunk_frames=4, stream_voice_prompts="emit")
    for r in reqs:
        cb.submit(**r)
    cb._admit()
    assert eng.events == [
        ("pen", 1), ("pen", 2), ("admit_rows", (0, 1, 2)), ("reset", 0, 3, True), ("reset", 1, 8, True), ("reset", 2, 1, True),
        ("pen", 4), ("admit_rows", (3, 4)), ("reset", 3, None, None), ("reset", 4, None, None),
    ]
    assert cb.admission_groups == [3, 2] and [r.cols for r in cb._slot[:5]] == [2 + 3, 2 + 8, 2 + 1, 2, 2] and not cb._queue


# ---- DecoderEngine.admit_rows(voices=) picks the call by value ------------------------------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.calls = []

    def ptts_admit_rows(self, *a):
        self.calls.append(("ptts_admit_rows", a))
        return 0

    def ptts_admit_rows_voice(self, *a):
        self.calls.append(("ptts_admit_rows_voice", a))
        return 0


def test_admit_rows_without_voices_makes_the_call_it_always_made(monkeypatch):
    assert inspect.signature(DecoderEngine.admit_rows).parameters["voices"].default is None
    import parler_tts_amd.engine as E

    monkeypatch.setattr(E, "_stream_ptr", lambda *a, **k: ctypes.c_void_p())
    eng = DecoderEngine.__new__(DecoderEngine)
    eng.lib, eng._h, eng.device, eng.K, eng.H, eng.P, eng.session_N = _Lib(), ctypes.c_void_p(), "cpu", 9, 8, 0, 3
    enc, mask = torch.zeros(2, 3, 8), torch.ones(2, 3, dtype=torch.long)
    eng.admit_rows([1, 0], enc, mask, None, None, max_lengths=[20, 12])
    eng.admit_rows([1, 0], enc, mask, None, None, max_lengths=[20, 12], voices=None)
    eng.admit_rows([1, 0], enc, mask, None, None, max_lengths=[20, 12], voices=[None, torch.zeros(9, 0, dtype=torch.long)])
    assert [c[0] for c in eng.lib.calls] == ["ptts_admit_rows"] * 3 and all(len(c[1]) == 11 for c in eng.lib.calls)
    codes = torch.arange(45).reshape(9, 5)
    eng.admit_rows([1, 0], enc, mask, None, None, max_lengths=[20, 12], voices=[None, codes])
    name, a = eng.lib.calls[-1]
    assert name == "ptts_admit_rows_voice" and len(a) == 13 and a[1] == 2 and list(a[2]) == [1, 0]
    assert list(a[8]) == [0, 5] and list(a[9]) == [20, 12] and a[7][0] is None and a[7][1] == eng._keep_rows[0][-1].data_ptr()
    with pytest.raises(ValueError, match="voices"):
        eng.admit_rows([1, 0], enc, mask, None, None, voices=[codes])
    with pytest.raises(ValueError, match="expected"):
        eng.admit_rows([1, 0], enc, mask, None, None, voices=[codes[:4], None])
