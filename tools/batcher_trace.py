"""What ``ContinuousBatcher`` asks of its engine and codec, and what it hands out, as one canonical text trace per session - to compare two
commits of parler_tts_amd/continuous.py on the CPU (profiles/continuous_refactor_trace.txt).

    python tools/batcher_trace.py [--tree DIR] [--out FILE]

Uses only the batcher's public API and the oracle-backed stand-ins of tests/ (``OracleSessionEngine``, ``GroupSessionEngine``,
``VoiceSessionEngine``, ``RecordingEngine``, ``StreamSessionEngine`` / ``OracleStreamCodec``, ``VoiceStreamEngine`` /
``OracleVoiceStreamCodec`` and their ``_model`` helpers), so ``--tree DIR`` can point at a checkout of another commit: its parler_tts_amd
and its tests are the ones imported. The stand-ins sit behind a recording proxy. A trace holds every call in order (method, scalar
arguments, keyword names, tensors as shape / dtype / hash of the bytes), everything the batcher yields (ticket, length or ``last``, hash
of the samples) and the counters at the end. ``torch.manual_seed`` is fixed per session; the oracle loop of a request is computed once."""
import argparse
import hashlib
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.tree)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import decoder_oracle as DO  # noqa: E402

import parler_tts_amd as P  # noqa: E402
import test_batched_admission_cpu as TB  # noqa: E402
import test_continuous_scheduler_cpu as TS  # noqa: E402
import test_continuous_streaming_cpu as TC  # noqa: E402
import test_continuous_streaming_voice_cpu as TSV  # noqa: E402
import test_per_request_sampling_scheduler_cpu as TP  # noqa: E402
import test_session_voice_cpu as TV  # noqa: E402

assert os.path.dirname(os.path.abspath(P.__file__)) == os.path.join(ROOT, "parler_tts_amd"), P.__file__


# ---- one oracle loop per distinct request (the stand-ins' own _TRACES caches cover only the streaming engines) -----------------------------
def _digest(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(b"-" if t is None else t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


_LOOPS, _sample_loop = {}, DO.sample_loop


def _cached_sample_loop(model, enc, enc_mask, prompt, prompt_mask, gp, *a, **kw):
    if a or set(kw) - {"decoder_input_ids"}:
        return _sample_loop(model, enc, enc_mask, prompt, prompt_mask, gp, *a, **kw)
    weights = _digest(*[model.w[k] for k in sorted(model.w) if "lm_heads" in k or "layer_norm" in k])
    key = (weights, repr(gp), _digest(enc, enc_mask, prompt, prompt_mask, kw.get("decoder_input_ids")))
    if key not in _LOOPS:
        _LOOPS[key] = _sample_loop(model, enc, enc_mask, prompt, prompt_mask, gp, **kw)
    return _LOOPS[key]


DO.sample_loop = _cached_sample_loop


# ---- the recording proxy ---------------------------------------------------------------------------------------------------------------------
def describe(x):
    if x is None or isinstance(x, (bool, int, float, str)):
        return repr(x)
    if isinstance(x, torch.Tensor):
        return f"T{tuple(x.shape)}:{str(x.dtype).replace('torch.', '')}:{_digest(x)}"
    if isinstance(x, (list, tuple)):
        return "[" + ", ".join(describe(v) for v in x) + "]"
    if isinstance(x, dict):
        return "{" + ", ".join(f"{k}: {describe(x[k])}" for k in sorted(x)) + "}"
    return f"<{type(x).__name__}>"


class Recorder:
    def __init__(self):
        self.lines = []

    def say(self, text):
        self.lines.append(text)

    def wrap(self, name, fn):
        def call(*a, **kw):
            self.say(f"call {name}(" + ", ".join([describe(v) for v in a] + [f"{k}={describe(kw[k])}" for k in sorted(kw)]) + ")")
            return fn(*a, **kw)
        return call


class Proxy:
    """Every method of the stand-in is recorded; its other attributes (``kv_fp8``, ``cfg``) are the stand-in's, a missing one is missing."""

    def __init__(self, target, rec, name):
        self.__dict__.update(_target=target, _rec=rec, _name=name)

    def __getattr__(self, attr):
        value = getattr(self._target, attr)
        return self._rec.wrap(f"{self._name}.{attr}", value) if callable(value) else value

    def __setattr__(self, attr, value):
        setattr(self._target, attr, value)


def instrument(m, rec):
    get_engine = m._get_engine
    m._get_engine = lambda *a, **kw: Proxy(rec.wrap("model._get_engine", get_engine)(*a, **kw), rec, "eng")
    ae = m.audio_encoder
    for name in ("stream_open", "stream_reset", "stream_decode", "decode_filtered"):
        if name in ae.__dict__:  # a stand-in: the real methods need the library
            setattr(ae, name, rec.wrap(f"codec.{name}", ae.__dict__[name]))


# ---- sessions --------------------------------------------------------------------------------------------------------------------------------
SESSIONS = []


def session(name, model, kw, requests, script=None, seed=1234):
    """model(): the ``_model`` helper's model; requests: submit()'s keywords; script(cb, i, item, tickets, say) runs behind the i-th yield
    (-1: before the first) and returns True to stop iterating."""
    def run():
        rec = Recorder()
        rec.say(f"session {name}")
        m = model()
        instrument(m, rec)
        torch.manual_seed(seed)
        cb = P.ContinuousBatcher(m, **kw)
        stream = kw.get("stream_chunk_frames") is not None
        tickets = [cb.submit(**r) for r in requests]
        rec.say(f"submitted {tickets} pending {cb.pending()}")
        stop = script(cb, -1, None, tickets, rec.say) if script else False
        if not stop:
            for i, (t, w, x) in enumerate(cb.chunks() if stream else cb):
                rec.say(f"yield ticket {t} {'last' if stream else 'length'} {x!r} {describe(w)}")
                if script and script(cb, i, (t, w, x), tickets, rec.say):
                    break
        rec.say(f"end pending {cb.pending()} " + " ".join(f"{c} {getattr(cb, c, None)!r}" for c in
                                                         ("admissions", "admission_groups", "codec_passes", "codec_rows", "whole_requests")))
        return rec.lines
    SESSIONS.append(run)


BASE = dict(max_description_tokens=9, max_prompt_tokens=5, do_sample=False)
MIXED = [24, 10, 16, 30, 15, 17, 12, 27]  # 2K - 1 = 17 columns = 16 new tokens: both sides of it
stream_model = lambda kind: (lambda: TC._model(kind)[0])
min_new = lambda kind, mx: 3 if kind in ("eos", "eosrow") else mx  # the other kinds never reach EOS: fixed lengths

# plain sessions
for kind in ("clean", "eos", "eosrow"):
    for slots in (1, 2, 3):
        for poll in (1, 4, 16):
            session(f"plain {kind} slots {slots} poll {poll}", stream_model(kind),
                    dict(BASE, slots=slots, poll_steps=poll, max_new_tokens=30, min_new_tokens=min_new(kind, 30)), TC._requests(MIXED, 1))
for gain, mn in ((None, 0), (6.0, 3)):
    session(f"plain OracleSessionEngine eos_gain {gain}", lambda gain=gain: TS._model(gain)[0],
            dict(BASE, slots=2, poll_steps=4, max_new_tokens=30, min_new_tokens=mn), TS._requests(8, seed=1))

# grouped admission
for slots in (2, 5, 9):
    for batch in (1, 2, 4):
        session(f"groups slots {slots} admit_batch {batch}", lambda: TB._model()[0],
                dict(TB.KW, slots=slots, admit_batch=batch, poll_steps=16), TS._requests(14, seed=2))
for slots in (5, 9):  # streaming: the one stand-in with admit_rows and ids_buffer is the voice one; groups end at the requests with a prompt
    session(f"groups slots {slots} admit_batch 4 streaming", lambda: TSV._model()[0],
            dict(TSV.KW, slots=slots, admit_batch=4, stream_voice_prompts="emit", **TSV.STREAM),
            TSV._requests([(0, 30), (0, 12), (0, 30), (6, 20), (0, 12), (0, 40), (0, 40), (0, 40), (0, 40), (0, 40), (40, 2), (0, 20), (0, 20), (0, 20)], seed=8))


# per-request options: records with and without seeds, in both modes
def options_model(streaming):
    def build():
        if streaming:
            m, eng0, _, _ = TC._model("clean")
            eng = TP.RecordingStreamEngine(eng0.spec, eng0.sd, "clean")
        else:
            m, spec, sd, _, _, _ = TS._model()
            eng = TP.RecordingEngine(spec, sd)
        m._get_engine = lambda B, N, Pp, L, T=0: eng
        return m
    return build


OPTIONS = [dict(temperature=0.7, seed=5), {}, dict(do_sample=False), dict(top_k=0, top_p=1.0, min_new_tokens=4, seed=2 ** 64 - 1), dict(temperature=0.9),
           dict(top_k=10), dict(do_sample=False, seed=9), dict(seed=11)]
for extra in ({}, dict(stream_chunk_frames=4)):
    session(f"options {'streaming' if extra else 'whole'}", options_model(bool(extra)),
            dict(slots=2, max_description_tokens=9, max_prompt_tokens=5, poll_steps=4, max_new_tokens=14, min_new_tokens=14, do_sample=True, temperature=0.8,
                 top_k=30, top_p=0.9, **extra), [dict(TP._req(i), **o) for i, o in enumerate(OPTIONS)])

# voice prompts, not streaming: T = 0 (no prompt, and a BOS column alone) and T = max_voice_frames = 8 among them
voiced = TV._voice_requests(8, seed=1)
voiced[2]["decoder_input_ids"] = torch.full((9, 1), 1025)
for gain, mn in ((None, 0), (6.0, 3)):
    session(f"voice eos_gain {gain}", lambda gain=gain: TV._voice_model(gain)[0],
            dict(BASE, slots=2, poll_steps=4, max_new_tokens=30, min_new_tokens=mn, max_voice_frames=8), voiced)
session("voice total max_length", lambda: TV._voice_model()[0], dict(BASE, slots=1, max_length=24, min_new_tokens=24, max_voice_frames=8),
        [dict(voiced[3], max_new_tokens=None), dict(voiced[4], max_new_tokens=None)])
grouped = TS._requests(14, seed=2)
for i, T in {2: 3, 3: 5, 9: 8, 12: 1}.items():
    grouped[i]["decoder_input_ids"] = torch.randint(0, 1024, (9, T), generator=torch.Generator().manual_seed(90 + i))
session("voice groups slots 10 admit_batch 4", lambda: TV._voice_model()[0],
        dict(BASE, slots=10, admit_batch=4, poll_steps=16, max_new_tokens=30, min_new_tokens=40, max_voice_frames=8), grouped)

# streaming
for kind in ("clean", "drops", "alldrop", "eosrow"):
    for n, (chunk, first) in enumerate(((4, 4), (8, 6), (8, 1))):
        for poll in (1, 16):
            session(f"stream {kind} chunk {chunk} first {first} poll {poll}", stream_model(kind),
                    dict(BASE, slots=2 + n % 2, poll_steps=poll, max_new_tokens=120, min_new_tokens=min_new(kind, 120), stream_chunk_frames=chunk,
                         stream_first_chunk_frames=first), TC._requests(TC.LENGTHS, 1))
session("stream clean one slot chunk 30", stream_model("clean"),
        dict(BASE, slots=1, max_new_tokens=120, min_new_tokens=120, stream_chunk_frames=30), TC._requests(TC.LENGTHS, 1))

# streamed voice prompts on the MIX of tests/test_continuous_streaming_voice_cpu.py, and the same requests not streamed
for slots in (2, 4):
    for mode in ("emit", "skip"):
        session(f"stream voice {mode} slots {slots}", lambda: TSV._model()[0], dict(TSV.KW, slots=slots, stream_voice_prompts=mode, **TSV.STREAM), TSV._requests())
session("stream voice MIX not streamed", lambda: TSV._model()[0], dict(TSV.KW, slots=2, poll_steps=16), TSV._requests())
session("stream voice skip one slot poll 1", lambda: TSV._model()[0],
        dict(TSV.KW, slots=1, stream_voice_prompts="skip", stream_chunk_frames=8, stream_first_chunk_frames=6, poll_steps=1), TSV._requests()[2:9])


# cancellation and early close, in both modes. Slots 2: ticket 0 is short and leaves first; tickets 1 then sits in slot 1, 2 and 3 are queued
def cancels(cb, i, item, tickets, say):
    if i == -1:
        say(f"cancel unknown {cb.cancel(17)!r} pending {cb.pending()}")
    elif i == 0:
        say(f"cancel queued {tickets[3]} {cb.cancel(tickets[3])!r} running {tickets[1]} {cb.cancel(tickets[1])!r} again {cb.cancel(tickets[1])!r} "
            f"pending {cb.pending()}")
    elif i == 2:
        say(f"cancel the first ticket, finished or running, {cb.cancel(tickets[0])!r} pending {cb.pending()}")


def closes(cb, i, item, tickets, say):
    if i == 1:
        cb.close()
        say(f"closed pending {cb.pending()}")
        return True


for label, script in (("cancel", cancels), ("close", closes)):
    for extra in ({}, dict(stream_chunk_frames=10), dict(stream_chunk_frames=8, stream_first_chunk_frames=1, poll_steps=1)):
        session(f"{label} {extra}", stream_model("clean"), dict(BASE, slots=2, max_new_tokens=100, min_new_tokens=100, **extra),
                TC._requests([20, 100, 60, 50, 30], 5), script)
session("cancel voice stream", lambda: TSV._model()[0], dict(TSV.KW, slots=2, stream_voice_prompts="emit", **TSV.STREAM),
        TSV._requests([(6, 4), (70, TSV.NEW), (6, TSV.NEW), (0, 30), (40, 2)], seed=7), cancels)
session("close before the first poll", stream_model("clean"), dict(BASE, slots=2, max_new_tokens=30),
        TC._requests([20, 12], 5), lambda cb, i, item, tickets, say: (cb.close(), say(f"closed pending {cb.pending()}"), True)[2])


def main():
    lines = []
    for n, run in enumerate(SESSIONS):
        got = run()
        print(f"[{n + 1}/{len(SESSIONS)}] {got[0]}: {len(got)} lines", file=sys.stderr, flush=True)
        lines += got
    text = "\n".join(lines) + "\n"
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print(f"{len(SESSIONS)} sessions, {len(lines)} trace lines, sha256 {hashlib.sha256(text.encode()).hexdigest()}", file=sys.stderr)


if __name__ == "__main__":
    main()
