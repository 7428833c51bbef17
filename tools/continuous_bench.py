#!/usr/bin/env python
"""Continuous batching against static batching on a request stream of mixed lengths (Mini-v1 shapes, bf16, synthetic weights).

  python tools/continuous_bench.py [--repeats 5] [--static-only] [--per-request] [--stream [--stream-chunks 43,86]]
                                   [--admit-batch 4,8 [--slots 64] [--burst-only]] [--kv8 [--slots 32,64,128] [--cache bf16|kv8]]
                                   [--voice [--voice-frames 43] [--voice-share 0.5]] [--out FILE]

256 requests whose lengths come from a fixed seeded list (uniform 150..860 frames, set through per-request max_new_tokens; EOS is blocked,
so lengths are exact), 32 slots. Reports
  (a) static   : model.generate() on consecutive groups of 32 in arrival order (every group runs to its longest request); audio-s/s counts the
                 frames that were ASKED for, not the padding a static batch generates beyond them
  (b) batcher  : parler_tts_amd.ContinuousBatcher on the same list
  (c) ideal    : sum over groups of (32 x the group's longest) / sum of lengths - the ratio (b)/(a) would reach with free admissions, a session
                 step as fast as the static one and no codec / encoder time
  (d) step time: one decode step of a session with 32 live slots, and with 16 live + 16 idle slots, against the static batch-32 step, at the
                 same context
  (e) admission: GPU time of one ptts_admit_row while the other slots hold live requests
A and B alternate inside one process after every graph has been warmed; medians and the observed spread are printed. --static-only runs (a)
and the static step of (d) alone (it needs nothing of the session interface, so it also runs on a tree without it).

--per-request adds (p): the batcher of (b) with every second request carrying its own sampler record (ptts_admit_row_gen) - alternately a greedy
one and a sampled one with a seed (temperature 0.7, top-k 50), min_new_tokens as the session's so that lengths stay exact - alternating with (b).

--stream measures the streaming mode instead of (a), (d), (e): (b) and the streaming batcher (`stream_chunk_frames`) alternate on the same list;
per chunk size it reports audio-s/s next to (b), the codec passes and the mean rows per pass, and per request the host time from its admission
and from its submission to its first chunk (p50 / p90 / max), next to admission -> whole waveform of the non-streaming batcher.

--admit-batch N[,M..] measures group admissions (ptts_admit_rows) instead of (a), (d), (e): (b) and the batcher with `admit_batch=N` alternate on
the same list (--slots sets the slot count of both); per N it reports audio-s/s next to (b), the total time in admissions (one run with a sync around
each phase) and the groups formed, and
  (g) group    : GPU time of one admission of n requests into n retired slots beside the other live slots, as ONE ptts_admit_rows and as n
                 ptts_admit_row
  (u) burst    : wall time from the first admission of a full session until every slot holds its first token, with one ptts_row_state after the
                 admissions - in groups of n, and one by one (n = 1)
--burst-only runs (g) and (u) alone (a short run, e.g. under a kernel trace).

--kv8 measures the session on the e4m3 self-attention cache (model.enable_fp8_kv_cache(): ptts_session_begin_kv8) instead of (a), (d), (e): per
slot count of --slots (a comma list here, e.g. 32,64,128) first the bf16-cache session, then the kv8 session, each after its own warm run (the
model keeps ONE decoder engine per cache mode, so the two cannot alternate inside a process; alternate processes with --cache bf16 / --cache kv8
for that), and every figure of the kv8 session beside the bf16-cache figure of the same run (--kv8-aggregate LABEL=FILE ... then gives medians with
min .. max over the saved reports of such processes): (b) audio-s/s on the request list, (d) the step
time with every slot live, (e) one admission and (g) one ptts_admit_rows of 8 beside the other live slots, and the K/V arena bytes per slot.

--voice measures voice prompts per request (ContinuousBatcher(max_voice_frames=T), ptts_admit_row_voice) instead of (a), (d), (e): (b) and the
batcher in which a seeded share (--voice-share) of the requests carries a prompt of T = --voice-frames frames alternate on the same list; it
reports requests per second and audio-s/s with the prompt's frames NOT counted (a request still generates the frames it was asked for, behind
its prompt), and
  (w) voice admission: GPU time of one ptts_admit_row_voice beside the other live slots at T = 43 and T = 430 (P + 1 + T positions in one
                 prefill pass), next to the plain admission of the same session."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (model shapes, synthetic inputs, HIP event timer)

SLOTS, N_REQ, FRAMES_LO, FRAMES_HI, LIST_SEED = 32, 256, 150, 860, 20240
K = bench.K_CODEBOOKS
SEC_PER_FRAME = 512 / 44100.0


def request_frames():
    g = torch.Generator().manual_seed(LIST_SEED)
    return [int(x) for x in torch.randint(FRAMES_LO, FRAMES_HI + 1, (N_REQ,), generator=g)]


def ideal_ratio(frames):
    groups = [frames[i:i + SLOTS] for i in range(0, len(frames), SLOTS)]
    return sum(SLOTS * max(g) for g in groups) / sum(frames)


def schedule_steps(frames):
    """(static, continuous) decode steps of the two schedules on this list, from the list alone: a static group runs max + K - 1 columns behind
    its prefill's first token; the FIFO slot schedule is simulated with every slot refilled the step its request ends (its drain at the end of
    the list, when nothing is left to admit, included)."""
    cols = [f + K - 1 for f in frames]  # columns to generate; the first comes with the prefill / admission
    static = sum(max(cols[i:i + SLOTS]) - 1 for i in range(0, len(cols), SLOTS))
    queue, left, steps = list(cols), [0] * SLOTS, 0
    while queue or any(left):
        for s in range(SLOTS):
            if left[s] == 0 and queue:
                left[s] = queue.pop(0) - 1
        n = min(x for x in left if x > 0) if any(left) else 0
        steps += n
        left = [max(0, x - n) for x in left]
    return static, steps


def inputs(device):
    g = torch.Generator().manual_seed(7)
    desc = torch.randint(3, 32100, (N_REQ, bench.N_DESC), generator=g)
    desc[:, -1] = 1
    prompt = torch.randint(3, 32100, (N_REQ, bench.N_PROMPT), generator=g)
    prompt[:, -1] = 1
    return desc.to(device), prompt.to(device)


def run_static(model, desc, prompt, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(0, N_REQ, SLOTS):
        new = max(frames[i:i + SLOTS]) + K - 1
        model.generate(input_ids=desc[i:i + SLOTS], prompt_input_ids=prompt[i:i + SLOTS], do_sample=False, max_new_tokens=new, min_new_tokens=new)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def request_options(i):
    """--per-request: the sampler options of request i - none for every second one, else alternately greedy and sampled with a seed."""
    if i % 2 == 0:
        return {}
    return {"do_sample": False} if i % 4 == 1 else {"do_sample": True, "temperature": 0.7, "top_k": 50, "seed": 1000 + i}


def voice_requests(share, seed=LIST_SEED + 1):
    """--voice: which requests of the list carry a prompt - a seeded choice of about `share` of them."""
    g = torch.Generator().manual_seed(seed)
    return [bool(x) for x in torch.rand(N_REQ, generator=g) < share]


def run_batcher(model, desc, prompt, frames, per_request=False, admit_batch=1, voice=None):
    """voice: None, or (T, [request carries a prompt], codes int64 [K, T] on the device): the session is opened with max_voice_frames = T."""
    import parler_tts_amd as P

    new_max = FRAMES_HI + K - 1
    kw = {"admit_batch": admit_batch} if admit_batch > 1 else {}
    if voice is not None:
        kw["max_voice_frames"] = voice[0]
    extra = lambda i: {"decoder_input_ids": voice[2]} if voice is not None and voice[1][i] else {}
    given = lambda i: voice[0] if voice is not None and voice[1][i] else 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cb = P.ContinuousBatcher(model, slots=SLOTS, max_description_tokens=bench.N_DESC, max_prompt_tokens=bench.N_PROMPT, poll_steps=16, do_sample=False,
                             max_new_tokens=new_max, min_new_tokens=new_max, **kw)
    tickets = [cb.submit(desc[i], prompt_input_ids=prompt[i], max_new_tokens=frames[i] + K - 1, **(request_options(i) if per_request else {}), **extra(i))
               for i in range(N_REQ)]
    torch.cuda.synchronize()
    t_submit = time.perf_counter() - t0
    got = {t: n for t, w, n in cb}
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert [got[t] for t in tickets] == [(f + given(i)) * 512 for i, f in enumerate(frames)], "the batcher returned other lengths than were asked for"
    return dt, t_submit, cb.eng


def _quantiles(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[min(len(xs) - 1, int(0.9 * len(xs)))], xs[-1]


def run_latency(model, desc, prompt, frames, chunk):
    """One run with host timestamps: per request its submission, its admission (FIFO: the i-th ptts_admit_row is ticket i) and the moment its
    first audio is in the caller's hands - the first chunk (streaming, `chunk` frames) or the whole waveform (chunk None). Both modes read the
    codec's counts back before they yield, so the samples exist by then."""
    import parler_tts_amd as P

    new_max = FRAMES_HI + K - 1
    kw = {} if chunk is None else {"stream_chunk_frames": chunk}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cb = P.ContinuousBatcher(model, slots=SLOTS, max_description_tokens=bench.N_DESC, max_prompt_tokens=bench.N_PROMPT, poll_steps=16, do_sample=False,
                             max_new_tokens=new_max, min_new_tokens=new_max, **kw)
    admitted, eng, real = [], cb.eng, cb.eng.admit_row

    def admit_row(*a, **k):
        admitted.append(time.perf_counter())
        return real(*a, **k)

    eng.admit_row = admit_row
    submitted, first, samples = {}, {}, {}
    try:
        for i in range(N_REQ):
            t = cb.submit(desc[i], prompt_input_ids=prompt[i], max_new_tokens=frames[i] + K - 1)
            submitted[t] = time.perf_counter()
        if chunk is None:
            for t, w, n in cb:
                first[t], samples[t] = time.perf_counter(), n
        else:
            for t, c, last in cb.chunks():
                first.setdefault(t, time.perf_counter())
                samples[t] = samples.get(t, 0) + c.shape[0]
    finally:
        eng.admit_row = real
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert [samples[t] for t in range(N_REQ)] == [f * 512 for f in frames], "the batcher returned other lengths than were asked for"
    since_admit = [first[t] - admitted[t] for t in range(N_REQ)]
    since_submit = [first[t] - submitted[t] for t in range(N_REQ)]
    return dt, since_admit, since_submit, (getattr(cb, "codec_passes", 0), getattr(cb, "codec_rows", 0))


def stream_report(model, desc, prompt, frames, audio_s, chunks, repeats, say):
    res = {}
    run_batcher(model, desc, prompt, frames)
    for c in chunks:
        run_latency(model, desc, prompt, frames, c)  # warm: the codec engine of this window size, the stream table
    base, runs = [], {c: [] for c in chunks}
    for r in range(repeats):
        base.append(run_batcher(model, desc, prompt, frames)[0])
        for c in chunks:
            runs[c].append(run_latency(model, desc, prompt, frames, c))
        say(f"  repeat {r}: batcher {base[-1]:.3f} s, " + ", ".join(f"streaming {c} frames {runs[c][-1][0]:.3f} s" for c in chunks))
    mb, lob, hib = med_spread(base)
    say(f"(b) ContinuousBatcher: median {mb:.3f} s = {audio_s / mb:.1f} audio-s/s (spread {audio_s / hib:.1f} .. {audio_s / lob:.1f})")
    res.update(batcher_s=mb, batcher_audio_s_per_s=audio_s / mb)
    _, adm, sub, _ = run_latency(model, desc, prompt, frames, None)
    a50, a90, amax = _quantiles(adm)
    s50, s90, smax = _quantiles(sub)
    say(f"    not streaming: admission -> whole waveform p50 {a50:.3f} s, p90 {a90:.3f} s, max {amax:.3f} s; submission -> whole waveform p50 {s50:.3f} s, "
        f"p90 {s90:.3f} s, max {smax:.3f} s")
    res["whole_since_admission_s"] = [round(a50, 4), round(a90, 4), round(amax, 4)]
    for c in chunks:
        m, lo, hi = med_spread([x[0] for x in runs[c]])
        adm = [v for x in runs[c] for v in x[1]]
        sub = [v for x in runs[c] for v in x[2]]
        a50, a90, amax = _quantiles(adm)
        s50, s90, smax = _quantiles(sub)
        passes, rows = runs[c][-1][3]
        say(f"(s) streaming, chunks of {c} frames ({c * SEC_PER_FRAME:.2f} s): median {m:.3f} s = {audio_s / m:.1f} audio-s/s (spread {audio_s / hi:.1f} .. "
            f"{audio_s / lo:.1f}) = {mb / m:.3f} of (b); {passes} codec passes, {rows / max(passes, 1):.1f} rows per pass")
        say(f"    admission -> first chunk p50 {a50 * 1e3:.1f} ms, p90 {a90 * 1e3:.1f} ms, max {amax * 1e3:.1f} ms; submission -> first chunk p50 {s50:.3f} s, "
            f"p90 {s90:.3f} s, max {smax:.3f} s (all {N_REQ} requests are submitted up front: this one is queueing time)")
        res[f"stream{c}"] = {"s": m, "audio_s_per_s": audio_s / m, "of_b": mb / m, "passes": passes, "rows_per_pass": rows / max(passes, 1),
                             "first_since_admission_ms": [round(a50 * 1e3, 2), round(a90 * 1e3, 2), round(amax * 1e3, 2)]}
    return res


def batcher_breakdown(model, desc, prompt, frames, admit_batch=1):
    """One extra run with a device synchronisation around each phase (so phases no longer overlap host work: an attribution, not a throughput)."""
    import parler_tts_amd as P

    new_max = FRAMES_HI + K - 1
    kw = {"admit_batch": admit_batch} if admit_batch > 1 else {}
    cb = P.ContinuousBatcher(model, slots=SLOTS, max_description_tokens=bench.N_DESC, max_prompt_tokens=bench.N_PROMPT, poll_steps=16, do_sample=False,
                             max_new_tokens=new_max, min_new_tokens=new_max, **kw)
    acc = {"admit": 0.0, "steps": 0.0, "poll": 0.0, "ids+retire": 0.0, "codec": 0.0}
    count = {k: 0 for k in acc}

    def timed(key, fn):
        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            acc[key] += time.perf_counter() - t
            count[key] += 1
            return out
        return wrapper

    eng = cb.eng
    saved = (eng.admit_row, eng.decode_steps, eng.row_state, eng.row_ids)
    eng.admit_row, eng.decode_steps = timed("admit", eng.admit_row), timed("steps", eng.decode_steps)
    if admit_batch > 1:
        eng.admit_rows = timed("admit", eng.admit_rows)
    eng.row_state, eng.row_ids = timed("poll", eng.row_state), timed("ids+retire", eng.row_ids)
    cb._decode_group = timed("codec", cb._decode_group)
    try:
        for i in range(N_REQ):
            cb.submit(desc[i], prompt_input_ids=prompt[i], max_new_tokens=frames[i] + K - 1)
        t0 = time.perf_counter()
        for _ in cb:
            pass
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        eng.admit_row, eng.decode_steps, eng.row_state, eng.row_ids = saved
        eng.__dict__.pop("admit_rows", None)
    if admit_batch > 1:
        count["groups"] = list(cb.admission_groups)
    return total, acc, count


class Events:
    def __init__(self):
        self.hip = bench.hip_event_timer()
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        self.hip.hipEventCreate(C.byref(self.e0)); self.hip.hipEventCreate(C.byref(self.e1))

    def ms(self, fn):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.hip.hipEventRecord(self.e0, st)
        fn()
        self.hip.hipEventRecord(self.e1, st)
        self.hip.hipEventSynchronize(self.e1)
        out = C.c_float()
        self.hip.hipEventElapsedTime(C.byref(out), self.e0, self.e1)
        return out.value


WARM_STEPS, TIMED_STEPS = 200, 200  # context ~ 33 + 2 + 200 .. + 400: the same 64-position buckets on both sides


def step_static(model, enc, pr, ev):
    eng = model._get_engine(SLOTS, bench.N_DESC, bench.N_PROMPT, bench.NEW_TOKENS + 1)
    eng.set_gen_params(max_length=bench.NEW_TOKENS + 1, min_new_tokens=bench.NEW_TOKENS)
    eng.prefill(enc[:SLOTS], None, pr[:SLOTS], None, sample=True)
    eng.decode_steps(WARM_STEPS)
    return ev.ms(lambda: eng.decode_steps(TIMED_STEPS)) / TIMED_STEPS


def begin_session(eng):
    """The session of SLOTS slots on whichever self-attention cache the engine was created with."""
    eng.begin_session(SLOTS, bench.N_DESC, bench.N_PROMPT, **({"kv_fp8": True} if eng.kv_fp8 else {}))


def step_session(model, enc, pr, ev, live):
    eng = model._get_engine(SLOTS, bench.N_DESC, bench.N_PROMPT, bench.NEW_TOKENS + 1)
    eng.set_gen_params(max_length=bench.NEW_TOKENS + 1, min_new_tokens=bench.NEW_TOKENS)
    begin_session(eng)
    for s in range(live):
        eng.admit_row(s, enc[s], None, pr[s], None)
    eng.decode_steps(WARM_STEPS)
    step = ev.ms(lambda: eng.decode_steps(TIMED_STEPS)) / TIMED_STEPS
    admit = None
    if live == SLOTS:  # one admission with the 31 other slots live: retire a slot, then time its re-admission
        eng.retire_row(5)
        admit = ev.ms(lambda: eng.admit_row(5, enc[40], None, pr[40], None))
    return step, admit


def group_admission(model, enc, pr, ev, n):
    """(g): every slot live, then slots 5 .. 5 + n - 1 retired and re-admitted - as one ptts_admit_rows, and one by one. GPU time, ms."""
    import parler_tts_amd as P

    spare = P.ContinuousBatcher.spare_rows(SLOTS, n)
    eng = model._get_engine(SLOTS + spare, bench.N_DESC, bench.N_PROMPT, bench.NEW_TOKENS + 1)
    eng.set_gen_params(max_length=bench.NEW_TOKENS + 1, min_new_tokens=bench.NEW_TOKENS)
    begin_session(eng)
    for s in range(SLOTS):
        eng.admit_row(s, enc[s], None, pr[s], None)
    eng.decode_steps(WARM_STEPS)
    rows = list(range(5, 5 + spare))
    out = []
    for grouped in (True, False):
        for s in rows:
            eng.retire_row(s)
        if grouped:
            out.append(ev.ms(lambda: eng.admit_rows(rows, enc[8:8 + spare], None, pr[8:8 + spare], None)))
        else:
            out.append(ev.ms(lambda: [eng.admit_row(s, enc[8 + j], None, pr[8 + j], None) for j, s in enumerate(rows)]))
        eng.decode_steps(4)
    return spare, out[0], out[1]


def burst(model, enc, pr, n):
    """(u): a full session start. Wall time from the first admission until ptts_row_state returns behind the last one, ms."""
    import parler_tts_amd as P

    spare = P.ContinuousBatcher.spare_rows(SLOTS, n)
    eng = model._get_engine(SLOTS + spare, bench.N_DESC, bench.N_PROMPT, bench.NEW_TOKENS + 1)
    eng.set_gen_params(max_length=bench.NEW_TOKENS + 1, min_new_tokens=bench.NEW_TOKENS)
    begin_session(eng)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if spare:
        for g0 in range(0, SLOTS, spare):
            g1 = min(g0 + spare, SLOTS)
            eng.admit_rows(list(range(g0, g1)), enc[g0:g1], None, pr[g0:g1], None)
    else:
        for s in range(SLOTS):
            eng.admit_row(s, enc[s], None, pr[s], None)
    cur, live = eng.row_state()
    dt = time.perf_counter() - t0
    assert cur == [2] * SLOTS and all(live), "a slot is without its first token"
    return dt * 1e3


def admit_batch_report(model, desc, prompt, frames, audio_s, sizes, repeats, burst_only, say):
    res = {}
    enc = model._encode_description(desc[:max(64, SLOTS)], None).float()
    pr = model.embed_prompts(prompt[:max(64, SLOTS)]).float()
    ev = Events()
    if not burst_only:
        run_batcher(model, desc, prompt, frames)
        for n in sizes:
            run_batcher(model, desc, prompt, frames, admit_batch=n)  # warm: the engine with spare rows, its step graphs
        base, runs = [], {n: [] for n in sizes}
        for r in range(repeats):
            base.append(run_batcher(model, desc, prompt, frames)[0])
            for n in sizes:
                runs[n].append(run_batcher(model, desc, prompt, frames, admit_batch=n)[0])
            say(f"  repeat {r}: batcher {base[-1]:.3f} s, " + ", ".join(f"admit_batch {n} {runs[n][-1]:.3f} s" for n in sizes))
        mb, lob, hib = med_spread(base)
        say(f"(b) ContinuousBatcher: median {mb:.3f} s = {audio_s / mb:.1f} audio-s/s (spread {audio_s / hib:.1f} .. {audio_s / lob:.1f})")
        total, acc, count = batcher_breakdown(model, desc, prompt, frames)
        say(f"    admissions of (b), one run with a sync around each phase: {acc['admit']:.3f} s in {count['admit']} calls of {total:.3f} s")
        res.update(batcher_s=mb, batcher_audio_s_per_s=audio_s / mb, admit_s=acc["admit"])
        for n in sizes:
            m, lo, hi = med_spread(runs[n])
            total, acc, count = batcher_breakdown(model, desc, prompt, frames, admit_batch=n)
            groups = count.get("groups", [])
            say(f"(n) admit_batch {n}: median {m:.3f} s = {audio_s / m:.1f} audio-s/s (spread {audio_s / hi:.1f} .. {audio_s / lo:.1f}) = {mb / m:.3f} of (b); "
                f"admissions {acc['admit']:.3f} s in {count['admit']} calls of {total:.3f} s; {len(groups)} groups, sizes " +
                ", ".join(f"{k}: {groups.count(k)}" for k in sorted(set(groups))))
            res[f"admit_batch{n}"] = {"s": m, "audio_s_per_s": audio_s / m, "of_b": mb / m, "admit_s": acc["admit"], "admit_calls": count["admit"]}
    for r in range(2):  # the first round warms the prefill kernels of these row counts
        singles = burst(model, enc, pr, 1)
        groups = {n: burst(model, enc, pr, n) for n in sizes}
        adm = {n: group_admission(model, enc, pr, ev, n) for n in sizes}
    say(f"(u) session start, {SLOTS} slots, first admission -> every slot holds its first token: one by one {singles:.2f} ms = {SLOTS} x {singles / SLOTS:.3f} ms; " +
        "; ".join(f"in groups of {n} {groups[n]:.2f} ms ({singles / groups[n]:.2f} x)" for n in sizes))
    for n in sizes:
        spare, g, one = adm[n]
        say(f"(g) {spare} requests beside {SLOTS - spare} live slots: one ptts_admit_rows {g:.3f} ms, {spare} x ptts_admit_row {one:.3f} ms ({one / spare:.3f} ms each): "
            f"{one / g:.2f} x")
        res[f"group{n}"] = {"rows": spare, "group_ms": g, "singles_ms": one}
    res.update(burst_single_ms=singles, burst_ms={str(n): groups[n] for n in sizes})
    return res


def voice_admission(model, enc, pr, ev, T, repeats):
    """(w): every slot live, then slot 5 retired and re-admitted with a T-frame prompt (T = 0: the plain admission). GPU time, ms, per repeat."""
    eng = model._get_engine(SLOTS, bench.N_DESC, bench.N_PROMPT, bench.NEW_TOKENS + 1 + T, T)
    eng.set_gen_params(max_length=bench.NEW_TOKENS + 1 + T, min_new_tokens=bench.NEW_TOKENS)
    begin_session(eng)
    for s in range(SLOTS):
        eng.admit_row(s, enc[s], None, pr[s], None)
    eng.decode_steps(WARM_STEPS)
    codes = torch.randint(0, 1024, (K, T), generator=torch.Generator().manual_seed(T), dtype=torch.long).to(enc.device) if T else None
    out = []
    for r in range(repeats + 1):  # the first one warms the prefill kernels of this row count
        eng.retire_row(5)
        out.append(ev.ms(lambda: eng.admit_row(5, enc[40], None, pr[40], None, **({"voice": codes} if T else {}))))
        eng.decode_steps(4)
    return out[1:]


def voice_report(model, desc, prompt, frames, audio_s, T, share, repeats, say):
    res = {}
    who = voice_requests(share)
    codes = torch.randint(0, 1024, (K, T), generator=torch.Generator().manual_seed(T), dtype=torch.long).to(desc.device)
    voice = (T, who, codes)
    run_batcher(model, desc, prompt, frames)
    run_batcher(model, desc, prompt, frames, voice=voice)  # warm: the engine with P + 1 + T prefill rows, its step graphs
    base, runs = [], []
    for r in range(repeats):
        base.append(run_batcher(model, desc, prompt, frames)[0])
        runs.append(run_batcher(model, desc, prompt, frames, voice=voice)[0])
        say(f"  repeat {r}: batcher {base[-1]:.3f} s, {sum(who)} of {N_REQ} requests with a {T}-frame prompt {runs[-1]:.3f} s")
    mb, lob, hib = med_spread(base)
    say(f"(b) ContinuousBatcher: median {mb:.3f} s = {N_REQ / mb:.2f} requests/s = {audio_s / mb:.1f} audio-s/s (spread {audio_s / hib:.1f} .. {audio_s / lob:.1f})")
    m, lo, hi = med_spread(runs)
    say(f"(v) max_voice_frames {T}, {sum(who)} of {N_REQ} requests (seeded share {share}) with a {T}-frame prompt: median {m:.3f} s = {N_REQ / m:.2f} requests/s = "
        f"{audio_s / m:.1f} audio-s/s without the prompts' frames (spread {audio_s / hi:.1f} .. {audio_s / lo:.1f}) = {mb / m:.3f} of (b); with them "
        f"{(audio_s + sum(who) * T * SEC_PER_FRAME) / m:.1f}")
    res.update(batcher_s=mb, batcher_audio_s_per_s=audio_s / mb, voice_s=m, voice_audio_s_per_s=audio_s / m, voice_requests_per_s=N_REQ / m, voice_requests=sum(who))
    enc = model._encode_description(desc[:64], None).float()
    pr = model.embed_prompts(prompt[:64]).float()
    ev = Events()
    for t in (0, 43, 430):
        mm, lo, hi = med_spread(voice_admission(model, enc, pr, ev, t, repeats))
        what = "plain admission (33-position row prefill" if t == 0 else f"voice admission, T = {t} ({bench.N_PROMPT + 1 + t}-position row prefill"
        say(f"(w) one {what} + cross K/V + first token) beside {SLOTS - 1} live slots: median {mm:.3f} ms ({lo:.3f} .. {hi:.3f})")
        res[f"admit_T{t}_ms"] = mm
    return res


def arena_bytes_per_slot(eng):
    """(self, cross) K/V arena bytes one slot owns: e4m3 self rows are 64 bytes + one fp32 scale, the cross arena stays in the engine dtype."""
    c = eng.cfg
    nkv, nkc = c.num_kv_heads or c.num_heads, c.num_cross_kv_heads or c.num_heads
    return c.num_layers * 2 * nkv * c.max_ctx * (64 + 4 if eng.kv_fp8 else 128), c.num_layers * 2 * nkc * c.max_enc * 128


def kv8_report(model, desc, prompt, frames, audio_s, slot_counts, caches, repeats, say):
    res = {}
    enc = model._encode_description(desc[:max(slot_counts) + 8], None).float()
    pr = model.embed_prompts(prompt[:max(slot_counts) + 8]).float()
    ev = Events()
    for slots in slot_counts:
        globals()["SLOTS"] = slots
        got = {}
        for cache in caches:
            model.enable_fp8_kv_cache(cache == "kv8")  # drops the other mode's engine: everything below is warmed again
            run_batcher(model, desc, prompt, frames)
            runs = []
            for _ in range(repeats):
                dt, _, eng = run_batcher(model, desc, prompt, frames)  # eng: the engine the batcher's session ran on
                assert eng.kv_fp8 == (cache == "kv8"), "the batcher ran on the other cache"
                runs.append(dt)
            arena, max_ctx = arena_bytes_per_slot(eng), eng.cfg.max_ctx
            steps, adm, grp = [], [], []
            for r in range(repeats + 1):  # the first round warms the step graphs of these contexts and the prefill kernels of these row counts
                y, ad = step_session(model, enc, pr, ev, slots)
                if r:
                    steps.append(y); adm.append(ad)
            for r in range(repeats + 1):
                spare, g, one = group_admission(model, enc, pr, ev, 8)
                if r:
                    grp.append(g)
            m, lo, hi = med_spread(runs)
            got[cache] = {"s": m, "audio_s_per_s": audio_s / m, "step_us": statistics.median(steps) * 1e3, "admit_ms": statistics.median(adm),
                          "admit_rows8_ms": statistics.median(grp), "self_arena_bytes_per_slot": arena[0], "cross_arena_bytes_per_slot": arena[1]}
            of = f"median of {repeats} runs {m:.3f} s" if repeats > 1 else f"one run {m:.3f} s"
            spread = f" (spread {audio_s / hi:.1f} .. {audio_s / lo:.1f})" if repeats > 1 else ""
            say(f"[{slots} slots, {cache} cache] (b) {of} = {audio_s / m:.1f} audio-s/s{spread}; "
                f"(d) step, every slot live, context ~235..435: {got[cache]['step_us']:.1f} us; (e) one admission beside {slots - 1} live slots "
                f"{got[cache]['admit_ms']:.3f} ms; (g) one ptts_admit_rows of {spare} beside {slots - spare} live slots {got[cache]['admit_rows8_ms']:.3f} ms; "
                f"arena per slot at max_ctx {max_ctx}: self {arena[0] / 2 ** 20:.2f} MiB + cross {arena[1] / 2 ** 20:.2f} MiB")
        if len(got) == 2:
            a, b = got["bf16"], got["kv8"]
            say(f"[{slots} slots] kv8 / bf16 cache: audio-s/s {b['audio_s_per_s'] / a['audio_s_per_s']:.3f}, step {b['step_us'] / a['step_us']:.3f}, admission "
                f"{b['admit_ms'] / a['admit_ms']:.3f}, admit_rows of 8 {b['admit_rows8_ms'] / a['admit_rows8_ms']:.3f}, self arena "
                f"{b['self_arena_bytes_per_slot'] / a['self_arena_bytes_per_slot']:.3f}")
        res[str(slots)] = got
    model.enable_fp8_kv_cache(False)
    return res


KV8_LINE = (r"\[(\d+) slots, (\w+) cache\] \(b\) .*? = ([\d.]+) audio-s/s.*?context ~235\.\.435: ([\d.]+) us; \(e\) one admission beside \d+ live slots "
            r"([\d.]+) ms; \(g\) one ptts_admit_rows of \d+ beside \d+ live slots ([\d.]+) ms; arena per slot at max_ctx \d+: self ([\d.]+) MiB")


def kv8_aggregate(specs):
    """--kv8-aggregate LABEL=FILE ...: the per-process reports of --kv8 --cache X (several processes per label), as medians with min .. max per
    label and slot count. No GPU needed: it reads what the processes printed."""
    import re

    data, labels = {}, []
    for spec in specs:
        label, path = spec.split("=", 1)
        if label not in labels:
            labels.append(label)
        for m in re.finditer(KV8_LINE, open(path).read()):
            data.setdefault((label, int(m.group(1))), []).append([float(x) for x in m.groups()[2:]])
    names = (("audio-s/s", "{:.1f}"), ("step us", "{:.1f}"), ("admission ms", "{:.3f}"), ("admit_rows of 8 ms", "{:.3f}"), ("self arena MiB per slot", "{:.2f}"))
    for slots in sorted({s for _, s in data}):
        for label in labels:
            v = data.get((label, slots))
            if not v:
                continue
            cols = []
            for j, (name, fmt) in enumerate(names):
                xs = [x[j] for x in v]
                cols.append(f"{name} {fmt.format(statistics.median(xs))} ({fmt.format(min(xs))} .. {fmt.format(max(xs))})")
            print(f"[{slots} slots, {label}] {len(v)} processes: median (min .. max): " + "; ".join(cols))
        base = data.get((labels[0], slots))
        for label in labels[1:]:
            v = data.get((label, slots))
            if base and v:
                r = [statistics.median(x[j] for x in v) / statistics.median(x[j] for x in base) for j in range(4)]
                print(f"[{slots} slots] {label} / {labels[0]}: audio-s/s {r[0]:.3f}, step {r[1]:.3f}, admission {r[2]:.3f}, admit_rows of 8 {r[3]:.3f}")


def med_spread(xs):
    return statistics.median(xs), min(xs), max(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--static-only", action="store_true")
    ap.add_argument("--per-request", action="store_true", help="also measure (p): every second request with its own sampler record")
    ap.add_argument("--stream", action="store_true", help="measure the streaming mode against (b) instead of (a), (d), (e)")
    ap.add_argument("--stream-chunks", default="43,86", help="stream_chunk_frames values to measure")
    ap.add_argument("--admit-batch", default=None, help="admit_batch values to measure against single admissions, e.g. 4,8")
    ap.add_argument("--slots", default=str(SLOTS), help="slots of the session (with --admit-batch; with --kv8 a comma list, e.g. 32,64,128)")
    ap.add_argument("--kv8", action="store_true", help="measure the session on the e4m3 self-attention cache beside the bf16-cache session")
    ap.add_argument("--cache", default="both", choices=["both", "bf16", "kv8"], help="with --kv8: one side only (for alternating processes)")
    ap.add_argument("--voice", action="store_true", help="measure requests with voice prompts against (b), and one voice admission at T = 43 and 430")
    ap.add_argument("--voice-frames", type=int, default=43, help="with --voice: frames of a request's prompt (43 = 0.5 s)")
    ap.add_argument("--voice-share", type=float, default=0.5, help="with --voice: seeded share of the requests that carry a prompt")
    ap.add_argument("--burst-only", action="store_true", help="with --admit-batch: only the session start and the group admission")
    ap.add_argument("--kv8-aggregate", nargs="+", default=None, metavar="LABEL=FILE",
                    help="no measurement: medians (min .. max) per label over the saved reports of several --kv8 --cache X processes")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if a.kv8_aggregate:
        kv8_aggregate(a.kv8_aggregate)
        return
    slot_counts = [int(n) for n in a.slots.split(",")]
    if slot_counts != [SLOTS]:
        if not (a.admit_batch or a.kv8) or (len(slot_counts) > 1 and not a.kv8):
            ap.error("--slots goes with --admit-batch (one value) or --kv8 (a list)")
        globals()["SLOTS"] = slot_counts[0]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    frames = request_frames()
    audio_s = sum(frames) * SEC_PER_FRAME
    model = bench.build_model_on_device(dev, torch.bfloat16, "mini")
    desc, prompt = inputs(dev)
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)

    say(f"[continuous_bench] Mini-v1 bf16 synthetic, {N_REQ} requests of {FRAMES_LO}..{FRAMES_HI} frames (seed {LIST_SEED}: sum {sum(frames)} frames = "
        f"{audio_s:.1f} s of audio, mean {sum(frames) / N_REQ:.0f}), {SLOTS} slots; ideal ratio (c) = {ideal_ratio(frames):.3f}")
    st_steps, cb_steps = schedule_steps(frames)
    say(f"  decode steps of the schedules themselves: static {st_steps}, FIFO slots {cb_steps} (ratio {st_steps / cb_steps:.3f}: (c) less the drain of the "
        f"last requests, when nothing is left to admit)")
    if a.kv8:
        with torch.no_grad():
            res = kv8_report(model, desc, prompt, frames, audio_s, slot_counts, ["bf16", "kv8"] if a.cache == "both" else [a.cache], a.repeats, say)
        say(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.admit_batch:
        with torch.no_grad():
            res = admit_batch_report(model, desc, prompt, frames, audio_s, [int(n) for n in a.admit_batch.split(",")], a.repeats, a.burst_only, say)
        say(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.voice:
        with torch.no_grad():
            res = voice_report(model, desc, prompt, frames, audio_s, a.voice_frames, a.voice_share, a.repeats, say)
        say(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.stream:
        with torch.no_grad():
            res = stream_report(model, desc, prompt, frames, audio_s, [int(c) for c in a.stream_chunks.split(",")], a.repeats, say)
        say(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    with torch.no_grad():
        enc = model._encode_description(desc[:64], None).float()
        pr = model.embed_prompts(prompt[:64]).float()
        ev = Events()
        # warm every graph of both paths (T5 graphs at batch 32 and 1, step graphs of every context bucket, codec engines)
        run_static(model, desc, prompt, frames)
        if not a.static_only:
            run_batcher(model, desc, prompt, frames)
        per_request = a.per_request and not a.static_only
        if per_request:
            run_batcher(model, desc, prompt, frames, per_request=True)
        st, cb, sub, pr_t = [], [], [], []
        for r in range(a.repeats):
            st.append(run_static(model, desc, prompt, frames))
            if not a.static_only:
                dt, ts, _ = run_batcher(model, desc, prompt, frames)
                cb.append(dt); sub.append(ts)
            if per_request:
                pr_t.append(run_batcher(model, desc, prompt, frames, per_request=True)[0])
            say(f"  repeat {r}: static {st[-1]:.3f} s" + ("" if a.static_only else f", batcher {cb[-1]:.3f} s (of which submit / encode {sub[-1]:.3f} s)") +
                (f", per-request records {pr_t[-1]:.3f} s" if per_request else ""))
        m, lo, hi = med_spread(st)
        say(f"(a) static batching : median {m:.3f} s = {audio_s / m:.1f} audio-s/s (spread {audio_s / hi:.1f} .. {audio_s / lo:.1f})")
        res = {"static_s": m, "static_audio_s_per_s": audio_s / m, "ideal_ratio": ideal_ratio(frames)}
        if not a.static_only:
            mb, lob, hib = med_spread(cb)
            say(f"(b) ContinuousBatcher: median {mb:.3f} s = {audio_s / mb:.1f} audio-s/s (spread {audio_s / hib:.1f} .. {audio_s / lob:.1f}); "
                f"submit (256 single-description encodes + prompt embeddings) median {statistics.median(sub):.3f} s of it")
            say(f"    (b)/(a) = {m / mb:.3f} against the ideal (c) = {ideal_ratio(frames):.3f}")
            res.update(batcher_s=mb, batcher_audio_s_per_s=audio_s / mb, ratio=m / mb, submit_s=statistics.median(sub))
            if per_request:
                mp, lop, hip_ = med_spread(pr_t)
                say(f"(p) ContinuousBatcher, every second request with its own sampler record (greedy / sampled with a seed): median {mp:.3f} s = "
                    f"{audio_s / mp:.1f} audio-s/s (spread {audio_s / hip_:.1f} .. {audio_s / lop:.1f}) = {mb / mp:.3f} of (b)")
                res.update(per_request_s=mp, per_request_audio_s_per_s=audio_s / mp)
            total, acc, count = batcher_breakdown(model, desc, prompt, frames)
            say(f"    where the batcher's time goes (one run with a sync around each phase, {total:.3f} s after the submits): " +
                ", ".join(f"{k} {acc[k]:.3f} s / {count[k]} calls" for k in acc) + f", rest (Python between the calls) {total - sum(acc.values()):.3f} s")
            res["breakdown_s"] = {k: round(v, 4) for k, v in acc.items()}
        s_static, s32, s16, adm = [], [], [], []
        for r in range(a.repeats + 1):  # first round warms the step graphs of these contexts
            x = step_static(model, enc, pr, ev)
            if not a.static_only:
                y, ad = step_session(model, enc, pr, ev, SLOTS)
                z, _ = step_session(model, enc, pr, ev, SLOTS // 2)
            if r == 0:
                continue
            s_static.append(x)
            if not a.static_only:
                s32.append(y); s16.append(z); adm.append(ad)
        m, lo, hi = med_spread(s_static)
        say(f"(d) static batch-32 step, context ~235..435: median {m * 1e3:.1f} us ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")
        res["static_step_us"] = m * 1e3
        if not a.static_only:
            for name, xs, key in (("session step, 32 live slots", s32, "session32_step_us"), ("session step, 16 live + 16 idle slots", s16, "session16_step_us")):
                mm, lo, hi = med_spread(xs)
                say(f"    {name}: median {mm * 1e3:.1f} us ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")
                res[key] = mm * 1e3
            mm, lo, hi = med_spread(adm)
            say(f"(e) one admission (33-position row prefill + cross K/V + first token) beside 31 live slots: median {mm:.3f} ms ({lo:.3f} .. {hi:.3f})")
            res["admit_ms"] = mm
    say(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
