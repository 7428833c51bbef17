"""Measurements behind DESIGN.md §6.1 "streaming a request that carries a voice prompt" (profiles/continuous_streaming_voice.txt).

    python tools/stream_voice_bench.py pass [--tree DIR] [--passes 200]
        One ptts_dac_stream_decode pass over 32 plain slots on the 44.1 kHz bf16 codec, every slot gaining 43 frames per pass (HIP events
        around each pass; median, min .. max of one process). Uses only the entry points of include/ptts.h, so `--tree DIR` can point at a
        checkout of another commit (its own parler_tts_amd and library) to compare in alternating processes.
    python tools/stream_voice_bench.py ttfc [--frames 43,430] [--repeats 3]
        Mini-v1 bf16, 32 slots, chunks of 43 frames: 31 requests without a prompt are decoding when a request with a T-frame prompt arrives;
        time from its admission (the call of admit_row) to its first chunk with stream_voice_prompts "emit" and "skip", and to its whole
        waveform in a non-streaming session.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, CHUNK = 32, 43


def stream_pass(tree, passes):
    sys.path.insert(0, tree)
    from parler_tts_amd.engine import DacEngine
    from parler_tts_amd.streamer import receptive_halo_frames
    from parler_tts_amd.synthetic import random_dac_state_dict

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    halo = receptive_halo_frames((8, 8, 4, 2))
    cap = 2 * halo + CHUNK * (passes + 4)
    dac = DacEngine(max_batch=SLOTS, max_frames=2 * halo + 2 * CHUNK, compute_dtype=torch.bfloat16)
    dac.load_state_dict({k: v.to(dev) for k, v in random_dac_state_dict(seed=4321).items()})
    codes = torch.randint(0, 1024, (SLOTS, 9, cap), generator=torch.Generator().manual_seed(3)).to(dev)
    dac.stream_open(SLOTS, cap)
    for s in range(SLOTS):
        dac.stream_reset(s)
    complete = halo
    times = []
    for i in range(passes + 3):
        complete += CHUNK
        rows = [(s, complete, 0, CHUNK) for s in range(SLOTS)]
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        wave, out = dac.stream_decode(codes, None, rows, halo)
        ev1.record()
        ev1.synchronize()
        if i >= 3:
            times.append(ev0.elapsed_time(ev1) * 1e3)
            assert int(out[0, 0]) == CHUNK
    res = {"tree": tree, "passes": passes, "median_us": statistics.median(times), "min_us": min(times), "max_us": max(times)}
    print(f"[stream pass] {SLOTS} plain slots x {CHUNK} frames, 44.1 kHz bf16, {passes} passes: median {res['median_us']:.1f} us "
          f"({res['min_us']:.1f} .. {res['max_us']:.1f})  [{tree}]")
    print(json.dumps(res), flush=True)


def ttfc(frames_list, repeats):
    sys.path.insert(0, ROOT)
    import bench
    import parler_tts_amd as P

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = bench.build_model_on_device(dev, torch.bfloat16, "mini")
    K = bench.K_CODEBOOKS
    g = torch.Generator().manual_seed(7)
    desc = torch.randint(3, 32100, (SLOTS, bench.N_DESC), generator=g)
    prompt = torch.randint(3, 32100, (SLOTS, bench.N_PROMPT), generator=g)
    desc[:, -1], prompt[:, -1] = 1, 1
    desc, prompt = desc.to(dev), prompt.to(dev)
    long_new, voice_new = 600 + K - 1, 200 + K - 1
    res = {}
    for T in frames_list:
        codes = torch.randint(0, 1024, (K, T), generator=g).to(dev)
        for mode in ("emit", "skip", None):
            took = []
            for _ in range(repeats + 1):
                kw = dict(stream_chunk_frames=CHUNK, stream_voice_prompts=mode) if mode else {}
                cb = P.ContinuousBatcher(model, slots=SLOTS, max_description_tokens=bench.N_DESC, max_prompt_tokens=bench.N_PROMPT, poll_steps=16, do_sample=False,
                                         max_new_tokens=long_new, min_new_tokens=long_new, max_voice_frames=T, **kw)
                admitted, real = {}, cb.eng.admit_row

                def admit_row(*a, **k):
                    if "voice" in k:
                        torch.cuda.synchronize()
                        admitted["t"] = time.perf_counter()
                    return real(*a, **k)

                cb.eng.admit_row = admit_row
                for i in range(SLOTS - 1):
                    cb.submit(desc[i], prompt_input_ids=prompt[i], max_new_tokens=long_new)
                first = None
                with torch.no_grad():
                    for _ in range(8):  # the others have been decoding (and streaming) for 8 polls when the voice request arrives
                        cb._poll()
                    voice_ticket = cb.submit(desc[-1], prompt_input_ids=prompt[-1], max_new_tokens=voice_new, decoder_input_ids=codes)
                    for t, w, _ in (cb.chunks() if mode else iter(cb)):
                        if t == voice_ticket:
                            torch.cuda.synchronize()
                            first = time.perf_counter()
                            break
                cb.eng.admit_row = real
                cb.close()
                took.append((first - admitted["t"]) * 1e3)
            took = took[1:]  # the first run of a configuration warms graphs and allocations up
            label = f"T={T} " + (f"stream {mode}: admission -> first chunk" if mode else "not streaming: admission -> whole waveform")
            res[f"{T}_{mode}"] = took
            print(f"[ttfc] {label}: median {statistics.median(took):.1f} ms ({min(took):.1f} .. {max(took):.1f})", flush=True)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["pass", "ttfc"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--frames", default="43,430")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.what == "pass":
        stream_pass(os.path.abspath(a.tree), a.passes)
    else:
        ttfc([int(x) for x in a.frames.split(",")], a.repeats)


if __name__ == "__main__":
    main()
