#!/usr/bin/env python
"""bench.py — BASELINE.json metric on the configuration it is quoted on.

  python bench.py --gpus N --steps K --warmup W
  (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...)

A "step" is ONE pass of the hot path over one batch of synthetic input = one ``generate()`` call: T5 description
encoder (stock PyTorch-ROCm) → HIP prefill → 867 hipGraph-replayed decode steps → un-delay → HIP DAC decode, for
``--bs`` utterances of 860 frames (9.985 s of 44.1 kHz audio each; EOS suppressed: min_new_tokens = max_new_tokens
= 868). N=1 workload = BASELINE.json configs[1]: parler-tts-mini-v1 shapes, bf16, bs=1, random-init
weights (no checkpoints offline). N>1: one process per GPU, utterances sharded statically, weights broadcast once
from rank 0 over RCCL; no collective on the data path ("scaling": "weak").

One JSON line on rank 0. value = whole-job audio-seconds generated per wall-second (max over ranks). A plain run sets up,
warms up, times the --steps generate() calls and prints the line. --full adds the side measurements: roofline (decode-step
graph vs HBM), cpu_baseline (oracle port on the host cores, bounded sample), ttft_p50_ms, bs=32 / bs=128, codec, streaming,
sampling, fp32 parity mode, Large-v1. --dump-outputs DIR writes the waveform the last timed step returned (rank 0's) as
DIR/audio_values.npy (float32), for output-by-output comparison of two builds.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FRAMES = 860
K_CODEBOOKS = 9
NEW_TOKENS = FRAMES + K_CODEBOOKS - 1  # 868 forward passes
AUDIO_S = FRAMES * 512 / 44100.0       # 9.985 s per utterance
N_DESC, N_PROMPT = 64, 32


def model_config(which: str = "mini"):
    """Decoder shapes of the two released sizes; text encoder = google/flan-t5-large (training/README.md:91), so Large-v1
    (hidden 1536) carries the 1024 -> 1536 `enc_to_dec_proj` (modeling:2388-2392)."""
    import parler_tts_amd as P
    from transformers import T5Config

    t5 = T5Config(vocab_size=32128, d_model=1024, d_kv=64, d_ff=2816, num_layers=24, num_heads=16, feed_forward_proj="gated-gelu",
                  tie_word_embeddings=False)
    if which == "large":  # helpers/model_init_scripts/init_large_model.py:25-43
        dec = P.ParlerTTSDecoderConfig(vocab_size=1088, max_position_embeddings=4096, num_hidden_layers=30, ffn_dim=6144,
                                       num_attention_heads=24, num_key_value_heads=24, hidden_size=1536, num_codebooks=9, pad_token_id=1024,
                                       eos_token_id=1024, bos_token_id=1025)
    else:  # helpers/model_init_scripts/init_model_600M.py:27-44
        dec = P.ParlerTTSDecoderConfig(vocab_size=1088, max_position_embeddings=4096, num_hidden_layers=24, ffn_dim=4096,
                                       num_attention_heads=16, hidden_size=1024, num_codebooks=9, pad_token_id=1024, eos_token_id=1024,
                                       bos_token_id=1025)
    return P.ParlerTTSConfig.from_sub_models_config(t5, P.DACConfig(), dec, vocab_size=32128)


def mini_config():
    return model_config("mini")


def build_model(rank: int, world: int, device: torch.device, dtype: torch.dtype, which: str = "mini"):
    """Rank 0 draws the synthetic weights (seed 1234); other ranks allocate and receive them by RCCL broadcast."""
    import parler_tts_amd as P
    from parler_tts_amd.synthetic import random_dac_state_dict

    torch.manual_seed(1234)
    # ranks != 0 allocate without drawing (their tensors are overwritten by rank 0's broadcast: no ~25 s random init per rank, and the
    # broadcast is observable - a rank that missed it would run on whatever the allocator returned)
    model = P.ParlerTTSForConditionalGeneration(model_config(which), init_weights=(rank == 0 or world == 1))
    # A trained checkpoint never emits the 64 padding ids >= codebook_size (vocab 1088 = 1024 + 64); random LM heads would,
    # and generate() (like the reference :3627-3636) drops every frame containing one. Zero those rows so each
    # utterance decodes exactly FRAMES frames (the arithmetic per step is unchanged).
    with torch.no_grad():
        for k in range(K_CODEBOOKS):
            getattr(model.decoder.lm_heads, str(k)).weight[1024:] = 0.0
    model.audio_encoder.load_state_dict({"model." + k: v for k, v in random_dac_state_dict(seed=4321).items()})
    model = model.to(device=device, dtype=dtype)
    if world > 1:  # the ONLY collective of the path: the weights, once, rank 0 -> all
        from parler_tts_amd.distributed import broadcast_model_weights

        broadcast_model_weights(model, src=0)
    return model


def build_model_on_device(device: torch.device, dtype: torch.dtype, which: str):
    """Side measurements on other shapes (Large-v1): the same architecture allocated empty and filled ON THE GPU (N(0, 0.02) matrices,
    LayerNorm (1, 0), sinusoidal tables kept) - seconds instead of the ~40 s host-side init of 1.5 G parameters. Values do not matter
    for a step-time / throughput figure; the parity tests build their Large models from the oracle's seeded weights instead."""
    import parler_tts_amd as P
    from parler_tts_amd.synthetic import random_dac_state_dict

    model = P.ParlerTTSForConditionalGeneration(model_config(which), init_weights=False)
    model.audio_encoder.load_state_dict({"model." + k: v for k, v in random_dac_state_dict(seed=4321).items()})
    model = model.to(device=device, dtype=dtype)
    g = torch.Generator(device=device).manual_seed(1234)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "embed_positions" in name:
                continue
            if p.dim() == 1:
                p.fill_(0.0 if name.endswith("bias") else 1.0)
            else:
                p.copy_((torch.randn(p.shape, device=device, generator=g) * 0.02).to(p.dtype))
        for k in range(K_CODEBOOKS):
            getattr(model.decoder.lm_heads, str(k)).weight[1024:] = 0.0
    model._engine = None
    return model


def synthetic_batch(bs: int, rank: int, device):
    g = torch.Generator().manual_seed(1 + 1000 * rank)
    desc = torch.randint(3, 32100, (bs, N_DESC), generator=g)
    desc[:, -1] = 1  # T5 EOS
    g2 = torch.Generator().manual_seed(2 + 1000 * rank)
    prompt = torch.randint(3, 32100, (bs, N_PROMPT), generator=g2)
    prompt[:, -1] = 1
    return desc.to(device), prompt.to(device)


def hip_event_timer():
    from parler_tts_amd import _native as N

    hip = N.hip_runtime()
    for name, args in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                       ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
        getattr(hip, name).restype = C.c_int
        getattr(hip, name).argtypes = args
    return hip


def _timed_replays(eng, n: int) -> float:
    """seconds per decode-step launch: HIP events on the stream the graph is launched on, around n replays."""
    hip = hip_event_timer()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
    hip.hipEventRecord(e0, stream)
    eng.decode_steps(n)
    hip.hipEventRecord(e1, stream)
    hip.hipEventSynchronize(e1)
    ms = C.c_float()
    hip.hipEventElapsedTime(C.byref(ms), e0, e1)
    return ms.value / 1e3 / n


def _prefilled_engine(model, bs: int, device, **gen):
    desc, prompt = synthetic_batch(bs, 0, device)
    enc = model._encode_description(desc, None).float()
    pr = model.embed_prompts(prompt).float()
    eng = model._get_engine(bs, N_DESC, N_PROMPT, NEW_TOKENS + 1)
    eng.set_gen_params(max_length=NEW_TOKENS + 1, min_new_tokens=NEW_TOKENS, **gen)
    eng.prefill(enc, None, pr, None, sample=True)
    return eng


NODE_FLOOR_US = 2.13  # a dependent, trivial kernel node inside a hipGraph on MI355X (profiles/r01_sync_and_chain_probes.txt, relay chain)


def step_graph_nodes(bs: int, layers: int, hidden: int, folded: bool, dtype: str = "bf16"):
    """Kernel nodes of the captured decode step (csrc/ptts_lm.hip forward<> + tail), by batch-size regime; sinusoidal positions."""
    if bs <= 8:   # GEMV step
        fused_w = hidden in ((512, 1024, 1536) if dtype != "f32" else (512, 1024))  # widths the fused nodes are instantiated for
        self_nodes = 2 if (bs <= 3 and fused_w) else 3  # [qkv_attn_kernel (up to 3 utterances) | LN1+QKV, attention], combine + out_proj
        if folded:  # single utterance, static cross-attention fold: [xfold_attn_kernel | LN2 + M x, softmax + U p]
            cross_nodes = 1 if (fused_w and hidden <= (1024 if dtype != "f32" else 512)) else 2
        else:       # [xq_attn_kernel | LN2 + q, cross-attention], out_proj
            cross_nodes = 2 if fused_w else 3
        return (self_nodes + cross_nodes + 2) * layers + 2  # + LN3 + fc1, fc2 per layer; + LM heads, sampler / embed tail
    if hidden in (1024, 1536):  # LN1+QKV (lnproj: 8 / 16 utterances per workgroup), attention, combine+out_proj, fused LN2+cross-q+cross-attn, out_proj, LN3+fc1 (lnproj), fc2
        return 7 * layers + 3   # + heads prep (final LN), LM heads, sampler / embed tail
    return None


def latency_model(nodes: int, us_per_launch: float) -> dict:
    """The step is a chain of `nodes` dependent kernels; each costs at least one kernel boundary whatever it computes. The HBM
    roofline says how far the step is from the byte floor, this says how far it is from the dependency floor of its own structure."""
    floor = nodes * NODE_FLOOR_US
    return {"nodes": nodes, "dependent_node_floor_us": NODE_FLOOR_US, "floor_us_per_launch": round(floor, 1),
            "us_per_node": round(us_per_launch / nodes, 2), "frac_of_node_floor": round(floor / us_per_launch, 3),
            "note": "floor = nodes x the measured cost of a dependent trivial kernel node in a hipGraph (profiles/r01_sync_and_chain_probes.txt); "
                    "in-kernel grid barriers measured no cheaper at >= 128 workgroups (same file)"}


def measure_traffic_live(bs: int, context: int, steps: int = 24, timeout_s: int = 120):
    """HBM bytes per decode step measured during THIS run, AT THE CONTEXT THE STEP IS TIMED AT (default; `--no-live-pmc` reads the
    committed pass under profiles/ instead): two separate `rocprofv3 --pmc` passes (FETCH_SIZE, WRITE_SIZE; never combined with trace domains) over
    tools/prof_eager.py (the step's kernels launched eagerly: --pmc does not survive graph replays in this image), summarised by
    tools/pmc_report2.py with the guide's gfx950 correction (FETCH_SIZE x2). Returns the report's dict or None (any failure, no
    rocprofv3, already running under a profiler): the caller then falls back to the committed pass."""
    import glob
    import shutil
    import subprocess
    import tempfile

    rp = shutil.which("rocprofv3")
    if rp is None or any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        return None
    tmp = tempfile.mkdtemp(prefix="ptts_pmc_", dir="/tmp")
    try:
        # a prompt of `context - steps - 1` positions puts the eager steps where the timed replays ran: the last 16 steps sit at
        # contexts context-16 .. context-1
        env = dict(os.environ, PROF_B=str(bs), PROF_STEPS=str(steps), PROF_P=str(max(8, context - steps - 1)), TMPDIR="/tmp")
        dbs = {}
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out_dir = os.path.join(tmp, counter)
            r = subprocess.run([rp, "--pmc", counter, "-d", out_dir, "-o", "p", "--", sys.executable, os.path.join(ROOT, "tools", "prof_eager.py")],
                               cwd="/tmp", env=env, timeout=timeout_s, capture_output=True)
            found = glob.glob(os.path.join(out_dir, "**", "*.db"), recursive=True)
            if r.returncode != 0 or not found:
                return None
            dbs[counter] = found[0]
        out_json = os.path.join(tmp, "traffic.json")
        context = max(8, context - steps - 1) + 1 + steps - 8  # mean self-KV length over the 16 steps summarised
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pmc_report2.py"), dbs["FETCH_SIZE"], dbs["WRITE_SIZE"], str(min(16, steps - 1)),
                            str(context), str(bs), out_json], timeout=60, capture_output=True)
        if r.returncode != 0 or not os.path.exists(out_json):
            return None
        j = json.load(open(out_json))
        j["source"] = "LIVE in this bench run: " + j.get("source", "")
        return j
    except Exception:  # noqa: BLE001 — a side measurement: never fatal
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


LIVE_PMC = True  # cleared by --no-live-pmc


def measure_decode_roofline(model, bs: int, device, live_pmc: bool = True) -> dict:
    """HIP events (on the stream the graph is launched on) around 400 replays of the captured decode step at
    mid-context. Algorithmic bytes per step = W_step*s + B*2*layers*H*(Lc+N)*s + B*(K*H*s + K*V*4)."""
    eng = _prefilled_engine(model, bs, device)
    n_warm, n = 230, 400
    eng.decode_steps(n_warm)
    step_s = _timed_replays(eng, n)
    d = model.config.decoder
    H, L, F, V, Kc = d.hidden_size, d.num_hidden_layers, d.ffn_dim, d.vocab_size, d.num_codebooks
    w_step = L * (4 * H * H + 2 * H * H + 2 * H * F) + Kc * V * H  # 362.3 M for Mini-v1, 1005.9 M for Large-v1
    lc = N_PROMPT + 1 + n_warm + n // 2  # mean self-KV length over the timed replays
    es = 2 if model.dtype == torch.bfloat16 else 4
    # e4m3 weights are streamed as bytes at EVERY batch size (GEMV step up to 8 utterances, e4m3 MFMA strips above: DESIGN.md §4.1 / §4.2)
    ws = 1 if getattr(model, "decoder_weights_fp8", False) else es
    # e4m3 self-attention cache (opt-in, engines of more than 8 utterances): 64 bytes + one fp32 scale per (head, position) row of 64 values
    kv8 = bool(getattr(model, "decoder_kv_fp8", False)) and bs > 8
    kv_es = (1.0 + 4.0 / 64.0) if kv8 else es
    bytes_step = int(w_step * ws + bs * 2 * L * H * (lc * kv_es + N_DESC * es) + bs * (Kc * H * es + Kc * V * 4))
    achieved = bytes_step / step_s / 1e9
    traffic, tnote = None, "PMC pass not available for this configuration"
    pmc = os.path.join(ROOT, "profiles", f"r03_pmc_step_bs{bs}.json")  # the same two passes, committed (context ~455), when the live ones are off / fail
    live = measure_traffic_live(bs, lc, timeout_s=120 if bs <= 32 else 240) if (LIVE_PMC and live_pmc and es == 2 and H == 1024 and L == 24 and ws == 2 and not kv8 and bs <= 128) else None
    # (the committed fallback only up to 32 utterances: the 128-utterance file is the round-3 pass, two kernel generations old - VERDICT r05 weak #3:
    #  above 32 the field is LIVE or null)
    if live is not None or (es == 2 and H == 1024 and not kv8 and bs <= 32 and os.path.exists(pmc)):  # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE summary (separate passes)
        j = live if live is not None else json.load(open(pmc))
        traffic = int(j["traffic_bytes_per_step"])
        tnote = (f"{j['source']}; measured at self-KV context ~{j['context']} (algorithmic there: ~{j.get('algorithmic_mb', '?')} MB). Every weight "
                 "matrix is fetched once at any context; the attention fetches are bounded by the host's context bound rounded up to 64 positions, "
                 "so the K/V part of the traffic grows with the context like the algorithmic term (bytes_per_launch is quoted at the timed context)")
    folded = bs == 1 and not getattr(d, "rope_embeddings", False) and N_DESC <= 64  # static cross-attention folding
    out = {"bound": "hbm", "achieved": round(achieved, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(achieved / 8000.0, 4),
           "traffic": traffic, "traffic_note": tnote,
           "kernel": "decode-step hipGraph: one hipGraphLaunch per generated frame",
           "us_per_launch": round(step_s * 1e6, 1), "bytes_per_launch": int(bytes_step), "context": lc,
           "frac_of_measured_copy_6.29TBps": round(achieved / 6290.0, 4)}
    try:  # side information only: must never break the contract line
        nodes = step_graph_nodes(bs, L, H, folded, "bf16" if es == 2 else "f32")
        real = int(eng.graph_nodes()) if hasattr(eng, "graph_nodes") else 0  # the captured step graph's own node count (ptts_debug_graph_nodes)
        if real > 0:
            out["graph_nodes_counted"] = real
            nodes = real
        if nodes:
            out["kernel"] += f" ({nodes} kernel nodes)" + (f": batch <= 8 runs {(nodes - 2) // L} row-per-wave GEMV / attention nodes per layer + LM heads "
                                                            "+ sampler/embed tail" if bs <= 8 else "")
            out["latency_model"] = latency_model(nodes, step_s * 1e6)
    except Exception:  # noqa: BLE001
        pass
    return out


def measure_sampling_step(model, bs: int, device) -> dict:
    """The same captured step with the sampler tail drawing (temperature 1.0, top_k 50, top_p 0.9) instead of taking the arg-max."""
    out = {}
    for name, gen in (("greedy", {}), ("sample_topk50", dict(do_sample=True, temperature=1.0, top_k=50, seed=1)),
                      ("sample_topk50_topp0.9", dict(do_sample=True, temperature=0.9, top_k=50, top_p=0.9, seed=1))):
        eng = _prefilled_engine(model, bs, device, **gen)
        eng.decode_steps(100)
        out[name + "_us_per_step"] = round(_timed_replays(eng, 300) * 1e6, 1)
    out["ratio_sampling_over_greedy"] = round(out["sample_topk50_topp0.9_us_per_step"] / out["greedy_us_per_step"], 3)
    return out


def measure_ttft(model, bs: int, device, reps: int = 20) -> float:
    """p50 wall time from the start of generate()'s work to the first sampled token on device: description encoder
    + prompt embedding + HIP prefill of P+1 positions + first sampler tail."""
    desc, prompt = synthetic_batch(bs, 0, device)
    eng = model._get_engine(bs, N_DESC, N_PROMPT, NEW_TOKENS + 1)
    eng.set_gen_params(max_length=NEW_TOKENS + 1, min_new_tokens=NEW_TOKENS)
    ts = []
    for i in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc = model._encode_description(desc, None).float()
        pr = model.embed_prompts(prompt).float()
        eng.prefill(enc, None, pr, None, sample=True)
        eng.first_token_sync()  # the sampler tail's event: the first token exists on the device (the fold enqueued behind it belongs to the decode steps)
        if i >= 3:
            ts.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def measure_ttft_breakdown(model, bs: int, device, reps: int = 20) -> dict:
    """Where the time to the first token goes: GPU time of each stage of the path `measure_ttft` times, from events
    on the stream the work is enqueued on, p50 over `reps` calls - description encoder (modeling_parler_tts.py:3048-3097), prompt
    embedding (:3100), HIP prefill of P + 1 positions (`_sample`'s first forward, :3564), first sampler tail (`ptts_first_token_times`) -
    all as they ran in sequence on the stream - beside the p50 wall time of the whole sequence; `host_and_gaps_ms` = wall - sum of the
    stages (host time before the first kernel, stream gaps between the stages, the event wait). `stock_t5_ms` = the same description through the stock transformers module replayed from a torch HIP graph (what
    rounds 1-4 shipped), for the before / after."""
    desc, prompt = synthetic_batch(bs, 0, device)
    eng = model._get_engine(bs, N_DESC, N_PROMPT, NEW_TOKENS + 1)
    eng.set_gen_params(max_length=NEW_TOKENS + 1, min_new_tokens=NEW_TOKENS)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    stages = {"t5_ms": [], "prompt_embed_ms": [], "prefill_ms": [], "first_tail_ms": [], "wall_ms": []}
    for i in range(reps + 3):
        e = [ev() for _ in range(3)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e[0].record()
        enc = model._encode_description(desc, None).float()
        e[1].record()
        pr = model.embed_prompts(prompt).float()
        e[2].record()
        eng.prefill(enc, None, pr, None, sample=True)
        eng.first_token_sync()
        wall = (time.perf_counter() - t0) * 1e3
        pre, tail = eng.first_token_times()  # the prefill as it ran IN SEQUENCE (host launches hidden behind the encoder's GPU time)
        torch.cuda.synchronize()
        if i >= 3:
            stages["t5_ms"].append(e[0].elapsed_time(e[1]))
            stages["prompt_embed_ms"].append(e[1].elapsed_time(e[2]))
            stages["prefill_ms"].append(pre)
            stages["first_tail_ms"].append(tail)
            stages["wall_ms"].append(wall)
    p50 = {k: sorted(v)[len(v) // 2] for k, v in stages.items()}
    t5e = model.__dict__.get("_t5_engine")
    native = t5e is not None
    t5_nodes = int(t5e.graph_nodes()) if (native and hasattr(t5e, "graph_nodes")) else 0  # the captured graph's own node count (ptts_t5_debug_graph_nodes)
    out = {k: round(p50[k], 3) for k in ("t5_ms", "prompt_embed_ms", "prefill_ms", "first_tail_ms")}
    out.update({"wall_p50_ms": round(p50["wall_ms"], 3), "bs": bs, "reps": reps,
                "host_and_gaps_ms": round(p50["wall_ms"] - sum(p50[k] for k in ("t5_ms", "prompt_embed_ms", "prefill_ms", "first_tail_ms")), 3),
                "t5_encoder": "native HIP (ptts_t5_encode)" if native else "stock transformers module (torch HIP graph replay)",
                "launches": {"t5": f"2 copies + 1 hipGraph of {t5_nodes} kernel nodes (counted at capture) + 1 final-norm launch" if native else "~50 per block (ATen / Tensile)",
                             "prompt_embed": 2, "first_tail": 1}})
    if native:  # before / after: the stock module on the same description
        try:
            model.use_native_text_encoder = False
            ts = []
            for i in range(8):
                a, b = ev(), ev()
                torch.cuda.synchronize()
                a.record()
                model._encode_description(desc, None)
                b.record()
                torch.cuda.synchronize()
                if i >= 3:
                    ts.append(a.elapsed_time(b))
            out["stock_t5_ms"] = round(sorted(ts)[len(ts) // 2], 3)
        except Exception as ex:  # noqa: BLE001
            out["stock_t5_ms"] = repr(ex)[:120]
        finally:
            model.use_native_text_encoder = True
            model.__dict__.pop("_enc_graphs", None)
    return out


def measure_ttfa(model, device, reps: int = 9, play_steps_in_s: float = 0.5) -> dict:
    """p50 time-to-first-audio (INFERENCE.md:3 "under 500 ms"): wall time from calling generate(streamer=...) in a thread
    (INFERENCE.md:130-148: play_steps = frame_rate * 0.5 s = 43 columns) to the first non-empty audio chunk in the queue:
    T5 + prefill + 42 graph replays + un-delay + chunked DAC decode of the 34 complete frames, minus the stride."""
    import threading

    import parler_tts_amd as P

    desc, prompt = synthetic_batch(1, 0, device)
    play_steps = int(model.audio_encoder.config.frame_rate * play_steps_in_s)
    kw = dict(input_ids=desc, prompt_input_ids=prompt, do_sample=False, max_new_tokens=3 * play_steps, min_new_tokens=3 * play_steps)
    ts, first_len = [], 0
    for i in range(reps + 2):
        streamer = P.ParlerTTSStreamer(model, device=device, play_steps=play_steps, timeout=60.0)  # a dead generate() thread raises here, never hangs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        th = threading.Thread(target=model.generate, kwargs=dict(streamer=streamer, **kw))
        th.start()
        t_first = None
        for chunk in streamer:
            if t_first is None and chunk.shape[0] > 0:
                t_first = time.perf_counter() - t0
                first_len = int(chunk.shape[0])
        th.join()
        if i >= 2 and t_first is not None:
            ts.append(t_first)
    ts.sort()
    return {"ttfa_p50_ms": round(ts[len(ts) // 2] * 1e3, 2), "play_steps": play_steps, "first_chunk_samples": first_len,
            "first_chunk_audio_ms": round(first_len / model.audio_encoder.config.sampling_rate * 1e3, 1)}


def cpu_baseline(budget_s: float = 20.0) -> dict:
    """The oracle (CPU restatement of the reference path, kind 'port') on the host cores: Mini-v1 shapes, fp32, greedy,
    bs=1, same synthetic input shapes. EVERYTHING reported is timed: prefill of P+1 positions + S cached decode passes
    (as many as fit the budget) + DAC decode of the S+1-8 frames those passes complete; value = that audio / that time.
    No extrapolation to 868 passes (so the prefill weighs ~5 % more than in the full run, and the context stays short:
    both favour neither side by more than a few per cent). profiles/r02_cpu_baseline_calibration.txt holds the ratio of
    this port to the reference's own ParlerTTSForCausalLM timed on the same host."""
    from oracle import dac_oracle as DA
    from oracle import decoder_oracle as DO

    ncpu = os.cpu_count() or 1
    spec = DO.MINI_V1
    torch.set_num_threads(min(ncpu, 16))
    sd = DO.make_decoder_weights(spec, seed=1234)
    orc = DO.DecoderOracle(spec, sd)
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(1, N_DESC, spec.hidden_size, generator=g)
    prompt = torch.randn(1, N_PROMPT, spec.hidden_size, generator=g) * 0.02
    ids = torch.full((9, 1), spec.bos_token_id, dtype=torch.long)
    with torch.no_grad():
        # bs=1 decode is GEMV-sized: more threads than memory channels only adds synchronisation cost. Sweep the thread
        # count (4 .. 64; 2 untimed + 10 timed cached passes each, median) and keep the fastest; `cores` = the threads actually used.
        orc.forward(ids, enc, None, prompt, None)
        best, cores, sweep = None, 1, {}
        for nt in sorted({c for c in (4, 8, 16, 32, 64) if c <= ncpu} | {min(ncpu, 8)}):
            torch.set_num_threads(nt)
            for _ in range(2):  # untimed: thread pool spin-up at this width
                orc.forward(torch.zeros(9, 1, dtype=torch.long))
            per = []
            for _ in range(10):
                ts = time.perf_counter()
                orc.forward(torch.zeros(9, 1, dtype=torch.long))
                per.append(time.perf_counter() - ts)
            per.sort()
            dt = per[len(per) // 2]  # median of 10 cached passes
            sweep[str(nt)] = round(dt * 1e3, 2)
            if best is None or dt < best:
                best, cores = dt, nt
        torch.set_num_threads(cores)
        dac = DA.DacOracle(DA.DAC_44KHZ, DA.make_dac_weights(DA.DAC_44KHZ, seed=4321))
        dac.decode(torch.randint(0, 1024, (1, 9, 4), generator=g))  # warm-up
        orc.reset()
        t0 = time.perf_counter()
        logits = orc.forward(ids, enc, None, prompt, None)
        t_prefill = time.perf_counter() - t0
        steps, t1 = 0, time.perf_counter()
        while time.perf_counter() - t1 < budget_s * 0.6 and steps < NEW_TOKENS - 1:
            nxt = logits[:, -1].argmax(-1, keepdim=True).clamp(max=1023)
            logits = orc.forward(nxt)
            steps += 1
        t_steps = time.perf_counter() - t1
        frames = max(1, steps + 1 - (K_CODEBOOKS - 1))  # passes - (K - 1): the delay pattern's tail produces no audio
        codes = torch.randint(0, 1024, (1, 9, frames), generator=g)
        t2 = time.perf_counter()
        dac.decode(codes)
        t_dac = time.perf_counter() - t2
    total = t_prefill + t_steps + t_dac
    audio = frames * 512 / 44100.0
    return {"value": round(audio / total, 4), "unit": "audio-seconds/sec", "cores": cores, "host_cores": ncpu, "kind": "port",
            "sample": f"oracle/ fp32 Mini-v1 bs=1, all timed: prefill of {N_PROMPT + 1} positions ({t_prefill:.2f} s) + {steps} cached decode passes "
                      f"({t_steps / max(steps, 1) * 1e3:.1f} ms each) + DAC decode of the {frames} frames they complete ({t_dac:.2f} s) = {audio:.2f} s of audio in "
                      f"{total:.1f} s on {cores} threads (thread count swept, host has {ncpu}); T5 encoder excluded",
            "ms_per_decode_step": round(t_steps / max(steps, 1) * 1e3, 2),
            "thread_sweep_ms_per_step": sweep}  # median of 10 cached passes per thread count; `cores` = the fastest


def _timed_generate(model, bs: int, device, reps: int = 1) -> float:
    """seconds per generate() of `bs` utterances x 860 frames (one warm-up, then the mean of `reps` timed calls)"""
    d, p = synthetic_batch(bs, 0, device)
    kw = dict(input_ids=d, prompt_input_ids=p, do_sample=False, max_new_tokens=NEW_TOKENS, min_new_tokens=NEW_TOKENS)
    model.generate(**kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        wav = model.generate(**kw)
    torch.cuda.synchronize()
    assert wav.shape == (bs, FRAMES * 512), wav.shape
    return (time.perf_counter() - t0) / reps


def dac_flops_per_frame(latent: int = 1024, dim: int = 1536, rates=(8, 8, 4, 2)) -> int:
    """Multiply-adds x 2 of DAC.decode per latent frame (1.608 GFLOP for the 44.1 kHz stack): Conv1d(latent -> dim, k7),
    per block a transposed conv (k = 2s, stride s: 2 taps per output sample) + 3 residual units (k7 + k1) at the block's rate, the final
    Conv1d(C -> 1, k7). The RVQ gather, Snake and tanh are not counted."""
    f, up = 2 * latent * dim * 7, 1
    for i, s in enumerate(rates):
        cin, cout = dim >> i, dim >> (i + 1)
        up *= s
        f += up * (2 * cin * cout * 2 + 3 * (2 * cout * cout * 7 + 2 * cout * cout))
    return f + up * 2 * (dim >> len(rates)) * 7


def _timed_dac(eng, codes, reps: int) -> float:
    """seconds per ptts_dac_decode call: HIP events on the stream the codec's kernels are launched on, around `reps` calls (after 2 warm-ups)."""
    hip = hip_event_timer()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        eng.decode(codes)
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0)); hip.hipEventCreate(C.byref(e1))
    hip.hipEventRecord(e0, stream)
    for _ in range(reps):
        eng.decode(codes)
    hip.hipEventRecord(e1, stream)
    hip.hipEventSynchronize(e1)
    ms = C.c_float()
    hip.hipEventElapsedTime(C.byref(ms), e0, e1)
    return ms.value / 1e3 / reps


def measure_dac(device, bs_list=(1, 32), with_f32: bool = True) -> dict:
    """SURVEY.md §8(d)'s SECOND bound of the path: DAC decode is MFMA-bound. One ptts_dac_decode of bs x 860 frames (what generate() calls
    after the token loop), timed by HIP events on its launch stream; achieved = algorithmic flops (1.608 GFLOP per frame x frames x bs)
    / time, against the dense bf16 MFMA peak (2.5 PFLOP/s) in the bf16-operand mode the headline configuration runs, and against the
    fp32 MFMA peak (157.3 TFLOP/s) in the exact-f32 parity mode (1 and 32 utterances). Same synthetic codec weights as the model (seed 4321)."""
    from parler_tts_amd.engine import DacEngine
    from parler_tts_amd.synthetic import random_dac_state_dict

    sd = {k: v.to(device) for k, v in random_dac_state_dict(seed=4321).items()}
    fl = dac_flops_per_frame()
    out = {"bound": "mfma", "unit": "TFLOP/s", "peak_bf16": 2500.0, "peak_f32": 157.3, "flops_per_frame": fl, "frames": FRAMES,
           "kernel": "ptts_dac_decode: RVQ gather + 30 conv launches (LDS-tiled bf16 MFMA k7 / transposed convs, fused residual units, tiled final conv + tanh)"}
    for mode, dt, peak, sizes in (("bf16", torch.bfloat16, 2500.0, bs_list), ("f32", torch.float32, 157.3, (1, 32) if with_f32 else ())):
        if not sizes:
            continue
        eng = DacEngine(max_batch=max(sizes), max_frames=FRAMES, device=device, compute_dtype=dt)
        eng.load_state_dict(sd)
        for bs in sizes:
            codes = torch.randint(0, 1024, (bs, K_CODEBOOKS, FRAMES), generator=torch.Generator().manual_seed(7)).to(device)
            sec = _timed_dac(eng, codes, 10 if bs == 1 else (3 if mode == "bf16" else 2))
            ach = fl * FRAMES * bs / sec / 1e12
            out[f"{mode}_bs{bs}"] = {"ms_per_launch": round(sec * 1e3, 3), "flops_per_launch": fl * FRAMES * bs, "achieved": round(ach, 1), "peak": peak,
                                     "frac": round(ach / peak, 4), "audio_seconds_per_sec": round(bs * AUDIO_S / sec, 1)}
            if mode == "bf16" and bs == 32:
                # round 6 (profiles/r06_pmc_dac_bs32_xin.txt: rocprofv3 --pmc FETCH_SIZE x 2 / WRITE_SIZE, separate passes over this very decode, on the
                # tree with the residual units on the fp32 stream): with one launch per layer the codec moves 197.29 GB per 32 x 860 frames - by bytes its
                # floor at 8 TB/s (24.7 ms) is ABOVE its floor by flops (17.7 ms at 2.5 PF): at this batch the dominant bound is HBM. Traffic from the
                # committed pass, time from this run.
                tb = 197.29e9
                out["bf16_bs32"]["hbm"] = {"traffic_bytes_per_launch_pmc": tb, "achieved_GBps": round(tb / sec / 1e9, 1), "peak_GBps": 8000.0,
                                           "frac": round(tb / sec / 8e12, 4), "source": "profiles/r06_pmc_dac_bs32_xin.txt (committed PMC pass) / this run's time"}
        eng.close()
    return out


def delayed_ids_from_codes(codes: torch.Tensor, frames, K: int, L: int, bos: int, pad: int):
    """The [B*K, L] id matrix the token loop leaves for utterances of frames[b] frames each (codebook k delayed by k columns behind the BOS
    column, the EOS / pad id from the end of the utterance on), and the delay-pattern mask generate() applies to it."""
    from parler_tts_amd.modeling_parler_tts import build_delay_pattern_mask

    B = codes.shape[0]
    ids = torch.full((B * K, L), pad, dtype=torch.long, device=codes.device)
    for b in range(B):
        n = int(frames[b])
        for k in range(K):
            ids[b * K + k, 1 + k: 1 + k + n] = codes[b, k, :n]
    bos_col = torch.full((B * K, 1), bos, dtype=torch.long, device=codes.device)
    _, pattern = build_delay_pattern_mask(bos_col, bos, pad, L, K)
    return ids, pattern, bos_col


def measure_ragged(model, device, bs: int = 32) -> dict:
    """What an EOS-terminated batch pays after the token loop (modeling_parler_tts.py:3585-3647: un-delay, per-sample special-id filter, codec,
    zero-padding): `bs` utterances whose lengths are uniform in [430, 860] frames through generate()'s own tail (`_undelay_and_decode`: one
    filter kernel + ONE ragged codec pass) beside the fixed-length batch of 860 frames (no special ids: one plain codec call). value = audio
    seconds produced per second of that tail; `ratio_vs_fixed` = ragged value / fixed value (1.0 = a ragged batch costs exactly its frames)."""
    d = model.config.decoder
    K, L, bos, pad = d.num_codebooks, NEW_TOKENS + 1, d.bos_token_id, d.pad_token_id
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(430, FRAMES + 1, (bs,), generator=g)
    codes = torch.randint(0, 1024, (bs, K, FRAMES), generator=g).to(device)
    out = {}
    for name, fr in (("fixed", torch.full((bs,), FRAMES)), ("ragged", lens)):
        ids, pattern, bos_col = delayed_ids_from_codes(codes, fr, K, L, bos, pad)
        model._undelay_and_decode(ids, pattern, bos_col, bos, pad)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            wav, lengths = model._undelay_and_decode(ids, pattern, bos_col, bos, pad)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 3
        assert lengths == [int(n) * 512 for n in fr], (name, lengths[:4])
        audio = float(fr.sum()) * 512 / 44100.0
        out[name] = {"ms": round(dt * 1e3, 2), "audio_seconds": round(audio, 1), "audio_seconds_per_sec": round(audio / dt, 1)}
    out["frames_min_max_mean"] = [int(lens.min()), int(lens.max()), round(float(lens.float().mean()), 1)]
    out["ratio_vs_fixed"] = round(out["ragged"]["audio_seconds_per_sec"] / out["fixed"]["audio_seconds_per_sec"], 3)
    out["unit"] = "audio-seconds/sec of the post-loop tail (un-delay + special-id filter + codec)"
    return out


def _trim_roofline(r: dict) -> dict:
    return {k: r[k] for k in ("achieved", "peak", "unit", "frac", "traffic", "us_per_launch", "bytes_per_launch", "context") if k in r}


def measure_fp32_parity_mode(device) -> dict:
    """The engine mode whose greedy ids are BIT-EXACT against the fp32 oracle on this very configuration (all 869 columns:
    tests/test_bench_config_parity_gpu.py) and whose DAC runs exact-f32 MFMA (waveform RMS <= 1e-4): north_star's "bit-exact greedy
    token ids" bar, timed. Its own model object (fp32 weights, same seeds); released afterwards."""
    model = build_model_on_device(device, torch.float32, "mini")
    dt = _timed_generate(model, 1, device)
    rf = measure_decode_roofline(model, 1, device, live_pmc=False)
    out = {"value": round(AUDIO_S / dt, 3), "unit": "audio-seconds/sec", "ms_per_step": round(dt * 1e3, 1), "dtype": "f32 (fp32 weights / KV / activations, exact-f32 MFMA DAC)",
           "roofline": _trim_roofline(rf)}
    model._engine = None
    return out


def measure_large(device) -> dict:
    """BASELINE configs[3] / configs[4] per-GPU shapes: parler-tts-large-v1 (30 layers, H 1536, F 6144; init_large_model.py:25-43),
    bf16 with 1 / 8 / 32 utterances per GPU, then e4m3 weights with 1 / 4 / 8 / 32. Random weights drawn on the device."""
    model = build_model_on_device(device, torch.bfloat16, "large")
    out = {}

    def point(bs):
        dt = _timed_generate(model, bs, device)
        return {"value": round(bs * AUDIO_S / dt, 3), "ms_per_step": round(dt * 1e3, 1), "roofline": _trim_roofline(measure_decode_roofline(model, bs, device, live_pmc=False))}

    for bs in (1, 8, 32):  # configs[3] is 1 utterance per GPU; 8 / 32 are the bf16 references of the e4m3 points below
        out[f"bf16_bs{bs}"] = point(bs)
    model.enable_fp8_weights()
    for bs in (1, 4, 8, 32):  # configs[4] is 4 per GPU; 32 per GPU is where one-byte weights should show (GEMV step up to 8, e4m3 MFMA strips above)
        out[f"fp8w_bs{bs}"] = point(bs)
    for bs in (8, 32):
        out[f"fp8w_over_bf16_step_bs{bs}"] = round(out[f"bf16_bs{bs}"]["roofline"]["us_per_launch"] / out[f"fp8w_bs{bs}"]["roofline"]["us_per_launch"], 3)
    out["unit"] = "audio-seconds/sec"
    model._engine = None
    return out


def arm_watchdog(out: dict, seconds: float):
    """Side measurements (bs=32, streaming, sampling, CPU baseline) run AFTER the contract numbers are in `out`. If one of them hangs, a
    daemon thread prints the line with what has been measured so far and ends the process with status 0: the headline number must never be
    lost to a side measurement. (A thread, not a signal: it also fires while the main thread sits inside a HIP call that released the
    GIL.) Returns the function that disarms it."""
    import threading

    done = threading.Event()

    def run():
        if not done.wait(seconds):
            out["watchdog"] = f"side measurements did not finish within {seconds:.0f} s: the line holds what was measured until then"
            try:
                line = json.dumps(out)
            except Exception:  # noqa: BLE001 — a half-written side object: keep the contract fields only
                line = json.dumps({k: v for k, v in out.items() if isinstance(v, (int, float, str, bool, type(None)))})
            print(line, flush=True)
            os._exit(3 if os.environ.get("PTTS_BENCH_STRICT") else 0)  # the builder's own runs surface a hung side measurement in the exit status

    threading.Thread(target=run, daemon=True).start()
    return done.set


DUMP_BYTES = 64 * 10 ** 6  # --dump-outputs writes at most this much in all


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """Writes each [rows, ...] output as out_dir/<name>.npy in float32. What does not fit DUMP_BYTES (split evenly between the arrays) is
    written as a fixed sample of whole rows - the first rows of a permutation drawn with seed 0, in ascending order - and the rows kept
    go to out_dir/<name>_rows.npy (float64), so that two builds dump the same rows of the same inputs."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_BYTES // max(1, len(arrays)) - 4096  # room for the .npy headers and a row index
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        row_bytes = max(1, a[0].nbytes if a.ndim > 1 else a.itemsize)
        if a.nbytes > budget:
            keep = max(1, budget // row_bytes)
            rows = np.sort(torch.randperm(a.shape[0], generator=torch.Generator().manual_seed(0))[:keep].numpy())
            a = a[rows]
            np.save(os.path.join(out_dir, f"{name}_rows.npy"), rows.astype(np.float64))
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a, dtype=np.float32))


def self_launch(args) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks here (one process per GPU over RCCL), relay
    rank 0's JSON line. Equivalent to `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...`."""
    import socket
    import subprocess

    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["PTTS_BENCH_LAUNCHED"] = "1"
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bs", type=int, default=1, help="utterances per GPU per step (configs[1]: 1; configs[2]: 32; configs[3]: --model large --bs 1)")
    ap.add_argument("--model", default="mini", choices=["mini", "large"], help="parler-tts-mini-v1 (BASELINE metric) or parler-tts-large-v1 shapes")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp8w"], help="fp8w: bf16 engine streaming OCP e4m3 weights in the decode step (BASELINE configs[4])")
    ap.add_argument("--sample", action="store_true", help="do_sample=True (temperature 1.0, top_k 50: the reference's default generation mode) instead of greedy")
    ap.add_argument("--full", action="store_true", help="also run the side measurements (roofline, TTFT, CPU baseline, bs=32 / bs=128, codec, "
                                                        "streaming, sampling, fp32 parity mode, Large-v1); a plain run times the headline steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step returned as DIR/<name>.npy (float32, <= 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the bs=32 / TTFT side measurements")
    ap.add_argument("--live-pmc", action="store_true", help="(default since round 3) measure roofline.traffic in this run: two rocprofv3 --pmc child "
                                                            "passes at the timed context, ~20 s per batch size")
    ap.add_argument("--no-live-pmc", action="store_true", help="read roofline.traffic from the committed pass under profiles/ (context 57) instead")
    args = ap.parse_args()
    global LIVE_PMC
    LIVE_PMC = not args.no_live_pmc
    extras = args.full and not args.no_extras
    with_cpu_baseline = args.full and not args.no_cpu_baseline

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    ndev = torch.cuda.device_count()
    if local >= ndev and not os.environ.get("PTTS_BENCH_SHARE_GPU"):
        raise SystemExit(f"rank {rank} wants GPU {local} but only {ndev} visible (set PTTS_BENCH_SHARE_GPU=1 for a functional run of N ranks on fewer GPUs)")
    dev_index = local % ndev
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("PTTS_DIST_BACKEND", "nccl")  # "nccl" is RCCL on ROCm; gloo only for functional runs of ranks sharing one GPU
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    import __graft_entry__ as ge

    if rank == 0 or world == 1:
        ge.build()
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
    dtype = torch.float32 if args.dtype == "fp32" else torch.bfloat16
    model = build_model(rank, world, device, dtype, args.model)
    if args.dtype == "fp8w":
        model.enable_fp8_weights()
    desc, prompt = synthetic_batch(args.bs, rank, device)
    gen_kw = dict(input_ids=desc, prompt_input_ids=prompt, do_sample=False, max_new_tokens=NEW_TOKENS, min_new_tokens=NEW_TOKENS)
    if args.sample:
        gen_kw.update(do_sample=True, temperature=1.0, top_k=50)

    def barrier():
        if world > 1:
            import torch.distributed as dist

            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        wav = model.generate(**gen_kw)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        wav = model.generate(**gen_kw)
    barrier()
    elapsed = time.perf_counter() - t0
    assert wav.shape == (args.bs, FRAMES * 512), wav.shape
    n_ranks = world
    per_rank = [elapsed]
    if world > 1:
        import torch.distributed as dist

        n_ranks = dist.get_world_size()  # the ranks the process group (RCCL) actually holds
        tdev = device if dist.get_backend() == "nccl" else torch.device("cpu")
        mine = torch.tensor([elapsed], device=tdev, dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(n_ranks)]
        dist.all_gather(every, mine)
        per_rank = [float(x.item()) for x in every]
        elapsed = max(per_rank)  # the slowest rank bounds the job
    value = n_ranks * args.bs * args.steps * AUDIO_S / elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"audio_values": wav})

    out = None
    mname = "parler-tts-mini-v1" if args.model == "mini" else "parler-tts-large-v1"
    ttft_ranks = None
    if world > 1 and extras:  # both halves of the metric on a multi-GPU run: every rank times ITS p50 time-to-first-token, the line carries the max
        import torch.distributed as dist

        mine = torch.tensor([measure_ttft(model, args.bs, device, reps=9)], device=device if dist.get_backend() == "nccl" else torch.device("cpu"), dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(n_ranks)]
        dist.all_gather(every, mine)
        ttft_ranks = [round(float(x.item()), 2) for x in every]
    if rank == 0:
        out = {
            "metric": "audio-seconds/sec (whole node) + p50 time-to-first-token, Mini-v1 bs=1/32", "value": round(value, 3),
            "unit": "audio-seconds/sec", "n_gpus": n_ranks, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"bf16": "bf16", "fp32": "f32", "fp8w": "bf16 activations + KV, e4m3 weights"}[args.dtype], "data": f"synthetic (random-init weights at {mname} shapes, seeded token ids)",
            "config": {"workload": f"{mname} {args.dtype} bs={args.bs}/GPU {'sampling (T=1, top_k=50)' if args.sample else 'greedy'}, {N_DESC} description + "
                                   f"{N_PROMPT} prompt tokens, {FRAMES} frames = {AUDIO_S:.3f} s audio/utterance ({NEW_TOKENS} decoder passes, hipGraph decode, DAC on-GPU)",
                       "global_batch": n_ranks * args.bs, "frames": FRAMES, "parallelism": f"utterance-sharded x{n_ranks}, weights broadcast once"},
        }
        if world > 1:
            out["config"]["world_size_reported_by_process_group"] = n_ranks
            out["config"]["backend"] = os.environ.get("PTTS_DIST_BACKEND", "nccl") + (" (RCCL)" if os.environ.get("PTTS_DIST_BACKEND", "nccl") == "nccl" else "")
            out["per_rank_ms_per_step"] = [round(t / args.steps * 1e3, 2) for t in per_rank]
            out["per_rank_value"] = [round(args.bs * args.steps * AUDIO_S / t, 3) for t in per_rank]
        if world > 1 and ndev < world:
            out["config"]["note"] = f"functional run: {world} ranks share {ndev} GPU(s), backend {os.environ.get('PTTS_DIST_BACKEND', 'nccl')}; not a scaling measurement"
        if extras:
            # (N > 1: the other ranks wait in the final barrier while rank 0 measures; no profiler child passes there - the committed PMC pass is quoted)
            out["roofline"] = measure_decode_roofline(model, args.bs, device, live_pmc=(world == 1))
            out["ttft_p50_ms"] = max(ttft_ranks) if ttft_ranks else round(measure_ttft(model, args.bs, device), 2)
            if ttft_ranks:
                out["per_rank_ttft_p50_ms"] = ttft_ranks  # ttft_p50_ms = the slowest rank's p50
            if world == 1:
                try:
                    out["ttft"] = measure_ttft_breakdown(model, args.bs, device)
                except Exception as e:  # noqa: BLE001 - side information
                    out["ttft"] = {"error": repr(e)[:200]}
        else:
            out["roofline"] = None
    if rank == 0 and world == 1 and with_cpu_baseline:  # a required object of the line: measured before the optional side measurements
        out["cpu_baseline"] = cpu_baseline()
        out["gpu_over_cpu"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
    disarm = arm_watchdog(out, float(os.environ.get("PTTS_BENCH_WATCHDOG_S", "600"))) if (rank == 0 and world == 1) else (lambda: None)
    if rank == 0 and world == 1 and extras and args.bs != 32 and args.model == "mini":
        # side measurement of BASELINE configs[2] (bs=32, same model): one warm-up + one timed generate()
        try:
            d32, p32 = synthetic_batch(32, 0, device)
            kw32 = dict(input_ids=d32, prompt_input_ids=p32, do_sample=False, max_new_tokens=NEW_TOKENS, min_new_tokens=NEW_TOKENS)
            model.generate(**kw32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(**kw32)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out["bs32"] = {"value": round(32 * AUDIO_S / dt, 2), "unit": "audio-seconds/sec", "ms_per_step": round(dt * 1e3, 1),
                           "ttft_p50_ms": round(measure_ttft(model, 32, device, reps=7), 2),
                           "roofline": measure_decode_roofline(model, 32, device)}
            try:
                out["bs32"]["ttft"] = measure_ttft_breakdown(model, 32, device, reps=7)
            except Exception as e:  # noqa: BLE001
                out["bs32"]["ttft"] = {"error": repr(e)[:200]}
        except Exception as e:  # side measurement must never break the contract line
            out["bs32"] = {"error": repr(e)[:200]}
    if rank == 0 and world == 1 and extras:
        try:  # the codec half of the path against ITS bound (MFMA): bf16-operand mode at 1 / 32 utterances, exact-f32 mode at 1
            out["dac"] = measure_dac(device)
        except Exception as e:
            out["dac"] = {"error": repr(e)[:200]}
    if rank == 0 and world == 1 and extras and args.model == "mini":
        try:  # EOS-terminated batches: the per-sample tail of generate() as one filter kernel + one ragged codec pass
            out["ragged_bs32"] = measure_ragged(model, device, 32)
        except Exception as e:
            out["ragged_bs32"] = {"error": repr(e)[:200]}
    if rank == 0 and world == 1 and extras and args.model == "mini" and args.dtype == "bf16":
        try:  # the whole-node lever: 128 utterances per GPU (the step is latency-bound at 32, utterances per step are nearly free until the KV stream dominates)
            dt = _timed_generate(model, 128, device)
            out["bs128"] = {"value": round(128 * AUDIO_S / dt, 2), "unit": "audio-seconds/sec", "ms_per_step": round(dt * 1e3, 1),
                            "roofline": _trim_roofline(measure_decode_roofline(model, 128, device, live_pmc=True))}
            try:  # the codec's share of that generate(): the model's own DACModel.decode on 128 x 860 frames (sub-batches as generate() runs them)
                codes128 = torch.randint(0, 1024, (1, 128, K_CODEBOOKS, FRAMES), device=device)
                model.audio_encoder.decode(codes128, [None])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.audio_encoder.decode(codes128, [None])
                torch.cuda.synchronize()
                tc = time.perf_counter() - t0
                out["bs128"]["codec_ms"] = round(tc * 1e3, 1)
                out["bs128"]["codec_share_of_generate"] = round(tc / dt, 4)
                del codes128
            except Exception as e:  # noqa: BLE001
                out["bs128"]["codec_ms"] = repr(e)[:120]
            for key in [k for k in getattr(model, "__dict__", {}).get("_engines", {}) if k[-1] == "b>8"]:  # its 11 GB KV arena is not needed any further
                model.__dict__["_engines"].pop(key).close()
        except Exception as e:
            out["bs128"] = {"error": repr(e)[:200]}
        try:  # opt-in numerics mode: e4m3 self-attention KV cache (ptts_config::kv_fp8), the lever SURVEY.md section 8(d) names for the bandwidth-bound third of the step
            model.enable_fp8_kv_cache(True)
            dt = _timed_generate(model, 128, device)
            out["bs128_kv8"] = {"value": round(128 * AUDIO_S / dt, 2), "unit": "audio-seconds/sec", "ms_per_step": round(dt * 1e3, 1),
                                "roofline": _trim_roofline(measure_decode_roofline(model, 128, device, live_pmc=False)),
                                "note": "opt-in: e4m3 self-attention cache rows + one power-of-two scale per (utterance, head, position); parity vs the oracle "
                                        "with the same quantiser (tests/test_lm_gpu.py::test_e4m3_kv_cache_mode); never the default"}
        except Exception as e:
            out["bs128_kv8"] = {"error": repr(e)[:200]}
        finally:
            try:
                model.enable_fp8_kv_cache(False)
            except Exception:  # noqa: BLE001
                pass
    if rank == 0 and world == 1 and extras and args.bs == 1:
        try:
            out["streaming"] = measure_ttfa(model, device)
        except Exception as e:
            out["streaming"] = {"error": repr(e)[:200]}
    if rank == 0 and world == 1 and extras and not args.sample and args.model == "mini":
        try:  # the reference's default generation mode (do_sample=True, init_model_600M.py:57-63): step time beside greedy
            out["sampling"] = measure_sampling_step(model, args.bs, device)
        except Exception as e:
            out["sampling"] = {"error": repr(e)[:200]}
    if rank == 0 and world == 1 and extras and args.model == "mini" and args.dtype == "bf16":
        try:  # the bit-exact (fp32) engine on the same configuration (its own model object: 288 GB of HBM hold all of them)
            out["fp32_parity_mode"] = measure_fp32_parity_mode(device)
            out["fp32_parity_mode"]["gpu_over_cpu"] = round(out["fp32_parity_mode"]["value"] / out["cpu_baseline"]["value"], 1) if "cpu_baseline" in out else None
        except Exception as e:
            out["fp32_parity_mode"] = {"error": repr(e)[:200]}
        try:  # Large-v1 shapes (configs[3] / configs[4] per GPU)
            out["large"] = measure_large(device)
        except Exception as e:
            out["large"] = {"error": repr(e)[:200]}
    disarm()
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
