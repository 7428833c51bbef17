"""Admission of n requests that carry voice prompts into a continuous session: n single ``admit_row(voice=)`` calls (one prefill pass of
P + 1 + T positions each) against ONE ``admit_rows(voices=)`` (``ptts_admit_rows_voice``: one pass of n x (P + 1 + Tmax) positions).

Shapes: Mini-v1 decoder, bf16, P = 32 prompt and N = 64 description positions, 16 slots of which 8 stay live and decode between the
admissions, n = 1 / 2 / 4 / 8 requests with T = 430 frames each (5 s) and with ragged T from 86 to 430 (n = 1: 86), on the bf16 self-attention cache and
with ``enable_fp8_kv_cache()``. Both sides are timed in the same process on the same engine, alternating, with device events around the
calls (the stream runs nothing else); the first round of every shape is a warm-up and is dropped. The figure is the GPU time from the first
launch of the admission to the first token of its last request.

    python tools/voice_admit_probe.py [--repeats 5] [--out profiles/voice_group_admission.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (model shapes, HIP event timer)

SLOTS, LIVE, T_MAX, T_MIN, NEW = 16, 8, 430, 86, 64
K = bench.K_CODEBOOKS


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


def lengths(n, ragged):
    return [int(round(x)) for x in torch.linspace(T_MIN, T_MAX, n).tolist()] if ragged else [T_MAX] * n


def measure(model, ev, n, ragged, repeats):
    """[(singles ms, group ms)] per repeat: slots LIVE .. LIVE + n - 1 are admitted, decoded for two steps and retired, once per side."""
    L = NEW + 1 + T_MAX
    eng = model._get_engine(SLOTS + 8, bench.N_DESC, bench.N_PROMPT, L, T_MAX)  # 8 spare rows for every n: one engine, one set of step graphs
    eng.set_gen_params(max_length=L, min_new_tokens=NEW)
    eng.begin_session(SLOTS, bench.N_DESC, bench.N_PROMPT, **({"kv_fp8": True} if eng.kv_fp8 else {}))
    dev = model.device
    g = torch.Generator().manual_seed(7)
    enc = torch.randn(SLOTS, bench.N_DESC, eng.H, generator=g).to(dev)
    pr = (torch.randn(SLOTS, bench.N_PROMPT, eng.H, generator=g) * 0.02).to(dev)
    for s in range(LIVE):
        eng.admit_row(s, enc[s], None, pr[s], None)
    eng.decode_steps(32)
    Ts = lengths(n, ragged)
    voices = [torch.randint(0, 1024, (K, t), generator=g, dtype=torch.long).to(dev) for t in Ts]
    rows = list(range(LIVE, LIVE + n))
    Ls = [NEW + 1 + t for t in Ts]

    def singles():
        for j, s in enumerate(rows):
            eng.admit_row(s, enc[s], None, pr[s], None, max_length=Ls[j], voice=voices[j])

    def group():
        eng.admit_rows(rows, enc[LIVE:LIVE + n], None, pr[LIVE:LIVE + n], None, max_lengths=Ls, voices=voices)

    out = []
    for r in range(repeats + 1):  # the first round warms the prefill kernels of both row counts
        pair = []
        for side in (singles, group):
            pair.append(ev.ms(side))
            eng.decode_steps(2)
            for s in rows:
                eng.retire_row(s)
        out.append(tuple(pair))
    return out[1:], eng.kv_fp8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voice_group_admission.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voice_admit_probe needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    lines = [f"voice_admit_probe: Mini-v1 bf16, P = {bench.N_PROMPT}, N = {bench.N_DESC}, {SLOTS} slots ({LIVE} live) + 8 spare rows, {args.repeats} timed repeats "
             f"per side (alternating, one warm-up round dropped), GPU ms by device events: median (min .. max)",
             f"{'cache':5} {'lengths':>14} {'n':>2} {'rows of the pass':>17} {'n x admit_row(voice=)':>30} {'one admit_rows(voices=)':>30} {'singles / group':>16}"]
    ev = Events()
    for kv8 in (False, True):
        model = bench.build_model_on_device(dev, torch.bfloat16, "mini")
        if kv8:
            model.enable_fp8_kv_cache()
        for ragged in (False, True):
            for n in (1, 2, 4, 8):  # n = 1: both sides run in place in the slot
                runs, on_kv8 = measure(model, ev, n, ragged, args.repeats)
                assert on_kv8 == kv8
                one, grp = [a for a, _ in runs], [b for _, b in runs]
                fmt = lambda xs: f"{statistics.median(xs):8.3f} ({min(xs):.3f} .. {max(xs):.3f})"
                Ts = lengths(n, ragged)
                what = f"T = {T_MAX}" if not ragged else f"T = {T_MIN}..{T_MAX}"
                pos = f"{n} x {bench.N_PROMPT + 1 + max(Ts)} ({sum(bench.N_PROMPT + 1 + t for t in Ts)} own)"
                lines.append(f"{'kv8' if kv8 else 'bf16':5} {what:>14} {n:>2} {pos:>17} {fmt(one):>30} {fmt(grp):>30} {statistics.median(one) / statistics.median(grp):>15.2f}x")
                print(lines[-1], flush=True)
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
