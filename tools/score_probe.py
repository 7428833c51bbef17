"""Device-event times of teacher-forced scoring at sizes a user would run: Mini-v1 widths, bf16, T = 860 and 2580 columns, 1 and 8 utterances.
  (a) ptts_score without logits, (b) with logits: the C call alone on preallocated buffers (no torch allocation or Python validation inside);
  (c) the heads + loss stage alone (score_launch through tests/native/score_harness.hip), no-store and store;
  (d) the baseline the parent commit offers: the existing PRO_LN / EPI_STORE projection over the same rows (rows_prep + GEMM, as
      ptts_lm.hip's ln_gemm runs it) into an fp32 [rows, K * V] buffer + torch.nn.functional.cross_entropy on it.
(c) and (d) alternate in one process; every figure is the median (min .. max) of REPS runs after WARM warm-ups. Also states the bytes the no-store
path never allocates. Prints and records through tests/helpers.py::log_parity (the record is committed as profiles/score_forward.txt)."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import score_harness as SH  # noqa: E402
from helpers import log_parity, make_engine  # noqa: E402
from oracle import decoder_oracle as DO  # noqa: E402
from parler_tts_amd import _native as N  # noqa: E402

OUT = "score_forward.txt"
WARM, REPS = 2, 7


def timed_alternating(fns):
    """[(median, min, max) ms per fn]; the functions run in turn inside every repetition."""
    for _ in range(WARM):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [(sorted(m)[len(m) // 2], min(m), max(m)) for m in ms]


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}) ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    layers = ap.parse_args().layers
    spec = DO.DecoderSpec(num_hidden_layers=layers, max_position_embeddings=4096)
    sd = DO.make_decoder_weights(spec, seed=1)
    N_ENC, P, K, V, H = 32, 16, spec.num_codebooks, spec.vocab_size, spec.hidden_size
    g = torch.Generator().manual_seed(2)
    har = SH.Harness(SH.build(SH.default_dir()))
    heads = torch.cat([sd[f"lm_heads.{k}.weight"] for k in range(K)]).float().cuda()
    packed = har.pack(True, heads)
    gamma, beta = sd["model.decoder.layer_norm.weight"].float().cuda(), sd["model.decoder.layer_norm.bias"].float().cuda()
    log_parity(f"--- tools/score_probe.py: Mini-v1 widths, {layers} layers, bf16, N = {N_ENC}, P = {P}; median (min .. max) of {REPS} runs after {WARM} "
               f"warm-ups, device events", OUT)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B in (1, 8):
        eng = make_engine(spec, sd, dtype=torch.bfloat16, max_batch=B, max_ctx=2600, max_enc=N_ENC, max_prompt=2600)
        for T in (860, 2580):
            Q = P + T
            enc = torch.randn(B, N_ENC, H, generator=g).cuda()
            prompt = (torch.randn(B, P, H, generator=g) * 0.5).cuda()
            ids = torch.randint(0, 1024, (B * K, T), generator=g).cuda()
            labels = torch.randint(0, 1024, (B, T, K), generator=g).cuda()
            nll = torch.empty(B, T, K, device="cuda")
            counted = torch.empty(B, T, K, dtype=torch.int32, device="cuda")
            logits = torch.empty(B * K, Q, V, device="cuda")
            p = lambda t: C.c_void_p(t.data_ptr())
            io0 = N.PttsScoreIO(p(ids), p(labels), p(nll), p(counted), C.c_void_p())
            io1 = N.PttsScoreIO(p(ids), p(labels), p(nll), p(counted), p(logits))

            def call(io):
                N.check(eng.lib.ptts_score(eng._h, p(enc), None, p(prompt), None, B, N_ENC, P, T, C.byref(io), stream), "ptts_score")

            ta, tb = timed_alternating([lambda: call(io0), lambda: call(io1)])
            # the stage alone, on the residual rows a pass leaves behind (random rows of the same shape: the stage's time does not depend on them)
            x = torch.randn(B * Q, H, generator=g).cuda()
            xt = x.view(B, Q, H)[:, P:].reshape(B * T, H).contiguous()  # the T labelled rows of each utterance, consecutive for the baseline
            common = dict(gamma=gamma.data_ptr(), beta=beta.data_ptr(), W=packed.data_ptr(), x_ld=H, H=H, K=K, V=V)
            a0 = SH.ShArgs(x=x.data_ptr(), ids=ids.data_ptr(), labels=labels.data_ptr(), nll=nll.data_ptr(), counted=counted.data_ptr(), logits=None,
                           B=B, Q=Q, Qs=T, T=T, bos=spec.bos_token_id, eos=spec.eos_token_id, **common)
            a1 = SH.ShArgs(x=x.data_ptr(), ids=ids.data_ptr(), labels=labels.data_ptr(), nll=nll.data_ptr(), counted=counted.data_ptr(),
                           logits=logits.data_ptr(), B=B, Q=Q, Qs=Q, T=T, bos=spec.bos_token_id, eos=spec.eos_token_id, **common)
            out = torch.empty(B * T, K * V, device="cuda")
            xw = torch.empty(B * T * H * 2, dtype=torch.uint8, device="cuda")
            pa = SH.ShArgs(x=xt.data_ptr(), xw=xw.data_ptr(), out=out.data_ptr(), M=B * T, **common)
            flat = labels.reshape(B * T * K)

            def baseline():
                har.check(har.project(True, pa))
                return torch.nn.functional.cross_entropy(out.view(B * T * K, V), flat, reduction="none")

            tc0, td, tc1 = timed_alternating([lambda: har.check(har.score(True, a0)), baseline, lambda: har.check(har.score(True, a1))])
            log_parity(f"B = {B} T = {T}: (a) ptts_score without logits {fmt(ta)}; (b) with logits {fmt(tb)}; (c) heads + loss stage alone, no-store "
                       f"{fmt(tc0)}, store (all {Q} rows) {fmt(tc1)}; (d) PRO_LN / EPI_STORE projection + torch cross_entropy {fmt(td)}; "
                       f"no-store / baseline = {tc0[0] / td[0]:.2f}; logits never allocated without the output: {B * K * Q * V * 4 / 2 ** 20:.0f} MiB", OUT)
            del logits, out, xw
            torch.cuda.empty_cache()
        eng.close()


if __name__ == "__main__":
    main()
