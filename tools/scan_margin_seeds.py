"""CPU tool (oracle only): scan candidate seeds of the free-running GPU tests for a top-2 margin >= tests/cases.MARGIN,
so that the tests can ASSERT the margin instead of guarding their bit-exact comparison with an `if`.
    python tools/scan_margin_seeds.py [case ...]
Prints, per case, the margin of the seeds currently written in tests/cases.py and the first few safe alternatives."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import cases as C
from oracle import decoder_oracle as DO


def margin_lm(spec, sd, enc, enc_mask, prompt, prompt_mask, gp, pre=None, precision="fp32"):
    tr = DO.sample_loop(DO.DecoderOracle(spec, sd, precision=precision), enc, enc_mask, prompt, prompt_mask, gp, decoder_input_ids=pre)
    return tr.min_margin


def scan(name, current, fn, cands, want=3):
    cur = fn(current)
    print(f"[{name}] current {current}: margin {cur:.2e} {'OK' if cur >= C.MARGIN * 1.5 else 'UNSAFE'}", flush=True)
    if cur >= C.MARGIN * 1.5:
        return
    found = 0
    for c in cands:
        m = fn(c)
        if m >= C.MARGIN * 1.5:
            print(f"    safe alternative {c}: margin {m:.2e}", flush=True)
            found += 1
            if found >= want:
                break


def gen_margin(model_seed, input_seed, kind, rope=False):
    with torch.no_grad():
        if kind == "eos":
            m, spec, sd, dsd = C.tiny_model(seed=model_seed, eos_gain=6.0)
            desc, dm, pid, pm, gp = C.gen_eos_inputs(input_seed)
            enc = m._encode_description_eager(desc, dm).float()
            return margin_lm(spec, sd, enc, dm, m.embed_prompts(pid).float(), pm, gp)
        if kind == "fixed":
            m, spec, sd, dsd = C.tiny_model(seed=model_seed, rope=rope)
            desc, pid, gp = C.gen_fixed_inputs(input_seed)
            enc = m._encode_description_eager(desc, None).float()
            return margin_lm(spec, sd, enc, None, m.embed_prompts(pid).float(), None, gp)
        m, spec, sd, dsd = C.tiny_model(seed=model_seed)
        desc, pid, voice, codes, gp = C.gen_voice_inputs(input_seed)
        enc = m._encode_description_eager(desc, None).float()
        return margin_lm(spec, sd, enc, None, m.embed_prompts(pid).float(), None, gp, pre=codes)


def main():
    only = set(sys.argv[1:])
    want = lambda n: not only or n in only
    torch.set_num_threads(8)
    if want("batch"):
        for b in (1, 3, 20):
            scan(f"batch{b}", C.BATCH_SEEDS[b], lambda s, b=b: margin_lm(*C.batch_case(b, s)), [(11, 100 + i) for i in range(40)])
    if want("block"):
        scan("block", C.BLOCK_SEEDS, lambda s: margin_lm(*C.block_case(s)), [(21, 100 + i) for i in range(40)])
    if want("gqa"):
        for b in (3, 12):
            scan(f"gqa{b}", C.GQA_SEEDS[b], lambda s, b=b: margin_lm(*C.gqa_case(b, s)), [(5, 100 + i) for i in range(40)])
    if want("voice_lm"):
        for sd_ in C.VOICE_LM_SEEDS:
            def f(s):
                spec, sd, enc, prompt, pre, gp = C.voice_lm_case(s)
                return min(margin_lm(spec, sd, enc, None, prompt, None, gp, pre=pre), margin_lm(spec, sd, enc, None, prompt, None, gp))
            scan(f"voice_lm{sd_}", sd_, f, list(range(100, 160)))
    if want("gen_eos"):
        scan("gen_eos", C.GEN_EOS_SEEDS, lambda s: gen_margin(s[0], s[1], "eos"), [(3, 100 + i) for i in range(40)])
    if want("gen_fixed"):
        for rope in (False, True):
            scan(f"gen_fixed rope={rope}", C.GEN_FIXED_SEEDS[rope], lambda s, rope=rope: gen_margin(s[0], s[1], "fixed", rope), [(2, 100 + i) for i in range(40)])
    if want("stream_e2e"):  # tests/test_continuous_streaming_gpu.py: one request per (input seed, max_new_tokens), each scanned on its own
        import test_continuous_streaming_gpu as TS

        m, spec, sd, dsd = C.tiny_model(seed=TS.E2E_MODEL_SEED)
        for seed, n in TS.E2E_SCANNED:
            f = lambda s, n=n: TS.e2e_oracle(m, spec, sd, dsd, TS.e2e_request(s, n), "cpu")[0].min_margin
            scan(f"stream_e2e {n} tokens", seed, f, list(range(500, 700)), want=1)
    if want("session_voice"):  # tests/session_voice_cases.py: one request per (T, max_length), each alone, with and without its prefix
        import session_voice_cases as VC

        sd = VC.weights()
        for T, L, seed in VC.FREE_RUNNING:
            scan(f"session_voice T={T} L={L}", seed, lambda s, T=T, L=L: VC.margin(T, L, s, sd), list(range(700, 900)), want=1)
        sde = VC.weights(eos_gain=6.0)
        L = VC.MIN_NEW_MAX_LENGTH
        scan("session_voice min_new", VC.MIN_NEW_SEED,
             lambda s: min(VC.margin(4, L, s, sde, min_new=3), VC.margin(0, L, s + 1, sde, min_new=5), VC.margin(4, L, s + 2, sde, min_new=4),
                           VC.margin(4, L, s + 2, sde, min_new=5)), list(range(720, 1400, 3)), want=1)
    if want("gen_voice"):
        scan("gen_voice", C.GEN_VOICE_SEEDS, lambda s: gen_margin(s[0], s[1], "voice"), [(0, 100 + i) for i in range(40)])


if __name__ == "__main__":
    main()
