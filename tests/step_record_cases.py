"""Inputs of the step-record tests, shared by the GPU file (tests/test_record_tail_gpu.py) and the CPU file that checks the host model and the
exclusion cap on the model alone (tests/test_step_record_model_cpu.py). numpy only."""
import numpy as np

import sampler_cases as SC
import warper_cases as WC
import warper_model as WM

F32 = np.float32
SHAPES = [(64, 4, 3), (1088, 9, 2), (2048, 9, 2)]  # (V, K, B): one shape per NV (8, 18, 32)
STEPS = 4
MIN_NEW = 2  # EOS blocked everywhere in steps 0 and 1, by the gate above first_unf afterwards


def plain_cases(V):
    """(name, Gen) without warpers: greedy and sampler_cases.sampled_configs."""
    out = [("greedy", SC.Gen(max_length=STEPS + 3, min_new_tokens=MIN_NEW, do_sample=False))]
    for name, T, top_k, top_p in SC.sampled_configs(V):
        out.append((name, SC.Gen(max_length=STEPS + 3, min_new_tokens=MIN_NEW, do_sample=True, temperature=T, top_k=top_k, top_p=top_p)))
    return out


def plain_logits(V, K, B, gp):
    """[B][K][V], the row kinds of sampler_cases.ROW_KINDS (flat, ties at top-k and top-p, -inf entries, peaked: entries whose numerators underflow)."""
    eos = SC.ids_of(V)[0]
    if not gp.do_sample:
        return SC.greedy_logits(V, K, B, 1, eos, seed=5)
    return SC.sampled_logits(V, K, B, gp, eos, seed=3)


def warp_cases(V):
    """(name, Gen, records [B]) with the WARP instances: warper_cases.CONFIGS, utterance 0 under the configuration's record, utterance 1 under the
    next one's, any further one neutral."""
    out = []
    n = len(WC.CONFIGS)
    for i, (name, wp, T, top_k, top_p) in enumerate(WC.CONFIGS):
        gp = SC.Gen(max_length=STEPS + 3, min_new_tokens=MIN_NEW, do_sample=True, temperature=T, top_k=top_k, top_p=top_p)
        out.append((name, gp, [wp, WC.CONFIGS[(i + 3) % n][1], WM.NEUTRAL]))
    return out


def warp_logits(V, K, B, case):
    return WC.random_rows(V, B * K, 40 + case).reshape(B, K, V)


def far_below_logits(V, K, B):
    """top_p == 1: rows with entries 110 .. 300 below the maximum (numerators underflow to 0 in fp32) and a band in fp32's subnormal range
    (88 .. 103 below): all of them must keep a finite score."""
    rng = np.random.default_rng([V, K, 77])
    lg = (rng.standard_normal((B, K, V)) * 2).astype(F32)
    for b in range(B):
        for k in range(K):
            top = lg[b, k].max()
            at = int(lg[b, k].argmax())
            far = rng.choice(V, size=V // 4, replace=False)
            far = far[far != at]
            lg[b, k, far] = top - rng.uniform(110.0, 300.0, far.size).astype(F32)
            sub = rng.choice(V, size=max(V // 16, 2), replace=False)
            sub = sub[sub != at]
            lg[b, k, sub] = top - rng.uniform(88.0, 103.0, sub.size).astype(F32)
    return lg


def session_case(V, K, S, L, sample, warp):
    """(Gen, warper records or None, logits [S][K][V]) of the session test: no EOS (-30), every slot ends on its own length."""
    eos = SC.ids_of(V)[0]
    gp = SC.Gen(max_length=L, min_new_tokens=1, do_sample=sample, temperature=0.7 if sample else 1.0, top_k=50 if sample else 0, top_p=0.9 if sample else 1.0)
    wps = [WM.Warp(min_p=0.05, typical_p=0.9)] * S if warp else None
    if warp and sample:
        lg = warp_logits(V, K, S, 3)
    elif sample:
        lg = SC.flat_logits(V, K, S, gp, eos, (V, K, 5), hot=-30.0)
    else:
        lg = (np.random.default_rng([V, K]).standard_normal((S, K, V)) * 2).astype(F32)
    lg[:, :, eos] = -30.0
    return gp, wps, lg


# the warper records the far-below rows also run under (WARP instances): each stage alone - an entry whose numerator underflowed to 0 is below
# every positive threshold, so each of them must record it as removed - and two of them together
FAR_BELOW_WARPS = [WM.Warp(min_p=0.05), WM.Warp(typical_p=0.9), WM.Warp(epsilon_cutoff=3e-4), WM.Warp(eta_cutoff=2e-3), WM.Warp(typical_p=0.9, eta_cutoff=2e-3)]
