"""Inputs shared by the warper tests: the records and sampler settings every file runs (tests/test_warper_model_cpu.py against transformers,
tests/test_warp_tail_gpu.py against the kernel), the random rows, and the crafted rows, each with whether the model must call it ambiguous.
numpy only."""
import numpy as np

import sampler_cases as SC
from warper_model import Warp

F32 = np.float32
ALL = Warp(0.05, 0.9, 3e-4, 2e-3)  # the values the 1 % cap of the random rows is stated for
# (name, record, temperature, top_k, top_p)
CONFIGS = [
    ("min_p", Warp(min_p=0.05), 1.0, 0, 1.0),
    ("typical_p", Warp(typical_p=0.9), 1.0, 0, 1.0),
    ("epsilon", Warp(epsilon_cutoff=3e-4), 1.0, 0, 1.0),
    ("eta", Warp(eta_cutoff=2e-3), 1.0, 0, 1.0),
    ("all four", ALL, 1.0, 0, 1.0),
    ("all four, T=0.7", ALL, 0.7, 0, 1.0),
    ("all four, T=1.4", ALL, 1.4, 0, 1.0),
    ("top-k 50, top-p 0.95, all four", ALL, 1.0, 50, 0.95),
    ("top-p 0.9, typical_p 0.5, eta", Warp(typical_p=0.5, eta_cutoff=2e-3), 0.9, 0, 0.9),
    ("top-k 20, min_p 0.2, epsilon", Warp(min_p=0.2, epsilon_cutoff=9e-3), 1.2, 20, 1.0),
]
SIGMAS = (1.5, 3.0, 5.0)


def gen(T=1.0, top_k=0, top_p=1.0, max_length=64, min_new_tokens=64, do_sample=True):
    return SC.Gen(max_length=max_length, min_new_tokens=min_new_tokens, do_sample=do_sample, temperature=T, top_k=top_k, top_p=top_p)


def random_rows(V, n, seed):
    """n rows N(0, sigma^2), sigma cycling through SIGMAS; every fourth row has 30 % of its entries at -inf."""
    rng = np.random.default_rng([V, seed])
    rows = np.empty((n, V), dtype=F32)
    for i in range(n):
        rows[i] = (rng.standard_normal(V) * SIGMAS[i % 3]).astype(F32)
        if i % 4 == 3:
            rows[i, rng.random(V) < 0.3] = -np.inf
    return rows


def crafted(V):
    """(name, row [V], record, (T, top_k, top_p), ambiguous: what the model must say) - V >= 256."""
    assert V >= 256
    ln = lambda p: np.log(np.asarray(p, dtype=np.float64)).astype(F32)  # noqa: E731
    out = []
    base = np.full(V, -9.0, dtype=F32)
    # min_p: the tied entries sit on the threshold up to the rounding of ln 0.5 - ambiguous, and all of the tie goes one way
    r = base.copy()
    r[[3, 70, 71, 200]] = [0.0, *ln([0.5] * 3)]
    out.append(("min_p tie at the threshold", r, Warp(min_p=0.5), (1.0, 0, 1.0), True))
    # min_p = 1: only entries AT the maximum survive (w = 1 exactly), a tie at the maximum stays whole
    r = base.copy()
    r[[5, 130, 131]] = [2.0, 2.0, np.nextafter(F32(2.0), F32(0.0))]
    out.append(("min_p = 1 keeps the tied maxima only", r, Warp(min_p=1.0), (1.0, 0, 1.0), True))  # the entry one ulp below has w within 4u of 1
    r = (np.random.default_rng(V).standard_normal(V) * 2).astype(F32)
    r[17] = 9.0
    out.append(("only the arg-max survives", r, Warp(min_p=1.0, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3), (1.0, 0, 1.0), False))
    r = np.full(V, -30.0, dtype=F32)
    r[64] = 0.0
    out.append(("near one-hot", r, ALL, (1.0, 0, 1.0), False))
    out.append(("uniform: every s equal, typical_p keeps all", np.full(V, 1.25, dtype=F32), Warp(typical_p=0.3, epsilon_cutoff=0.5 / V, eta_cutoff=2e-3),
                (1.0, 0, 1.0), False))
    r = (np.random.default_rng(V + 1).standard_normal(V) * 3).astype(F32)
    r[np.random.default_rng(V + 2).random(V) < 0.5] = -np.inf
    r[[0, V - 1]] = -np.inf
    out.append(("-inf entries", r, ALL, (0.8, 0, 0.98), None))  # random values: whatever the model says
    # typical_p: three tied entries straddle the boundary - one value, one s, all stay
    mass = np.full(V, 0.15 / (V - 4))
    mass[[9, 40, 41, 42]] = [0.4, 0.15, 0.15, 0.15]
    out.append(("typical_p boundary inside a tie", ln(mass), Warp(typical_p=0.6), (1.0, 0, 1.0), False))
    # typical_p drops the arg-max (its -ln p is far from the entropy of the flat rest), and epsilon then spares the maximum of what is left
    mass = np.full(V, 0.7 / (V - 1))
    mass[33] = 0.3
    out.append(("typical_p drops the arg-max, epsilon spares the rest", ln(mass), Warp(typical_p=0.5, epsilon_cutoff=0.9, eta_cutoff=0.9), (1.0, 0, 1.0), False))
    # epsilon: V entries, p = 1 / 1024 for all but one at twice that: epsilon = 2^-10 sits on the tie up to rounding
    r = np.full(1023, 0.0, dtype=F32)
    r[11] = ln(2.0)
    r = np.concatenate([r, np.full(V - 1023, -np.inf, dtype=F32)]) if V >= 1023 else None
    if r is not None:
        out.append(("epsilon tie at the threshold", r, Warp(epsilon_cutoff=2.0 ** -10), (1.0, 0, 1.0), True))
    # epsilon with every entry at the maximum: p = epsilon exactly, and ties at the maximum stay
    r = np.full(V, -np.inf, dtype=F32)
    r[:256] = 0.5
    out.append(("epsilon = p at the maximum", r, Warp(epsilon_cutoff=2.0 ** -8 * 1.5), (1.0, 0, 1.0), False))
    # eta: eta = sqrt(v) exp(-H) placed on the low group's probability
    mass = np.full(V, 0.5 / (V - 8))
    mass[:8] = 0.5 / 8
    H = -(mass * np.log(mass)).sum()
    v = float((mass[-1] * np.exp(H)) ** 2)
    assert v < 1.0 and np.sqrt(v) * np.exp(-H) < v
    out.append(("eta tie at the threshold", ln(mass), Warp(eta_cutoff=v), (1.0, 0, 1.0), True))
    return out
