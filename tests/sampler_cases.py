"""Inputs of the sampler-tail tests, shared by the GPU file (tests/test_sampler_tail_gpu.py) and the CPU file that checks the
restatement and the exclusion cap on the reference alone (tests/test_sampler_model_cpu.py). numpy only."""
from dataclasses import dataclass

import numpy as np

import sampler_model as SM

F32 = np.float32
AMBIGUOUS_CAP = 0.04  # largest share of draws a sampled configuration may exclude as ambiguous

# found by find_special_seeds() (tests/test_sampler_model_cpu.py): at column SPECIAL_T, global row SPECIAL_ROW the hash's top 24 bits
# are all ones (u == 1.0f) / all zeros (u == 2^-25, the smallest)
SPECIAL_T, SPECIAL_ROW = 1, 0
SEED_U_ONE = 24613444
SEED_U_MIN = 6276048


@dataclass
class Gen:
    """DevGen without the seed."""
    max_length: int
    min_new_tokens: int = 0
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    use_eos_gate: bool = True


def ids_of(V):
    """(eos, pad, bos) every shape uses: eos = pad = V - 8, bos = V (the table's extra row)."""
    return V - 8, V - 8, V


# ---- greedy ------------------------------------------------------------------------------------------------------------------------
GREEDY_SHAPES = [(16, 1, 1), (64, 4, 3), (512, 9, 2), (528, 10, 2), (1088, 9, 5), (1152, 17, 2), (1168, 9, 2), (2048, 32, 2)]
GREEDY_MIN_NEW = 2


def greedy_steps(K):
    return 2 * K + 6


def greedy_max_length(K):
    return 2 * K + 3  # the utterance that never draws EOS ends on it at step 2K + 1; the steps after are no-ops


def greedy_logits(V, K, B, step, eos, seed=0):
    """Scripted logits [B][K][V] of one step: random rows whose maximum is an exact tie (the first index must win) - across lanes, and
    across the 64 i stride of one lane where the vocabulary has one; a hot EOS (blocked by MinNewTokens in the first steps and by the gate
    for k > first_unf afterwards, so that it cascades codebook by codebook) from step GREEDY_MIN_NEW + b on for every utterance but the
    last of several, which runs into max_length; and, at step 1, a row whose only finite entry is the blocked EOS (token 0)."""
    rng = np.random.default_rng([seed, V, K, step])
    lg = (rng.standard_normal((B, K, V)) * 2).astype(F32)
    for b in range(B):
        for k in range(K):
            r = lg[b, k]
            top = F32(r.max() + 1.0)
            if V > 64 and (b + k + step) % 2:  # same lane, 64 i stride: v and v + 64 (+ 128)
                v = int(rng.integers(0, 64))
                tie = [v + 64 * i for i in range(1, min(4, (V - v - 1) // 64 + 1))]
            else:  # different lanes
                tie = sorted(int(v) for v in rng.choice(V, size=min(3, V), replace=False))
            tie = [v for v in tie if v != eos] or [0]
            r[tie] = top
            hot = step >= GREEDY_MIN_NEW + b if (B == 1 or b < B - 1) else False
            if hot or (step < GREEDY_MIN_NEW and (b + k) % 2 == 0):
                r[eos] = top + F32(5.0)  # wins unless blocked
    if step == 1:
        lg[0, K - 1, :] = -np.inf
        lg[0, K - 1, eos] = 1.0
    return lg


# ---- sampled -----------------------------------------------------------------------------------------------------------------------
SAMPLED_SHAPES = [(64, 4), (512, 9), (1088, 9), (1152, 17), (2048, 9)]
SAMPLED_STEPS = 6


def sampled_configs(V):
    """(name, temperature, top_k, top_p)"""
    out = [(f"T{T}", T, 0, 1.0) for T in (0.05, 0.7, 1.0, 3.0)]
    out += [(f"k{n}", 1.0, k, 1.0) for n, k in (("1", 1), ("2", 2), ("50", 50), ("V-1", V - 1), ("V", V), ("V+5", V + 5))]
    out += [(f"p{p}", 1.0, 0, p) for p in (0.1, 0.9, 0.999)]
    out += [("T0.7_k50_p0.9", 0.7, 50, 0.9)]
    return out


def sampled_batch(K):
    """Utterances so that B * K * SAMPLED_STEPS >= 500 draws."""
    return -(-500 // (K * SAMPLED_STEPS))


ROW_KINDS = ("flat", "tie_k", "tie_p", "neg_inf", "peaked")


def _row(kind, V, top_p, rng, sigma=2.0):
    if kind == "flat":
        r = rng.standard_normal(V) * sigma
    elif kind == "tie_k":  # one maximum, then a tie of 3 at the second value: top_k = 2 keeps all four
        r = rng.standard_normal(V) * sigma
        top = r.max()
        pos = rng.choice(V, size=4, replace=False)
        r[pos[0]] = top + 2.0
        r[pos[1:]] = top + 1.0
    elif kind == "tie_p":  # a tie of 3 that straddles the top-p boundary: mass p - d strictly above it, d each, the rest below
        p = top_p if top_p < 1.0 else 0.9
        d = min((1.0 - p) / 3, p / 4)
        rest = rng.uniform(0.5, 1.0, V - 4)
        rest *= (1.0 - (p - d) - 3 * d) / rest.sum()
        assert rest.max() < d
        mass = np.concatenate([[p - d, d, d, d], rest])
        r = np.log(mass)[rng.permutation(V)]
    elif kind == "neg_inf":
        r = rng.standard_normal(V) * sigma
        r[rng.random(V) < 0.3] = -np.inf
        r[int(rng.integers(0, V))] = 1.0
    else:  # peaked: the numerators of most entries underflow to 0 at every temperature used (exp(-400 / 3) < 2^-149)
        r = np.full(V, -400.0)
        pos = rng.choice(V, size=3, replace=False)
        r[pos] = [0.0, -1.0, -2.5]
    return r.astype(F32)


def sampled_logits(V, K, B, gp, eos, seed=0):
    """[B][K][V]: row (b, k) is of kind ROW_KINDS[(b + k) % 5]. A row whose KEPT SET is ambiguous under gp (a mass within the rounding band
    of top_p) would make every draw from it ambiguous, so it is drawn again: the inputs are chosen on the reference alone."""
    lg = np.empty((B, K, V), dtype=F32)
    for b in range(B):
        for k in range(K):
            for attempt in range(50):
                rng = np.random.default_rng([seed, V, b, k, attempt])
                # flatter rows after 10 / 20 attempts: at top_p = 0.999 over 2048 entries the entries at the boundary of an N(0, 2^2) row
                # weigh less than the band, at N(0, 0.5^2) they weigh 25 times as much
                r = _row(ROW_KINDS[(b + k) % 5], V, gp.top_p, rng, sigma=(2.0, 1.0, 0.5, 0.5, 0.5)[attempt // 10])
                if not SM.kept_set(r, gp, True, eos).ambiguous and not SM.kept_set(r, gp, False, eos).ambiguous:
                    break
            else:
                raise AssertionError("no unambiguous row found")
            lg[b, k] = r
    return lg


def flat_logits(V, K, B, gp, eos, seed, hot=None):
    """[B][K][V] of flat random rows, each drawn again (as in sampled_logits, on the reference alone) until its kept set under gp is
    unambiguous with EOS blocked, with EOS free and - ``hot`` given - with EOS raised to ``hot``. Greedy gp: plain random rows."""
    lg = np.empty((B, K, V), dtype=F32)
    for b in range(B):
        for k in range(K):
            for attempt in range(50):
                rng = np.random.default_rng([*seed, b, k, attempt])
                r = _row("flat", V, gp.top_p, rng, sigma=(2.0, 1.0, 0.5, 0.5, 0.5)[attempt // 10])
                rows = [(r, True), (r, False)]
                if hot is not None:
                    h = r.copy()
                    h[eos] = hot
                    rows.append((h, False))
                if not gp.do_sample or not any(SM.kept_set(x, gp, blocked, eos).ambiguous for x, blocked in rows):
                    break
            else:
                raise AssertionError("no unambiguous row found")
            lg[b, k] = r
    return lg


# ---- the gate under sampling ----------------------------------------------------------------------------------------------------------
GATE_SHAPES = [(512, 9, 3), (1168, 4, 2)]
GATE_HOT = 30.0  # EOS logit: e^-20 of the mass is left for everything else


def gate_gen(K):
    return Gen(max_length=K + 8, min_new_tokens=3, do_sample=True, temperature=0.9, top_k=50, top_p=0.95)


def gate_steps(K):
    return K + 7


def gate_logits(V, K, B, step, gp, eos):
    lg = flat_logits(V, K, B, gp, eos, (V, step), hot=GATE_HOT)
    lg[:, :, eos] = GATE_HOT
    return lg


# ---- sessions ---------------------------------------------------------------------------------------------------------------------------
SESSION_CASES = [(64, 4, 3, False), (64, 4, 3, True), (1088, 9, 12, False), (1088, 9, 12, True), (2048, 17, 3, False), (2048, 17, 3, True)]
SESSION_HOT = 40.0


def session_gen(sample):
    """DevGen of a session case; its max_length is not what a slot stops on."""
    return Gen(max_length=5, min_new_tokens=0, do_sample=sample, temperature=0.9, top_k=50 if sample else 0, top_p=0.95 if sample else 1.0)


def session_steps(K):
    return 2 * K + 8


def session_maxlen(K):
    """slot 0: below 2K - 1 (no delay pattern); slot 1: ends mid-run on its own length; every other slot: never reached."""
    return {0: max(2 * K - 3, 3), 1: 2 * K + 2}


def session_events(V, K, B, sample):
    """The launches of one session case, in order: ("reset", slot, live, max_length), ("admit", slot, logits) - the grid-1 launch with row0 =
    slot - and ("step", s, logits). Every slot starts idle; slot b < B - 1 is admitted at step b % 4, slot 0 a second time (after it has
    finished) 6 steps before the end, the last slot never; of 12 slots, 2, 5 and 8 end on EOS cascading through the gate (hot from step 5 + b).
    Sampled: one set of re-drawn rows serves every launch (the hash differs by column and row); greedy: fresh random rows per launch."""
    eos = V - 8
    gp, steps, maxlen = session_gen(sample), session_steps(K), session_maxlen(K)
    for b in range(B):
        yield ("reset", b, 0, steps + 6)
    base = flat_logits(V, K, B, gp, eos, (V, K), hot=SESSION_HOT) if sample else None
    for s in range(steps):
        rng = np.random.default_rng([V, K, s])
        for b in [b for b in range(B - 1) if b % 4 == s] + ([0] if s == steps - 6 else []):
            yield ("reset", b, 1, maxlen.get(b, steps + 6))
            yield ("admit", b, base.copy() if sample else (rng.standard_normal((B, K, V)) * 2).astype(F32))
        lg = base.copy() if sample else (rng.standard_normal((B, K, V)) * 2).astype(F32)
        for b in range(2, B, 3):
            if s >= 5 + b:
                lg[b, :, eos] = SESSION_HOT
        yield ("step", s, lg)
