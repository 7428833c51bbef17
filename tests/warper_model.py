"""A host restatement, in float64, of the four stages the WARP instances of the sampler tail add behind top-p (``wave_sample_row<NV, true>``,
parler_tts_amd/csrc/ptts_lm_kernels.h): min_p -> typical_p -> epsilon_cutoff -> eta_cutoff, each on the distribution renormalised over the
survivors of the stage before. It stands on ``sampler_model.kept_set`` (temperature -> top-k -> top-p) and returns the same ``Kept`` record, so
``sampler_model.TailModel`` steps with it unchanged (``step_with_records``). tests/test_warper_model_cpu.py pins it against transformers' own
chain; tests/test_warp_tail_gpu.py compares the kernel with it token for token.

The contract, in exact arithmetic (w_i = exp(x_i - max x) over the survivors, tot = sum w, p_i = w_i / tot, H = -sum p ln p):
  min_p           drop i iff p_i < v p_max, i.e. w_i < v (the arg-max has w = 1)
  typical_p       s_i = |-ln p_i - H|; keep i iff mass{j : s_j < s_i} < v tot. Entries tied with the boundary value stay, the smallest s stays
  epsilon_cutoff  drop i iff p_i < v and x_i is below the largest surviving score
  eta_cutoff      eta = min(v, sqrt(v) exp(-H)); drop i iff p_i < eta and x_i is below the largest surviving score
A stage at its neutral value (0, 1, 0, 0) is skipped.

Rounding bands. u = 2^-24 is half an ulp, relative. The device holds w_i = expf(fl(x_i - max x)), within 2 ulp = 4u of the float64 value the
model computes from the same fp32 difference d_i = fl(max x - x_i) (a subtraction of two fp32 numbers: the model forms it in fp32 too, so d_i
carries no band). Every fp32 sum over a row is NV per-lane adds and 6 wave levels, each rounding at most u of the (non-negative) total.
  * min_p: w_i (4u) against the fp32 constant v (exact): a comparison within 4u v is ambiguous. An entry at the maximum has w = expf(0) = 1
    exactly and is never ambiguous.
  * masses against v tot (typical_p): the top-p predicate's chain, ``sampler_model.band``.
  * p_i against epsilon: the device compares w_i (4u) with fl(v tot): tot is (NV + 6) roundings and the numerators' 4u, the product one more -
    (NV + 7 + 4 + 4) u = (NV + 15) u relative. The band used is ``sampler_model.band(V, 1)`` = (2 NV + 16) u, which covers it.
  * H: the device never forms ln tot. It computes A = (sum w_i d_i) / tot = H - ln tot, and -ln p_i - H = d_i - A. A term w_i d_i is 4u of w and
    one rounding of the product (5u), the sum (NV + 6) u, tot (NV + 10) u, the quotient u: dA <= (2 NV + 22) u A, used as (2 NV + 23) u A.
  * p_i against eta: fl(sqrtf(v) expf(-A)) is u (sqrtf) + dA absolute in the exponent, i.e. relative in the value, + 4u (expf) + u (product);
    against w_i (4u): (2 NV + 23) A u + 10 u relative. The other branch of the min is the epsilon comparison; the band is the larger of the two.
  * the ORDER of s_i = fl(|d_i - A|) at the typical-p boundary: d_i is exact, A is off by dA and the subtraction rounds once (u s). Two entries
    on the same side of A keep their order whatever A is (rounding is monotone; at worst they collapse into a tie: one ulp of s separates
    "strictly below" from "tied"), and entries with equal d have equal s bit for bit. Two entries on opposite sides of A move against each
    other: their s differ reliably only beyond 2 dA + one ulp. An entry within dA of A itself is on neither side for certain.
    So mass{s_j < s_i} is bracketed: surely below = the mass of entries below by more than the tolerance of the pair, possibly below = that plus
    the entries within it; i is kept for certain if possibly-below + band < v tot, dropped for certain if surely-below - band >= v tot.
A row where any decision falls inside its band is AMBIGUOUS; ``variants`` then holds the weight vectors with the doubtful groups dropped and
kept (every later stage applied to each), which is what ``TailModel.step`` accepts a draw from."""
import collections
import types

import numpy as np

import sampler_model as SM

F32 = np.float32
U = 2.0 ** -24

Warp = collections.namedtuple("Warp", "min_p typical_p epsilon_cutoff eta_cutoff", defaults=(0.0, 1.0, 0.0, 0.0))
NEUTRAL = Warp()


def _h_band(V):
    """Relative error of A = H - ln tot as the device computes it, per unit of A."""
    return (2 * SM.nv_of(V) + 23) * U


def _split(w, keep, near):
    """(nominal, doubtful groups dropped, doubtful groups kept) of one stage over the entries with w > 0."""
    on = w > 0
    nom, lo, hi = (np.where(on & m, w, 0.0) for m in (keep, keep & ~near, keep | near))
    if not lo.any():  # the arg-max (min_p, cut-offs) or the smallest s (typical_p) always stays on the device
        lo = nom
    return nom, lo, hi


def _spread(w, d):
    """A = sum w_i d_i / tot over the survivors: H - ln tot."""
    on = w > 0
    return float((w[on] * d[on]).sum() / w.sum())


def _min_p(w, d, v, V):
    keep = w >= v
    near = (np.abs(w - v) <= 4 * U * v) & (d > 0)
    return _split(w, keep | (d == 0), near)


def _typical(w, d, v, V):
    on = np.nonzero(w > 0)[0]
    tot = w.sum()
    A = _spread(w, d)
    dA = _h_band(V) * A
    vals, inv = np.unique(d[on], return_inverse=True)  # entries with equal d share their s bit for bit
    gm = np.bincount(inv, weights=w[on])
    s = np.abs(vals - A)
    side = np.where(np.abs(vals - A) > dA, np.sign(vals - A), 0.0)
    ulp = 2 * U * max(float(s.max()), A, 1e-30)
    opp = 2 * dA + ulp
    sure, maybe, below = np.zeros(len(s)), np.zeros(len(s)), np.zeros(len(s))
    for c in (1.0, -1.0, 0.0):  # the groups of one side, sorted by s, and the mass of those with s < t
        sel = np.nonzero(side == c)[0]
        order = sel[np.argsort(s[sel])]
        cum = np.concatenate([[0.0], np.cumsum(gm[order])])
        mass_lt = lambda t: cum[np.searchsorted(s[order], t, side="left")]  # noqa: E731
        same = (side == c) & (c != 0)
        sure += mass_lt(s - np.where(same, ulp, opp))
        maybe += mass_lt(s + np.where(same, 0.0, opp))
        below += mass_lt(s)
    maybe -= np.where(side == 0, gm, 0.0)  # an entry is never below itself
    thr, bd = v * tot, SM.band(V, tot)
    keep_g = below < thr
    near_g = ~((maybe + bd < thr) | (sure - bd >= thr))
    keep, near = np.zeros(w.shape, bool), np.zeros(w.shape, bool)
    keep[on], near[on] = keep_g[inv], near_g[inv]
    return _split(w, keep, near)


def _cutoff(w, d, thr_p, rel, V):
    """drop p_i < thr_p below the maximum; ``rel``: the relative band of the comparison."""
    p = w / w.sum()
    below = d > d[w > 0].min()  # under the largest surviving score (typical_p may have dropped the arg-max)
    keep = ~((p < thr_p) & below)
    near = (np.abs(p - thr_p) <= rel * thr_p) & below
    return _split(w, keep, near)


def _epsilon(w, d, v, V):
    return _cutoff(w, d, v, SM.band(V, 1.0), V)


def _eta(w, d, v, V):
    A = _spread(w, d)
    H = A + np.log(w.sum())
    eta = min(v, np.sqrt(v) * np.exp(-H))
    return _cutoff(w, d, eta, max(SM.band(V, 1.0), _h_band(V) * A + 10 * U), V)


def stages(wp):
    """The active stages of a record, in the kernel's (= transformers') order, with their fp32 constants."""
    out = []
    if wp.min_p > 0.0:
        out.append((_min_p, float(F32(wp.min_p))))
    if wp.typical_p < 1.0:
        out.append((_typical, float(F32(wp.typical_p))))
    if wp.epsilon_cutoff > 0.0:
        out.append((_epsilon, float(F32(wp.epsilon_cutoff))))
    if wp.eta_cutoff > 0.0:
        out.append((_eta, float(F32(wp.eta_cutoff))))
    return out


def warp_kept(logits_f32, gp, wp, eos_blocked, eos):
    """``sampler_model.kept_set`` followed by the stages of ``wp``: a ``sampler_model.Kept``."""
    ks = SM.kept_set(logits_f32, gp, eos_blocked, eos)
    todo = stages(Warp(*wp))
    if not todo:
        return ks
    V = ks.weights.shape[0]
    x = np.asarray(logits_f32, dtype=F32).copy()  # the scores the device recomputes: the processors' -inf, then l / T in fp32
    if eos_blocked:
        x[eos] = -np.inf
    with np.errstate(invalid="ignore"):
        x = (x / F32(gp.temperature)).astype(F32)
        d = (x.max() - x).astype(F32).astype(np.float64)
    nominal, variants = ks.weights, list(ks.variants)
    for fn, v in todo:
        nominal = fn(nominal, d, v, V)[0]
        nxt = []
        for w in variants:
            for r in fn(w, d, v, V):
                if not any(np.array_equal(r, o) for o in nxt):
                    nxt.append(r)
        variants = nxt
    ambiguous = ks.ambiguous or len(variants) > 1
    mask = nominal > 0
    return SM.Kept(mask, nominal, ambiguous, variants if ambiguous else [nominal], ks.tiny & mask)


class _Cache:
    """Stands in for ``TailModel._kept``: the kept set of (row, EOS blocked, temperature, top_k, top_p) under the record ``wp`` in force."""

    def __init__(self, eos):
        self.eos, self.wp, self.sets = eos, NEUTRAL, {}

    def get(self, key, default=None):
        full = (key, tuple(self.wp))
        if full not in self.sets:
            gp = types.SimpleNamespace(temperature=key[2], top_k=key[3], top_p=key[4])
            self.sets[full] = warp_kept(np.frombuffer(key[0], dtype=F32), gp, self.wp, key[1], self.eos)
        return self.sets[full]


def step_with_records(model, logits, gp, recs, slots=None, **kw):
    """``TailModel.step`` with utterance b under the record ``recs[b]``. One call per utterance, last first: the static model's "has the loop
    exited" reads cur_len[0] and flags that a row finishing in this very launch still satisfies, so it answers the same for every call."""
    if not isinstance(model._kept, _Cache):
        model._kept = _Cache(model.eos)
    live = []
    for b in sorted(range(model.B) if slots is None else slots, reverse=True):
        model._kept.wp = Warp(*recs[b])
        live += model.step(logits, gp, slots=[b], **kw)
    return sorted(live)
