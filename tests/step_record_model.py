"""A host model of one recorded row of the step records (include/ptts_step_record.h): what the RECORD instances of the sampler tail store for
a codebook row, i.e. the vector transformers' ``_sample`` appends to ``scores``. It stands on ``sampler_model.kept_set`` (temperature -> top-k ->
top-p) and ``warper_model.warp_kept`` (the four stages behind top-p) for WHICH entries survive, and on the fp32 division the sampler itself
performs for their values, so outside the entries it calls doubtful the comparison with the device is bit for bit.

  greedy    the logits as the tail reads them, -inf at the EOS entry where it is blocked; every other entry keeps its bits
  sampling  float32(l) / float32(T) (IEEE: the device's bits), -inf at the blocked EOS and at every entry a stage removed

The kept mask comes from the stages' thresholds, never from "the numerator is non-zero": with top_p == 1 and no warper stage every finite
entry is kept, also one whose numerator underflows in fp32 (``Kept.tiny`` and below). A warper stage compares a probability with a positive
threshold, so it removes such an entry; so does top-p < 1 (its mass lies below every boundary).

``maybe`` marks the entries of an AMBIGUOUS row that may be kept or dropped: the ``near`` groups of the top-p boundary and whatever differs
between the ``variants`` of the warper stages (a decision inside its rounding band, sampler_model.band / warper_model). Exact ties at the
top-p boundary are not doubtful here: the device keeps all of the tie; transformers' sort keeps some of it."""
import numpy as np

import sampler_model as SM
import warper_model as WM

F32 = np.float32


def recorded_row(logits_f32, gp, wp, eos_blocked, eos):
    """(expected float32 [V], maybe bool [V]) of one codebook row under the sampler settings ``gp`` and the warper record ``wp``."""
    lg = np.asarray(logits_f32, dtype=F32)
    V = lg.shape[0]
    if not gp.do_sample:
        x = lg.copy()
        if eos_blocked:
            x[eos] = -np.inf
        return x, np.zeros(V, dtype=bool)
    x = lg.copy()
    if eos_blocked:
        x[eos] = -np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        x = (x / F32(gp.temperature)).astype(F32)
    wp = WM.Warp(*wp) if wp is not None else WM.NEUTRAL
    ks = WM.warp_kept(lg, gp, wp, eos_blocked, eos)
    if WM.stages(wp):
        mask = ks.mask  # survivors of the last stage: each stage drops what is below a positive threshold, underflowed numerators included
    else:
        mask = SM.kept_set(lg, gp, eos_blocked, eos).mask  # threshold-based: finite entries under top_p == 1, whatever their numerator
    maybe = np.zeros(V, dtype=bool)
    if ks.ambiguous:
        on = np.stack([w > 0 for w in ks.variants])
        maybe = on.any(0) & ~on.all(0)
    return np.where(mask, x, F32(-np.inf)).astype(F32), maybe


def eos_blocked_rows(m, b, gp, t_prefix=None):
    """bool [K]: where the tail blocks EOS for utterance b of the sampler_model.TailModel ``m`` at its NEXT step (the state before the step):
    min_new_tokens over the whole utterance, the Parler EOS gate above first_unf - which advances by at most one per step, first."""
    K = m.K
    t = int(m.cur_len[b])
    T = m.T_prefix if t_prefix is None else t_prefix
    fu = int(m.first_unf[b])
    if m.has_eos[b * K + fu] > 0 and fu < K - 1:
        fu += 1
    block_all = (t - 1 - T) < gp.min_new_tokens
    return np.array([block_all or (bool(gp.use_eos_gate) and k > fu) for k in range(K)])


def live_utterances(m, slots=None):
    """The utterances whose tail runs at the next launch over ``slots`` (TailModel.step's own rule)."""
    K = m.K
    slots = range(m.B) if slots is None else slots
    if m.session:
        return [b for b in slots if (m.unfinished[b * K:(b + 1) * K] > 0).any()]
    t0 = int(m.cur_len[0])
    return list(slots) if ((m.unfinished > 0) | (m.unfinished <= -(t0 + 1))).any() else []


def expected_step(m, logits, gp, recs=None, slots=None, t_prefix=None, gps=None):
    """What the next launch records, from the model's state BEFORE ``m.step``: {b: (idx, expected [K][V], maybe [K][V])} for every utterance the
    tail runs - finished rows of a running static batch included, as the reference records them. ``recs[b]``: the warper record of utterance b
    (None: neutral); ``gps[b]``: the utterance's own sampler settings (a slot record), default ``gp``; ``t_prefix[b]``: its voice-prompt frames."""
    out = {}
    for b in live_utterances(m, slots):
        g = gp if gps is None or gps.get(b) is None else gps[b]
        T = (m.T_prefix if t_prefix is None else t_prefix[b])
        blocked = eos_blocked_rows(m, b, g, T)
        rows = [recorded_row(logits[b, k], g, None if recs is None else recs[b], bool(blocked[k]), m.eos) for k in range(m.K)]
        out[b] = (int(m.cur_len[b]) - 1 - T, np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
    return out


def same_bits(a, b):
    """float32 arrays equal bit for bit (so -0.0 != +0.0 and every -inf is the one -inf)."""
    return np.array_equal(np.asarray(a, dtype=F32).view(np.uint32), np.asarray(b, dtype=F32).view(np.uint32))
