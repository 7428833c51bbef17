"""A host restatement of the sampler tail (``tail_kernel<NV, SESSION>``, parler_tts_amd/csrc/ptts_lm_kernels.h) in numpy / float64:
the draw hash, the kept set of temperature -> top-k -> top-p, the inverse-CDF draw in the kernel's order, and ``TailModel``, one tail
step for B utterances (static or session) with the state the kernel keeps on the device. The GPU tests compare the kernel with it after
every step (tests/test_sampler_tail_gpu.py); tests/test_sampler_model_cpu.py pins it against transformers' warpers and
``oracle.decoder_oracle.sample_loop``.

What is exact and what has a band:
  * scores are float32(l) / float32(T): IEEE division, bit for bit the device's, so keys and the top-k set carry no tolerance;
  * the softmax numerators are exp(float32(x - max)): the device's expf is within 2 ulp of it, and every fp32 sum of the kernel is a chain of
    per-lane adds and wave levels (the longest, the inverse CDF's, 2 NV + 7 roundings). ``band`` below bounds what that can move
    a cumulative mass by; a comparison of a mass with a threshold closer than that is AMBIGUOUS and the caller is told so.
"""
import functools
import math

import numpy as np
import torch

from oracle import decoder_oracle as DO

F32 = np.float32
_M1, _M2, _GOLD = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB), np.uint64(0x9E3779B97F4A7C15)


def splitmix64(x):
    """splitmix64 of uint64 array(s), in wrapping 64-bit arithmetic."""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
    with np.errstate(over="ignore"):
        x = x + _GOLD
        x = (x ^ (x >> np.uint64(30))) * _M1
        x = (x ^ (x >> np.uint64(27))) * _M2
        return x ^ (x >> np.uint64(31))


def draw_hash(seed, t, row):
    """splitmix64(seed ^ splitmix64(t << 32 ^ row)): uint64 array over the broadcast of the arguments."""
    seed, t, row = (np.asarray(v, dtype=np.uint64) for v in (seed, t, row))
    return splitmix64(seed ^ splitmix64((t << np.uint64(32)) ^ row))


def draw_u(seed, t, row):
    """The uniform of draw (seed, column t, global row b * K + k) with the kernel's roundings: the top 24 bits n of the hash,
    float32(float64(n) + 0.5) * 2^-24. n + 0.5 needs 25 bits once n >= 2^23 and rounds to even, so u lies in [2^-25, 1.0]: n = 2^24 - 1
    gives exactly 1.0f (the kernel's `pick < 0 -> last` fallback covers it), n = 0 the smallest value 2^-25."""
    n = (draw_hash(seed, t, row) >> np.uint64(40)).astype(np.float64)
    u = (n + 0.5).astype(F32) * F32(2.0 ** -24)
    return u if u.size > 1 else F32(u[0])


def nv_of(V):
    """Logits per lane of the tail_kernel instance that serves vocabulary V (tail_launch)."""
    return 8 if V <= 512 else 18 if V <= 1152 else 32


def band(V, total):
    """Bound on the distance between a cumulative mass as the device compares it and the float64 one, in ulps of ``total`` (2^-24 total;
    every partial sum is <= total, every rounding at most half an ulp of it).
    The longest chain is the inverse CDF's: NV per-lane adds (ls), 6 scan levels, the subtraction ``incl - ls``, then up to NV more adds
    (``run += e[i]``) - 2 NV + 7 roundings - compared with ``u * tot``, whose tot is NV adds + 6 wave_sum levels + the multiply: NV + 7
    more. The top-p predicate is shorter (NV + 6 against NV + 7). So at most 3 NV + 14 half-ulps of accumulation, plus expf at <= 2 ulp of
    each numerator (<= 2 ulp of the sum, on each side): below (3 NV + 14) / 2 + 4 ulp. The band used, (2 (NV + 6) + 4) ulp = (4 NV + 32)
    half-ulps, covers that with room; it is not the count of one chain and must not be tightened as if it were."""
    return (2 * (nv_of(V) + 6) + 4) * 2.0 ** -24 * total


@functools.lru_cache(maxsize=None)
def draw_order(V):
    """The order the kernel walks the vocabulary in: lane-major, lane l owns l, l + 64, ... - sorted by (v % 64, v // 64)."""
    v = np.arange(V)
    return v[np.lexsort((v // 64, v % 64))]


class Kept:
    """Result of kept_set: ``mask`` bool [V] (the kept set), ``weights`` float64 [V] (softmax numerators of the kept entries, 0 elsewhere),
    ``ambiguous``, ``variants``: the weight vectors the device may hold when ambiguous (the boundary groups dropped / kept), and ``tiny``
    bool [V]: kept entries whose numerator lies in fp32's subnormal range (see draw)."""

    def __init__(self, mask, weights, ambiguous, variants, tiny):
        self.mask, self.weights, self.ambiguous, self.variants, self.tiny = mask, weights, ambiguous, variants, tiny


def kept_set(logits_f32, gp, eos_blocked, eos):
    """TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper on one row, as the kernel applies them.
    top-k keeps every entry >= the k-th largest value, ties included (HF: `scores < kth` is removed).
    top-p keeps an entry iff the softmax mass STRICTLY ABOVE ITS VALUE is < top_p: the arg-max always stays, and ALL entries tied at the
    boundary value stay. This is the kernel's contract; at an exact tie it differs from HF, whose sort splits the tie arbitrarily
    (sampler)."""
    x = np.asarray(logits_f32, dtype=F32).copy()
    V = x.shape[0]
    if eos_blocked:
        x[eos] = -np.inf
    with np.errstate(invalid="ignore"):
        x = (x / F32(gp.temperature)).astype(F32)  # -inf stays -inf
    if gp.top_k and 0 < gp.top_k < V:
        kth = np.sort(x)[::-1][gp.top_k - 1]
        x = np.where(x >= kth, x, F32(-np.inf)).astype(F32)
    mx = x.max()
    with np.errstate(invalid="ignore"):
        d = (x - mx).astype(F32)
    w = np.where(np.isfinite(x), np.exp(d.astype(np.float64)), 0.0)
    w[w.astype(F32) == 0] = 0.0  # exp underflows to 0 in fp32
    # numerators in fp32's subnormal range (2^-149 = e^-103.3 .. 2^-126 = e^-87.3): whether the device's expf flushes them to 0 is not part
    # of the contract. Their mass is far below the band; what they can change is WHICH entry is the last one with a non-zero weight.
    tiny = (d > -104.5) & (d < -87.0) & np.isfinite(x)
    ambiguous = False
    total = w.sum()
    mask = np.isfinite(x)
    variants = None
    if gp.top_p < 1.0:
        thr = float(F32(gp.top_p)) * total
        bd = band(V, total)
        fin = np.isfinite(x)
        vals, inv = np.unique(x[fin], return_inverse=True)  # distinct present values, ascending
        group = np.bincount(inv, weights=w[fin])
        above = np.concatenate([np.cumsum(group[::-1])[::-1][1:], [0.0]])  # mass strictly above each value
        keep_v = above < thr
        near = np.abs(above - thr) <= bd
        near[-1] = False  # nothing lies above the arg-max: 0 < thr always
        mask = fin.copy()
        mask[fin] = keep_v[inv]
        if near.any():
            ambiguous = True
            lo, hi = fin.copy(), fin.copy()
            lo[fin] = (keep_v & ~near)[inv]
            hi[fin] = (keep_v | near)[inv]
            variants = [np.where(lo, w, 0.0), np.where(hi, w, 0.0)]
    weights = np.where(mask, w, 0.0)
    return Kept(mask, weights, ambiguous, variants or [weights], tiny & mask)


def _last_sure(order, tiny):
    """Index (into order) of the last entry whose weight is certainly non-zero on the device."""
    sure = np.nonzero(~tiny[order])[0] if tiny is not None else np.arange(len(order))
    return int(sure[-1]) if len(sure) else 0


def accept_set(weights, u, V, tiny=None):
    """Every token a draw at u may return when its cumulative masses are only known to within the band: the entries (non-zero weight, draw
    order) whose interval [cum_before, cum] comes within the band of u * total, plus the last entry when the target may lie beyond it."""
    order = draw_order(V)
    order = order[weights[order] > 0]
    cum = np.cumsum(weights[order])
    total = cum[-1]
    target, bd = float(u) * total, band(V, total)
    before = cum - weights[order]
    ok = (before <= target + bd) & (cum >= target - bd)
    if target + bd >= total:  # the fallback "last entry with a non-zero weight"
        ok[_last_sure(order, tiny):] = True
    return set(int(v) for v in order[ok])


def draw(kept, weights, u, tiny=None):
    """Inverse CDF over the kept entries with non-zero weight in draw order: the first entry whose cumulative weight is >= u * total, the
    last kept entry if none is. None (ambiguous) when u * total lies within the band of a cumulative boundary - except the last one,
    where "reached" and "not reached" both give the last entry - unless entries with a subnormal numerator (``tiny``) follow the last
    certain one: then the device's last non-zero entry is not determined either."""
    V = weights.shape[0]
    order = draw_order(V)
    order = order[kept[order] & (weights[order] > 0)]
    cum = np.cumsum(weights[order])
    total = cum[-1]
    target = float(u) * total
    if (np.abs(cum[:-1] - target) <= band(V, total)).any():
        return None
    if target + band(V, total) >= total and _last_sure(order, tiny) != len(order) - 1:
        return None
    hit = np.nonzero(cum >= target)[0]
    return int(order[hit[0]] if len(hit) else order[-1])


def embed_column(tables, pos_table, toks, pos):
    """float32 SEQUENTIAL sum over k = 0..K-1 of tables[k][toks[k]], then + pos_table[pos]: the order of both device paths, so the result
    is reproducible bit for bit. ``tables`` float32 [K][V+1][H] (a bf16 table: its values widened)."""
    acc = np.zeros(tables.shape[2], dtype=F32)
    for k, tok in enumerate(toks):
        acc = (acc + tables[k, int(tok)]).astype(F32)
    if pos_table is not None:
        acc = (acc + pos_table[pos]).astype(F32)
    return acc


class TailModel:
    """One tail step for B utterances. static: one shared clock, stop on gp.max_length, no-op once every row finished before the step.
    session: every slot has its own clock and max_length (row_maxlen), a slot is live iff one of its K flags is positive, idle and
    finished slots are left untouched; slots enter through admit().
    State (as on the device): ids int64 [B*K][ld], cur_len [B], unfinished [B*K] (1 | -(t+1)), has_eos [B*K], first_unf [B], row_maxlen [B]."""

    def __init__(self, B, K, V, eos, pad, bos, ld, session=False, P=0, prefix=None, max_length=None, fill=0):
        self.B, self.K, self.V, self.eos, self.pad, self.bos, self.ld, self.session, self.P = B, K, V, eos, pad, bos, ld, session, P
        self.ids = np.full((B * K, ld), fill, dtype=np.int64)  # fill: what the columns nobody wrote hold
        self.cur_len = np.ones(B, dtype=np.int32)
        self.unfinished = np.zeros(B * K, dtype=np.int32)
        self.has_eos = np.zeros(B * K, dtype=np.int32)
        self.first_unf = np.zeros(B, dtype=np.int32)
        self.row_maxlen = np.zeros(B, dtype=np.int32) if session else None
        self.gate = [None] * B
        self.pattern = [None] * B
        self.T_prefix = 0
        self.stats = {"draws": 0, "ambiguous": 0}
        self._kept = {}
        if not session:  # prefill: BOS (+ the voice prompt's delayed columns), every row live
            self.T_prefix = 0 if prefix is None else prefix.shape[-1]
            for b in range(B):
                seq = torch.full((K, 1), bos, dtype=torch.long)
                if self.T_prefix:
                    seq = torch.cat([seq, torch.as_tensor(prefix[b * K:(b + 1) * K]).long()], dim=-1)
                self._begin(b, seq, max_length)
            self.unfinished[:] = 1

    def _begin(self, b, seq, max_length):
        K = self.K
        given, pattern = DO.build_delay_pattern_mask(seq, self.bos, self.pad, max_length, K)
        self.pattern[b] = pattern
        self.gate[b] = DO.EosGate(self.eos, K, 1)
        self.ids[b * K:(b + 1) * K, :given.shape[-1]] = given.numpy()
        self.cur_len[b] = given.shape[-1]
        self.has_eos[b * K:(b + 1) * K] = 0
        self.first_unf[b] = 0

    def reset_row(self, b, live, max_length):
        """session_reset_rows_kernel on one slot: BOS in column 0, clock 1, the K flags = live, the request's max_length."""
        K = self.K
        self.ids[b * K:(b + 1) * K, 0] = self.bos
        self._begin(b, torch.full((K, 1), self.bos, dtype=torch.long), max_length)
        self.unfinished[b * K:(b + 1) * K] = live
        self.row_maxlen[b] = max_length

    def fed_column(self, b, j):
        """What the model is fed at column j of utterance b: the delay pattern over the raw ids."""
        K = self.K
        raw = torch.from_numpy(self.ids[b * K:(b + 1) * K, :j + 1])
        return DO.apply_delay_pattern_mask(raw, self.pattern[b])[:, j].numpy()

    def step(self, logits, gp, slots=None, seed=0, choose=None, tables=None, pos_table=None, h=None):
        """logits float32 [B][K][V]; ``slots``: the slots this launch covers (default all). Sampling: seed is DevGen::seed; an ambiguous draw
        is settled by ``choose(row, accepted_tokens)``. With ``tables`` the embedding of the new column is written into h[b] (float32 [B][H])."""
        B, K = self.B, self.K
        slots = range(B) if slots is None else slots
        if self.session:
            live = [b for b in slots if (self.unfinished[b * K:(b + 1) * K] > 0).any()]
        else:  # the reference loop has exited iff every row finished BEFORE this step
            t0 = int(self.cur_len[0])
            live = list(slots) if ((self.unfinished > 0) | (self.unfinished <= -(t0 + 1))).any() else []
        for b in live:
            t = int(self.cur_len[b])
            rows = slice(b * K, (b + 1) * K)
            maxlen = int(self.row_maxlen[b]) if self.session else gp.max_length
            scores = torch.zeros(K, self.V)
            if gp.use_eos_gate:
                self.gate[b](torch.from_numpy(self.ids[rows, :t]), scores)
                self.first_unf[b] = int(self.gate[b].first_unfinished[0])
            else:  # the kernel advances first_unf whether or not the gate is applied
                fu = int(self.first_unf[b])
                if self.has_eos[b * K + fu] > 0 and fu < K - 1:
                    self.first_unf[b] = fu + 1
            block_all = (t - 1 - self.T_prefix) < gp.min_new_tokens
            for k in range(K):
                row = b * K + k
                blocked = bool(block_all or scores[k, self.eos] == -math.inf)
                unf = self.unfinished[row] > 0
                lg = np.asarray(logits[b, k], dtype=F32)
                if not unf:
                    tok = self.pad  # next_tokens * unfinished + pad * (1 - unfinished): the choice of a finished row is never seen
                elif not gp.do_sample:
                    x = lg.copy()
                    if blocked:
                        x[self.eos] = -np.inf
                    tok = int(np.argmax(x))  # first index on ties
                else:
                    key = (lg.tobytes(), blocked, gp.temperature, gp.top_k, gp.top_p)  # rows and parameters repeat over steps
                    ks = self._kept.get(key)
                    if ks is None:
                        ks = self._kept[key] = kept_set(lg, gp, blocked, self.eos)
                    u = draw_u(seed, t, row)
                    tok = None if ks.ambiguous else draw(ks.mask, ks.weights, u, ks.tiny)
                    self.stats["draws"] += 1
                    if tok is None:
                        self.stats["ambiguous"] += 1
                        acc = set().union(*(accept_set(w, u, self.V, ks.tiny) for w in ks.variants))
                        tok = choose(row, acc)
                nxt = tok
                self.ids[row, t] = nxt
                if nxt == self.eos:
                    self.has_eos[row] = 1
                if unf and (nxt == self.eos or t + 1 >= maxlen):
                    self.unfinished[row] = -(t + 1)
            self.cur_len[b] = t + 1
            if tables is not None:
                h[b] = embed_column(tables, pos_table, self.fed_column(b, t), self.P + t)
        return live
