"""Host side of the per-slot sampler record tests: ``SlotSession``, the restatement of a session tail whose slots may hold their own record
(one ``sampler_model.TailModel(B=1, session=True)`` per such slot, stepped with that slot's parameters and seed - its row index is then the
codebook index k, which is the contract - and the B-slot model with the session's seed and rows b * K + k for every other slot), and the
inputs of the mixed-slots and placement cases, shared by the GPU file (tests/test_slot_gen_tail_gpu.py) and the CPU file that checks on the
model alone that the ambiguous draws stay under the cap (tests/test_slot_gen_cpu.py). numpy only."""
import functools

import numpy as np

import sampler_cases as SC
import sampler_model as SM
import slot_gen_harness as SG
import tail_harness as TH

F32 = np.float32
FILL = -777  # ids columns nobody wrote
SHAPES = [(64, 4), (1088, 9), (2048, 17)]  # the three NV instances; K = 17: the second trip of the wave loop
SLOTS, STEPS, HIDDEN, P = 6, 12, 32, 2
SESSION_SEED, SEED_A, SEED_B, SEED_C = 7, 0x5EEDA0000001, 0xB0B0000000000002, 3
MAXLEN = STEPS + 6  # never reached
MIN_NEW_4 = 6       # slot 4's own bound (the session's is 0)
HOT = SC.SESSION_HOT


def dev_gen(gp, max_length, seed):
    return TH.DevGen(max_length, gp.min_new_tokens, int(gp.do_sample), gp.top_k, int(gp.use_eos_gate), gp.temperature, gp.top_p, seed)


def record_words(gp, max_length, seed):
    """The 32-bit words of the record set_slot_gen_kernel writes for (gp, seed): own = 1, row_base 0."""
    return np.frombuffer(bytes(SG.SlotGen(dev_gen(gp, max_length, seed), 1, 0)), dtype=np.int32).copy()


class SlotSession:
    """State of a B-slot session as the device holds it (``full``: ids, cur_len, unfinished, has_eos, first_unf, row_maxlen; ``recs``: the B
    records as 32-bit words) and one tail launch on it."""

    def __init__(self, B, K, V, ld, session_gp, session_seed, special_ids=None, P=P):
        eos, pad, bos = special_ids or SC.ids_of(V)
        self.P = P
        self.B, self.K, self.V, self.gp, self.seed = B, K, V, session_gp, session_seed
        self.full = SM.TailModel(B, K, V, eos, pad, bos, ld=ld, session=True, P=P, fill=FILL)
        self.own = {}  # slot -> (TailModel of that slot alone, its Gen, its seed)
        self.recs = np.zeros((B, SG.WORDS), dtype=np.int32)
        self.stats = {"draws": 0, "ambiguous": 0}

    def _pull(self, b):
        """The one-slot model's state into the slot's place in ``full``."""
        sub, f, K = self.own[b][0], self.full, self.K
        f.ids[b * K:(b + 1) * K] = sub.ids
        f.unfinished[b * K:(b + 1) * K], f.has_eos[b * K:(b + 1) * K] = sub.unfinished, sub.has_eos
        f.cur_len[b], f.first_unf[b], f.row_maxlen[b] = sub.cur_len[0], sub.first_unf[0], sub.row_maxlen[0]

    def reset(self, b, live, max_length, rec=None):
        """session_reset_rows_kernel on slot b, then set_slot_gen_kernel: rec = (Gen, seed) is the slot's own record, None the cleared one."""
        f, K = self.full, self.K
        f.reset_row(b, live, max_length)
        self.own.pop(b, None)
        self.recs[b] = 0
        if rec is not None:
            gp, seed = rec
            sub = SM.TailModel(1, K, self.V, f.eos, f.pad, f.bos, ld=f.ld, session=True, P=self.P, fill=FILL)
            sub.ids[:] = f.ids[b * K:(b + 1) * K]  # the columns an earlier request left in the slot stay
            sub.reset_row(0, live, max_length)
            self.own[b] = (sub, gp, seed)
            self.recs[b] = record_words(gp, max_length, seed)

    def step(self, lg, slots=None, choose=None, tables=None, pos_table=None, h=None):
        """One launch over ``slots`` (default all). ``choose(global row, accepted tokens)`` settles an ambiguous draw. Returns the live slots."""
        slots = list(range(self.B) if slots is None else slots)
        f = self.full
        before = dict(f.stats)
        live = f.step(lg, self.gp, slots=[b for b in slots if b not in self.own], seed=self.seed, choose=choose, tables=tables, pos_table=pos_table, h=h)
        for k in before:
            self.stats[k] += f.stats[k] - before[k]
        for b in slots:
            if b not in self.own:
                continue
            sub, gp, seed = self.own[b]
            before = dict(sub.stats)
            got = sub.step(lg[b:b + 1], gp, seed=seed, choose=None if choose is None else (lambda row, acc, b=b: choose(b * self.K + row, acc)),
                           tables=tables, pos_table=pos_table, h=None if h is None else h[b:b + 1])
            for k in before:
                self.stats[k] += sub.stats[k] - before[k]
            self._pull(b)
            if got:
                live.append(b)
        return sorted(live)


# ---- mixed slots in one launch --------------------------------------------------------------------------------------------------------
def session_gen():
    """The session's DevGen: sampled (seed SESSION_SEED); its max_length is not what a slot stops on."""
    return SC.session_gen(True)


def mixed_records():
    """slot -> (Gen, seed, the step it is admitted at). Slot 3 has no record (the session's parameters), slot 5 stays idle."""
    return {0: (SC.Gen(max_length=MAXLEN, min_new_tokens=0, do_sample=False), 11, 0),
            1: (SC.Gen(max_length=MAXLEN, do_sample=True, temperature=0.7, top_k=20, top_p=0.9), SEED_A, 2),
            2: (SC.Gen(max_length=MAXLEN, do_sample=True, temperature=1.3, top_k=0, top_p=1.0), SEED_B, 5),
            4: (SC.Gen(max_length=MAXLEN, min_new_tokens=MIN_NEW_4, do_sample=True, temperature=0.9, top_k=50, top_p=0.95), SEED_C, 0)}


@functools.lru_cache(maxsize=None)
def mixed_base_logits(V, K):
    """[SLOTS][K][V]: the rows of a sampled slot are re-drawn (on the reference alone, sampler_cases.flat_logits) until their kept set under
    that slot's own parameters is unambiguous; one set serves every launch (the hash differs by column). Slot 4: EOS holds nearly all the mass."""
    eos = V - 8
    recs = mixed_records()
    lg = np.empty((SLOTS, K, V), dtype=F32)
    for b in range(SLOTS):
        gp = recs[b][0] if b in recs else session_gen()
        lg[b] = SC.flat_logits(V, K, 1, gp, eos, (V, K, b), hot=HOT if b == 4 else None)[0]
    lg[4, :, eos] = HOT
    return lg


def mixed_events(V, K):
    """The launches of the mixed case, in order: ("clear",) - the range clear of every record -, ("reset", slot, live, max_length, rec | None),
    ("admit", slot, logits) - the grid-1 launch with row0 = slot - and ("step", s, logits)."""
    recs = mixed_records()
    base = mixed_base_logits(V, K)
    yield ("clear",)
    for b in range(SLOTS):
        yield ("reset", b, 0, MAXLEN, None)
    for s in range(STEPS):
        lg = base.copy()
        lg[0] = (np.random.default_rng([V, K, s]).standard_normal((K, V)) * 2).astype(F32)  # the greedy slot: fresh rows per launch
        for b in [b for b, (_, _, at) in recs.items() if at == s] + ([3] if s == 0 else []):
            yield ("reset", b, 1, MAXLEN, recs[b][:2] if b in recs else None)
            yield ("admit", b, lg)
        yield ("step", s, lg)


def run_mixed_on_the_model(V, K, choose=lambda row, acc: min(acc)):
    """The mixed case on the host model alone."""
    m = SlotSession(SLOTS, K, V, MAXLEN + 3, session_gen(), SESSION_SEED)
    for ev in mixed_events(V, K):
        if ev[0] == "reset":
            m.reset(*ev[1:])
        elif ev[0] == "admit":
            m.step(ev[2], slots=[ev[1]], choose=choose)
        elif ev[0] == "step":
            m.step(ev[2], choose=choose)
    return m


def assert_slot4_waits_for_its_own_bound(m, K, V):
    """Slot 4 (EOS nearly certain from its first column on, the session's min_new_tokens 0): no EOS in the MIN_NEW_4 columns its own record
    blocks, EOS on codebook 0 in the very next one."""
    eos = V - 8
    rows = m.full.ids[4 * K:5 * K]
    assert not (rows[:, 1:MIN_NEW_4 + 1] == eos).any(), rows[:, :MIN_NEW_4 + 2]
    assert rows[0, MIN_NEW_4 + 1] == eos, rows[:, :MIN_NEW_4 + 2]


# ---- placement ------------------------------------------------------------------------------------------------------------------------
PLACE_STEPS = 8
PLACE_GEN = SC.Gen(max_length=MAXLEN, do_sample=True, temperature=0.7, top_k=20, top_p=0.9)


@functools.lru_cache(maxsize=None)
def placement_logits(V, K):
    """[K][V] of the request under test (the same at each of its launches) and [SLOTS][K][V] for the slots beside it (shared: copy to change)."""
    eos = V - 8
    mine = SC.flat_logits(V, K, 1, PLACE_GEN, eos, (V, K, 77))[0]
    others = SC.flat_logits(V, K, SLOTS, session_gen(), eos, (V, K, 78))
    return mine, others


def placement_events(V, K, slot, admit_at, with_record):
    """The request under test in `slot`, admitted at step `admit_at` with PLACE_GEN / SEED_A (with_record) or, after a retire, plainly; beside
    it a plain slot and a greedy slot with its own record, live from step 0."""
    mine, others = placement_logits(V, K)
    beside = [b for b in range(SLOTS) if b != slot][1:3]
    greedy = (SC.Gen(max_length=MAXLEN, do_sample=False), 0)
    yield ("clear",)
    for b in range(SLOTS):
        yield ("reset", b, 0, MAXLEN, None)
    lg = others.copy()
    lg[slot] = mine
    for s in range(admit_at + PLACE_STEPS):
        for b, rec in ((beside[0], None), (beside[1], greedy)) if s == 0 else ():
            yield ("reset", b, 1, MAXLEN, rec)
            yield ("admit", b, lg)
        if s == admit_at:
            if not with_record:  # a request with a record was here before: retired, then a plain admission
                yield ("reset", slot, 1, MAXLEN, (PLACE_GEN, SEED_A))
                yield ("reset", slot, 0, MAXLEN, None)
            yield ("reset", slot, 1, MAXLEN, (PLACE_GEN, SEED_A) if with_record else None)
            yield ("admit", slot, lg)
        yield ("step", s, lg)
