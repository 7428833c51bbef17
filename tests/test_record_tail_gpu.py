"""The step-record kernels called directly (tests/native/record_tail_harness.hip): the RECORD instances of the sampler tail through tail_launch
and the raw-logits node through step_logits_record_launch, the functions the engine calls.

Every case runs two rigs on the same inputs, one with the records and one without: ids, unfinished, has_eos, first_unf, cur_len and the
embedded next column h must be bit-identical after every launch. The recorded scores are compared bit for bit with the host model
(tests/step_record_model.py) outside the entries it calls doubtful - tests/test_step_record_model_cpu.py holds the share of rows that have any
under sampler_cases.AMBIGUOUS_CAP on these very inputs - and the recorded logits with the launch's input. Both arenas start as a sentinel bit
pattern with a guard step behind cap_steps, and at the end of a case every word outside the expected records still holds it."""
import ctypes as C

import numpy as np
import pytest
import torch

import record_tail_harness as RH
import sampler_cases as SC
import sampler_model as SM
import step_record_cases as RC
import step_record_model as RM
import warper_model as WM
from helpers import log_parity
from tail_harness import DevDims, DevGen

pytestmark = pytest.mark.gpu

LOG = "record_tail.txt"
DEV = "cuda"
FILL = -777
SENT = 0x7FC5A5A5  # a NaN no kernel produces: compared as bits
HID = 32
F32 = np.float32


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return RH.Harness(RH.build(str(tmp_path_factory.mktemp("record_tail_harness"))))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_bytes(struct):
    return torch.frombuffer(bytearray(bytes(struct)), dtype=torch.uint8).to(DEV)


def _dev_gen(gp, seed):
    return DevGen(gp.max_length, gp.min_new_tokens, int(gp.do_sample), gp.top_k, int(gp.use_eos_gate), gp.temperature, gp.top_p, seed)


class Rig:
    """The device side of one case: TailModel's state in device tensors, DevGen / DevDims, warper records, and - ``cap`` given - the record table
    with both arenas (static: [cap + 1][B][K][V]; session: [B][cap + 1][K][V], one buffer per slot) under a sentinel, plus their host shadows."""

    def __init__(self, H, m, gp, seed, cap=None, embed=True, slot_T=None, null_slots=(), kinds=("scores", "logits")):
        self.H, self.m, self.cap = H, m, cap
        B, K, V = m.B, m.K, m.V
        self.ids = torch.full((B * K + 2, m.ld), FILL, dtype=torch.int64, device=DEV)  # a guard row on either side
        self.cur_len, self.first_unf = (torch.zeros(B, dtype=torch.int32, device=DEV) for _ in range(2))
        self.unfinished, self.has_eos = (torch.zeros(B * K, dtype=torch.int32, device=DEV) for _ in range(2))
        self.row_maxlen = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.logits = torch.zeros(B, K, V, dtype=torch.float32, device=DEV)
        self.warp = torch.zeros(B, 4, dtype=torch.float32, device=DEV)
        self.slot_gen = torch.zeros(B, C.sizeof(RH.SlotGen), dtype=torch.uint8, device=DEV)
        self.slot_T = torch.zeros(B, dtype=torch.int32, device=DEV) if slot_T is None else torch.tensor(slot_T, dtype=torch.int32, device=DEV)
        self.prefix = torch.zeros(B * K, 8, dtype=torch.int64, device=DEV)
        self.gen = _dev_bytes(_dev_gen(gp, seed))
        self.dims = _dev_bytes(DevDims(m.P, 0, gp.max_length, m.T_prefix, self.prefix.data_ptr(), 8))
        g = torch.Generator().manual_seed(V + K)
        self.tables = torch.randn(K, V + 1, HID, generator=g).to(DEV) if embed else None
        self.pos = torch.randn(m.P + m.ld + 2, HID, generator=g).to(DEV) if embed else None
        self.h = torch.zeros(B, HID, dtype=torch.float32, device=DEV)
        self.rec = None
        if cap is not None:
            self.rec = torch.zeros(B + 1, C.sizeof(RH.StepRecord), dtype=torch.uint8, device=DEV)  # one guard record
            shape = (B, cap + 1, K, V) if m.session else (cap + 1, B, K, V)
            self.arena = {kind: torch.full(shape, SENT, dtype=torch.int32, device=DEV) for kind in ("scores", "logits")}
            self.shadow = {kind: np.full(shape, SENT, dtype=np.int32) for kind in ("scores", "logits")}
            ptr = lambda kind, off=0: (self.arena[kind].data_ptr() + 4 * off) if kind in kinds else None  # noqa: E731
            if m.session:
                for b in range(B):
                    if b not in null_slots:
                        off = b * (cap + 1) * K * V
                        assert H.set_step_record(self.rec.data_ptr(), b, 1, ptr("scores", off), ptr("logits", off), cap, K * V, 0, _stream()) == RH.PTTS_OK, H.error()
            else:
                assert H.set_step_record(self.rec.data_ptr(), 0, B, ptr("scores"), ptr("logits"), cap, B * K * V, K * V, _stream()) == RH.PTTS_OK, H.error()
            torch.cuda.synchronize()
            assert not bool(self.rec[B].any()), "set_step_record_kernel wrote past its records"
            self.kinds, self.null_slots = kinds, set(null_slots)
        self.upload()

    def upload(self):
        m = self.m
        self.ids[1:-1].copy_(torch.from_numpy(m.ids))
        for t, v in ((self.cur_len, m.cur_len), (self.first_unf, m.first_unf), (self.unfinished, m.unfinished), (self.has_eos, m.has_eos)):
            t.copy_(torch.from_numpy(v))
        if m.session:
            self.row_maxlen.copy_(torch.from_numpy(m.row_maxlen))

    def set_warp(self, recs):
        for b, wp in enumerate(recs):
            assert self.H.set_warp(self.warp.data_ptr(), b, 1, tuple(WM.Warp(*wp)), _stream()) == RH.PTTS_OK, self.H.error()

    def launch(self, lg, warp=False, grid=None, row0=0):
        """The engine's order: the logits node (records on), then the tail."""
        m = self.m
        self.logits.copy_(torch.from_numpy(lg))
        a = RH.RhArgs()
        a.logits, a.ids, a.cur_len, a.unfinished = self.logits.data_ptr(), self.ids[1:].data_ptr(), self.cur_len.data_ptr(), self.unfinished.data_ptr()
        a.has_eos, a.first_unf, a.gen, a.dims = self.has_eos.data_ptr(), self.first_unf.data_ptr(), self.gen.data_ptr(), self.dims.data_ptr()
        a.row_maxlen, a.slot_gen, a.slot_tprefix = self.row_maxlen.data_ptr(), self.slot_gen.data_ptr(), self.slot_T.data_ptr()
        a.warp = self.warp.data_ptr() if warp else None
        a.rec = None if self.rec is None else self.rec.data_ptr()
        if self.tables is not None:
            a.tables, a.pos_table, a.h, a.H, a.bos = self.tables.data_ptr(), self.pos.data_ptr(), self.h.data_ptr(), HID, m.bos
        a.ids_ld, a.B, a.K, a.V, a.eos, a.pad = m.ld, m.B, m.K, m.V, m.eos, m.pad
        a.session, a.row0, a.grid = int(m.session), row0, m.B if grid is None else grid
        if self.rec is not None:
            assert self.H.logits_record(a, _stream()) == RH.PTTS_OK, self.H.error()
        assert self.H.tail(a, _stream()) == RH.PTTS_OK, self.H.error()
        torch.cuda.synchronize()

    def dev_ids(self):
        return self.ids[1:-1].cpu().numpy()

    def chooser(self, what, m=None, row0=0):
        m = m or self.m
        dev = self.dev_ids()

        def choose(row, accepted):
            tok = int(dev[row0 + row, int(m.cur_len[row // m.K])])
            assert tok in accepted, (what, row0 + row, tok, sorted(accepted))
            return tok

        return choose

    def state(self):
        return [t.cpu().numpy().copy() for t in (self.ids, self.cur_len, self.first_unf, self.unfinished, self.has_eos, self.h.view(torch.int32))]

    def assert_equals_model(self, what):
        m = self.m
        assert bool((self.ids[0] == FILL).all()) and bool((self.ids[-1] == FILL).all()), f"{what}: a guard row was overwritten"
        got = self.dev_ids()
        assert np.array_equal(got, m.ids), (what, np.argwhere(got != m.ids)[:8])
        for name, t, v in (("cur_len", self.cur_len, m.cur_len), ("first_unf", self.first_unf, m.first_unf), ("unfinished", self.unfinished, m.unfinished),
                           ("has_eos", self.has_eos, m.has_eos)):
            assert np.array_equal(t.cpu().numpy(), v), (what, name)

    def where(self, kind, idx, b):
        return (b, idx) if self.m.session else (idx, b)

    def check_records(self, what, expected, lg, gp):
        """``expected`` (step_record_model.expected_step, taken before the model stepped) against the arenas; the shadows follow. Returns
        (rows compared, rows with a doubtful entry)."""
        rows = doubtful = 0
        dev = {kind: self.arena[kind].cpu().numpy() for kind in ("scores", "logits")}
        for b, (idx, exp, maybe) in expected.items():
            if idx >= self.cap or b in self.null_slots:
                continue
            at = self.where("scores", idx, b)
            if "scores" in self.kinds:
                got = dev["scores"][at]
                bad = (got != exp.view(np.int32)) & ~maybe
                assert not bad.any(), (what, b, idx, np.argwhere(bad)[:6], got[bad][:6].view(F32), exp[bad][:6])
                if maybe.any():  # a doubtful entry is kept (its own score, the sampler's division) or dropped (-inf), nothing else
                    with np.errstate(invalid="ignore", divide="ignore"):
                        kept = (lg[b] / F32(gp.temperature)).astype(F32).view(np.int32)
                    ok = (got == kept) | (got == np.array(-np.inf, dtype=F32).view(np.int32))
                    assert ok[maybe].all(), (what, b, idx, "a doubtful entry is neither kept nor dropped")
                self.shadow["scores"][at] = np.where(maybe, got, exp.view(np.int32))
                rows += exp.shape[0]
                doubtful += int(maybe.any(1).sum())
            if "logits" in self.kinds:
                self.shadow["logits"][at] = lg[b].view(np.int32)
                assert np.array_equal(dev["logits"][at], lg[b].view(np.int32)), (what, "logits", b, idx)
        return rows, doubtful

    def assert_nothing_else_changed(self, what):
        for kind in ("scores", "logits"):
            got = self.arena[kind].cpu().numpy()
            assert np.array_equal(got, self.shadow[kind]), (what, kind, np.argwhere(got != self.shadow[kind])[:8])


def _pair(H, make_model, gp, seed, cap, **kw):
    """The rig with the records and its twin without them, on equal state."""
    return Rig(H, make_model(), gp, seed, cap=cap, **kw), Rig(H, make_model(), gp, seed, cap=None, **{k: v for k, v in kw.items() if k in ("embed", "slot_T")})


def _same_state(a, b, what):
    for name, x, y in zip(("ids", "cur_len", "first_unf", "unfinished", "has_eos", "h"), a.state(), b.state()):
        assert np.array_equal(x, y), (what, name, "differs between the RECORD instance and the instance without the feature")


def _static_model(V, K, B, gp, T=0):
    eos, pad, bos = SC.ids_of(V)
    prefix = None
    if T:
        prefix = np.random.default_rng(V).integers(0, eos, (B * K, T))
    return SM.TailModel(B, K, V, eos, pad, bos, ld=gp.max_length + 2, P=2, prefix=prefix, max_length=gp.max_length, fill=FILL)


def _run_static(H, V, K, B, gp, seed, steps, logits_of, recs=None, warp=False, cap=None, T=0, embed=True, what=""):
    cap = steps if cap is None else cap
    rig, twin = _pair(H, lambda: _static_model(V, K, B, gp, T), gp, seed, cap, embed=embed)
    if warp:
        rig.set_warp(recs), twin.set_warp(recs)
    rows = doubtful = 0
    for s in range(steps):
        lg = logits_of(s)
        w = f"{what} step {s}"
        expected = RM.expected_step(rig.m, lg, gp, recs if warp else None)
        rig.launch(lg, warp=warp), twin.launch(lg, warp=warp)
        _same_state(rig, twin, w)
        if warp:
            WM.step_with_records(rig.m, lg, gp, recs, seed=seed, choose=rig.chooser(w))
        else:
            rig.m.step(lg, gp, seed=seed, choose=rig.chooser(w))
        rig.assert_equals_model(w)
        r, d = rig.check_records(w, expected, lg, gp)
        rows, doubtful = rows + r, doubtful + d
    rig.assert_nothing_else_changed(what)
    return rig, rows, doubtful


# ---- static -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K,B", RC.SHAPES)
def test_static_records_equal_the_model_and_the_tokens_those_of_the_plain_instance(H, V, K, B):
    rows = doubtful = 0
    for name, gp in RC.plain_cases(V):
        lg = RC.plain_logits(V, K, B, gp)
        _, r, d = _run_static(H, V, K, B, gp, 4321, RC.STEPS, lambda s: lg, what=f"V={V} K={K} {name}")
        rows, doubtful = rows + r, doubtful + d
    log_parity(f"static NV={SM.nv_of(V)} V={V} K={K} B={B}: {len(RC.plain_cases(V))} configurations x {RC.STEPS} steps, {rows} recorded rows equal to the "
               f"model bit for bit, {doubtful} with doubtful entries; state equal to the plain instance after every step", LOG)
    assert rows == len(RC.plain_cases(V)) * RC.STEPS * B * K and doubtful / rows <= SC.AMBIGUOUS_CAP


@pytest.mark.parametrize("V,K,B", RC.SHAPES)
def test_static_records_with_the_warp_instances(H, V, K, B):
    rows = doubtful = 0
    for i, (name, gp, recs) in enumerate(RC.warp_cases(V)):
        lg = RC.warp_logits(V, K, B, i)
        _, r, d = _run_static(H, V, K, B, gp, 99, RC.STEPS, lambda s: lg, recs=recs[:B], warp=True, what=f"warp V={V} K={K} {name}")
        rows, doubtful = rows + r, doubtful + d
    log_parity(f"static WARP NV={SM.nv_of(V)} V={V} K={K} B={B}: {rows} recorded rows, {doubtful} with doubtful entries", LOG)
    assert rows == len(RC.warp_cases(V)) * RC.STEPS * B * K and doubtful / rows <= SC.AMBIGUOUS_CAP


@pytest.mark.parametrize("V,K,B", RC.SHAPES)
def test_entries_far_below_the_maximum_stay_finite_under_top_p_one(H, V, K, B):
    gp = SC.Gen(max_length=6, min_new_tokens=0, do_sample=True)
    lg = RC.far_below_logits(V, K, B)
    rig, rows, _ = _run_static(H, V, K, B, gp, 7, 3, lambda s: lg, what=f"far below V={V}")
    got = rig.arena["scores"][:3].cpu().view(torch.float32).numpy()
    far = lg < lg.max(-1, keepdims=True) - 104.0
    far[:, :, SC.ids_of(V)[0]] = False  # (the gate may block EOS)
    assert far.sum() >= B * K * V // 5 and np.isfinite(got[:, far]).all() and rows == 3 * B * K


@pytest.mark.parametrize("V,K,B", RC.SHAPES)
def test_entries_far_below_the_maximum_are_removed_by_every_warper_stage(H, V, K, B):
    """The same rows under the WARP instances, each stage alone and two together: an entry whose numerator underflowed to 0 is below every
    positive threshold (min_p, the typical-p boundary, epsilon, eta), so its record is -inf - the RECORD lines that mark what a cut-off leaves
    at e == 0, and the typical-p key of such an entry - and everything else equals the model bit for bit."""
    gp = SC.Gen(max_length=6, min_new_tokens=0, do_sample=True)
    lg = RC.far_below_logits(V, K, B)
    far = lg < lg.max(-1, keepdims=True) - 105.0
    rows = doubtful = 0
    for wp in RC.FAR_BELOW_WARPS:
        rig, r, d = _run_static(H, V, K, B, gp, 7, 2, lambda s: lg, recs=[wp] * B, warp=True, what=f"far below V={V} {tuple(wp)}")
        got = rig.arena["scores"][:2].cpu().view(torch.float32).numpy()
        assert far.sum() >= B * K * V // 5 and (got[:, far] == -np.inf).all(), tuple(wp)
        assert np.isfinite(got).any(-1).all()  # no row is emptied
        rows, doubtful = rows + r, doubtful + d
    assert rows == len(RC.FAR_BELOW_WARPS) * 2 * B * K and doubtful / rows <= SC.AMBIGUOUS_CAP


@pytest.mark.parametrize("V,K,B", RC.SHAPES)
def test_the_eos_gate_under_sampling_is_recorded_and_a_finished_batch_writes_nothing(H, V, K, B):
    """sampler_cases.gate_logits: a hot EOS, blocked by min_new_tokens, then cascading codebook by codebook through the gate; the blocked entry is
    -inf in the record also where everything else is kept. The steps after the last row finished are no-ops: no record, clocks unchanged."""
    eos = SC.ids_of(V)[0]
    gp = SC.gate_gen(K)
    steps = SC.gate_steps(K)
    rig, rows, doubtful = _run_static(H, V, K, B, gp, 11, steps, lambda s: SC.gate_logits(V, K, B, s, gp, eos), what=f"gate V={V} K={K}")
    made = int(rig.m.cur_len[0]) - 1
    assert made < steps and (rig.m.unfinished < 0).all() and rows == made * B * K and doubtful / rows <= SC.AMBIGUOUS_CAP
    got = rig.arena["scores"].cpu().view(torch.float32).numpy()
    assert (got[:3, :, :, eos] == -np.inf).all() and np.isfinite(got[made - 1, :, 0, eos]).all()  # min_new_tokens = 3; codebook 0 is never gated


@pytest.mark.parametrize("V,K,B", RC.SHAPES)
def test_an_utterance_that_finished_early_is_still_recorded_and_cap_steps_bounds_the_writes(H, V, K, B):
    """sampler_cases.greedy_logits: utterance b draws EOS from step 2 + b on, the last one runs into max_length. cap_steps is two below the steps
    made: the last two steps record nothing, the guard step behind the arena keeps its sentinel."""
    eos = SC.ids_of(V)[0]
    gp = SC.Gen(max_length=SC.greedy_max_length(K), min_new_tokens=SC.GREEDY_MIN_NEW, do_sample=False)
    steps, cap = SC.greedy_steps(K), 2 * K
    rig, rows, _ = _run_static(H, V, K, B, gp, 0, steps, lambda s: SC.greedy_logits(V, K, B, s, eos), cap=cap, what=f"early V={V} K={K}")
    made = int(rig.m.cur_len[0]) - 1
    assert made == 2 * K + 2 > cap and made < steps and rows == cap * B * K
    if B > 1:
        first_done = -int(rig.m.unfinished[:K].min()) - 1  # the column at which the last row of utterance 0 finished
        assert first_done < cap  # ... and its rows were recorded (and compared) in every later step up to cap


@pytest.mark.parametrize("V,K,B", RC.SHAPES)
def test_a_voice_prompt_of_three_frames_records_step_zero_at_index_zero(H, V, K, B):
    gp = SC.Gen(max_length=3 + RC.STEPS + 3, min_new_tokens=2, do_sample=True, temperature=0.7, top_k=50, top_p=0.9)
    lg = RC.plain_logits(V, K, B, gp)
    rig, rows, _ = _run_static(H, V, K, B, gp, 5, RC.STEPS, lambda s: lg, T=3, embed=False, what=f"voice V={V}")
    assert rig.m.T_prefix == 3 and int(rig.m.cur_len[0]) == 4 + RC.STEPS and rows == RC.STEPS * B * K
    eos = SC.ids_of(V)[0]
    got = rig.arena["scores"].cpu().view(torch.float32).numpy()
    assert (got[:2, :, :, eos] == -np.inf).all()  # min_new_tokens counts from the given 1 + 3 columns


@pytest.mark.parametrize("kinds", [("scores",), ("logits",)])
def test_a_null_arena_leaves_that_kind_out(H, kinds):
    V, K, B = 1088, 9, 2
    gp = SC.Gen(max_length=8, min_new_tokens=2, do_sample=True, temperature=0.7, top_k=50, top_p=0.9)
    lg = RC.plain_logits(V, K, B, gp)
    rig = Rig(H, _static_model(V, K, B, gp), gp, 3, cap=3, kinds=kinds)
    for s in range(3):
        expected = RM.expected_step(rig.m, lg, gp)
        rig.launch(lg)
        rig.m.step(lg, gp, seed=3, choose=rig.chooser("null arena"))
        rig.check_records("null arena", expected, lg, gp)
    rig.assert_nothing_else_changed(f"only {kinds}")
    other = "logits" if kinds == ("scores",) else "scores"
    assert bool((rig.arena[other] == SENT).all()) and not bool((rig.arena[kinds[0]][:3] == SENT).any())


# ---- the logits node alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K,B", [(67, 3, 3), (1088, 9, 2)])
def test_the_logits_node_is_a_bit_copy_on_the_scalar_and_on_the_vector_path(H, V, K, B):
    """V = 67, K = 3: K * V = 201 floats per utterance, so utterances 1 and 2 and every odd step start off a 16-byte boundary (the scalar path);
    V = 1088: every base is aligned (16-byte loads and stores). NaN payloads, -0.0 and infinities travel as bits."""
    gp = SC.Gen(max_length=8, min_new_tokens=0, do_sample=False)
    rig = Rig(H, _static_model(V, K, B, gp), gp, 0, cap=3, embed=False, kinds=("logits",))
    assert ((K * V) % 4 != 0) == (V == 67)
    for s in range(5):  # two steps beyond cap_steps
        rng = np.random.default_rng([V, s])
        lg = rng.integers(-2 ** 31, 2 ** 31, (B, K, V)).astype(np.int32).view(F32)  # arbitrary bit patterns
        lg[:, :, 0], lg[:, :, 1] = -0.0, -np.inf
        expected = RM.expected_step(rig.m, np.nan_to_num(lg.copy(), nan=0.0), gp)
        a = RH.RhArgs()
        rig.logits.copy_(torch.from_numpy(lg.view(np.int32)).view(torch.float32))
        a.logits, a.cur_len, a.unfinished, a.dims, a.rec = rig.logits.data_ptr(), rig.cur_len.data_ptr(), rig.unfinished.data_ptr(), rig.dims.data_ptr(), rig.rec.data_ptr()
        a.B, a.K, a.V, a.session, a.row0, a.grid = B, K, V, 0, 0, B
        assert H.logits_record(a, _stream()) == RH.PTTS_OK, H.error()
        torch.cuda.synchronize()
        rig.check_records(f"logits node V={V} step {s}", expected, lg, gp)
        rig.m.cur_len += 1  # the clock alone moves: no tail here
        rig.upload()
    rig.assert_nothing_else_changed(f"logits node V={V}")
    # every row finished before this step: the node skips, as the tail would
    rig.m.cur_len[:] = 2
    rig.m.unfinished[:] = -2
    rig.upload()
    rig.shadow["logits"][:] = SENT
    rig.arena["logits"].fill_(SENT)
    assert H.logits_record(a, _stream()) == RH.PTTS_OK, H.error()
    torch.cuda.synchronize()
    rig.assert_nothing_else_changed("logits node after the batch finished")


# ---- session --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warp", [False, True])
@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("V,K,B", RC.SHAPES)
def test_session_slots_idle_null_finished_and_voice(H, V, K, B, sample, warp):
    """Five slots: 0 idle with a record (nothing may be written), 1 live with a record, 2 live with null pointers, 3 with a record and a short
    max_length (it finishes, then records nothing), 4 with a voice prompt of 3 frames of its own (its admission is step 0 at index 0).
    Admissions are grid 1 with row0 = the slot, steps grid 5."""
    S, L, steps, cap = 5, 12, 5, 4
    eos, pad, bos = SC.ids_of(V)
    gp, wps, lg = RC.session_case(V, K, S, L, sample, warp)
    slot_T = [0, 0, 0, 0, 3]
    maxlen = {1: L, 2: L, 3: 4, 4: L}

    def make():
        m = SM.TailModel(S, K, V, eos, pad, bos, ld=L + 2, session=True, P=2, fill=FILL)
        for b in range(S):
            m.reset_row(b, 0, L)
        return m

    rig, twin = _pair(H, make, gp, 21, cap, embed=False, slot_T=slot_T, null_slots=(2,))
    twin.m = rig.m  # one model: the twin's uploads at the admissions write the state the rig's device holds
    if warp:
        rig.set_warp(wps), twin.set_warp(wps)
    rows = doubtful = 0

    def launch(what, slots, **kw):
        nonlocal rows, doubtful
        expected = RM.expected_step(rig.m, lg, gp, wps, slots=slots, t_prefix=slot_T)
        rig.launch(lg, warp=warp, **kw), twin.launch(lg, warp=warp, **kw)
        _same_state(rig, twin, what)
        for b in sorted(slots, reverse=True):  # one slot at a time: slot 4 counts its new tokens from its own prefix
            rig.m.T_prefix = slot_T[b]
            if warp:
                WM.step_with_records(rig.m, lg, gp, wps, slots=[b], seed=21, choose=rig.chooser(what))
            else:
                rig.m.step(lg, gp, slots=[b], seed=21, choose=rig.chooser(what))
        rig.m.T_prefix = 0
        rig.assert_equals_model(what)
        r, d = rig.check_records(what, expected, lg, gp)
        rows, doubtful = rows + r, doubtful + d
        return sorted(expected)

    for b in (1, 2, 3, 4):
        rig.m.reset_row(b, 1, maxlen[b])
        if b == 4:  # BOS + 3 given columns
            rig.m.ids[b * K:(b + 1) * K, 1:4] = 7
            rig.m.cur_len[b] = 4
        rig.upload(), twin.upload()
        assert launch(f"admit slot {b}", [b], grid=1, row0=b) == [b]
    live = [launch(f"session V={V} K={K} step {s}", list(range(S))) for s in range(steps)]
    assert live[0] == [1, 2, 3, 4] and live[-1] == [1, 2, 4] and 3 not in live[2]  # slot 3: max_length 4 = the admission's token + 2 steps
    rig.assert_nothing_else_changed("session")
    for kind in ("scores", "logits"):
        a = rig.arena[kind]
        assert bool((a[0] == SENT).all()) and bool((a[2] == SENT).all())  # the idle slot and the one with null pointers
        assert not bool((a[1, :cap] == SENT).any()) and bool((a[1, cap] == SENT).all())  # cap_steps 4 < the 6 steps slot 1 made
        assert not bool((a[3, :3] == SENT).any()) and bool((a[3, 3:] == SENT).all())  # three steps, then finished
        assert not bool((a[4, :cap] == SENT).any())
    assert rows == (cap + 3 + cap) * K
