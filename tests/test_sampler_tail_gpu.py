"""The sampler tail called directly (tests/native/tail_harness.hip -> tail_launch -> tail_kernel<NV, SESSION>) against its host restatement
(tests/sampler_model.py), on every instance, at the vocabulary edges of NV (512 | 528, 1152 | 1168, 2048) and the codebook counts where the
kernel changes path (K < 4: idle waves; K > 9: a second batch of embedding loads; K > 16: a second trip of the wave loop).

After EVERY launch the whole state - ids, cur_len, unfinished, has_eos, first_unf, row_maxlen and the embedding h of the next column - must
equal TailModel's bit for bit. ids, h, cur_len and the flag arrays sit between sentinel guards that must survive, the logits must be
untouched, and every launch runs twice from the same state with bitwise equal results.
Sampled tokens are predicted exactly from the draw hash; the draws whose target lies within the fp32 rounding band of a cumulative boundary
(sampler_model.band) are excluded from the exact comparison - at most 4 % per configuration - and must still come from the neighbourhood
of that boundary."""

import numpy as np
import pytest
import torch

import sampler_cases as SC
import sampler_model as SM
import tail_harness as TH
from helpers import log_parity

pytestmark = pytest.mark.gpu

LOG = "sampler_tail.txt"
DEV = "cuda"
SENT32 = 0x7FBADBAD  # as a float: a NaN payload no kernel produces
FILL = -777          # ids columns nobody wrote
F32 = np.float32


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return TH.Harness(TH.build(str(tmp_path_factory.mktemp("tail_harness"))))


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A tensor of `shape` inside a flat buffer of 32-bit sentinels: `pad` words before it and after it."""

    def __init__(self, shape, dtype, pad=1024):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
        self.pad, self.n = pad, n
        self.buf = torch.full((pad + n + pad,), SENT32, dtype=torch.int32, device=DEV)
        self.t = self.buf[pad:pad + n].view(dtype).view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.pad] == SENT32).all()) and bool((self.buf[self.pad + self.n:] == SENT32).all())


def _dev_bytes(struct):
    return torch.frombuffer(bytearray(bytes(struct)), dtype=torch.uint8).to(DEV)


class Rig:
    """The device side of one case: the sampler state of TailModel in guarded buffers, DevGen / DevDims as raw bytes, the embedding tables."""

    def __init__(self, H, model, gp, seed, hidden=0, bf16=False, pos=True, prefix=None, dims_max_length=None):
        m = self.m = model
        self.H, self.hidden, self.bf16 = H, hidden, bf16
        B, K, V = m.B, m.K, m.V
        self.ids = Guarded((B * K, m.ld), torch.int64)
        self.cur_len, self.first_unf = Guarded((B,), torch.int32), Guarded((B,), torch.int32)
        self.unfinished, self.has_eos = Guarded((B * K,), torch.int32), Guarded((B * K,), torch.int32)
        self.h = Guarded((B, max(hidden, 4)), torch.float32)
        self.h2 = Guarded((B, max(hidden, 4)), torch.float32)  # th_embed's output
        self.guarded = [self.ids, self.cur_len, self.first_unf, self.unfinished, self.has_eos, self.h]
        self.row_maxlen = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.logits = torch.zeros(B, K, V, dtype=torch.float32, device=DEV)
        self.gen = _dev_bytes(TH.DevGen(gp.max_length, gp.min_new_tokens, int(gp.do_sample), gp.top_k, int(gp.use_eos_gate), gp.temperature,
                                        gp.top_p, seed))
        self.prefix = None if prefix is None else torch.from_numpy(np.ascontiguousarray(prefix)).to(DEV)
        self.dims = _dev_bytes(TH.DevDims(m.P, 0, dims_max_length if dims_max_length is not None else gp.max_length, m.T_prefix,
                                          self.prefix.data_ptr() if self.prefix is not None else None,
                                          self.prefix.shape[1] if self.prefix is not None else 0))
        self.tables = self.pos_table = self.tables_host = self.pos_host = None
        self.model_h = np.full((B, max(hidden, 4)), SENT32, dtype=np.int32).view(F32)
        if hidden:
            g = torch.Generator().manual_seed(V * 131 + K)
            tab = torch.randn(K, V + 1, hidden, generator=g)
            self.tables = (tab.bfloat16() if bf16 else tab).to(DEV)
            self.tables_host = (tab.bfloat16().float() if bf16 else tab).numpy()  # a bf16 table holds bf16-rounded values, widened
            if pos:
                p = torch.randn(m.P + m.ld + 1, hidden, generator=g)
                self.pos_table, self.pos_host = p.to(DEV), p.numpy()
        self.upload()

    def args(self, grid=None, row0=0, with_tables=True, h=None):
        m = self.m
        a = TH.ThArgs()
        a.logits, a.ids, a.cur_len, a.unfinished = self.logits.data_ptr(), self.ids.ptr(), self.cur_len.ptr(), self.unfinished.ptr()
        a.has_eos, a.first_unf, a.gen, a.dims = self.has_eos.ptr(), self.first_unf.ptr(), self.gen.data_ptr(), self.dims.data_ptr()
        if self.tables is not None and with_tables:
            a.tables = self.tables.data_ptr()
            a.pos_table = self.pos_table.data_ptr() if self.pos_table is not None else None
        a.h = (h or self.h).ptr()
        a.row_maxlen = self.row_maxlen.data_ptr()
        a.ids_ld, a.B, a.K, a.V, a.eos, a.pad, a.H, a.bos = m.ld, m.B, m.K, m.V, m.eos, m.pad, self.hidden, m.bos
        a.bf16_tables, a.session, a.row0, a.grid = int(self.bf16), int(m.session), row0, m.B if grid is None else grid
        return a

    def upload(self):
        m = self.m
        self.ids.t.copy_(torch.from_numpy(m.ids))
        for g, v in ((self.cur_len, m.cur_len), (self.first_unf, m.first_unf), (self.unfinished, m.unfinished), (self.has_eos, m.has_eos)):
            g.t.copy_(torch.from_numpy(v))
        self.h.t.copy_(torch.from_numpy(self.model_h))
        if m.session:
            self.row_maxlen.copy_(torch.from_numpy(m.row_maxlen))

    def snapshot(self):
        return [g.buf.clone() for g in self.guarded] + [self.row_maxlen.clone()]

    def restore(self, snap):
        for g, s in zip(self.guarded, snap):
            g.buf.copy_(s)
        self.row_maxlen.copy_(snap[-1])

    def twice(self, launch):
        """Run `launch` twice from the same state; both results (guards included) must be bitwise equal."""
        before = self.snapshot()
        launch()
        first = self.snapshot()
        self.restore(before)
        launch()
        torch.cuda.synchronize()
        for a, b in zip(first, self.snapshot()):
            assert torch.equal(a, b), "two launches from the same state differ"

    def assert_equals_model(self, what):
        m = self.m
        for g in self.guarded + [self.h2]:
            assert g.guards_intact(), f"{what}: a guard was overwritten"
        assert np.array_equal(self.ids.t.cpu().numpy(), m.ids), (what, np.argwhere(self.ids.t.cpu().numpy() != m.ids)[:8])
        for name, g, v in (("cur_len", self.cur_len, m.cur_len), ("first_unf", self.first_unf, m.first_unf),
                           ("unfinished", self.unfinished, m.unfinished), ("has_eos", self.has_eos, m.has_eos)):
            assert np.array_equal(g.t.cpu().numpy(), v), (what, name, g.t.cpu().numpy(), v)
        if m.session:
            assert np.array_equal(self.row_maxlen.cpu().numpy(), m.row_maxlen), what
        got = self.h.t.cpu().numpy().view(np.int32)
        assert np.array_equal(got, self.model_h.view(np.int32)), (what, "h", np.argwhere(got != self.model_h.view(np.int32))[:8])

    def tail(self, lg, gp, seed, what, grid=None, row0=0, slots=None, with_tables=True):
        """One tail launch (twice), then the same step on the model, then the whole-state comparison. Returns the live slots."""
        m = self.m
        self.logits.copy_(torch.from_numpy(lg))
        kept = self.logits.clone()
        a = self.args(grid, row0, with_tables)

        def launch():
            assert self.H.tail(a, _stream()) == TH.PTTS_OK, self.H.error()

        self.twice(launch)
        assert torch.equal(self.logits.view(torch.int32), kept.view(torch.int32)), f"{what}: the logits changed"
        dev_ids = self.ids.t.cpu().numpy()

        def choose(row, accepted):  # an ambiguous draw: the device's token, which must come from the neighbourhood of the boundary
            tok = int(dev_ids[row, int(m.cur_len[row // m.K])])
            assert tok in accepted, (what, row, tok, sorted(accepted))
            return tok

        tabs = self.tables_host if with_tables else None
        live = m.step(lg, gp, slots=slots, seed=seed, choose=choose, tables=tabs, pos_table=self.pos_host, h=self.model_h)
        self.assert_equals_model(what)
        return live

    def embed_matches(self, what, slots):
        """embed_kernel<WT, SESSION> of the column just written (cur_len - 1) must give h bit for bit (rows of `slots`)."""
        self.h2.buf.fill_(SENT32)
        assert self.H.embed(self.args(h=self.h2), _stream()) == TH.PTTS_OK, self.H.error()
        a, b = self.h.t.view(torch.int32).cpu(), self.h2.t.view(torch.int32).cpu()
        for s in slots:
            assert torch.equal(a[s], b[s]), (what, s, torch.nonzero(a[s] != b[s])[:8])
        assert self.h2.guards_intact()


def _static(H, V, K, B, gp, seed=0, pad=None, **kw):
    eos, pad0, bos = SC.ids_of(V)
    prefix = kw.get("prefix")
    m = SM.TailModel(B, K, V, eos, pad0 if pad is None else pad, bos, ld=gp.max_length + 3, P=kw.pop("P", 2), prefix=prefix, max_length=gp.max_length,
                     fill=FILL)
    return Rig(H, m, gp, seed, **kw)


# ---- greedy, exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K,B,pad_is_eos", [(*s, True) for s in SC.GREEDY_SHAPES] + [(64, 4, 3, False)])
def test_greedy_state_after_every_step(H, V, K, B, pad_is_eos):
    eos = V - 8
    gp = SC.Gen(max_length=SC.greedy_max_length(K), min_new_tokens=SC.GREEDY_MIN_NEW)
    rig = _static(H, V, K, B, gp, pad=None if pad_is_eos else V - 7, hidden=32)
    noops = 0
    for s in range(SC.greedy_steps(K)):
        live = rig.tail(SC.greedy_logits(V, K, B, s, eos), gp, 0, f"greedy V={V} K={K} step {s}")
        noops += not live
    m = rig.m
    stamps = -m.unfinished.reshape(B, K)
    assert (m.unfinished < 0).all() and noops >= 4, (m.unfinished, noops)  # every row finished; the steps after that were no-ops
    assert (m.ids[:, :int(m.cur_len[0])] == eos).any()
    assert B == 1 or len(set(stamps.max(axis=1))) > 1  # utterances finish at different steps
    assert K == 1 or B == 1 or len(set(stamps[0])) == K  # EOS cascades codebook by codebook through the gate
    assert m.ids[K - 1, 2] == 0  # step 1: the only finite entry is the blocked EOS
    log_parity(f"greedy NV={SM.nv_of(V)} V={V} K={K} B={B} pad{'==' if pad_is_eos else '!='}eos: {SC.greedy_steps(K)} steps ({noops} no-ops), "
               f"{int(m.cur_len[0])} columns, state and h bit-exact after every step", LOG)


# ---- sampled, exact token -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", SC.SAMPLED_SHAPES)
@pytest.mark.parametrize("cfg", range(14))
def test_sampled_tokens_equal_the_predicted_draw(H, V, K, cfg):
    name, T, top_k, top_p = SC.sampled_configs(V)[cfg]
    eos = V - 8
    B = SC.sampled_batch(K)
    gp = SC.Gen(max_length=SC.SAMPLED_STEPS + 2, min_new_tokens=SC.SAMPLED_STEPS + 2, do_sample=True, temperature=T, top_k=top_k, top_p=top_p)
    lg = SC.sampled_logits(V, K, B, gp, eos)
    rig = _static(H, V, K, B, gp, seed=1234)
    for s in range(SC.SAMPLED_STEPS):
        rig.tail(lg, gp, 1234, f"sampled V={V} K={K} {name} step {s}")
    st = rig.m.stats
    share = st["ambiguous"] / st["draws"]
    log_parity(f"sampled NV={SM.nv_of(V)} V={V} K={K} B={B} {name}: {st['draws']} draws, {st['draws'] - st['ambiguous']} exact, "
               f"ambiguous {st['ambiguous']} ({100 * share:.2f} %), all within the accepted neighbourhood", LOG)
    assert st["draws"] >= 500, st
    assert share <= SC.AMBIGUOUS_CAP, st
    assert not (rig.m.ids[:, 1:SC.SAMPLED_STEPS + 1] == eos).any()  # MinNewTokens: the blocked EOS is never drawn


@pytest.mark.parametrize("V", [64, 1088, 2048])
def test_special_seeds_u_one_picks_the_last_kept_entry_and_the_smallest_u_the_first(H, V):
    K, B, eos = 4, 1, V - 8
    gp = SC.Gen(max_length=8, min_new_tokens=8, do_sample=True)
    lg = SC.sampled_logits(V, K, B, gp, eos)
    lg[0, 0] = SC._row("neg_inf", V, 1.0, np.random.default_rng(V))
    lg[0, 0, [0, V - 1]] = -np.inf  # neither end of the draw order is kept
    ks = SM.kept_set(lg[0, 0], gp, True, eos)
    order = [int(v) for v in SM.draw_order(V) if ks.weights[v] > 0]
    for seed, want in ((SC.SEED_U_ONE, order[-1]), (SC.SEED_U_MIN, order[0])):
        rig = _static(H, V, K, B, gp, seed=seed)
        assert SM.draw(ks.mask, ks.weights, SM.draw_u(seed, SC.SPECIAL_T, SC.SPECIAL_ROW), ks.tiny) == want
        rig.tail(lg, gp, seed, f"special seed {seed} V={V}")
        assert rig.m.ids[SC.SPECIAL_ROW, SC.SPECIAL_T] == want
    log_parity(f"special seeds NV={SM.nv_of(V)} V={V}: u == 1.0f -> last kept entry {order[-1]}, u == 2^-25 -> first {order[0]}", LOG)


@pytest.mark.parametrize("V,K,B", SC.GATE_SHAPES)
def test_blocked_eos_is_never_drawn_even_with_almost_all_the_mass(H, V, K, B):
    eos = V - 8
    gp = SC.gate_gen(K)
    rig = _static(H, V, K, B, gp, seed=99)
    m = rig.m
    for s in range(SC.gate_steps(K)):
        lg = SC.gate_logits(V, K, B, s, gp, eos)
        unf = m.unfinished.copy() > 0
        t = int(m.cur_len[0])
        if not rig.tail(lg, gp, 99, f"gate V={V} K={K} step {s}"):
            continue  # every row has finished: a no-op step
        col = m.ids[:, t].reshape(B, K)
        gate = np.arange(K)[None, :] > m.first_unf[:, None]
        blocked = gate | (s < gp.min_new_tokens)
        assert not (col[blocked & unf.reshape(B, K)] == eos).any(), (s, col)
        assert (col[~blocked] == eos).all(), (s, col)  # and where it is not blocked it is (practically) certain
    assert (m.unfinished < 0).all()
    st = m.stats
    log_parity(f"sampled gate NV={SM.nv_of(V)} V={V} K={K} B={B}: EOS with 1 - e^-20 of the mass drawn only where unblocked; {st['draws']} draws, "
               f"ambiguous {st['ambiguous']} ({100 * st['ambiguous'] / st['draws']:.2f} %)", LOG)
    assert st["draws"] > 0 and st["ambiguous"] / st["draws"] <= SC.AMBIGUOUS_CAP, st


# ---- session instances ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K,B,sample", SC.SESSION_CASES)
def test_session_slots_admitted_at_different_steps(H, V, K, B, sample):
    eos, pad, bos = SC.ids_of(V)
    steps, maxlen = SC.session_steps(K), SC.session_maxlen(K)
    gp = SC.session_gen(sample)
    m = SM.TailModel(B, K, V, eos, pad, bos, ld=steps + 8, session=True, P=2, fill=FILL)
    rig = Rig(H, m, gp, 7, hidden=32, dims_max_length=3)  # DevGen / DevDims max_length are not what a session slot stops on
    a = rig.args()
    launches = 0
    for ev in SC.session_events(V, K, B, sample):
        if ev[0] == "reset":
            _, slot, live, L = ev

            def launch():
                assert H.reset_rows(a, rig.row_maxlen.data_ptr(), slot, 1, live, L, _stream()) == TH.PTTS_OK, H.error()

            rig.twice(launch)
            m.reset_row(slot, live, L)
            rig.assert_equals_model(f"session V={V} K={K} reset slot {slot} live {live}")
        elif ev[0] == "admit":
            _, slot, lg = ev
            live = rig.tail(lg, gp, 7, f"session V={V} K={K} admit slot {slot}", grid=1, row0=slot, slots=[slot])
            assert live == [slot]
            rig.embed_matches(f"admit slot {slot}", [slot])
            launches += 1
        else:
            _, s, lg = ev
            live = rig.tail(lg, gp, 7, f"session V={V} K={K} step {s}", slots=None)
            rig.embed_matches(f"step {s}", live)
            launches += 1
    assert (m.unfinished[K * (B - 1):] == 0).all() and m.cur_len[B - 1] == 1  # the idle slot
    assert (m.unfinished[K:2 * K] == -maxlen[1]).all() and m.cur_len[1] == maxlen[1]
    assert B < 12 or all((m.unfinished[b * K:(b + 1) * K] < 0).all() and m.cur_len[b] < steps for b in (2, 5, 8))
    assert m.cur_len[0] == min(maxlen[0], 8)  # slot 0's second request: BOS, the admission's token, 6 steps
    st = m.stats
    share = st["ambiguous"] / st["draws"] if st["draws"] else 0.0
    log_parity(f"session NV={SM.nv_of(V)} V={V} K={K} slots={B} {'sampled' if sample else 'greedy'}: {launches} launches, state and h bit-exact "
               f"after each, idle and finished slots untouched; {st['draws']} draws, ambiguous {st['ambiguous']} ({100 * share:.2f} %)", LOG)
    assert (st["draws"] > 0) == sample and share <= SC.AMBIGUOUS_CAP, st


# ---- next-column embedding --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,bf16,pos,K,V,session,T_prefix,short", [
    (32, False, True, 4, 64, False, 0, False), (160, True, False, 9, 512, False, 3, False), (1536, False, True, 10, 64, False, 0, False),
    (1536, True, True, 17, 64, False, 0, False), (32, True, True, 9, 64, False, 0, True), (160, False, False, 10, 64, True, 0, False),
    (32, True, True, 17, 64, True, 0, False), (160, False, True, 17, 1152, False, 3, False)])
def test_next_column_embedding_is_bit_exact_on_both_paths(H, hidden, bf16, pos, K, V, session, T_prefix, short):
    eos, pad, bos = SC.ids_of(V)
    B = 2
    L = 2 * K - 2 if short else 2 * K + 3 + T_prefix  # short: below 2K - 1, no pattern at all
    gp = SC.Gen(max_length=L, min_new_tokens=L)  # no EOS: the columns run through the BOS triangle, the free band and the pad triangle
    prefix = np.random.default_rng(K).integers(0, V - 16, (B * K, T_prefix)) if T_prefix else None
    if session:
        m = SM.TailModel(B, K, V, eos, pad, bos, ld=L + 3, session=True, P=2, fill=FILL)
        rig = Rig(H, m, gp, 0, hidden=hidden, bf16=bf16, pos=pos, dims_max_length=3)
        for b, Lb in ((0, L), (1, 2 * K - 2)):  # slot 1 has no pattern
            assert H.reset_rows(rig.args(), rig.row_maxlen.data_ptr(), b, 1, 1, Lb, _stream()) == TH.PTTS_OK
            m.reset_row(b, 1, Lb)
    else:
        rig = _static(H, V, K, B, gp, hidden=hidden, bf16=bf16, pos=pos, prefix=prefix)
        m = rig.m
    bos_cols = pad_cols = 0
    for s in range(L - 1 - T_prefix):
        t = int(m.cur_len[0])
        lg = (np.random.default_rng([V, K, s]).standard_normal((B, K, V)) * 2).astype(F32)
        live = rig.tail(lg, gp, 0, f"embed H={hidden} K={K} step {s}")
        rig.embed_matches(f"embed H={hidden} K={K} step {s}", live)
        if not short:
            fed = m.fed_column(0, t)
            bos_cols += int((fed == bos).any())
            pad_cols += int((fed == pad).any())
    assert short or (bos_cols >= K - 1 - T_prefix and pad_cols >= K - 1), (bos_cols, pad_cols)
    # tables == null: the same launch writes nothing to h
    m.unfinished[:] = 1
    m.cur_len[:] = 2
    rig.model_h[:] = np.full_like(rig.model_h.view(np.int32), SENT32).view(F32)
    rig.upload()
    rig.tail(lg, gp, 0, "tables == null", with_tables=False)
    log_parity(f"embedding H={hidden} {'bf16' if bf16 else 'f32'} pos={'yes' if pos else 'null'} K={K} V={V} {'session' if session else 'static'} "
               f"T_prefix={T_prefix}{' no-pattern' if short else ''}: {L - 1 - T_prefix} columns, tail_embed_next == restatement == embed_kernel bitwise", LOG)
