"""GPU: step records (include/ptts_step_record.h) through every layer above the kernels - the engine through the ABI on the tiny fp32 model
(the step graph's node count, logits[i] against ptts_logits of a second, identically driven engine, scores[i] against the host model applied
to the recorded logits[i], also behind the penalty and the logit-edit node), ``generate()`` with ``model.enable_device_step_records()`` against
the host loop, sessions at the engine level (a recording request beside a plain one, two slots, slot reuse, group and voice admissions, the
e4m3 cache, refusals) and ``ContinuousBatcher`` end to end. The kernels themselves: tests/test_record_tail_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import cases as C
import logit_edit_model as LM
import penalty_model as PM
import sampler_cases as SC
import step_record_model as RM
import warper_model as WM
from helpers import log_parity, make_engine
from parler_tts_amd.generation_extras import logit_edits_of

pytestmark = pytest.mark.gpu

LOG = "device_step_records.txt"
EOS, K, V = 1024, 9, 1088
N_ENC, N_PROMPT = 9, 4
L = 10  # max_length of the engine-level runs: 9 generated columns
SENT = 0x7FC5A5A5
F32 = np.float32


@pytest.fixture(scope="module")
def pool():
    return C.batch_case(20)


def _arena(steps, lead):
    """[steps + 1 (a guard step), lead, V] under the sentinel, as float32."""
    return torch.full((steps + 1, lead, V), SENT, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _untouched(t):
    return bool((t.view(torch.int32) == SENT).all())


# ---- the engine through the ABI: static calls -------------------------------------------------------------------------------------------------
SEL = [0, 1, 2]


def _static(pool, scores=False, logits=False, gen=None, setup=None):
    spec, sd, enc, em, pr, pm, _ = pool
    eng = make_engine(spec, sd, torch.float32, max_batch=3)
    eng.set_gen_params(max_length=L, min_new_tokens=L, **(gen or dict(do_sample=False)))  # EOS blocked throughout: every row runs to max_length
    if setup:
        setup(eng)
    S = _arena(L - 1, 3 * K) if scores else None
    G = _arena(L - 1, 3 * K) if logits else None
    if scores or logits:
        eng.set_step_records(S, G, L - 1)
    ids = eng.generate_ids(enc[SEL], em[SEL], pr[SEL], pm[SEL]).cpu()
    assert ids.shape == (3 * K, L)
    return eng, ids, S, G


def test_graph_nodes_and_the_logits_equal_ptts_logits_of_a_second_engine(pool):
    spec, sd, enc, em, pr, pm, _ = pool
    plain, ids0, _, _ = _static(pool)
    n0 = plain.graph_nodes()
    layers = spec.num_hidden_layers
    assert n0 > layers  # (the count per configuration is pinned by tests/test_lm_gpu.py; here: what an engine that never heard of the feature captures)
    eng_s, ids_s, S, _ = _static(pool, scores=True)
    assert eng_s.graph_nodes() == n0  # scores alone: another instance of the tail, not another node
    eng_l, ids_l, _, G1 = _static(pool, logits=True)
    assert eng_l.graph_nodes() == n0 + 1
    eng, ids, S2, G = _static(pool, scores=True, logits=True)
    assert eng.graph_nodes() == n0 + 1
    for other in (ids_s, ids_l, ids):
        assert torch.equal(other, ids0)  # the tokens do not know about the records
    assert np.array_equal(_bits(S), _bits(S2)) and np.array_equal(_bits(G), _bits(G1))
    assert _untouched(S[L - 1]) and _untouched(G[L - 1])  # nothing at or beyond cap_steps
    # a second engine, driven through ptts_step_forward / ptts_push_tokens with the same tokens: its ptts_logits after step i
    ref = make_engine(spec, sd, torch.float32, max_batch=3)
    ref.set_gen_params(max_length=L, min_new_tokens=L, do_sample=False)
    ref.prefill(enc[SEL], em[SEL], pr[SEL], pm[SEL], sample=False)
    for i in range(L - 1):
        raw = ref.logits().reshape(3 * K, V)
        assert np.array_equal(_bits(raw), _bits(G[i])), f"logits[{i}] differ from ptts_logits after the same step"
        last = i == L - 2
        ref.push_tokens(ids[:, 1 + i], torch.full((3 * K,), int(last), dtype=torch.int32))
        if not last:
            ref.step_forward()
        # greedy scores: the recorded logits with the blocked EOS at -inf, every other entry with its bits; their arg-max is the token
        want = G[i].clone()
        want[:, EOS] = -float("inf")
        assert np.array_equal(_bits(S[i]), _bits(want)), i
        assert torch.equal(S[i].argmax(-1).cpu(), ids[:, 1 + i])
    # the feature off again on the same engine: the plain graphs, the same tokens, and the arenas are left alone
    eng.set_step_records(enabled=False)
    before = _bits(S2).copy()
    eng.set_gen_params(max_length=L, min_new_tokens=L, do_sample=False)
    assert torch.equal(eng.generate_ids(enc[SEL], em[SEL], pr[SEL], pm[SEL]).cpu(), ids0) and np.array_equal(_bits(S2), before)
    for e in (plain, eng_s, eng_l, eng, ref):
        e.close()
    log_parity(f"static B=3: graph nodes {n0} (off, scores only) / {n0 + 1} (logits); {L - 1} steps of logits bit-equal to ptts_logits of a second engine", LOG)


def test_graph_nodes_against_the_count_the_step_kernel_tests_pin():
    """tests/test_lm_gpu.py pins the step graph of a bf16 engine of 3 utterances at 6 nodes per layer + heads + tail. With the feature off that
    is the count; scores alone keep it (another instance of the tail), the logits add one node."""
    from oracle import decoder_oracle as DO

    spec = DO.DecoderSpec(num_hidden_layers=2, max_position_embeddings=256)
    sd = DO.make_decoder_weights(spec, seed=5)
    g = torch.Generator().manual_seed(2)
    enc, prompt = torch.randn(3, 9, spec.hidden_size, generator=g), torch.randn(3, 4, spec.hidden_size, generator=g)
    pinned = 6 * spec.num_hidden_layers + 2
    Kc, Vc = spec.num_codebooks, spec.vocab_size
    for scores, logits, want in ((False, False, pinned), (True, False, pinned), (False, True, pinned + 1), (True, True, pinned + 1)):
        eng = make_engine(spec, sd, torch.bfloat16, max_batch=3, max_ctx=64, max_enc=16, max_prompt=5)
        eng.set_gen_params(max_length=12, min_new_tokens=11)
        bufs = [torch.zeros(11, 3 * Kc, Vc, device="cuda") if on else None for on in (scores, logits)]
        if scores or logits:
            eng.set_step_records(bufs[0], bufs[1], 11)
        eng.prefill(enc, None, prompt, None, sample=True)
        eng.decode_steps(2)
        assert eng.graph_nodes() == want, (scores, logits, eng.graph_nodes())
        torch.cuda.synchronize()
        for t in bufs:
            assert t is None or (bool(t[:3].abs().sum(-1).gt(0).all()) and not bool(t[3:].any()))  # the prefill's tail + 2 steps, nothing else
        eng.close()


def test_an_arena_too_small_for_the_batch_is_refused_at_prefill(pool):
    spec, sd, enc, em, pr, pm, _ = pool
    eng = make_engine(spec, sd, torch.float32, max_batch=3)
    eng.set_gen_params(max_length=L, min_new_tokens=L, do_sample=False)
    small = _arena(L - 1, 2 * K)  # room for 2 utterances: the batch is not known when the arenas are set
    eng.set_step_records(small, None, L)
    with pytest.raises(ValueError, match="need more"):
        eng.prefill(enc[SEL], em[SEL], pr[SEL], pm[SEL], sample=True)
    torch.cuda.synchronize()
    assert _untouched(small)
    eng.prefill(enc[:2], em[:2], pr[:2], pm[:2], sample=True)  # the same arenas serve a batch of 2
    torch.cuda.synchronize()
    assert not _untouched(small[0]) and _untouched(small[1:])
    eng.close()


@pytest.mark.parametrize("warp", [False, True])
def test_sampled_scores_equal_the_model_on_the_recorded_logits_and_the_drawn_token_is_finite(pool, warp):
    gen = dict(do_sample=True, temperature=0.8, top_k=40, top_p=0.9, seed=1234)
    wp = WM.Warp(min_p=0.05, epsilon_cutoff=3e-4) if warp else WM.NEUTRAL
    setup = (lambda e: e.set_sample_warp(min_p=wp.min_p, epsilon_cutoff=wp.epsilon_cutoff)) if warp else None
    eng, ids, S, G = _static(pool, scores=True, logits=True, gen=gen, setup=setup)
    gp = SC.Gen(max_length=L, min_new_tokens=L, do_sample=True, temperature=0.8, top_k=40, top_p=0.9)
    rows = doubtful = 0
    Sn, Gn = S.cpu().numpy(), G.cpu().numpy()
    for i in range(L - 1):
        for r in range(3 * K):
            want, maybe = RM.recorded_row(Gn[i, r], gp, wp, True, EOS)
            bad = (Sn[i, r].view(np.int32) != want.view(np.int32)) & ~maybe
            assert not bad.any(), (i, r, np.nonzero(bad)[0][:6])
            rows, doubtful = rows + 1, doubtful + bool(maybe.any())
            assert np.isfinite(Sn[i, r, int(ids[r, 1 + i])]), (i, r)
        assert (Sn[i][:, EOS] == -np.inf).all() and (np.isfinite(Sn[i]).sum(-1) <= 40).all()
    assert doubtful / rows <= SC.AMBIGUOUS_CAP, (doubtful, rows)
    eng.close()


def test_scores_behind_the_penalty_and_the_logit_edit_node(pool):
    """scores[i] = the tail's vector over what the two nodes made of logits[i]: their host models (tests/penalty_model.py, tests/logit_edit_model.py)
    applied to the recorded raw logits, then the blocked EOS. The raw logits are the heads' - what the same engine shows without the nodes."""
    rec = LM.Record(sequence_bias={(7,): 3.0, (EOS,): -1.0}, suppress_tokens=list(range(0, 512)), begin_suppress_tokens=list(range(512, 600)))
    _, ids_plain, _, G_plain = _static(pool, logits=True)
    eng, ids, S, G = _static(pool, scores=True, logits=True, setup=lambda e: e.set_logit_edits(logit_edits_of(V, EOS, L, **rec._asdict())))
    assert eng.graph_nodes() > 0 and np.array_equal(_bits(G[0]), _bits(G_plain[0]))  # step 0: the same prefill, the logits as the heads wrote them
    Gn = G.cpu().numpy()
    for i in range(L - 1):
        want = np.concatenate([LM.apply_row(Gn[i, b * K:(b + 1) * K], rec, 1 + i, 1, EOS) for b in range(3)]).astype(F32)
        want[:, EOS] = -np.inf
        assert np.array_equal(_bits(S[i]), want.view(np.int32)), i
        assert torch.equal(S[i].argmax(-1).cpu(), ids[:, 1 + i])
    eng.close()
    eng, ids, S, G = _static(pool, scores=True, logits=True, setup=lambda e: e.set_history_penalty(1.3, 2))
    Gc = G.cpu()
    for i in range(L - 1):
        want = torch.stack([PM.apply_row(Gc[i, r], ids[r, :1 + i], 1.3, 2) for r in range(3 * K)])
        want[:, EOS] = -float("inf")
        assert np.array_equal(_bits(S[i]), _bits(want)), i
        assert torch.equal(S[i].argmax(-1).cpu(), ids[:, 1 + i])
    eng.close()


# ---- generate() -----------------------------------------------------------------------------------------------------------------------------
def _gen_inputs(B):
    g = torch.Generator().manual_seed(5)
    desc = torch.randint(3, 128, (B, 6), generator=g).cuda()
    prompt_ids = torch.randint(3, 128, (B, 3), generator=g).cuda()
    mask = torch.ones(B, 6, dtype=torch.long)
    for b in range(1, B):
        mask[b, 6 - b:] = 0  # rows of different lengths
    return dict(input_ids=desc, attention_mask=mask.cuda(), prompt_input_ids=prompt_ids, do_sample=False, return_dict_in_generate=True, output_scores=True,
                output_logits=True)


@pytest.mark.parametrize("B,voice,min_new", [(1, False, 4), (3, False, 4), (3, True, 4), (3, False, 20), (1, True, 0)])
def test_generate_with_the_switch_against_the_host_loop(B, voice, min_new):
    """Greedy fp32, eos_gain 6 (the rows of a batch end on EOS at different columns). The bar between the device loop and the host loop that
    tests/test_generate_gpu.py already uses is equality of the tokens; the logits of both loops come from the same kernels on the same
    inputs, and on this model they are bit-equal, so equality is what is asserted - of the logits, of the scores (hence of their -inf
    patterns), of the tuple lengths and of the waveforms."""
    m, *_ = C.tiny_model(seed=6, eos_gain=6.0)
    m = m.to("cuda")
    kw = dict(_gen_inputs(B), max_new_tokens=36, min_new_tokens=min_new)
    if voice:
        kw["decoder_input_ids"] = torch.randint(0, 1024, (B * K, 5), generator=torch.Generator().manual_seed(3)).cuda()
    host = m.generate(**kw)
    host_ids = m._engine.ids().cpu()
    m.enable_device_step_records()
    dev = m.generate(**kw)
    dev_ids = m._engine.ids().cpu()
    assert m._engine.step_records is None  # the engine let go of the arenas
    assert torch.equal(dev_ids, host_ids) and torch.equal(dev.sequences, host.sequences) and dev["audios_length"] == host["audios_length"]
    given = 6 if voice else 1
    for name in ("scores", "logits"):
        a, b = dev[name], host[name]
        assert isinstance(a, tuple) and len(a) == len(b) == dev_ids.shape[1] - given
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape == (B * K, V)
            assert torch.equal(torch.isinf(x), torch.isinf(y)), (name, i)
            assert np.array_equal(_bits(x), _bits(y.float())), (name, i, float((x - y).abs().nan_to_num(0).max()))
    if min_new:
        assert all(bool((s[:, EOS] == -float("inf")).all()) for s in dev["scores"][:min_new])
    plain = m.generate(**{k: v for k, v in kw.items() if not k.startswith("output_")})
    assert torch.equal(plain.sequences, host.sequences)


def test_generate_on_the_overlap_codec_path():
    """model.overlap_codec: the token graph runs a chunk ahead of the codec on a side stream. The records are those of the plain device loop,
    and the waveform is the overlapped one."""
    m, *_ = C.tiny_model(seed=6)
    m = m.to("cuda").enable_device_step_records()
    kw = dict(_gen_inputs(2), max_new_tokens=120, min_new_tokens=120)
    ref = m.generate(**kw)
    calls = []
    loop = m._run_device_loop_overlap
    m._run_device_loop_overlap = lambda *a, **k: calls.append(1) or loop(*a, **k)
    m.overlap_codec = True
    out = m.generate(**kw)
    m.overlap_codec = False
    assert calls == [1] and torch.equal(out.sequences, ref.sequences)
    for name in ("scores", "logits"):
        assert len(out[name]) == len(ref[name]) == 120
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(out[name], ref[name])), name


def test_generate_with_the_streamer_and_with_a_sampled_call():
    import threading

    import parler_tts_amd as P

    m, *_ = C.tiny_model(seed=6, eos_gain=6.0)
    m = m.to("cuda").enable_device_step_records()
    kw = dict(_gen_inputs(1), max_new_tokens=36, min_new_tokens=4)
    ref = m.generate(**kw)
    streamer = P.ParlerTTSStreamer(m, device="cuda", play_steps=10)
    got = {}
    th = threading.Thread(target=lambda: got.update(out=m.generate(streamer=streamer, **kw)))
    th.start()
    chunks = [c for c in streamer]
    th.join()
    out = got["out"]
    assert len(chunks) >= 1 and len(out["scores"]) == len(ref["scores"]) == len(out["logits"])
    for name in ("scores", "logits"):
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(out[name], ref[name])), name
    # sampling: the drawn token has a finite score, top-k bounds the finite entries, and the raw logits are unprocessed
    torch.manual_seed(11)
    out = m.generate(**dict(kw, do_sample=True, top_k=30, temperature=0.9))
    ids = m._engine.ids().cpu()
    assert len(out["scores"]) == ids.shape[1] - 1
    unfinished = torch.ones(K, dtype=torch.bool)
    for i, (s, lg) in enumerate(zip(out["scores"], out["logits"])):
        tok = ids[:, 1 + i]
        s = s.cpu()
        assert bool(torch.isfinite(s[torch.arange(K), tok])[unfinished].all()), i
        assert bool((torch.isfinite(s).sum(-1) <= 30).all()) and bool(torch.isfinite(lg).all())
        unfinished &= tok != EOS


# ---- sessions at the engine level -----------------------------------------------------------------------------------------------------------
MAXLEN, MIN_NEW = 14, 2
BYSTANDER, REC, NEXT = 19, 9, 5


def _session(pool, slots, feature, max_batch=None, max_length=MAXLEN, **engine_kw):
    spec, sd = pool[0], pool[1]
    eng = make_engine(spec, sd, engine_kw.pop("dtype", torch.float32), max_batch=max_batch or slots, max_prompt=16, **engine_kw)
    eng.set_gen_params(max_length=max_length, min_new_tokens=MIN_NEW, do_sample=False)
    if feature:
        eng.set_step_records(None, None, 0)  # on, no slot records yet
    eng.begin_session(slots, N_ENC, N_PROMPT, **({"kv_fp8": True} if engine_kw.get("kv_fp8") else {}))
    return eng


def _admit(eng, slot, pool, i, bufs=None, cap=MAXLEN - 1, **kw):
    _, _, enc, em, pr, pm, _ = pool
    if bufs is not None:
        eng.set_slot_step_records(slot, bufs[0], bufs[1], cap)
    eng.admit_row(slot, enc[i], em[i], pr[i], pm[i], sample=True, **kw)


def _bufs(steps=MAXLEN - 1):
    return _arena(steps, K), _arena(steps, K)


def _steps_of(eng, slot, T=0):
    cur, _ = eng.row_state()
    return cur[slot] - 1 - T


def _greedy_scores_hold(S, G, ids, steps, given=1):
    """scores[i] = logits[i] but for the EOS entry (blocked: -inf; free: its bits), and the token is its arg-max."""
    for i in range(steps):
        s, g = _bits(S[i]), _bits(G[i])
        other = np.arange(V) != EOS
        assert np.array_equal(s[:, other], g[:, other]), i
        assert all(s[k, EOS] == g[k, EOS] or S[i][k, EOS] == -float("inf") for k in range(K)), i
        assert torch.equal(S[i].argmax(-1).cpu(), ids[:, given + i]), i


def test_a_recording_request_beside_a_plain_one_two_slots_and_slot_reuse(pool):
    def run(feature):
        eng = _session(pool, 3, feature)
        _admit(eng, 0, pool, BYSTANDER)
        eng.decode_steps(2)
        b1 = _bufs() if feature else None
        _admit(eng, 1, pool, REC, b1)
        eng.decode_steps(3)
        b2 = _bufs() if feature else None
        _admit(eng, 2, pool, REC, b2)  # the same request, another slot, another time
        eng.decode_steps(MAXLEN)
        cur, live = eng.row_state()
        assert live == [False, False, False]
        return eng, [eng.row_ids(s, cur[s]).cpu() for s in range(3)], b1, b2, cur

    off, ids_off, _, _, _ = run(False)
    nodes_off = off.graph_nodes()
    off.close()
    eng, ids_on, b1, b2, cur = run(True)
    assert eng.graph_nodes() == nodes_off + 1  # the logits node; the tail is another instance
    for a, b in zip(ids_on, ids_off):
        assert torch.equal(a, b)  # the plain slot (and the recording ones): the tokens of the session without the feature
    steps = cur[1] - 1
    assert cur[1] == cur[2] and 1 <= steps <= MAXLEN - 1
    for kind in (0, 1):
        assert np.array_equal(_bits(b1[kind][:steps]), _bits(b2[kind][:steps]))  # equal records in two slots
        assert _untouched(b1[kind][steps:]) and _untouched(b2[kind][steps:])  # and nothing behind the steps made
    _greedy_scores_hold(b1[0], b1[1], ids_on[1], steps)
    # the slot is reused by a request without a record: the previous buffers keep their bytes
    before = [_bits(t).copy() for t in b1]
    eng.retire_row(1)
    _admit(eng, 1, pool, NEXT)
    eng.decode_steps(MAXLEN)
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(t), x) for t, x in zip(b1, before))
    # ... and a record set and cleared before the admission records nothing either
    eng.retire_row(2)
    b3 = _bufs()
    eng.set_slot_step_records(2, b3[0], b3[1], MAXLEN - 1)
    eng.set_slot_step_records(2, default=True)
    _admit(eng, 2, pool, NEXT)
    eng.decode_steps(3)
    torch.cuda.synchronize()
    assert _untouched(b3[0]) and _untouched(b3[1])
    # cap_steps below the steps made: the guard steps behind it keep the sentinel
    eng.retire_row(2)
    b4 = _bufs()
    _admit(eng, 2, pool, REC, b4, cap=3)
    eng.decode_steps(MAXLEN)
    torch.cuda.synchronize()
    for kind in (0, 1):
        assert np.array_equal(_bits(b4[kind][:3]), _bits(b1[kind][:3])) and _untouched(b4[kind][3:])
    eng.close()


def test_step_zero_is_present_after_group_and_voice_admissions(pool):
    _, _, enc, em, pr, pm, _ = pool
    T = 5
    total = MAXLEN + T
    voice = lambda seed: torch.randint(0, 1024, (K, T), generator=torch.Generator().manual_seed(seed)).cuda()  # noqa: E731
    eng = _session(pool, 4, True, max_batch=8, max_length=total)
    a, b = 7, 2
    ba, bb = _bufs(total), _bufs(total)
    eng.set_slot_step_records(1, ba[0], ba[1], total)
    eng.set_slot_step_records(0, bb[0], None, total)  # scores only
    eng.admit_rows([1, 0], enc[[a, b]], em[[a, b]], pr[[a, b]], pm[[a, b]], max_lengths=[MAXLEN, MAXLEN], sample=True)  # ptts_admit_rows
    bc, bd = _bufs(total), _bufs(total)
    eng.set_slot_step_records(2, bc[0], bc[1], total)
    eng.set_slot_step_records(3, None, bd[1], total)  # logits only
    eng.admit_rows([2, 3], enc[[3, 13]], em[[3, 13]], pr[[3, 13]], pm[[3, 13]], max_lengths=[total, MAXLEN + 3], sample=True,
                   voices=[voice(77), voice(78)[:, :3]])  # ptts_admit_rows_voice, ragged
    torch.cuda.synchronize()
    for bufs in (ba, bc):
        assert not _untouched(bufs[0][0]) and not _untouched(bufs[1][0]) and _untouched(bufs[0][1:]) and _untouched(bufs[1][1:])  # step 0, at index 0
    assert not _untouched(bb[0][0]) and _untouched(bb[1]) and not _untouched(bd[1][0]) and _untouched(bd[0])
    eng.decode_steps(MAXLEN)
    cur, live = eng.row_state()
    assert not any(live)
    for slot, bufs, Tv in ((1, ba, 0), (2, bc, T)):
        steps = cur[slot] - 1 - Tv
        _greedy_scores_hold(bufs[0], bufs[1], eng.row_ids(slot, cur[slot]).cpu(), steps, given=1 + Tv)
        assert bool((bufs[0][:MIN_NEW, :, EOS] == -float("inf")).all())  # min_new_tokens counts from the slot's own given columns
        assert _untouched(bufs[0][steps:]) and _untouched(bufs[1][steps:])
    assert _untouched(bd[1][cur[3] - 1 - 3:]) and not _untouched(bd[1][cur[3] - 1 - 3 - 1])
    # one request with a prompt alone: ptts_admit_row_voice
    eng.retire_row(2)
    be = _bufs(total)
    _admit(eng, 2, pool, 3, be, cap=total, voice=voice(77), max_length=total)
    eng.decode_steps(MAXLEN)
    cur, live = eng.row_state()
    steps = cur[2] - 1 - T
    assert not live[2] and steps >= MIN_NEW
    _greedy_scores_hold(be[0], be[1], eng.row_ids(2, cur[2]).cpu(), steps, given=1 + T)
    assert _untouched(be[0][steps:]) and _untouched(be[1][steps:])
    eng.close()


def test_a_session_on_the_e4m3_cache_records(pool):
    eng = _session(pool, 12, True, max_batch=12, dtype=torch.bfloat16, kv_fp8=True, max_ctx=64)
    bufs = _bufs()
    _admit(eng, 0, pool, BYSTANDER)
    _admit(eng, 7, pool, REC, bufs)
    eng.decode_steps(MAXLEN)
    cur, live = eng.row_state()
    assert not live[7]
    steps = cur[7] - 1
    _greedy_scores_hold(bufs[0], bufs[1], eng.row_ids(7, cur[7]).cpu(), steps)
    assert _untouched(bufs[0][steps:]) and _untouched(bufs[1][steps:]) and bool(torch.isfinite(bufs[1][:steps]).all())
    eng.close()


def test_refusals_are_values_and_change_nothing(pool):
    from parler_tts_amd import _native as N

    spec, sd = pool[0], pool[1]
    eng = make_engine(spec, sd, torch.float32, max_batch=2, max_prompt=16)
    eng.set_gen_params(max_length=MAXLEN, min_new_tokens=MIN_NEW, do_sample=False)
    buf = _arena(4, K)
    for bad in (N.PttsStepRecords(None, None, -1), N.PttsStepRecords(buf.data_ptr(), None, 0), N.PttsStepRecords(None, buf.data_ptr(), 0)):
        assert eng.lib.ptts_set_step_records(eng._h, ctypes.byref(bad), None) == N.PTTS_E_INVALID
    eng.set_step_records(None, None, 0)  # the feature on, and no session
    with pytest.raises(ValueError, match="no continuous session"):
        eng.set_slot_step_records(0, buf, None, 4)
    eng.close()
    eng = _session(pool, 2, False)
    with pytest.raises(ValueError, match="without step records"):
        eng.set_slot_step_records(0, buf, None, 4)  # a session begun with the feature off
    _admit(eng, 0, pool, BYSTANDER)
    with pytest.raises(ValueError, match="running session"):
        eng.set_step_records(None, None, 0)  # the setter inside a session that holds a request
    assert eng.step_records is None
    eng.close()
    eng = _session(pool, 2, True)
    _admit(eng, 0, pool, BYSTANDER)
    with pytest.raises(ValueError, match="still holds a request"):
        eng.set_slot_step_records(0, buf, None, 4)  # a busy slot
    with pytest.raises(ValueError, match="outside the session"):
        eng.set_slot_step_records(2, buf, None, 4)
    with pytest.raises(ValueError, match="running session"):
        eng.set_step_records(enabled=False)
    for bad in (N.PttsStepRecords(buf.data_ptr(), None, -2), N.PttsStepRecords(buf.data_ptr(), None, 0)):
        assert eng.lib.ptts_set_slot_step_records(eng._h, 1, ctypes.byref(bad), None) == N.PTTS_E_INVALID
    with pytest.raises(ValueError, match="float32"):
        eng.set_slot_step_records(1, buf.double(), None, 4)  # the wrapper's own checks
    with pytest.raises(ValueError, match="need more"):
        eng.set_slot_step_records(1, buf, None, 9)
    _admit(eng, 1, pool, NEXT)  # the refused calls left slot 1 without a record
    eng.decode_steps(MAXLEN)
    torch.cuda.synchronize()
    assert _untouched(buf)
    eng.close()


# ---- ContinuousBatcher end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", [False, True])
def test_continuous_batcher_end_to_end(stream):
    """Mixed requests through the scheduler: the ones that ask for records get what the same request gives alone in a session of one slot,
    the ones that ask for none decode as in a batcher on a model without the switch. Streaming mode: the records are there with the last chunk."""
    import parler_tts_amd as P

    m, *_ = C.tiny_model(seed=2, eos_gain=6.0)
    m = m.to("cuda")
    g = torch.Generator().manual_seed(313)
    base = [dict(input_ids=torch.randint(3, 128, (9 - i % 3,), generator=g), prompt_input_ids=torch.randint(3, 128, (5 - i % 2,), generator=g), max_new_tokens=24)
            for i in range(4)]
    kw = dict(max_description_tokens=9, max_prompt_tokens=5, poll_steps=5, do_sample=False, max_new_tokens=24, min_new_tokens=2)
    if stream:
        kw.update(stream_chunk_frames=4)
    opts = [dict(output_scores=True), dict(), dict(output_scores=True, output_logits=True), dict(output_logits=True)]

    def run(reqs, slots):
        cb = P.ContinuousBatcher(m, slots=slots, **kw)
        tickets = [cb.submit(**r) for r in reqs]
        wav, recs = {}, {}
        if stream:
            for t, chunk, last in cb.chunks():
                wav[t] = torch.cat([wav[t], chunk]) if t in wav else chunk
                if last and any(reqs[tickets.index(t)].get(k) for k in ("output_scores", "output_logits")):
                    recs[t] = cb.step_records(t)
        else:
            for t, w, n in cb:
                wav[t] = w
                if any(reqs[tickets.index(t)].get(k) for k in ("output_scores", "output_logits")):
                    recs[t] = cb.step_records(t)
        cb.close()
        return [wav[t] for t in tickets], [recs.get(t) for t in tickets]

    plain_wav, _ = run(base, 2)
    with pytest.raises(ValueError, match="enable_device_step_records"):
        P.ContinuousBatcher(m, slots=2, **kw).submit(**base[0], output_scores=True)
    m.enable_device_step_records()
    wav, recs = run([dict(r, **o) for r, o in zip(base, opts)], 2)
    for a, b in zip(wav, plain_wav):
        assert torch.equal(a, b)  # every waveform, the plain request's included: as in a session without the feature
    assert recs[1] is None and sorted(recs[0]) == ["scores"] and sorted(recs[2]) == ["logits", "scores"] and sorted(recs[3]) == ["logits"]
    for i in (0, 2, 3):
        solo_wav, solo = run([dict(base[i], **opts[i])], 1)  # the same request alone
        assert torch.equal(solo_wav[0], wav[i])
        for kind, t in recs[i].items():
            assert t.shape == solo[0][kind].shape and t.shape[1:] == (K, V) and 2 <= t.shape[0] <= 24
            assert np.array_equal(_bits(t), _bits(solo[0][kind])), (i, kind)
    s, lg = recs[2]["scores"], recs[2]["logits"]
    other = torch.arange(V) != EOS
    assert np.array_equal(_bits(s[:, :, other]), _bits(lg[:, :, other])) and bool((s[:2, :, EOS] == -float("inf")).all())


def test_continuous_batcher_records_a_request_with_a_voice_prompt():
    """A request that continues a voice prompt of 4 frames beside a plain recording one: its records start at its own first generated column
    (min_new_tokens counts from there), have one entry per token it generated, and equal those of the same request alone."""
    import parler_tts_amd as P

    m, *_ = C.tiny_model(seed=2, eos_gain=6.0)
    m = m.to("cuda").enable_device_step_records()
    g = torch.Generator().manual_seed(99)
    reqs = [dict(input_ids=torch.randint(3, 128, (9,), generator=g), prompt_input_ids=torch.randint(3, 128, (5,), generator=g), max_new_tokens=20,
                 output_scores=True, output_logits=True) for _ in range(3)]
    reqs[1]["decoder_input_ids"] = torch.randint(0, 1024, (K, 4), generator=g)
    kw = dict(max_description_tokens=9, max_prompt_tokens=5, poll_steps=5, do_sample=False, max_new_tokens=20, min_new_tokens=3, max_voice_frames=4)

    def run(rs, slots):
        cb = P.ContinuousBatcher(m, slots=slots, **kw)
        tickets = [cb.submit(**r) for r in rs]
        steps = {}
        orig = cb.eng.retire_row

        def retire(s):  # the tokens a request generated, read when the scheduler lets its slot go
            cur, _ = cb.eng.row_state()
            steps[cb._slot[s].ticket] = cur[s] - 1 - cb._slot[s].T
            orig(s)

        cb.eng.retire_row = retire
        wav = {t: w for t, w, n in cb}
        recs = [cb.step_records(t) for t in tickets]
        cb.close()
        cb.eng.retire_row = orig  # the engine is the model's: the next batcher gets it back as it was
        return [wav[t] for t in tickets], recs, [steps[t] for t in tickets]

    wav, recs, steps = run(reqs, 2)
    solo_wav, solo, solo_steps = run(reqs[1:2], 1)
    assert torch.equal(wav[1], solo_wav[0]) and steps[1] == solo_steps[0] and 3 <= steps[1] <= 20
    for kind in ("scores", "logits"):
        assert recs[1][kind].shape == (steps[1], K, V) and np.array_equal(_bits(recs[1][kind]), _bits(solo[0][kind])), kind
    s, lg = recs[1]["scores"], recs[1]["logits"]
    other = torch.arange(V) != EOS
    assert np.array_equal(_bits(s[:, :, other]), _bits(lg[:, :, other])) and bool((s[:3, :, EOS] == -float("inf")).all())
    assert bool(torch.isfinite(s[3, 0, EOS]))  # ... and no longer: the count started behind the prompt's 4 frames
    for i in (0, 2):
        assert recs[i]["scores"].shape[0] == steps[i]
