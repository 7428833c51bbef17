"""Continuous batching on the GPU: a session of utterance slots with per-slot clocks (ptts_session_begin / ptts_admit_row /
ptts_row_state / ptts_retire_row), judged against the CPU oracle run on every request ALONE: the oracle on one row equals the same
row of its batched run, so row independence is a property of the reference.

Tolerances are those of tests/test_lm_gpu.py: fp32 logits 2e-5, bf16 2e-2 against DecoderOracle(precision="bf16"); free-running ids
are compared bit for bit on requests whose oracle top-2 margin is asserted >= cases.MARGIN."""
import functools

import pytest
import torch

import cases as C
from helpers import make_engine
from oracle import decoder_oracle as DO

pytestmark = pytest.mark.gpu

# per-request max_length of the 20 requests of cases.batch_case(20): both sides of the 2K - 1 = 17 delay-pattern threshold
LENGTHS = [11, 12, 13, 14, 15, 16, 17, 20, 19, 20, 11, 12, 13, 17, 15, 16, 17, 18, 19, 20]
N_ENC, N_PROMPT = 9, 4


@functools.lru_cache(maxsize=None)
def _pool(precision="fp32"):
    """The request pool and the oracle's trace of every request on its own (EOS blocked, so every request runs to its own max_length)."""
    spec, sd, enc, enc_mask, prompt, prompt_mask, _ = C.batch_case(20)
    orc = DO.DecoderOracle(spec, sd, precision=precision)
    refs = []
    with torch.no_grad():
        for i, L in enumerate(LENGTHS):
            sl = slice(i, i + 1)
            refs.append(DO.sample_loop(orc, enc[sl], enc_mask[sl], prompt[sl], prompt_mask[sl], DO.GenParams(max_length=L, min_new_tokens=L - 1),
                                       keep_logits=True))
    return spec, sd, enc, enc_mask, prompt, prompt_mask, refs


def _admit(eng, slot, pool, i, sample=True, max_length=None):
    _, _, enc, enc_mask, prompt, prompt_mask, _ = pool
    eng.admit_row(slot, enc[i], enc_mask[i], prompt[i], prompt_mask[i], max_length=LENGTHS[i] if max_length is None else max_length, sample=sample)


def _free_run(eng, pool, slots, chunk, order=None):
    """FIFO admission into idle slots, `chunk` steps per poll; returns {request: ids [K, columns]} and the (request, slot) admission log."""
    eng.begin_session(slots, N_ENC, N_PROMPT)
    queue = list(range(len(LENGTHS)) if order is None else order)
    in_slot = [None] * slots
    out, log = {}, []
    polls = 0
    while queue or any(r is not None for r in in_slot):
        for s in range(slots):
            if in_slot[s] is None and queue:
                in_slot[s] = queue.pop(0)
                _admit(eng, s, pool, in_slot[s])
                log.append((in_slot[s], s))
        eng.decode_steps(chunk)
        cur, live = eng.row_state()
        for s in range(slots):
            if in_slot[s] is not None and not live[s]:
                out[in_slot[s]] = eng.row_ids(s, cur[s]).cpu()
                eng.retire_row(s)
                in_slot[s] = None
        polls += 1
        assert polls < 2000, "the session does not drain"
    return out, log


@pytest.mark.parametrize("chunk", [1, 3, 16])
@pytest.mark.parametrize("slots", [3, 12])
def test_free_running_mixed_ages_and_per_request_lengths(slots, chunk):
    """20 requests with their own max_length through 3 slots (GEMV step) and 12 slots (MFMA strips), admitted whenever a slot frees up:
    every request's ids equal the oracle's run of that request alone, bit for bit."""
    pool = _pool()
    spec, sd, refs = pool[0], pool[1], pool[6]
    for i, ref in enumerate(refs):
        assert ref.min_margin >= C.MARGIN, (i, ref.min_margin)
    eng = make_engine(spec, sd, torch.float32, max_batch=slots)
    eng.set_gen_params(max_length=20, min_new_tokens=19)
    out, log = _free_run(eng, pool, slots, chunk)
    eng.close()
    assert sorted(out) == list(range(20))
    assert [r for r, _ in log] == list(range(20))  # FIFO
    for i, ref in enumerate(refs):
        assert out[i].shape == ref.sequences.shape, (i, out[i].shape, ref.sequences.shape)
        assert torch.equal(out[i], ref.sequences), i


def _teacher_forced_session(eng, slots, n_enc, n_prompt, reqs, refs, lengths, tol, K):
    """Manual path: rows admitted (un-sampled) at steps 0, 3, 5, 7, ...; every live row is fed the oracle's own tokens and its logits are
    compared with the oracle's at the row's own step, after the admission and after every forward."""
    eng.begin_session(slots, n_enc, n_prompt)
    queue = list(range(len(lengths)))
    in_slot, col = [None] * slots, [0] * slots  # col: columns the slot holds
    worst, checked, step, done = 0.0, 0, 0, 0
    while done < len(lengths):
        if (step == 0 or (step >= 3 and step % 2 == 1)) and queue and None in in_slot:
            s = in_slot.index(None)
            i = queue.pop(0)
            enc, enc_mask, prompt, prompt_mask = reqs
            eng.admit_row(s, enc[i], None if enc_mask is None else enc_mask[i], prompt[i], None if prompt_mask is None else prompt_mask[i],
                          max_length=lengths[i], sample=False)
            in_slot[s], col[s] = i, 1
        lg = eng.logits().cpu().view(slots, K, -1)
        tokens = torch.zeros(slots * K, dtype=torch.long)
        for s, i in enumerate(in_slot):
            if i is None:
                continue
            err = float((lg[s] - refs[i].step_logits[col[s] - 1]).abs().max())
            worst, checked = max(worst, err), checked + 1
            assert err < tol, (i, s, col[s], err)
            tokens[s * K:(s + 1) * K] = refs[i].sequences[:, col[s]]
        eng.push_tokens(tokens)
        cur, live = eng.row_state()
        for s, i in enumerate(in_slot):
            if i is None:
                assert cur[s] == 1 and not live[s]
                continue
            col[s] += 1
            assert cur[s] == col[s]
            if col[s] == lengths[i]:  # the request's last column: the slot has finished by its own max_length
                assert not live[s]
                eng.retire_row(s)
                in_slot[s] = None
                done += 1
            else:
                assert live[s]
        eng.step_forward()
        step += 1
        assert step < 4000
    return worst, checked


@pytest.mark.parametrize("dtype,prec,tol", [(torch.float32, "fp32", 2e-5), (torch.bfloat16, "bf16", 2e-2)])
@pytest.mark.parametrize("slots", [3, 12])
def test_teacher_forced_logits_at_each_rows_own_step(slots, dtype, prec, tol):
    pool = _pool(prec)
    spec, sd, enc, enc_mask, prompt, prompt_mask, refs = pool
    eng = make_engine(spec, sd, dtype, max_batch=slots)
    eng.set_gen_params(max_length=20, min_new_tokens=19)
    worst, checked = _teacher_forced_session(eng, slots, N_ENC, N_PROMPT, (enc, enc_mask, prompt, prompt_mask), refs, LENGTHS, tol, spec.num_codebooks)
    eng.close()
    print(f"[continuous teacher-forced {prec} slots={slots}] {checked} (row, step) logits, max |d| {worst:.2e}")
    assert checked == sum(L - 1 for L in LENGTHS)


@pytest.mark.parametrize("slots", [3, 6, 12])
def test_teacher_forced_logits_mini_width_bf16(slots):
    """Mini-v1 widths, 2 layers, bf16, slots of mixed ages: 12 slots = the producer-statistics LayerNorm / fused-node MFMA step of 9..32
    utterances; 3 and 6 slots = the row-per-wave GEMV step (fused LN1 + QKV + attention node up to 3 utterances, 8-utterance register groups
    above 4), which the 128-wide pool above does not reach."""
    spec = DO.DecoderSpec(num_hidden_layers=2, max_position_embeddings=512)
    sd = DO.make_decoder_weights(spec, seed=47)
    n_req, N, P = 14, 21, 6
    lengths = [12, 18, 14, 20, 13, 17, 19, 12, 16, 18, 15, 20, 13, 17]
    g = torch.Generator().manual_seed(12)
    enc = torch.randn(n_req, N, spec.hidden_size, generator=g)
    prompt = torch.randn(n_req, P, spec.hidden_size, generator=g) * 0.5
    enc_mask, prompt_mask = C.ragged_masks(n_req, N, P, enc_step=2)
    enc = enc * enc_mask[..., None]
    orc = DO.DecoderOracle(spec, sd, precision="bf16")
    refs = []
    with torch.no_grad():
        for i, L in enumerate(lengths):
            sl = slice(i, i + 1)
            refs.append(DO.sample_loop(orc, enc[sl], enc_mask[sl], prompt[sl], prompt_mask[sl], DO.GenParams(max_length=L, min_new_tokens=L - 1),
                                       keep_logits=True))
    eng = make_engine(spec, sd, torch.bfloat16, max_batch=slots, max_ctx=64, max_enc=N, max_prompt=P + 1)
    eng.set_gen_params(max_length=20, min_new_tokens=19)
    worst, checked = _teacher_forced_session(eng, slots, N, P, (enc, enc_mask, prompt, prompt_mask), refs, lengths, 2e-2, spec.num_codebooks)
    eng.close()
    print(f"[continuous teacher-forced bf16 Mini width, {slots} slots] {checked} (row, step) logits, max |d| {worst:.2e}")
    assert checked == sum(L - 1 for L in lengths)


@pytest.mark.parametrize("do_sample", [False, True])
@pytest.mark.parametrize("slots", [3, 12])
def test_bystanders_are_untouched_by_an_admission(slots, do_sample):
    """The same schedule twice, once with an extra request admitted into an idle slot midway: ids and last logits of every other slot are
    identical. With do_sample the run without the admission is also repeated: same seed, same schedule, same ids."""
    pool = _pool()
    spec, sd = pool[0], pool[1]
    K, V = spec.num_codebooks, spec.vocab_size
    stay = [7, 9] if slots == 3 else [7, 9, 19, 18, 8, 17, 16, 6, 15, 14]  # long requests in slots 0 .. len - 1; the last slots stay idle

    def run(extra):
        eng = make_engine(spec, sd, torch.float32, max_batch=slots)
        eng.set_gen_params(max_length=20, min_new_tokens=19, do_sample=do_sample, temperature=0.9, top_k=50, top_p=0.95, seed=7)
        eng.begin_session(slots, N_ENC, N_PROMPT)
        for s, i in enumerate(stay):
            _admit(eng, s, pool, i, max_length=20)
        eng.decode_steps(4)
        if extra:
            _admit(eng, slots - 1, pool, 0)
        eng.decode_steps(3)
        eng.decode_steps(5)
        cur, live = eng.row_state()
        ids = [eng.row_ids(s, cur[s]).cpu() for s in range(len(stay))]
        lg = eng.logits().cpu().view(slots, K, V)[: len(stay)].clone()
        extra_cols = cur[slots - 1]
        eng.close()
        return cur[: len(stay)], live[: len(stay)], ids, lg, extra_cols

    cur_a, live_a, ids_a, lg_a, idle_cols = run(False)
    cur_b, live_b, ids_b, lg_b, extra_cols = run(True)
    assert cur_a == cur_b == [14] * len(stay) and all(live_a) and all(live_b)  # BOS + the admission's token + 12 steps
    assert idle_cols == 1 and extra_cols == 10  # the idle slot never moved; the admitted one holds BOS + its first token + 8 steps
    for a, b in zip(ids_a, ids_b):
        assert torch.equal(a, b)
    assert torch.equal(lg_a, lg_b)
    if do_sample:
        _, _, ids_c, lg_c, _ = run(False)
        for a, c in zip(ids_a, ids_c):
            assert torch.equal(a, c)
        assert torch.equal(lg_a, lg_c)


def _eos_weights(spec):
    """tests/test_lm_gpu.py::test_early_stop_when_all_rows_hit_eos: every codebook emits EOS as soon as the gate lets it."""
    sd = DO.make_decoder_weights(spec, seed=3)
    boost = torch.zeros(spec.hidden_size)
    for k in range(spec.num_codebooks):
        w = sd[f"lm_heads.{k}.weight"]
        eos_row = w[spec.eos_token_id].clone()
        w.zero_()
        w[spec.eos_token_id] = eos_row
        boost += eos_row
    sd["model.decoder.layer_norm.bias"] = sd["model.decoder.layer_norm.bias"] + 40.0 * boost
    return sd


@pytest.mark.parametrize("slots", [3, 12])
def test_eos_ends_each_row_on_its_own_clock(slots):
    spec = DO.TINY
    K = spec.num_codebooks
    sd = _eos_weights(spec)
    g = torch.Generator().manual_seed(0)
    enc = torch.randn(3, 5, spec.hidden_size, generator=g)
    gp = DO.GenParams(max_length=64, min_new_tokens=2)
    orc = DO.DecoderOracle(spec, sd)
    refs = [DO.sample_loop(orc, enc[i:i + 1], None, None, None, gp) for i in range(3)]
    end = 1 + 2 + K  # BOS + min_new + one EOS per codebook, staggered by the gate
    assert all(r.sequences.shape[1] == end for r in refs)
    eng = make_engine(spec, sd, torch.float32, max_batch=slots)
    eng.set_gen_params(max_length=64, min_new_tokens=2)
    eng.begin_session(slots, 5, 0)
    admit_at = {0: 0, 3: 1, 7: 2}  # step -> request (= slot)
    admitted = {}
    snap = {}
    for step in range(32):
        if step in admit_at:
            i = admit_at[step]
            eng.admit_row(i, enc[i], None, None, None)
            admitted[i] = step
        eng.decode_steps(1)
        cur, live = eng.row_state()
        for i, s0 in admitted.items():
            cols = min(2 + (step - s0) + 1, end)  # BOS, the admission's token, one per step since
            assert cur[i] == cols, (step, i, cur[i], cols)
            assert live[i] == (cols < end), (step, i)
            if cols == end and i not in snap:
                snap[i] = eng.row_ids(i, end + 4).cpu()  # with the 4 columns past the end as they are at the first poll after it
        for s in range(slots):
            if s not in admitted:
                assert cur[s] == 1 and not live[s]
    assert sorted(snap) == [0, 1, 2]
    for i in range(3):
        now = eng.row_ids(i, end + 4).cpu()
        assert torch.equal(now[:, :end], refs[i].sequences), i
        assert torch.equal(now, snap[i]), i  # nothing was written past the row's end in the steps that followed
    eng.close()


LONG_INPUT_SEED, LONG_LENGTH = 1139, 200  # scanned on the oracle with the weights of cases.batch_case: margin 2.4e-4


def test_context_growth_across_fetch_buckets_while_short_requests_cycle():
    """Slot 0 runs one request of 200 columns (context 5 .. 204 = the arena end, four 64-position fetch buckets) while the 20 short requests
    cycle through the other two slots; afterwards the bound falls back and two more short requests run at the small bucket."""
    pool = _pool()
    spec, sd, penc, penc_mask, pprompt, pprompt_mask, shorts = pool
    g = torch.Generator().manual_seed(LONG_INPUT_SEED)
    enc = torch.randn(1, N_ENC, spec.hidden_size, generator=g)
    prompt = torch.randn(1, N_PROMPT, spec.hidden_size, generator=g) * 0.5
    L = LONG_LENGTH
    with torch.no_grad():
        ref = DO.sample_loop(DO.DecoderOracle(spec, sd), enc, None, prompt, None, DO.GenParams(max_length=L, min_new_tokens=L - 1))
    assert ref.min_margin >= C.MARGIN, ref.min_margin
    ok = list(range(20))
    for i in ok:
        assert shorts[i].min_margin >= C.MARGIN, (i, shorts[i].min_margin)
    eng = make_engine(spec, sd, torch.float32, max_batch=3, max_ctx=N_PROMPT + L, max_enc=16, max_prompt=N_PROMPT + 1)
    eng.set_gen_params(max_length=L, min_new_tokens=L - 1)
    eng.begin_session(3, N_ENC, N_PROMPT)
    eng.admit_row(0, enc[0], None, prompt[0], None, max_length=L)
    queue = ok + ok[:2]
    tail = len(queue) - 2
    in_slot, got, long_ids = [None, None], [], None
    polls = 0
    while queue or any(r is not None for r in in_slot) or long_ids is None:
        for s in (0, 1):
            if in_slot[s] is None and queue and (len(queue) > 2 or long_ids is not None):  # the last two wait for the long request to retire
                in_slot[s] = queue.pop(0)
                i = in_slot[s]
                eng.admit_row(1 + s, penc[i], penc_mask[i], pprompt[i], pprompt_mask[i], max_length=LENGTHS[i])
        eng.decode_steps(7)
        cur, live = eng.row_state()
        if long_ids is None and not live[0]:
            long_ids = eng.row_ids(0, cur[0]).cpu()
            eng.retire_row(0)
        for s in (0, 1):
            if in_slot[s] is not None and not live[1 + s]:
                got.append((in_slot[s], eng.row_ids(1 + s, cur[1 + s]).cpu()))
                eng.retire_row(1 + s)
                in_slot[s] = None
        polls += 1
        assert polls < 400
    eng.close()
    assert long_ids.shape == ref.sequences.shape and torch.equal(long_ids, ref.sequences)
    assert len(got) == tail + 2
    for i, ids in got:
        assert torch.equal(ids, shorts[i].sequences), i


def test_refusals_are_values():
    pool = _pool()
    spec, sd, enc, enc_mask, prompt, prompt_mask, _ = pool
    eng = make_engine(spec, sd, torch.float32, max_batch=3)
    eng.set_gen_params(max_length=20, min_new_tokens=19)
    with pytest.raises(ValueError, match="no continuous session"):
        eng.B, eng.P, eng.session_N = 3, N_PROMPT, N_ENC
        _admit(eng, 0, pool, 0)
    with pytest.raises(ValueError, match="no continuous session"):
        eng.row_state()
    with pytest.raises(ValueError, match="no continuous session"):
        eng.retire_row(0)
    with pytest.raises(ValueError, match="max_batch"):
        eng.begin_session(4, N_ENC, N_PROMPT)
    with pytest.raises(ValueError, match="max_enc"):
        eng.begin_session(3, 33, N_PROMPT)
    with pytest.raises(ValueError, match="prompt width"):
        eng.begin_session(3, N_ENC, 16)
    eng.begin_session(3, N_ENC, N_PROMPT)
    _admit(eng, 1, pool, 0)
    with pytest.raises(ValueError, match="still holds a request"):
        _admit(eng, 1, pool, 1)
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="outside the session"):
            _admit(eng, bad, pool, 1)
        with pytest.raises(ValueError, match="outside the session"):
            eng.retire_row(bad)
    with pytest.raises(ValueError, match="exceeds the session's"):
        _admit(eng, 0, pool, 1, max_length=21)
    with pytest.raises(ValueError, match="max_length must be"):
        _admit(eng, 0, pool, 1, max_length=1)
    eng.set_audio_prefix(torch.randint(0, 1024, (1, spec.num_codebooks, 3)))
    with pytest.raises(NotImplementedError, match="voice prompt"):
        _admit(eng, 0, pool, 1)
    with pytest.raises(NotImplementedError, match="voice prompt"):
        eng.begin_session(3, N_ENC, N_PROMPT)
    eng.set_audio_prefix(None)
    # the refusals left the session intact: the admitted request still runs to its end, and a static batch ends the session
    eng.decode_steps(12)
    cur, live = eng.row_state()
    assert cur == [1, 11, 1] and live == [False, False, False]
    assert torch.equal(eng.row_ids(1, 11).cpu(), pool[6][0].sequences)
    eng.prefill(enc[:3], enc_mask[:3], prompt[:3], prompt_mask[:3])
    with pytest.raises(ValueError, match="no continuous session"):
        eng.row_state()
    eng.close()
    # the e4m3 KV cache is refused in a session
    mspec = DO.DecoderSpec(num_hidden_layers=1, max_position_embeddings=128)
    e8 = make_engine(mspec, DO.make_decoder_weights(mspec, seed=1), torch.bfloat16, max_batch=12, max_ctx=64, kv_fp8=True)
    e8.set_gen_params(max_length=20)
    with pytest.raises(NotImplementedError, match="kv_fp8"):
        e8.begin_session(12, N_ENC, N_PROMPT)
    e8.close()


# ---- end to end: ContinuousBatcher on the tiny model (T5 -> session -> un-delay -> ragged codec) ------------------------------------------
E2E_SEEDS = (2, 313)  # (model seed, input seed): scanned on the oracle over _e2e_requests, min margin 2.1e-4
E2E_N, E2E_P, E2E_NEW = 9, 5, [30, 12, 22, 17, 26, 10, 19, 24]


def _e2e_requests(input_seed):
    g = torch.Generator().manual_seed(input_seed)
    reqs = []
    for i, n in enumerate(E2E_NEW):
        reqs.append(dict(input_ids=torch.randint(3, 128, (E2E_N - i % 3,), generator=g), prompt_input_ids=torch.randint(3, 128, (E2E_P - i % 2,), generator=g),
                         max_new_tokens=n))
    return reqs


def _e2e_reference(m, spec, sd, dsd, req, device):
    """tests/test_generate_gpu.py::_oracle_pipeline on ONE request padded (masked) to the session widths, with its own max_length."""
    from oracle import dac_oracle as DA

    ids, mask = torch.zeros(1, E2E_N, dtype=torch.long), torch.zeros(1, E2E_N, dtype=torch.long)
    pids, pmask = torch.zeros(1, E2E_P, dtype=torch.long), torch.zeros(1, E2E_P, dtype=torch.long)
    d, p = req["input_ids"], req["prompt_input_ids"]
    ids[0, : d.shape[0]], mask[0, : d.shape[0]] = d, 1
    pids[0, : p.shape[0]], pmask[0, : p.shape[0]] = p, 1
    with torch.no_grad():
        if device == "cpu":
            enc = m._encode_description_eager(ids, mask).float()
        else:
            enc = m._encode_description(ids.to(device), mask.to(device)).float().cpu()
        prompt = m.embed_prompts(pids.to(device)).float().cpu()
        L = req["max_new_tokens"] + 1
        tr = DO.sample_loop(DO.DecoderOracle(spec, sd), enc, mask, prompt, pmask, DO.GenParams(max_length=L, min_new_tokens=L - 1))
    c = DO.valid_frames(DO.undelay(tr.sequences, spec, L)[0])
    return tr, DA.DacOracle(DA.DAC_TINY, dsd).decode(c[None])[0, 0] if c.shape[1] else torch.zeros(1)


def test_continuous_batcher_end_to_end_against_the_oracle_pipeline():
    """8 requests through 2 slots: each waveform within RMS 1e-4 of the oracle pipeline on that request alone (the bar of
    tests/test_generate_gpu.py), lengths by each request's own max_new_tokens, run() in submission order, iteration in finishing order."""
    import parler_tts_amd as P
    from oracle import dac_oracle as DA

    ms, isd = E2E_SEEDS
    m, spec, sd, dsd = C.tiny_model(seed=ms)
    m = m.to("cuda")
    reqs = _e2e_requests(isd)
    refs = [_e2e_reference(m, spec, sd, dsd, r, "cuda") for r in reqs]
    for i, (tr, _) in enumerate(refs):
        assert tr.min_margin >= C.MARGIN, (i, tr.min_margin)
    cb = P.ContinuousBatcher(m, slots=2, max_description_tokens=E2E_N, max_prompt_tokens=E2E_P, poll_steps=5, do_sample=False, max_new_tokens=30, min_new_tokens=30)
    out = cb.run(reqs)
    assert len(out) == len(reqs)
    hop = DA.DAC_TINY.hop_length
    for i, ((wav, n), (tr, ref)) in enumerate(zip(out, refs)):
        cols = E2E_NEW[i] + 1
        assert n == wav.shape[0] == ref.shape[0] == hop * (cols - 9 if cols >= 17 else cols - 1), (i, n, ref.shape)
        err = float((wav.cpu() - ref).pow(2).mean().sqrt())
        assert err <= 1e-4, (i, err)
    # the same session keeps serving: iteration hands requests out as they finish (the short one first), then a static generate() ends the session
    t = [cb.submit(**reqs[0]), cb.submit(**reqs[1])]
    order = [(tk, n) for tk, w, n in cb]
    assert [tk for tk, _ in order] == [t[1], t[0]] and [n for _, n in order] == [out[1][1], out[0][1]]
    g = m.generate(input_ids=reqs[0]["input_ids"][None].cuda(), prompt_input_ids=reqs[0]["prompt_input_ids"][None].cuda(), do_sample=False,
                   max_new_tokens=30, min_new_tokens=30)
    assert g.shape == (1, out[0][1])  # request 0 is not padded (full widths): the static path gives the same utterance
    assert float((g[0].cpu() - refs[0][1]).pow(2).mean().sqrt()) <= 1e-4
