"""MI355X: streaming out of a continuous session. (1) ``ptts_dac_stream_open / _reset / _decode`` alone against ``ptts_dac_compact_codes`` +
``ptts_dac_decode_ragged`` on the same engine and against a host model of the stream table (tests/stream_model.py); (2-5) the streaming
``ContinuousBatcher`` end to end against the non-streaming one, the oracle pipeline, and the decoder's own state."""
import numpy as np
import pytest
import torch

from oracle import dac_oracle as DA
from oracle import decoder_oracle as DO

from helpers import log_parity
from stream_model import StreamTableModel

LOG = "continuous_streaming_gpu.txt"
_DACS = {}


def _dac(spec_name, dtype, max_batch, max_frames):
    """One engine per (stack, dtype) for the whole module: loading the 44.1 kHz weights dominates a case otherwise."""
    from parler_tts_amd.engine import DacEngine
    from parler_tts_amd.synthetic import random_dac_state_dict

    key = (spec_name, dtype)
    d = _DACS.get(key)
    if d is None or d.max_batch < max_batch or d.max_frames < max_frames:
        if spec_name == "tiny":
            spec, dsd = DA.DAC_TINY, DA.make_dac_weights(DA.DAC_TINY, seed=4321)
            d = DacEngine(num_codebooks=spec.num_codebooks, codebook_size=spec.codebook_size, codebook_dim=spec.codebook_dim, latent_dim=spec.latent_dim,
                          decoder_dim=spec.decoder_dim, rates=spec.decoder_rates, max_batch=max_batch, max_frames=max_frames)
        else:
            dsd = random_dac_state_dict(seed=4321)
            d = DacEngine(max_batch=max_batch, max_frames=max_frames, compute_dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
        d.load_state_dict({k: v.cuda() for k, v in dsd.items()})
        _DACS[key] = d
    return d


def _utterances(S, T, halo, seed):
    """Plain codes [S, K, T] with special ids planted per slot (by slot % 5): scattered frames; runs longer than the halo; frame 0; the last
    frame; nowhere. A single slot gets all of them. Frames beyond a slot's own length hold a special id in codebook 0 (the reference drops
    them, the stream never absorbs them). Returns (codes, lengths)."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 1024, (S, 9, T), generator=g)
    lens = [T - (37 * s) % 120 for s in range(S)]

    def plant(s, f):
        codes[s, int(torch.randint(0, 9, (1,), generator=g)), f] = int(torch.randint(1024, 1088, (1,), generator=g))

    for s in range(S):
        L = lens[s]
        kinds = {0: ("scattered",), 1: ("runs",), 2: ("first", "scattered"), 3: ("last", "scattered"), 4: ()}[s % 5] if S > 1 else ("scattered", "runs", "first", "last")
        if "scattered" in kinds:
            for f in torch.randperm(L, generator=g)[: L // 9].tolist():
                plant(s, f)
        if "runs" in kinds:
            for f0 in (40, 170):
                for f in range(f0, min(L, f0 + halo + 5)):
                    plant(s, f)
        if "first" in kinds:
            plant(s, 0)
        if "last" in kinds:
            plant(s, L - 1)
        codes[s, 0, L:] = 1024
    return codes, lens


def _layout(codes, delayed, seed):
    """plain: the codes themselves (col0 = 0, delay = 0). delayed: codebook k shifted right by 1 + k columns as in the engine's raw id buffer
    (col0 = 1, delay = 1), the triangles filled with OTHER valid codes: a read there would change the waveform instead of dropping a frame."""
    if not delayed:
        return codes.contiguous(), 0, 0
    S, K, T = codes.shape
    ids = torch.randint(0, 1024, (S, K, T + K + 1), generator=torch.Generator().manual_seed(seed + 1))
    for k in range(K):
        ids[:, k, 1 + k: 1 + k + T] = codes[:, k]
    return ids.contiguous(), 1, 1


def _increments(s, seed):
    """Uneven steps of `complete`: some below min_emit, some of 150 and more (a window then spans two 128-frame tiles and a ragged last one)."""
    base = [7, 150, 3, 61, 19, 180, 11, 33, 5, 95]
    r = (s * 3 + seed) % len(base)
    return base[r:] + base[:r]


def _stream_all(dac, ids, col0, delay, lens, halo, min_emit, model, seed, skip_rule=True):
    """Drives every slot to its end; returns per slot the list of emitted chunks. Every pass is compared with the host model's (emit, kept)."""
    S = len(lens)
    hop = dac.hop
    complete, done, chunks = [0] * S, [False] * S, [[] for _ in range(S)]
    incs = [_increments(s, seed) for s in range(S)]
    frames_of = lambda s, f0, f1: np.stack([ids[s, k, col0 + f0 + k * delay: col0 + f1 + k * delay].numpy() for k in range(ids.shape[1])])
    dev_ids = ids.cuda()
    call = 0
    while not all(done):
        rows = []
        for s in range(S):
            if done[s] or (skip_rule and S > 1 and (call + s) % 4 == 3):  # slots that are not listed stay untouched
                continue
            nxt = complete[s] + incs[s][call % len(incs[s])]
            if complete[s] == lens[s]:
                rows.append((s, lens[s], 1, 0))
                done[s] = True
            else:
                complete[s] = min(nxt, lens[s])
                rows.append((s, complete[s], 0, min_emit))
        call += 1
        if not rows:
            continue
        wave, out = dac.stream_decode(dev_ids, None, rows, halo, col0=col0, delay=delay)
        want = model.decode(frames_of, rows, halo)
        out = out.cpu().tolist()
        assert [tuple(o) for o in out] == [(e, k) for e, k, _, _ in want], (call, rows, out, [(e, k) for e, k, _, _ in want])
        wave = wave.cpu()
        for r, (s, _, final, _) in enumerate(rows):
            e = out[r][0]
            if wave.shape[1] > e * hop:
                assert float(wave[r, e * hop:].abs().max()) == 0.0  # the tail of every row is zero
            if e:
                chunks[s].append(wave[r, : e * hop].clone())
    return chunks


def _reference(dac, codes):
    cc, fr = dac.compact_codes(codes.cuda())
    wav = dac.decode_ragged(cc, fr).cpu()
    return wav, fr.cpu().tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("delayed", [False, True], ids=["plain", "delayed"])
@pytest.mark.parametrize("S", [1, 5, 12])
@pytest.mark.parametrize("spec_name,dtype", [("tiny", "f32"), ("44k", "f32"), ("44k", "bf16")])
def test_stream_decode_concatenates_to_the_filtered_ragged_decode(spec_name, dtype, S, delayed):
    """Per slot, the chunks of successive ``ptts_dac_stream_decode`` passes concatenate to ``ptts_dac_compact_codes`` +
    ``ptts_dac_decode_ragged`` of the whole utterance on the SAME engine: max |d| <= 1e-5, the bar of
    tests/test_streamer_vs_reference.py::test_dac_decode_chunk_equals_full_decode_window. The (emit, kept) pairs equal the host model."""
    from parler_tts_amd.streamer import receptive_halo_frames

    T = 330
    dac = _dac(spec_name, dtype, 12, T)
    halo = receptive_halo_frames(DA.DAC_TINY.decoder_rates if spec_name == "tiny" else (8, 8, 4, 2))
    codes, lens = _utterances(S, T, halo, seed=10 + S)
    ids, col0, delay = _layout(codes, delayed, seed=S)
    ref, ref_frames = _reference(dac, codes)
    dac.stream_open(S, T)
    model = StreamTableModel(S, 9, 1024)
    chunks = _stream_all(dac, ids, col0, delay, lens, halo, 20, model, seed=S)
    worst, exact = 0.0, True
    for s in range(S):
        got = torch.cat(chunks[s]) if chunks[s] else torch.zeros(0)
        n = ref_frames[s] * dac.hop
        assert got.shape[0] == n and model.kept[s].shape[1] == ref_frames[s], (s, got.shape, n)
        if S > 1 and s % 5 == 4:
            assert ref_frames[s] == lens[s]  # the slot without a special id keeps every frame
        d = float((got - ref[s, 0, :n]).abs().max()) if n else 0.0
        worst, exact = max(worst, d), exact and torch.equal(got, ref[s, 0, :n])
        assert len(chunks[s]) >= 2  # it really came in pieces
    log_parity(f"stream_decode vs compact+ragged [{spec_name} {dtype} S={S} {'delayed' if delayed else 'plain'}]: max|d| {worst:.3e}, "
               f"bit-identical {exact}, kept {ref_frames} of {lens}", LOG)
    assert worst <= 1e-5, worst


@pytest.mark.gpu
def test_stream_reset_of_one_slot_while_the_others_continue():
    from parler_tts_amd.streamer import receptive_halo_frames

    T, S = 200, 3
    dac = _dac("tiny", "f32", 12, 330)
    halo = receptive_halo_frames(DA.DAC_TINY.decoder_rates)
    a, lens_a = _utterances(S, T, halo, seed=71)
    b, lens_b = _utterances(S, T, halo, seed=72)
    ref_a, fr_a = _reference(dac, a)
    ref_b, fr_b = _reference(dac, b)
    dac.stream_open(S, T)
    hop = dac.hop
    got = {("a", s): [] for s in range(S)}
    got["b", 1] = []

    def step(codes, rows, tags):
        wave, out = dac.stream_decode(codes.cuda(), None, rows, halo)
        for r, ((s, _, _, _), tag) in enumerate(zip(rows, tags)):
            e = int(out[r, 0])
            if e:
                got[tag, s].append(wave[r, : e * hop].cpu())

    step(a, [(0, 90, 0, 10), (1, 120, 0, 10), (2, 60, 0, 10)], "aaa")
    step(a, [(1, lens_a[1], 1, 0)], "a")  # slot 1 ends ...
    dac.stream_reset(1)                   # ... and a new request enters it
    mixed = a.clone()
    mixed[1] = b[1]
    step(mixed, [(0, 150, 0, 10), (1, 70, 0, 10), (2, 110, 0, 10)], "aba")
    step(mixed, [(0, lens_a[0], 1, 0), (1, lens_b[1], 1, 0), (2, lens_a[2], 1, 0)], "aba")
    for (tag, s), parts in got.items():
        ref, fr = (ref_a, fr_a) if tag == "a" else (ref_b, fr_b)
        w = torch.cat(parts)
        assert w.shape[0] == fr[s] * hop
        assert float((w - ref[s, 0, : fr[s] * hop]).abs().max()) <= 1e-5
    with pytest.raises(ValueError, match="decreases"):  # without a reset the slot still counts the old request
        dac.stream_decode(a.cuda(), None, [(0, 10, 0, 10)], halo)


@pytest.mark.gpu
def test_stream_decode_refusals():
    dac = _dac("tiny", "f32", 12, 330)
    halo = 26
    codes = torch.randint(0, 1024, (4, 9, 400)).cuda()
    dac.stream_open(4, 400)
    with pytest.raises(ValueError, match="out of range"):
        dac.stream_decode(codes, None, [(4, 10, 0, 5)], halo)
    with pytest.raises(ValueError, match="listed twice"):
        dac.stream_decode(codes, None, [(1, 10, 0, 5), (1, 20, 0, 5)], halo)
    with pytest.raises(ValueError, match="beyond the table"):
        dac.stream_decode(codes, None, [(0, 401, 0, 5)], halo)
    with pytest.raises(ValueError, match="beyond ids_ld"):
        dac.stream_decode(codes[:, :, :100].contiguous(), None, [(0, 101, 0, 5)], halo)
    with pytest.raises(ValueError, match="rows for 4 slots"):
        dac.stream_decode(codes, None, [(s % 4, 10, 0, 5) for s in range(5)], halo)
    with pytest.raises(ValueError, match="max_frames"):  # PTTS_E_CAPACITY: a window of 26 + 400 kept frames on an engine of 330
        dac.stream_decode(codes, None, [(0, 400, 1, 0)], halo)
    with pytest.raises(ValueError, match="out of range"):
        dac.stream_reset(7)
    with pytest.raises(ValueError, match="max_batch"):
        dac.stream_open(13, 100)
    # a refused pass counts nothing: the same slots still start from 0
    wave, out = dac.stream_decode(codes, None, [(0, 100, 0, 5), (1, 30, 0, 5)], halo)
    assert out.cpu().tolist() == [[74, 100], [0, 30]]
    with pytest.raises(ValueError, match="decreases"):
        dac.stream_decode(codes, None, [(0, 99, 0, 5)], halo)


# ---- end to end: the streaming ContinuousBatcher on the tiny model -----------------------------------------------------------------------
# The tiny codec's halo is 26 frames: requests of 60..200 new tokens, so that second and later chunks exist.
E2E_N, E2E_P = 9, 5
E2E_MODEL_SEED = 2
# (input seed, max_new_tokens): scanned on the oracle (python tools/scan_margin_seeds.py stream_e2e), margins behind the list
E2E_SCANNED = [(646, 200), (503, 60), (549, 120), (550, 90), (590, 160), (594, 75)]  # 1.7e-4, 3.0e-4, 1.8e-4, 1.8e-4, 1.9e-4, 3.2e-4
E2E_EXTRA = [(900 + i, n) for i, n in enumerate([64, 150, 88, 70, 131, 99, 180, 61])]  # compared with run() only: no margin needed
CHUNK, FIRST = 16, 8


def e2e_request(seed, n):
    g = torch.Generator().manual_seed(seed)
    return dict(input_ids=torch.randint(3, 128, (E2E_N - seed % 3,), generator=g), prompt_input_ids=torch.randint(3, 128, (E2E_P - seed % 2,), generator=g),
                max_new_tokens=n)


def e2e_oracle(m, spec, sd, dsd, req, device):
    """tests/test_generate_gpu.py::_oracle_pipeline on ONE request padded (masked) to the session widths, with its own max_length."""
    ids, mask = torch.zeros(1, E2E_N, dtype=torch.long), torch.zeros(1, E2E_N, dtype=torch.long)
    pids, pmask = torch.zeros(1, E2E_P, dtype=torch.long), torch.zeros(1, E2E_P, dtype=torch.long)
    d, p = req["input_ids"], req["prompt_input_ids"]
    ids[0, : d.shape[0]], mask[0, : d.shape[0]] = d, 1
    pids[0, : p.shape[0]], pmask[0, : p.shape[0]] = p, 1
    with torch.no_grad():
        enc = m._encode_description_eager(ids, mask).float() if device == "cpu" else m._encode_description(ids.to(device), mask.to(device)).float().cpu()
        prompt = m.embed_prompts(pids.to(device)).float().cpu()
        L = req["max_new_tokens"] + 1
        tr = DO.sample_loop(DO.DecoderOracle(spec, sd), enc, mask, prompt, pmask, DO.GenParams(max_length=L, min_new_tokens=L - 1))
    c = DO.valid_frames(DO.undelay(tr.sequences, spec, L)[0])
    return tr, DA.DacOracle(DA.DAC_TINY, dsd).decode(c[None])[0, 0] if c.shape[1] else torch.zeros(1)


def drops_model(seed=3):
    """cases.tiny_model with only the EOS row of every head zeroed: the 63 padding-id rows stay random, random heads emit them all the time,
    and every frame that holds one is dropped - the kept frames of a request are scattered runs."""
    import cases as C

    m, spec, sd, dsd = C.tiny_model(seed=seed)
    sd = DO.make_decoder_weights(spec, seed=1234 + seed)
    for k in range(9):
        sd[f"lm_heads.{k}.weight"][1024] = 0.0
    m.decoder.load_state_dict(sd, strict=False)
    return m, spec, sd, dsd


def _stream_run(cb, reqs):
    tickets = [cb.submit(**r) for r in reqs]
    by, closed, order = {t: [] for t in tickets}, set(), []
    for t, c, last in cb.chunks():
        assert t not in closed and c.dim() == 1 and c.dtype == torch.float32
        by[t].append(c)
        order.append(t)
        if last:
            closed.add(t)
    assert closed == set(tickets)
    return [torch.cat(by[t]) for t in tickets], [len(by[t]) for t in tickets], order


def _compare_with_run(m, reqs, slots, tag, **kw):
    """Streaming against the non-streaming run() of the same model: equal lengths, max |d| <= 1e-5."""
    import parler_tts_amd as P

    base = dict(slots=slots, max_description_tokens=E2E_N, max_prompt_tokens=E2E_P, poll_steps=16, **kw)
    ref = P.ContinuousBatcher(m, **base).run(reqs)
    cb = P.ContinuousBatcher(m, stream_chunk_frames=CHUNK, stream_first_chunk_frames=FIRST, **base)
    got, pieces, order = _stream_run(cb, reqs)
    worst = 0.0
    for i, (w, (wav, n)) in enumerate(zip(got, ref)):
        assert w.shape[0] == n == wav.shape[0], (i, w.shape, n)
        worst = max(worst, float((w - wav).abs().max()))
    log_parity(f"streaming vs run() [{tag}, {slots} slots]: {len(reqs)} requests, pieces {pieces}, {cb.codec_passes} codec passes, "
               f"{cb.codec_rows / max(cb.codec_passes, 1):.2f} rows per pass, {cb.whole_requests} ended below 2K - 1 columns, max|d| {worst:.3e}", LOG)
    assert worst <= 1e-5, worst
    return ref, got, pieces, order, cb


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [2, 12])
def test_streaming_batcher_end_to_end_clean_model(slots):
    """Chunks concatenate to run()'s waveform (max |d| <= 1e-5) and, per request, to the oracle pipeline on that request alone (RMS <= 1e-4,
    the bar of tests/test_generate_gpu.py; every such request's oracle top-2 margin is asserted)."""
    import cases as C

    m, spec, sd, dsd = C.tiny_model(seed=E2E_MODEL_SEED)
    m = m.to("cuda")
    scanned = [e2e_request(s, n) for s, n in E2E_SCANNED]
    reqs = scanned + ([e2e_request(s, n) for s, n in E2E_EXTRA] if slots == 12 else [])
    refs = [e2e_oracle(m, spec, sd, dsd, r, "cuda") for r in scanned]
    for i, (tr, _) in enumerate(refs):
        assert tr.min_margin >= C.MARGIN, (i, tr.min_margin)
    ref, got, pieces, order, cb = _compare_with_run(m, reqs, slots, "clean", do_sample=False, max_new_tokens=200, min_new_tokens=200)
    hop = DA.DAC_TINY.hop_length
    for i, ((tr, wav), w) in enumerate(zip(refs, got)):
        assert w.shape[0] == wav.shape[0] == hop * (E2E_SCANNED[i][1] + 1 - 9)
        err = float((w.cpu() - wav).pow(2).mean().sqrt())
        assert err <= 1e-4, (i, err)
    assert all(p >= 2 for p in pieces) and max(pieces) >= 5  # every request came in pieces
    assert len(set(order[:8])) > 1  # chunks of different tickets interleave


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [2, 12])
def test_streaming_batcher_end_to_end_scattered_drops(slots):
    m, spec, sd, dsd = drops_model()
    m = m.to("cuda")
    reqs = [e2e_request(s, n) for s, n in (E2E_SCANNED + E2E_EXTRA if slots == 12 else E2E_SCANNED)]
    ref, got, pieces, order, cb = _compare_with_run(m, reqs, slots, "scattered drops", do_sample=False, max_new_tokens=200, min_new_tokens=200)
    hop = DA.DAC_TINY.hop_length
    kept, frames = sum(n // hop for _, n in ref), sum(r["max_new_tokens"] + 1 - 9 for r in reqs)
    log_parity(f"    kept share {kept / frames:.3f} ({kept} of {frames} frames)", LOG)
    assert 0.2 <= kept / frames <= 0.9, kept / frames  # a condition on the input: every chunk window holds dropped frames
    assert max(pieces) >= 3


EOS_SHIFT = 0.02  # scanned on the CPU oracle: the 16 requests below end at 13..14 and at 22..23 columns (2K - 1 = 17)


def eos_model(seed=3):
    """An EOS-terminated model whose requests end on BOTH sides of 2K - 1 columns. Scaling the EOS row of random heads (``eos_gain``, as
    cases.GEN_EOS_SEEDS) does not do: all nine codebooks have to emit EOS one after the other, and on this model not one of 16 requests got
    there within 100 columns at gains 6..40 (CPU oracle). Here every head keeps ONE row, the same EOS row, so a codebook emits EOS as soon as
    the gate lets it and row . hidden > 0; a small shift of the final layer norm's bias along that row puts the sign change near the
    min_new_tokens boundary, where the requests' own hidden states decide."""
    import cases as C

    m, spec, sd, dsd = C.tiny_model(seed=seed, eos_gain=1.0)
    row = sd["lm_heads.0.weight"][1024].clone()
    for k in range(9):
        sd[f"lm_heads.{k}.weight"].zero_()
        sd[f"lm_heads.{k}.weight"][1024] = row
    sd["model.decoder.layer_norm.bias"] = sd["model.decoder.layer_norm.bias"] + EOS_SHIFT * row / row.pow(2).sum()
    m.decoder.load_state_dict(sd, strict=False)
    return m, spec, sd, dsd


@pytest.mark.gpu
def test_streaming_batcher_eos_terminated_requests():
    """Requests that end on EOS, some below 2K - 1 columns (no delay pattern: today's un-delay + filtered decode, one last chunk), some above
    (flushed out of the stream table). Lengths and samples equal the non-streaming run, which needs no margin."""
    m, spec, sd, dsd = eos_model()
    m = m.to("cuda")
    reqs = [e2e_request(700 + i, 100) for i in range(16)]
    ref, got, pieces, order, cb = _compare_with_run(m, reqs, 3, "eos", do_sample=False, max_new_tokens=100, min_new_tokens=3)
    hop = DA.DAC_TINY.hop_length
    assert all(n < hop * (101 - 9) for _, n in ref)  # every request ended on EOS, long before its max_length
    assert 0 < cb.whole_requests < len(reqs), cb.whole_requests  # ... on both sides of 2K - 1 columns


@pytest.mark.gpu
def test_streaming_and_not_streaming_sample_the_same_waveforms():
    """do_sample with a fixed seed: the ids do not depend on the delivery mode (EOS blocked: the admission schedule is the same in both)."""
    import cases as C
    import parler_tts_amd as P

    m, spec, sd, dsd = C.tiny_model(seed=E2E_MODEL_SEED)
    m = m.to("cuda")
    reqs = [e2e_request(s, n) for s, n in E2E_EXTRA]
    base = dict(slots=3, max_description_tokens=E2E_N, max_prompt_tokens=E2E_P, do_sample=True, temperature=0.9, top_k=50, max_new_tokens=180, min_new_tokens=180)
    torch.manual_seed(11)
    ref = P.ContinuousBatcher(m, **base).run(reqs)
    torch.manual_seed(11)
    got, pieces, _ = _stream_run(P.ContinuousBatcher(m, stream_chunk_frames=CHUNK, **base), reqs)
    torch.manual_seed(12)
    other = P.ContinuousBatcher(m, **base).run(reqs)
    for w, (wav, n) in zip(got, ref):
        assert w.shape[0] == n and float((w - wav).abs().max()) <= 1e-5
    assert any(a.shape != b.shape or float((a - b).abs().max()) > 1e-3 for (a, _), (b, _) in zip(ref, other))  # the seed matters: sampling is on


@pytest.mark.gpu
@pytest.mark.parametrize("do_sample", [False, True])
@pytest.mark.parametrize("slots", [3, 12])
def test_stream_passes_only_read_the_decoder(slots, do_sample):
    """The same engine-level schedule with and without ptts_dac_stream_decode passes between the steps (on the engine's raw id buffer, in
    place): ids and last logits of every slot are identical. After tests/test_continuous_batching_gpu.py::test_bystanders_are_untouched_by_an_admission."""
    import cases as C
    from helpers import make_engine

    spec, sd, enc, enc_mask, prompt, prompt_mask, _ = C.batch_case(20)
    K, V, L = spec.num_codebooks, spec.vocab_size, 90
    n_req = min(slots, 10)
    dac = _dac("tiny", "f32", 12, 330)

    def run(stream):
        eng = make_engine(spec, sd, torch.float32, max_batch=slots, max_ctx=128)
        eng.set_gen_params(max_length=L, min_new_tokens=L - 1, do_sample=do_sample, temperature=0.9, top_k=50, top_p=0.95, seed=7)
        eng.begin_session(slots, 9, 4)
        emitted = 0
        if stream:
            dac.stream_open(slots, L)
        for s in range(n_req):
            eng.admit_row(s, enc[s], enc_mask[s], prompt[s], prompt_mask[s], max_length=L)
        for n in (20, 7, 30, 1, 12, 18):
            eng.decode_steps(n)
            if stream:
                cur, live = eng.row_state()
                ptr, ld = eng.ids_buffer()
                rows = [(s, min(cur[s], L) - K, 0 if live[s] else 1, 5) for s in range(n_req)]
                wave, out = dac.stream_decode(ptr, ld, rows, 26, col0=1, delay=1)
                emitted += int(out[:, 0].sum())
        cur, live = eng.row_state()
        ids = [eng.row_ids(s, cur[s]).cpu() for s in range(n_req)]
        lg = eng.logits().cpu().view(slots, K, V)[:n_req].clone()
        eng.close()
        return cur, live, ids, lg, emitted

    cur_a, live_a, ids_a, lg_a, _ = run(False)
    cur_b, live_b, ids_b, lg_b, emitted = run(True)
    assert cur_a == cur_b and live_a == live_b and cur_a[:n_req] == [L] * n_req
    assert emitted > 0  # the passes did decode
    for a, b in zip(ids_a, ids_b):
        assert torch.equal(a, b)
    assert torch.equal(lg_a, lg_b)
