"""MI355X: streaming requests that carry a voice prompt. (1-3) ``ptts_dac_stream_open_voice / _reset_voice / _decode_capped`` alone against
``ptts_dac_compact_codes`` + ``ptts_dac_decode_ragged`` of [prefix ++ generated frames] on the same engine and against the host model of
tests/stream_voice_model.py, pass by pass; (4-5) ``ContinuousBatcher(stream_voice_prompts=)`` end to end against the non-streaming batcher
on the same model. Bars (none is new): streaming chunks against the whole-utterance decode on the same engine max |d| <= 1e-5
(tests/test_continuous_streaming_gpu.py)."""
import numpy as np
import pytest
import torch

from oracle import dac_oracle as DA

from helpers import log_parity
from stream_voice_model import StreamVoiceTableModel
from test_continuous_streaming_gpu import CHUNK, E2E_MODEL_SEED, E2E_N, E2E_P, FIRST, _dac, _reference, _stream_run, drops_model, e2e_request

LOG = "continuous_streaming_voice_gpu.txt"
K, FRAMES, MAX_EMIT = 9, 330, 40


def _halo(spec_name):
    from parler_tts_amd.streamer import receptive_halo_frames

    return receptive_halo_frames(DA.DAC_TINY.decoder_rates if spec_name == "tiny" else (8, 8, 4, 2))


def _prefix_lengths(S, halo):
    """0, 1, halo - 1, halo + max_emit + 3 (the prompt needs more than one capped pass), 260 (the prompt / id-buffer boundary falls inside
    the absorb loop's second 256-frame block); a single slot takes the last."""
    return [0, 1, halo - 1, halo + MAX_EMIT + 3, 260][:S] if S > 1 else [260]


def _voice_utterances(Ts, halo, seed):
    """Per slot the whole utterance [K, FRAMES] = prefix (frames below T) ++ generated frames, with special ids planted at the prompt's first
    frame, as a run longer than the halo that straddles frame T, and scattered. The id buffer is the delayed layout (col0 = delay = 1): the
    cells of every frame f >= T hold the utterance, ALL others - the cells of the frames below T, the K(K-1)/2 cells behind column T among
    them - hold other valid codes, so that a read from the buffer below T changes the waveform instead of dropping a frame."""
    S = len(Ts)
    g = torch.Generator().manual_seed(seed)
    whole = torch.randint(0, 1024, (S, K, FRAMES), generator=g)

    def plant(s, f):
        whole[s, int(torch.randint(0, K, (1,), generator=g)), f] = int(torch.randint(1024, 1088, (1,), generator=g))

    for s, T in enumerate(Ts):
        for f in torch.randperm(FRAMES, generator=g)[: FRAMES // 12].tolist():
            plant(s, f)
        if T > 0:
            plant(s, 0)
            for f in range(max(0, T - halo // 2 - 3), min(FRAMES, T + halo // 2 + 3)):
                plant(s, f)
    ids = torch.randint(0, 1024, (S, K, FRAMES + K + 1), generator=g)
    for s, T in enumerate(Ts):
        for k in range(K):
            ids[s, k, 1 + k + T: 1 + k + FRAMES] = whole[s, k, T:]
    return whole, [whole[s, :, :T].contiguous() for s, T in enumerate(Ts)], ids.contiguous()


def _schedule(s, T, S):
    """Steps of `complete`. The slot with the 260-frame prompt lists 300 frames at once (a prompt that is ready at admission); slot 0 ends
    `final` with more than 2 * max_emit frames ready."""
    if T == 260:
        return [300, 3, 27]
    if s == 0 and S > 1:
        return [7, 61, 19, None]  # None: the request ends here, every remaining frame becomes final in the `final` row itself
    base = [7, 150, 3, 61, 19, 180, 11, 33, 5, 95]
    return base[s:] + base[:s]


def _drive(dac, model, dev_ids, ids, slots, Ts, halo, min_emit, chunks, skip_rule=True):
    """Drives the listed slots to their ends, a final row again and again until the host model says it is flushed. Every pass: the library's
    (emit, kept) pairs equal the host model's, the tail of every row is zero."""
    hop = dac.hop
    complete, done = {s: 0 for s in slots}, {s: False for s in slots}
    frames_of = lambda s, f0, f1: np.stack([ids[s, k, 1 + f0 + k: 1 + f1 + k].numpy() for k in range(K)])
    call, final_passes, listed = 0, {s: 0 for s in slots}, {s: 0 for s in slots}
    while not all(done.values()):
        rows = []
        for s in slots:
            if done[s] or (skip_rule and len(slots) > 1 and (call + s) % 4 == 3):  # slots that are not listed stay untouched
                continue
            sched = _schedule(s, Ts[s], len(Ts))
            inc = sched[listed[s] % len(sched)]
            listed[s] += 1
            if complete[s] == FRAMES or inc is None:
                complete[s] = FRAMES
                rows.append((s, FRAMES, 1, 0))
            else:
                complete[s] = min(complete[s] + inc, FRAMES)
                rows.append((s, complete[s], 0, min_emit))
        call += 1
        assert call < 200
        if not rows:
            continue
        wave, out = dac.stream_decode(dev_ids, None, rows, halo, col0=1, delay=1, max_emit=MAX_EMIT)
        want = model.decode(frames_of, rows, halo, max_emit=MAX_EMIT)
        out = out.cpu().tolist()
        assert [tuple(o) for o in out] == [(e, k) for e, k, _, _ in want], (call, rows, out, [(e, k) for e, k, _, _ in want])
        wave = wave.cpu()
        assert wave.shape[1] <= hop * MAX_EMIT
        for r, (s, _, final, _) in enumerate(rows):
            e = out[r][0]
            assert e <= MAX_EMIT
            if wave.shape[1] > e * hop:
                assert float(wave[r, e * hop:].abs().max()) == 0.0  # the tail of every row is zero
            if e:
                chunks[s].append(wave[r, : e * hop].clone())
            if final:
                final_passes[s] += 1
                done[s] = model.flushed(s)
    return final_passes


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["emit", "skip"])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("spec_name,dtype", [("tiny", "f32"), ("44k", "bf16")])
def test_capped_voice_stream_concatenates_to_the_filtered_ragged_decode(spec_name, dtype, S, mode):
    dac = _dac(spec_name, dtype, 12, FRAMES)
    halo = _halo(spec_name)
    Ts = _prefix_lengths(S, halo)
    whole, prefixes, ids = _voice_utterances(Ts, halo, seed=40 + S)
    ref, ref_frames = _reference(dac, whole)
    dac.stream_open(S, FRAMES, max_voice_frames=260)
    model = StreamVoiceTableModel(S, K, 1024, max_voice_frames=260)
    for s in range(S):
        if Ts[s]:
            dac.stream_reset(s, voice=prefixes[s].cuda(), emit_prompt=mode == "emit")
        else:
            dac.stream_reset(s)
        model.reset(s, prefixes[s].numpy() if Ts[s] else None, mode == "emit")
    chunks = [[] for _ in range(S)]
    final_passes = _drive(dac, model, ids.cuda(), ids, list(range(S)), Ts, halo, 20, chunks)
    worst = 0.0
    for s in range(S):
        got = torch.cat(chunks[s]) if chunks[s] else torch.zeros(0)
        assert model.kept[s].shape[1] == ref_frames[s]
        pk = int(((prefixes[s] >= 0) & (prefixes[s] < 1024)).all(dim=0).sum())
        assert model.prompt_kept[s] == pk and (Ts[s] == 0 or pk < Ts[s])
        first = dac.hop * pk if mode == "skip" else 0
        n = ref_frames[s] * dac.hop
        assert got.shape[0] == n - first, (s, got.shape, n, first)
        worst = max(worst, float((got - ref[s, 0, first:n]).abs().max()))
        assert len(chunks[s]) >= 2
    if S > 1:
        assert final_passes[0] >= 3  # more than 2 * max_emit frames were ready when slot 0 ended
        assert len(chunks[3]) >= 3 if mode == "emit" else True
    log_parity(f"capped voice stream vs compact+ragged [{spec_name} {dtype} S={S} {mode}]: prefixes {Ts}, max|d| {worst:.3e}, kept {ref_frames}, "
               f"final passes {final_passes}", LOG)
    assert worst <= 1e-5, worst


@pytest.mark.gpu
def test_voice_then_plain_then_a_shorter_voice_in_one_slot_while_the_others_continue():
    dac = _dac("tiny", "f32", 12, FRAMES)
    halo, S = _halo("tiny"), 3
    hop = dac.hop
    Ts_a, Ts_c = [halo - 1, 69, 0], [0, 30, 0]
    whole_a, pre_a, ids_a = _voice_utterances(Ts_a, halo, seed=81)
    whole_b, _, ids_b = _voice_utterances([0, 0, 0], halo, seed=82)
    whole_c, pre_c, ids_c = _voice_utterances(Ts_c, halo, seed=83)
    refs = {t: _reference(dac, w) for t, w in (("a", whole_a), ("b", whole_b), ("c", whole_c))}
    dac.stream_open(S, FRAMES, max_voice_frames=80)
    model = StreamVoiceTableModel(S, K, 1024, max_voice_frames=80)
    for s in range(S):
        dac.stream_reset(s, voice=pre_a[s].cuda() if Ts_a[s] else None)
        model.reset(s, pre_a[s].numpy() if Ts_a[s] else None)
    got = {("a", 0): [], ("a", 1): [], ("a", 2): [], ("b", 1): [], ("c", 1): []}

    def step(ids, rows, tags):
        frames_of = lambda s, f0, f1: np.stack([ids[s, k, 1 + f0 + k: 1 + f1 + k].numpy() for k in range(K)])
        while rows:
            wave, out = dac.stream_decode(ids.cuda(), None, rows, halo, col0=1, delay=1, max_emit=MAX_EMIT)
            want = model.decode(frames_of, rows, halo, max_emit=MAX_EMIT)
            assert [tuple(o) for o in out.cpu().tolist()] == [(e, k) for e, k, _, _ in want]
            for r, ((s, _, _, _), tag) in enumerate(zip(rows, tags)):
                e = int(out[r, 0])
                if e:
                    got[tag, s].append(wave[r, : e * hop].cpu())
            keep = [i for i, r in enumerate(rows) if r[2] and not model.flushed(r[0])]  # a capped final row is listed again
            rows, tags = [rows[i] for i in keep], [tags[i] for i in keep]

    step(ids_a, [(0, 90, 0, 10), (1, 120, 0, 10), (2, 60, 0, 10)], "aaa")
    step(ids_a, [(1, FRAMES, 1, 0)], "a")  # the voice request in slot 1 ends ...
    dac.stream_reset(1)                    # ... a plain request enters it: it must not see the old prefix
    model.reset(1)
    mixed = ids_a.clone()
    mixed[1] = ids_b[1]
    step(mixed, [(0, 150, 0, 10), (1, 100, 0, 10), (2, 110, 0, 10)], "aba")
    step(mixed, [(1, FRAMES, 1, 0)], "b")
    dac.stream_reset(1, voice=pre_c[1].cuda())  # ... and a voice request with a shorter prompt
    model.reset(1, pre_c[1].numpy())
    mixed[1] = ids_c[1]
    step(mixed, [(0, 220, 0, 10), (1, 80, 0, 10)], "ac")
    step(mixed, [(0, FRAMES, 1, 0), (1, FRAMES, 1, 0), (2, FRAMES, 1, 0)], "aca")
    for (tag, s), parts in got.items():
        ref, fr = refs[tag]
        w = torch.cat(parts)
        assert w.shape[0] == fr[s] * hop, (tag, s)
        assert float((w - ref[s, 0, : fr[s] * hop]).abs().max()) <= 1e-5, (tag, s)


@pytest.mark.gpu
def test_voice_stream_refusals_change_nothing():
    from parler_tts_amd import _native as N
    from parler_tts_amd.engine import _stream_ptr

    dac = _dac("tiny", "f32", 12, FRAMES)
    halo = 26
    codes = torch.randint(0, 1024, (4, K, 400)).cuda()
    voice = torch.randint(0, 1024, (K, 50)).cuda()
    st = lambda: _stream_ptr(device=dac.device)
    dac.stream_open(4, 400)  # no prefix storage
    with pytest.raises(ValueError, match="no prefix storage"):
        dac.stream_reset(0, voice=voice)
    dac.stream_reset(0, voice=voice[:, :0])  # T == 0 is ptts_dac_stream_reset
    with pytest.raises(ValueError, match="max_emit"):
        dac.stream_decode(codes, None, [(0, 100, 0, 5)], halo, max_emit=0)
    dac.stream_open(4, 400, max_voice_frames=40)
    with pytest.raises(ValueError, match="opened for 40"):
        dac.stream_reset(0, voice=voice)
    with pytest.raises(ValueError, match="-1 frames"):
        N.check(dac.lib.ptts_dac_stream_reset_voice(dac._h, 0, N.C.c_void_p(voice.data_ptr()), -1, 1, st()), "ptts_dac_stream_reset_voice")
    with pytest.raises(ValueError, match="null voice prompt"):
        N.check(dac.lib.ptts_dac_stream_reset_voice(dac._h, 0, None, 3, 1, st()), "ptts_dac_stream_reset_voice")
    with pytest.raises(ValueError, match="out of range"):
        dac.stream_reset(4, voice=voice[:, :10])
    with pytest.raises(ValueError, match="max_emit"):
        dac.stream_decode(codes, None, [(0, 100, 0, 5)], halo, max_emit=0)
    with pytest.raises(ValueError, match="max_emit"):
        dac.stream_decode(codes, None, [(0, 100, 0, 5)], halo, max_emit=-3)
    with pytest.raises(ValueError, match="listed twice"):  # what ptts_dac_stream_decode refuses
        dac.stream_decode(codes, None, [(1, 10, 0, 5), (1, 20, 0, 5)], halo, max_emit=40)
    with pytest.raises(ValueError, match="beyond the table"):
        dac.stream_decode(codes, None, [(0, 401, 0, 5)], halo, max_emit=40)
    with pytest.raises(ValueError, match="max_batch"):
        dac.stream_open(13, 100, max_voice_frames=8)
    # a refused call counts nothing: the slots still start from 0 and hold no prefix; the cap holds, and the rest follows
    wave, out = dac.stream_decode(codes, None, [(0, 100, 0, 5), (1, 30, 0, 5)], halo, max_emit=40)
    assert out.cpu().tolist() == [[40, 100], [0, 30]]
    want = dac.decode(codes[:1, :, :100])[0, 0, : 40 * dac.hop + 0]
    assert float((wave[0, : 40 * dac.hop] - want).abs().max()) <= 1e-5
    wave, out = dac.stream_decode(codes, None, [(0, 100, 0, 5)], halo, max_emit=40)
    assert out.cpu().tolist() == [[34, 100]]  # 100 - 40 - halo
    with pytest.raises(ValueError, match="decreases"):
        dac.stream_decode(codes, None, [(0, 99, 0, 5)], halo, max_emit=40)


# ---- end to end: ContinuousBatcher(stream_voice_prompts=) on the tiny model -------------------------------------------------------------------
NEW, TMAX = 120, 70


def _voice_requests():
    """A waveform prompt (6 frames), code prompts of 40 and 70 frames, requests without a prompt, and one that ends with max_length - K = 34
    frames, fewer than its 40-frame prompt."""
    import cases as C

    desc, prompt_ids, voice, _, _ = C.gen_voice_inputs(C.GEN_VOICE_SEEDS[1])
    g = torch.Generator().manual_seed(77)
    reqs = [dict(input_ids=desc[0], prompt_input_ids=prompt_ids[0], max_new_tokens=90, input_values=voice.cuda()),
            dict(e2e_request(646, NEW)),
            dict(e2e_request(503, 100), decoder_input_ids=torch.randint(0, 1024, (K, 40), generator=g).cuda()),
            dict(e2e_request(549, NEW), decoder_input_ids=torch.randint(0, 1024, (K, 70), generator=g).cuda()),
            dict(e2e_request(550, 2), decoder_input_ids=torch.randint(0, 1024, (K, 40), generator=g).cuda()),
            dict(e2e_request(590, 75)),
            dict(e2e_request(594, 60), decoder_input_ids=torch.randint(0, 1024, (K, 70), generator=g).cuda()),
            dict(e2e_request(901, 88))]
    return reqs, [6, 0, 40, 70, 40, 0, 70, 0]


def _e2e(m, slots, tag, min_share=None):
    import parler_tts_amd as P

    reqs, Ts = _voice_requests()
    base = dict(slots=slots, max_description_tokens=E2E_N, max_prompt_tokens=E2E_P, poll_steps=16, do_sample=False, max_new_tokens=NEW, min_new_tokens=NEW,
                max_voice_frames=TMAX)
    ref = P.ContinuousBatcher(m, **base).run(reqs)
    hop = DA.DAC_TINY.hop_length
    for mode in ("emit", "skip"):
        cb = P.ContinuousBatcher(m, stream_chunk_frames=CHUNK, stream_first_chunk_frames=FIRST, stream_voice_prompts=mode, **base)
        got, pieces, order = _stream_run(cb, reqs)
        worst = 0.0
        for i, (w, (wav, n), T, r) in enumerate(zip(got, ref, Ts, reqs)):
            first = 0
            if mode == "skip" and T:  # the prompt's kept frames: it holds valid codes only, and max_length - K frames of the request exist
                first = hop * min(T, T + r["max_new_tokens"] + 1 - K)
            assert w.shape[0] == n - first == wav.shape[0] - first, (mode, i, w.shape, n, first)
            if w.shape[0]:
                worst = max(worst, float((w - wav[first:]).abs().max()))
        log_parity(f"voice streaming vs run() [{tag}, {slots} slots, {mode}]: pieces {pieces}, {cb.codec_passes} codec passes, max|d| {worst:.3e}", LOG)
        assert worst <= 1e-5, (mode, worst)
        if mode == "emit":
            assert pieces[3] >= 3  # the request with the 70-frame prompt came in pieces
            assert ref[4][1] == hop * 34
    if min_share is not None:  # a condition on the input: every window behind a prompt holds filtered frames
        kept = sum(n // hop - min(T, T + r["max_new_tokens"] + 1 - K) for (_, n), T, r in zip(ref, Ts, reqs))
        frames = sum(max(0, r["max_new_tokens"] + 1 - K) for r in reqs)
        log_parity(f"    kept share of generated frames {kept / frames:.3f} ({kept} of {frames})", LOG)
        assert 0.2 <= kept / frames <= 0.9, kept / frames
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [2, 12])
def test_voice_streaming_batcher_end_to_end_clean_model(slots):
    import cases as C
    import parler_tts_amd as P

    m, spec, sd, dsd = C.tiny_model(seed=E2E_MODEL_SEED)
    m = m.to("cuda")
    _e2e(m, slots, "clean")
    if slots == 2:  # requests without a prompt: the chunk lengths of a streaming session built without the option
        plain = [e2e_request(646, NEW), e2e_request(590, 75), e2e_request(901, 88)]
        base = dict(slots=slots, max_description_tokens=E2E_N, max_prompt_tokens=E2E_P, poll_steps=16, do_sample=False, max_new_tokens=NEW, min_new_tokens=NEW,
                    max_voice_frames=TMAX, stream_chunk_frames=CHUNK, stream_first_chunk_frames=FIRST)
        lengths = []
        for extra in ({}, {"stream_voice_prompts": "emit"}):
            cb = P.ContinuousBatcher(m, **base, **extra)
            tickets = [cb.submit(**r) for r in plain]
            lengths.append([(t, c.shape[0], last) for t, c, last in cb.chunks()])
        assert lengths[0] == lengths[1] and len(lengths[0]) > 6


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [2, 12])
def test_voice_streaming_batcher_end_to_end_scattered_drops(slots):
    m, spec, sd, dsd = drops_model()
    m = m.to("cuda")
    _e2e(m, slots, "scattered drops", min_share=True)
