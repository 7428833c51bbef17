"""Continuous batching on top of the engine's session interface (``ptts_session_begin`` / ``ptts_admit_row`` / ``ptts_row_state`` /
``ptts_retire_row``): a fixed number of utterance slots decode together, a request is admitted into a slot as soon as the previous one
there has finished, and finished requests are handed out while the others keep going. ``generate()`` is a static batch: it runs until
its LAST row has finished (reference ``_sample``, modeling_parler_tts.py:3564), which on requests of mixed lengths spends a large share
of every step on rows that are already done.

A request is computed exactly as a row of a static batch padded to the session's widths: the description is padded (masked) to
``max_description_tokens``, the prompt to ``max_prompt_tokens`` (padding to the right, so the prompt tokens keep their positions), and
its ``max_new_tokens`` sets its own delay pattern and end.

Streaming mode (``stream_chunk_frames``): a request's audio leaves in chunks while its slot is still decoding. The codec engine keeps, per
slot and on the device, the request's kept (un-delayed, special-id filtered) codes and how many of them were emitted
(``ptts_dac_stream_decode``); every poll lists the slots that have a chunk ready and ONE windowed codec pass serves them all, reading the
decoder engine's raw id buffer in place on the stream the decode steps run on. The concatenation of a request's chunks is the waveform
the non-streaming mode yields for it."""
from __future__ import annotations

import collections
import copy
import math
from typing import Deque, Dict, Iterable, Iterator, List, Optional, Tuple

import torch

from .engine import DecoderEngine
from .generation_extras import LOGIT_EDIT_OPTIONS, active_extras, check_generation_mode, logit_edit_rule_broken, logit_edits_of
from .modeling_parler_tts import apply_delay_pattern_mask, build_delay_pattern_mask

_HOST_LOOP_ARGUMENTS = ("logits_processor", "stopping_criteria", "output_scores", "output_logits")
_VOICE_ARGUMENTS = ("input_values", "decoder_input_ids")
_DEVICE_PENALTIES = ("repetition_penalty", "no_repeat_ngram_size")
_DEVICE_WARPERS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


class _Request:
    __slots__ = ("ticket", "enc", "enc_mask", "prompt", "prompt_mask", "max_length", "gen", "voice", "prompt_kept", "pen", "warp", "edits",
                 "cols", "absorbed", "kept", "emitted", "first_out", "want_records", "records")

    def __init__(self, ticket, enc, enc_mask, prompt, prompt_mask, max_length, gen=None, voice=None, prompt_kept=None, pen=None, warp=None, edits=None):
        self.edits = edits  # the request's own generation_extras.LogitEdits (set_slot_logit_edits), or None: the session's
        self.warp = warp  # the request's own (min_p, typical_p, epsilon_cutoff, eta_cutoff) (set_slot_sample_warp), or None: the session's
        self.pen = pen  # the request's own (repetition_penalty, no_repeat_ngram_size) (set_slot_history_penalty), or None: the session's
        self.ticket, self.enc, self.enc_mask, self.prompt, self.prompt_mask, self.max_length = ticket, enc, enc_mask, prompt, prompt_mask, max_length
        self.gen = gen  # the request's own sampler record (DecoderEngine.admit_row's `gen`), or None: the session's
        self.voice = voice  # un-delayed codes [K, T >= 1] of the voice prompt the request continues (admit_row's `voice`), or None
        # stream_voice_prompts="skip": prompt_kept[n] = frames the special-id filter keeps of the prompt's first n, n = 0..T (else None)
        self.prompt_kept = prompt_kept
        # The request's progress in its slot (it occupies one slot, once). cols: columns the slot holds if it has not stopped on EOS, set at
        # admission (BOS + the given columns + the first token), then one per step.
        self.cols = 0
        # Streaming: raw frames the stream table has absorbed, frames it kept of them and frames emitted; the first chunk is still outstanding
        self.absorbed, self.kept, self.emitted, self.first_out = 0, 0, 0, True
        # step records (submit's output_scores / output_logits): the kinds asked for, and the slot's buffers {kind: [max_new_tokens, K, V]} from
        # the admission on
        self.want_records, self.records = (False, False), None

    @property
    def T(self) -> int:
        return 0 if self.voice is None else int(self.voice.shape[1])

    @property
    def skipped(self) -> int:
        """Frames of the prompt that are never emitted (stream_voice_prompts="skip"), else 0."""
        return 0 if self.prompt_kept is None else self.T

    def new_raw(self, complete: int) -> int:
        """Raw frames of [absorbed, complete) that may become ready: all of them, less those of a prompt that is not emitted."""
        return max(complete, self.skipped) - max(self.absorbed, self.skipped)


class ContinuousBatcher:
    """``slots`` utterances decode together on ``model``'s HIP engine; ``submit`` queues a request (FIFO), iterating yields
    ``(ticket, waveform 1-D, length)`` as requests finish, ``run(requests)`` returns ``[(waveform, length), ...]`` in submission order.

    ``generation_kwargs`` are ``generate()``'s: ``max_new_tokens`` / ``max_length`` (the session's limit; a request may ask for less),
    ``min_new_tokens``, ``do_sample``, ``temperature``, ``top_k``, ``top_p``: the session's values, which ``submit`` may override per request
    (with a ``seed`` of its own, see there). Everything that needs the host loop or a streamer raises ``NotImplementedError``; so does a
    voice prompt given HERE: it belongs to a request (``submit(input_values=...)`` / ``submit(decoder_input_ids=...)``). ``poll_steps``: decode steps between two looks at the slots (each look is one host sync);
    a request that ends by its own ``max_new_tokens`` is known in advance and is met exactly.

    ``stream_chunk_frames`` (default ``None``: off) switches to streaming: ``chunks()`` yields ``(ticket, chunk 1-D float32, last)`` as soon as
    a slot holds ``stream_chunk_frames`` kept frames beyond the codec's right halo (``stream_first_chunk_frames`` for a request's first chunk,
    default the same), ``last`` is True exactly once per ticket, and ``__iter__`` / ``run()`` raise. ``cancel(ticket)`` drops a request in either
    mode. The stream table lives in ONE codec engine, sized at construction for ``slots`` windows; should another call replace that engine
    (``DACModel._get_engine`` does when it needs more capacity), the next codec pass raises ``RuntimeError`` - the requests in flight are lost,
    nothing is restarted silently.

    ``admit_batch`` (default 1: one ``ptts_admit_row`` per request): with N > 1, the requests that find an idle slot at the same poll are
    admitted in groups of up to N through one prefill pass each (``ptts_admit_rows``). The engine is then created with that many spare rows
    behind the slots (``spare_rows``: clamped to the batch-size class of ``slots``; fewer than 2 left = single admissions). A request admitted
    in a group is within the engine's tolerance of the reference, not bit-identical to the same request admitted alone.

    A model with ``enable_fp8_kv_cache()`` runs the session on the e4m3 self-attention cache whenever the engine holds more than 8 rows
    (slots + spare; ``ptts_session_begin_kv8``), half the self-attention arena per slot; with 8 rows or fewer it keeps the bf16 cache, as
    ``generate()`` does. There is no argument for it here: the model's switch is the opt-in, and ``self.eng.kv_fp8`` says which cache runs.

    ``max_voice_frames`` (default 0: no request brings a voice prompt, and every call on the model and the engine is the one made without
    this argument): the longest voice prompt, in codec frames, a request may bring. The engine's prefill is then sized for
    ``max_prompt_tokens + 1 + max_voice_frames`` positions. A limit given as ``max_new_tokens`` counts NEW tokens, as in ``generate()``: the
    session's ``max_length`` grows by ``max_voice_frames`` and a request with T frames gets ``max_new_tokens + 1 + T`` columns; a limit
    given as ``max_length`` stays the total. A request with a voice prompt is admitted alone (``ptts_admit_row_voice``), also with
    ``admit_batch > 1`` (but see ``admit_voice_groups``), and in streaming mode only with ``stream_voice_prompts`` (without it ``submit`` raises ``NotImplementedError``).

    ``stream_voice_prompts`` (default ``None``; needs ``stream_chunk_frames`` and ``max_voice_frames > 0``): a streaming session takes voice
    prompts. ``"emit"``: a request's chunks concatenate to the waveform of the non-streaming mode, the prompt's frames included. ``"skip"``:
    to that waveform without its leading ``hop * (kept prompt frames)`` samples - the continuation alone, for a caller who has the reference
    audio already. The codec's stream table then keeps each slot's prompt (``ptts_dac_stream_open_voice`` / ``_reset_voice``) and no pass
    emits more than ``max_emit = window_frames - 2 * halo`` frames per slot (``ptts_dac_stream_decode_capped``): a long prompt leaves in
    several chunks, starting at the poll that admits it, and a finished slot is drained by repeated final passes before it is reused. A
    request without a prompt never has that much ready: its chunks are the ones of a session without the option.

    A model with ``enable_device_step_records()`` opens the session with step records on (``ptts_step_record.h``): ``submit(output_scores=True)`` /
    ``submit(output_logits=True)`` then records that request's per-step scores / raw logits on the device, and ``step_records(ticket)`` hands them
    out once the request has finished. Requests that ask for none run beside them untouched.

    ``admit_voice_groups`` (default ``False``; needs ``max_voice_frames > 0`` and ``admit_batch > 1``, ``ValueError`` otherwise): requests with
    voice prompts are admitted in groups too. The FIFO queue is cut into runs of the same kind - with a prompt, without - and each run into
    groups of at most ``spare``; a group of requests with prompts is ONE prefill pass over ``max_prompt_tokens + 1 + (the group's longest
    prompt)`` positions per request (``ptts_admit_rows_voice``), the shorter ones padded. The order of admission stays FIFO, and
    ``admission_groups`` counts these groups too. Like any group admission: within the engine's tolerance of the same request admitted alone."""

    def __init__(self, model, slots: int, max_description_tokens: int, max_prompt_tokens: int, poll_steps: int = 16,
                 stream_chunk_frames: Optional[int] = None, stream_first_chunk_frames: Optional[int] = None, admit_batch: int = 1, max_voice_frames: int = 0,
                 stream_voice_prompts: Optional[str] = None, admit_voice_groups: bool = False, **generation_kwargs):
        if int(admit_batch) < 1:
            raise ValueError("`admit_batch` must be >= 1")
        if int(max_voice_frames) < 0:
            raise ValueError("`max_voice_frames` must be >= 0")
        if admit_voice_groups and (int(max_voice_frames) < 1 or int(admit_batch) < 2):
            raise ValueError("`admit_voice_groups` needs `max_voice_frames` > 0 and `admit_batch` > 1")
        if stream_voice_prompts not in (None, "emit", "skip"):
            raise ValueError(f"`stream_voice_prompts` must be None, 'emit' or 'skip', got {stream_voice_prompts!r}")
        if stream_voice_prompts is not None and (stream_chunk_frames is None or int(max_voice_frames) < 1):
            raise ValueError("`stream_voice_prompts` needs `stream_chunk_frames` (streaming mode) and `max_voice_frames` > 0")
        if slots < 1 or max_description_tokens < 1 or max_prompt_tokens < 0 or poll_steps < 1:
            raise ValueError("slots, max_description_tokens and poll_steps must be >= 1 and max_prompt_tokens >= 0")
        if stream_chunk_frames is None and stream_first_chunk_frames is not None:
            raise ValueError("`stream_first_chunk_frames` needs `stream_chunk_frames` (streaming mode)")
        if stream_chunk_frames is not None and (int(stream_chunk_frames) < 1 or (stream_first_chunk_frames is not None and int(stream_first_chunk_frames) < 1)):
            raise ValueError("`stream_chunk_frames` and `stream_first_chunk_frames` must be >= 1")
        for name in ("streamer",) + _HOST_LOOP_ARGUMENTS:
            if generation_kwargs.get(name):
                raise NotImplementedError(f"`{name}` needs generate()'s host loop / streamer, one utterance at a time: not available in a continuous batch")
            generation_kwargs.pop(name, None)
        for name in _VOICE_ARGUMENTS:
            if generation_kwargs.get(name) is not None:
                raise NotImplementedError(f"`{name}` (voice prompt): a continuous session takes no audio prefix of its own; give it to submit()")
            generation_kwargs.pop(name, None)
        if getattr(model, "prompt_cross_attention", False):
            raise NotImplementedError("prompt_cross_attention models: the prompt joins the cross-attention context, which a session keeps at a fixed width")
        gc = copy.deepcopy(model.generation_config)
        unused = gc.update(**generation_kwargs)
        if unused:
            raise ValueError(f"The following arguments are not generation options: {sorted(unused)}")
        check_generation_mode(gc)
        extras = active_extras(gc)
        # model.enable_device_penalties(): the two history penalties run as a device node of the session's step (ptts_penalty.h)
        self.device_penalties = bool(getattr(model, "device_penalties", False))
        if self.device_penalties:
            extras = [x for x in extras if x not in _DEVICE_PENALTIES]
        # model.enable_device_warpers(): min_p / typical_p / epsilon_cutoff / eta_cutoff inside the session's sampler tail (ptts_warp.h)
        self.device_warpers = bool(getattr(model, "device_warpers", False))
        if self.device_warpers:
            extras = [x for x in extras if x not in _DEVICE_WARPERS]
        # model.enable_device_logit_edits(): the five position / token edits as a device node of the session's step (ptts_logit_edit.h)
        self.device_logit_edits = bool(getattr(model, "device_logit_edits", False))
        if self.device_logit_edits:
            extras = [x for x in extras if x not in LOGIT_EDIT_OPTIONS]
        if extras:
            raise NotImplementedError(f"generation options {extras} run on generate()'s host loop (generation_extras): not available in a continuous batch")
        if int(getattr(gc, "num_return_sequences", 1) or 1) != 1:
            raise NotImplementedError("num_return_sequences > 1: submit the request several times")
        self.model, self.slots, self.N, self.P, self.poll_steps = model, int(slots), int(max_description_tokens), int(max_prompt_tokens), int(poll_steps)
        self.max_voice_frames = int(max_voice_frames)
        self.voice_groups = bool(admit_voice_groups)
        # new tokens of a request that names no limit of its own (None: the session's limit is a total, `max_length`)
        self._max_new = int(gc.max_new_tokens) if gc.max_new_tokens is not None else None
        self.max_length = self._max_new + 1 + self.max_voice_frames if self._max_new is not None else int(gc.max_length)
        if self.max_length < 2:
            raise ValueError("`max_length` / `max_new_tokens` leave no room for a generated token")
        min_new = int(gc.min_new_tokens or 0)
        if getattr(gc, "min_length", 0):
            min_new = max(min_new, int(gc.min_length) - 1)
        do_sample = bool(gc.do_sample)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if do_sample else 0  # follows torch.manual_seed(), as generate() does
        d = model.config.decoder
        self.K, self.bos = d.num_codebooks, d.bos_token_id
        self.pad = gc.pad_token_id if gc.pad_token_id is not None else d.pad_token_id
        # admit_batch > 1: the engine carries `spare` arena rows behind the slots, where a group of requests is prefilled in one pass
        self.spare = self.spare_rows(self.slots, int(admit_batch))
        self.admissions, self.admission_groups = 0, []  # requests admitted; sizes of the groups that went through admit_rows
        # An option that is off adds nothing to a call: no fifth argument here, no keyword below. With voice prompts the prefill of one slot
        # runs P + 1 + T positions
        voice_room = (self.max_voice_frames,) if self.max_voice_frames else ()
        # the session's own penalties (neutral where the caller gave none), checked before anything touches the engine
        self._pen = self._penalty(gc.repetition_penalty, gc.no_repeat_ngram_size, (1.0, 0)) if self.device_penalties else None
        self._warp = (self._warpers(gc.min_p, gc.typical_p, gc.epsilon_cutoff, gc.eta_cutoff, (0.0, 1.0, 0.0, 0.0))
                      if self.device_warpers else None)
        # ... and its logit edits: the options as given (what a request's own start from) and their record, under the two rules of the node's place
        self.V, self.eos = d.vocab_size, d.eos_token_id
        self._edit_opts = {n: getattr(gc, n, None) for n in LOGIT_EDIT_OPTIONS} if self.device_logit_edits else None
        self._edits = self._logit_edits(self._edit_opts, self.max_length, gc.repetition_penalty, gc.no_repeat_ngram_size, min_new) if self.device_logit_edits else None
        self._min_new = min_new
        self.eng = model._get_engine(self.slots + self.spare, self.N, self.P, self.max_length, *voice_room)
        self.eng.set_gen_params(max_length=self.max_length, min_new_tokens=min_new, do_sample=do_sample, temperature=float(gc.temperature or 1.0),
                                top_k=int(gc.top_k or 0) if do_sample else 0, top_p=float(gc.top_p if gc.top_p is not None else 1.0), use_eos_gate=True, seed=seed)
        # The penalty node is part of the session's step from its begin: on with the session's values (a request may bring its own), or off -
        # also where an earlier call left it on. A model without the switch, on an engine that never had the node, makes no call here.
        if self.device_penalties:
            self.eng.set_history_penalty(*self._pen)
        elif getattr(self.eng, "history_penalty", None) is not None:
            self.eng.set_history_penalty(enabled=False)
        # The warpers likewise: the tail instance of the session is fixed at its begin
        if self.device_warpers:
            self.eng.set_sample_warp(*self._warp)
        elif getattr(self.eng, "sample_warp", None) is not None:
            self.eng.set_sample_warp(enabled=False)
        # The logit-edit node likewise: part of the session's step from its begin
        if self.device_logit_edits:
            self.eng.set_logit_edits(self._edits)
        elif getattr(self.eng, "logit_edits", None) is not None:
            self.eng.set_logit_edits(enabled=False)
        # Step records likewise: "on, no slot records yet" before the session begins; a request's buffers are set at its admission
        self.device_step_records = bool(getattr(model, "device_step_records", False))
        self._records: Dict[int, Dict[str, torch.Tensor]] = {}  # ticket -> the finished request's records, until step_records() reads them
        if self.device_step_records:
            self.eng.set_step_records(None, None, 0)
        elif getattr(self.eng, "step_records", None) is not None:
            self.eng.set_step_records(enabled=False)
        # model.enable_fp8_kv_cache() and more than 8 rows: the session runs on the e4m3 self-attention cache
        self.eng.begin_session(self.slots, self.N, self.P, **({"kv_fp8": True} if getattr(self.eng, "kv_fp8", False) else {}))
        # what a request's own record starts from (submit): the session's values as the caller gave them (top_k is not zeroed for a greedy session)
        self._gen = dict(min_new_tokens=min_new, do_sample=do_sample, temperature=float(gc.temperature or 1.0), top_k=int(gc.top_k or 0),
                         top_p=float(gc.top_p if gc.top_p is not None else 1.0))
        self._queue: Deque[_Request] = collections.deque()
        self._slot: List[Optional[_Request]] = [None] * self.slots
        self._done: Deque[Tuple[int, torch.Tensor, int]] = collections.deque()
        self._next_ticket = 0
        self.chunk = None if stream_chunk_frames is None else int(stream_chunk_frames)
        self.stream_voice = stream_voice_prompts
        if self.chunk is not None:
            from .streamer import receptive_halo_frames

            ae = model.audio_encoder
            self.first_chunk = self.chunk if stream_first_chunk_frames is None else int(stream_first_chunk_frames)
            self.halo = receptive_halo_frames(getattr(ae, "decoder_rates", (8, 8, 4, 2)))
            # a window = left halo + what is ready. Ready stays below chunk + halo + poll_steps on the host's own count; the library bounds it
            # without reading the device (ptts.h), which after dropped frames is looser by up to another chunk + halo
            big = max(self.chunk, self.first_chunk)
            self.window_frames = min(3 * self.halo + 2 * big + self.poll_steps + 8, max(self.max_length, 1))
            ae.stream_open(self.slots, self.max_length, self.window_frames, **({} if self.stream_voice is None else {"max_voice_frames": self.max_voice_frames}))
            if self.stream_voice is not None:
                # a capped window = halo + max_emit + halo frames. A request without a prompt has fewer than chunk + poll_steps frames to emit
                # at a poll, which is below this cap; a window as long as the longest request needs none
                self.max_emit = self.window_frames - 2 * self.halo if self.window_frames < self.max_length else self.max_length
            self._out: Deque[Tuple[int, torch.Tensor, bool]] = collections.deque()
            self.codec_passes, self.codec_rows, self.whole_requests = 0, 0, 0  # passes, listed rows, requests that ended below 2K - 1 columns

    @staticmethod
    def spare_rows(slots: int, admit_batch: int) -> int:
        """Spare engine rows of a batcher of ``slots`` slots asked for groups of ``admit_batch``: clamped so that ``slots + spare`` stays in the
        batch-size class of ``slots`` (<= 4, <= 8, wider: the class decides the kernels of the decode step, which must not change), and 0 -
        single admissions - where fewer than 2 would be left."""
        if admit_batch <= 1:
            return 0
        top = 4 if slots <= 4 else (8 if slots <= 8 else None)
        spare = admit_batch if top is None else min(admit_batch, top - slots)
        return spare if spare >= 2 else 0

    # -- requests ---------------------------------------------------------------------------------------------------------------
    def _pad_ids(self, ids, mask, width: int, what: str):
        ids = torch.as_tensor(ids).long()
        if ids.dim() == 2 and ids.shape[0] == 1:
            ids = ids[0]
        if ids.dim() != 1:
            raise ValueError(f"{what}: one request at a time ([tokens] or [1, tokens]), got {tuple(ids.shape)}")
        n = int(ids.shape[0])
        if n > width:
            raise ValueError(f"{what} has {n} tokens, the session was opened for {width}")
        if mask is None:
            mask = torch.ones(n, dtype=torch.long)
        mask = torch.as_tensor(mask).long().reshape(-1)
        if mask.shape[0] != n:
            raise ValueError(f"{what}: attention mask of {mask.shape[0]} positions for {n} tokens")
        out_ids, out_mask = torch.zeros(width, dtype=torch.long), torch.zeros(width, dtype=torch.long)
        out_ids[:n], out_mask[:n] = ids.cpu(), mask.cpu()
        return out_ids, out_mask

    def _request_gen(self, do_sample, temperature, top_k, top_p, min_new_tokens, seed) -> Optional[dict]:
        """The sampler record of a request that sets any of these options (the session's values fill the rest), or None. ``seed`` stays
        ``None`` here where the caller gave none: submit draws it once nothing can refuse the request any more."""
        given = dict(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, min_new_tokens=min_new_tokens)
        if seed is None and all(v is None for v in given.values()):
            return None
        gen = dict(self._gen)
        gen.update({k: v for k, v in given.items() if v is not None})
        gen["do_sample"], gen["temperature"], gen["top_p"] = bool(gen["do_sample"]), float(gen["temperature"]), float(gen["top_p"])
        gen["top_k"], gen["min_new_tokens"] = int(gen["top_k"]), int(gen["min_new_tokens"])
        if not (math.isfinite(gen["temperature"]) and gen["temperature"] > 0.0):
            raise ValueError(f"`temperature` must be a finite number > 0, got {gen['temperature']}")
        if not 0.0 < gen["top_p"] <= 1.0:
            raise ValueError(f"`top_p` must be in (0, 1], got {gen['top_p']}")
        if gen["top_k"] < 0:
            raise ValueError(f"`top_k` must be >= 0, got {gen['top_k']}")
        if gen["min_new_tokens"] < 0:
            raise ValueError(f"`min_new_tokens` must be >= 0, got {gen['min_new_tokens']}")
        gen["use_eos_gate"] = True
        gen["seed"] = None if seed is None else int(seed) & (2 ** 64 - 1)  # without effect on a greedy request
        return gen

    @staticmethod
    def _penalty(repetition_penalty, no_repeat_ngram_size, default) -> Tuple[float, int]:
        """(repetition_penalty, no_repeat_ngram_size) with ``default``'s value for an option left ``None``; ``ValueError`` on a bad value."""
        p = default[0] if repetition_penalty is None else repetition_penalty
        n = default[1] if no_repeat_ngram_size is None else no_repeat_ngram_size
        DecoderEngine._history_penalty(p, n)  # the engine wrapper's own checks, here so that a bad value never reaches the queue
        return float(p), int(n)

    @staticmethod
    def _warpers(min_p, typical_p, epsilon_cutoff, eta_cutoff, default) -> Tuple[float, float, float, float]:
        """(min_p, typical_p, epsilon_cutoff, eta_cutoff) with ``default``'s value for an option left ``None``; ``ValueError`` on a bad value."""
        vals = tuple(d if v is None else v for v, d in zip((min_p, typical_p, epsilon_cutoff, eta_cutoff), default))
        DecoderEngine._sample_warp(*vals)  # the engine wrapper's own checks, here so that a bad value never reaches the queue
        return tuple(float(v) for v in vals)

    def _logit_edits(self, options: dict, max_length: int, repetition_penalty, no_repeat_ngram_size, min_new_tokens):
        """The five options as the node's record; ``ValueError`` on what the node does not compute (a multi-token key, a bad value) and on the
        two combinations in which its place in the chain is not transformers' order, beside the penalties and ``min_new_tokens`` in effect."""
        edits = logit_edits_of(self.V, self.eos, max_length, **options)
        broken = logit_edit_rule_broken(edits, repetition_penalty, no_repeat_ngram_size, min_new_tokens)
        if broken:
            raise ValueError(broken + ": not available in a continuous batch")
        return edits

    @torch.no_grad()
    def submit(self, input_ids, attention_mask=None, prompt_input_ids=None, prompt_attention_mask=None, max_new_tokens: Optional[int] = None,
               do_sample: Optional[bool] = None, temperature: Optional[float] = None, top_k: Optional[int] = None, top_p: Optional[float] = None,
               min_new_tokens: Optional[int] = None, seed: Optional[int] = None, input_values=None, decoder_input_ids=None,
               repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None, min_p: Optional[float] = None,
               typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None, eta_cutoff: Optional[float] = None, sequence_bias=None,
               bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, exponential_decay_length_penalty=None,
               output_scores: bool = False, output_logits: bool = False) -> int:
        """Queues one request and returns its ticket. The description is encoded here (the model's own T5 path).
        ``do_sample`` / ``temperature`` / ``top_k`` / ``top_p`` / ``min_new_tokens``: the request's own sampler settings; an option left ``None``
        takes the session's value. A request that sets any of them (or ``seed``) draws from its own stream ``(seed, column, codebook)``: with a
        ``seed`` it gives the same tokens in whichever slot and at whatever time it runs, with ``seed=None`` one is drawn from torch's RNG here
        (``torch.manual_seed`` governs the run). A request that sets none is admitted on the session's parameters and draw stream.
        ``input_values`` (a waveform [1, 1, samples], encoded on the model's own DAC encoder) or ``decoder_input_ids`` (codes [K, T], a leading
        BOS column is dropped): the voice prompt the request continues, as ``generate()`` takes it; needs ``max_voice_frames >= T``. The
        request's waveform contains the prompt's frames, and ``max_new_tokens`` counts what follows them.
        ``repetition_penalty`` / ``no_repeat_ngram_size`` (a model with ``enable_device_penalties()``; ``NotImplementedError`` otherwise): the
        request's own history penalties, an option left ``None`` taking the session's value. They are computed over the request's own
        columns - BOS, the voice prompt's, what it generated - as ``generate()`` computes them for the same request alone.
        ``min_p`` / ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff`` (a model with ``enable_device_warpers()``; ``NotImplementedError``
        otherwise): the request's own warpers behind top-p, an option left ``None`` taking the session's value; without effect on a greedy
        request.
        ``sequence_bias`` / ``bad_words_ids`` (single-token keys) / ``suppress_tokens`` / ``begin_suppress_tokens`` /
        ``exponential_decay_length_penalty`` (a model with ``enable_device_logit_edits()``; ``NotImplementedError`` otherwise): the request's
        own logit edits, an option left ``None`` taking the session's value. The begin index and the decay's start count from the request's
        own given columns (BOS and its voice prompt's). ``ValueError``: a multi-token key, a token outside the vocabulary, ``sequence_bias``
        beside a history penalty, a decay with ``min_new_tokens > start + 1``.
        ``output_scores`` / ``output_logits`` (a model with ``enable_device_step_records()``; ``ValueError`` otherwise): the request's per-step
        processed scores / raw logits are recorded on the device into buffers ``[max_new_tokens, K, V]`` (fp32, allocated at its admission);
        ``step_records(ticket)`` returns them once the request has finished."""
        if (output_scores or output_logits) and not self.device_step_records:
            raise ValueError("`output_scores` / `output_logits` need the session's step records: call model.enable_device_step_records() before "
                             "constructing the batcher")
        own_edits = dict(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, suppress_tokens=suppress_tokens,
                         begin_suppress_tokens=begin_suppress_tokens, exponential_decay_length_penalty=exponential_decay_length_penalty)
        if any(v is not None for v in own_edits.values()) and not self.device_logit_edits:
            raise NotImplementedError(f"generation options {list(LOGIT_EDIT_OPTIONS)} run on generate()'s host loop "
                                      "(generation_extras): not available in a continuous batch without model.enable_device_logit_edits()")
        warp = None
        if any(v is not None for v in (min_p, typical_p, epsilon_cutoff, eta_cutoff)):
            if not self.device_warpers:
                raise NotImplementedError("generation options ['min_p', 'typical_p', 'epsilon_cutoff', 'eta_cutoff'] run on generate()'s host loop "
                                          "(generation_extras): not available in a continuous batch without model.enable_device_warpers()")
            warp = self._warpers(min_p, typical_p, epsilon_cutoff, eta_cutoff, self._warp)
        pen = None
        if repetition_penalty is not None or no_repeat_ngram_size is not None:
            if not self.device_penalties:
                raise NotImplementedError("generation options ['repetition_penalty', 'no_repeat_ngram_size'] run on generate()'s host loop "
                                          "(generation_extras): not available in a continuous batch without model.enable_device_penalties()")
            pen = self._penalty(repetition_penalty, no_repeat_ngram_size, self._pen)
        voice = self._voice(input_values, decoder_input_ids)
        T = 0 if voice is None else int(voice.shape[1])
        if max_new_tokens is not None:
            max_length = int(max_new_tokens) + 1 + T
        else:
            max_length = self.max_length if self._max_new is None else self._max_new + 1 + T
        if max_length < T + 2:
            raise ValueError("`max_new_tokens` leaves no room for a generated token" if T == 0 or max_new_tokens is not None else
                             f"a voice prompt of {T} frames leaves no room for a generated token below the session's max_length {self.max_length}")
        room = self.max_length - 1 - T if self._max_new is None else self._max_new  # new tokens the session grants this request
        if max_length - 1 - T > room:
            raise ValueError(f"max_new_tokens {max_length - 1 - T} exceeds the session's {room}")
        gen = self._request_gen(do_sample, temperature, top_k, top_p, min_new_tokens, seed)
        edits = None
        if self.device_logit_edits:  # the record in effect - the request's own over the session's - beside the penalties and min_new_tokens in effect
            opts = {n: self._edit_opts[n] if v is None else v for n, v in own_edits.items()}
            rp, ng = pen if pen is not None else (self._pen if self._pen is not None else (None, None))
            in_effect = self._logit_edits(opts, max_length, rp, ng, self._min_new if gen is None else gen["min_new_tokens"])
            if any(v is not None for v in own_edits.values()):
                edits = in_effect
        dev = self.model.device
        ids, mask = self._pad_ids(input_ids, attention_mask, self.N, "description")
        enc = self.model._encode_description(ids[None].to(dev), mask[None].to(dev))[0].float()
        prompt = pmask = None
        if self.P > 0:
            if prompt_input_ids is None:
                raise ValueError(f"the session was opened for prompts of up to {self.P} tokens: `prompt_input_ids` is required")
            pids, pmask = self._pad_ids(prompt_input_ids, prompt_attention_mask, self.P, "prompt")
            prompt = self.model.embed_prompts(pids[None].to(dev))[0].float()
        elif prompt_input_ids is not None:
            raise ValueError("the session was opened without prompt positions (max_prompt_tokens = 0)")
        if gen is not None and gen["seed"] is None:  # follows torch.manual_seed(), as the session's seed does; a refused submit draws nothing
            gen["seed"] = int(torch.randint(0, 2 ** 62, (1,)).item()) if gen["do_sample"] else 0
        ticket = self._next_ticket
        self._next_ticket += 1
        prompt_kept = None
        if voice is not None and self.stream_voice == "skip":  # what the filter keeps of the prompt, known here: the codec's pairs do not say
            prompt_kept = [0] + self._valid_frames(voice).long().cumsum(0).tolist()
        req = _Request(ticket, enc, mask, prompt, pmask, max_length, gen, voice, prompt_kept, *(() if pen is None else (pen,)),
                       **({} if warp is None else {"warp": warp}), **({} if edits is None else {"edits": edits}))
        req.want_records = (bool(output_scores), bool(output_logits))
        self._queue.append(req)
        return ticket

    def step_records(self, ticket: int) -> Dict[str, torch.Tensor]:
        """The step records of a finished request that asked for them: ``{"scores": [steps, K, V], "logits": [steps, K, V]}`` with the kinds it
        asked for, ``steps`` = the tokens it generated (step i: what ``generate()`` returns as ``scores[i]`` / ``logits[i]`` for the same request
        alone). Available once the request's waveform (its last chunk) has been yielded; handed out once - the batcher keeps no reference.
        Until then the batcher holds the tensors (``max_new_tokens x K x V x 4`` bytes per kind and request as allocated): a caller that asks for
        records reads them - ``run()`` does not - or drops them with ``close()``.
        ``KeyError``: an unknown, unfinished or cancelled ticket, one that asked for no record, or one read before."""
        return self._records.pop(ticket)

    def _voice(self, input_values, decoder_input_ids) -> Optional[torch.Tensor]:
        """The voice prompt of one request as un-delayed codes [K, T >= 1], or None: generate()'s own preparation (``input_values`` through
        the model's DAC encoder and over ``decoder_input_ids`` when both are given, a leading BOS column dropped), then this session's limits."""
        if input_values is None and decoder_input_ids is None:
            return None
        if self.chunk is not None and self.stream_voice is None:
            raise NotImplementedError("a voice prompt in streaming mode: the windowed codec pass reads the slot's raw ids, which hold the delay pattern "
                                      "behind the prompt; submit it to a batcher without `stream_chunk_frames`, or open this one with "
                                      "`stream_voice_prompts`")
        if input_values is not None:
            decoder_input_ids = self.model._voice_prompt_codes(torch.as_tensor(input_values))
        else:
            decoder_input_ids = torch.as_tensor(decoder_input_ids)
            if decoder_input_ids.dim() != 2 or decoder_input_ids.shape[0] != self.K:
                raise ValueError(f"decoder_input_ids: one request at a time, [{self.K} codebooks, frames]; got {tuple(decoder_input_ids.shape)}")
        codes = self.model._voice_prompt_rows(decoder_input_ids)
        if codes.shape[0] != self.K:
            raise ValueError(f"voice prompt: one request at a time, [{self.K} codebooks, frames]; got {tuple(codes.shape)}")
        T = int(codes.shape[1])
        if T > self.max_voice_frames:
            raise ValueError(f"voice prompt of {T} frames, the session was opened for {self.max_voice_frames} (`max_voice_frames`)")
        return codes.contiguous() if T > 0 else None

    # -- scheduler ----------------------------------------------------------------------------------------------------------------
    def pending(self) -> int:
        """Requests queued or in a slot (finished ones waiting to be iterated are not counted)."""
        return len(self._queue) + sum(r is not None for r in self._slot)

    def _admit(self):
        """The one admission path of both modes. Idle slots in ascending order meet the queue in FIFO order; the pairs are cut into groups of
        at most ``max(spare, 1)``, a request with a voice prompt going alone - or, with ``admit_voice_groups``, a group holding requests of one
        kind only, with a prompt or without. A group of one is one ``admit_row``, a larger one ONE prefill pass (``admit_rows``, with ``voices=``
        for a group with prompts); behind each group its slots' stream tables are reset (streaming mode). A request
        leaves the queue immediately before the engine call that admits it: if that call raises, the requests behind it are still queued."""
        groups = []
        for s, r in zip((s for s in range(self.slots) if self._slot[s] is None), self._queue):
            full = not groups or len(groups[-1]) == max(self.spare, 1)
            if full or self._ends_group(groups[-1][0][1], r):
                groups.append([])
            groups[-1].append((s, r))
        for group in groups:
            for s, r in group:  # the record each slot's admission runs under, its first token included (retire_row put the session's back)
                if r.pen is not None:
                    self.eng.set_slot_history_penalty(s, *r.pen)
                if r.warp is not None:
                    self.eng.set_slot_sample_warp(s, *r.warp)
                if r.edits is not None:
                    self.eng.set_slot_logit_edits(s, r.edits)
                if any(r.want_records):  # the slot's own buffers, set before the admission: its first-token tail is step 0
                    cap = r.max_length - 1 - r.T
                    r.records = {kind: torch.empty([cap, self.K, self.V], dtype=torch.float32, device=self.model.device)
                                 for kind, on in zip(("scores", "logits"), r.want_records) if on}
                    self.eng.set_slot_step_records(s, r.records.get("scores"), r.records.get("logits"), cap)
            reqs = [self._queue.popleft() for _ in group]
            if len(reqs) == 1:
                (s, r), = group
                # a request without a record or a prompt of its own goes through the same call as ever (no `gen`, no `voice` keyword)
                kw = {} if r.gen is None else {"gen": dict(r.gen)}
                if r.voice is not None:
                    kw["voice"] = r.voice
                self.eng.admit_row(s, r.enc, r.enc_mask, r.prompt, r.prompt_mask, max_length=r.max_length, sample=True, **kw)
            else:
                stack = lambda ts: None if ts[0] is None else torch.stack(ts)
                gens = None if all(r.gen is None for r in reqs) else [None if r.gen is None else dict(r.gen) for r in reqs]
                self.eng.admit_rows([s for s, _ in group], stack([r.enc for r in reqs]), stack([r.enc_mask for r in reqs]), stack([r.prompt for r in reqs]),
                                    stack([r.prompt_mask for r in reqs]), max_lengths=[r.max_length for r in reqs], sample=True, gens=gens,
                                    **({} if reqs[0].voice is None else {"voices": [r.voice for r in reqs]}))  # no keyword for a plain group
                self.admission_groups.append(len(group))
            self.admissions += len(group)
            for s, r in group:
                self._slot[s], r.cols = r, 2 + r.T  # BOS + the given columns + the first token
                if self.chunk is not None:  # a prompt comes only with stream_voice_prompts: submit refuses it otherwise
                    voice = {} if r.voice is None else {"voice": r.voice, "emit_prompt": self.stream_voice == "emit"}
                    self.model.audio_encoder.stream_reset(s, **voice)

    def _ends_group(self, first: _Request, r: _Request) -> bool:
        """Whether `r` may not join the group that `first` opened: a voice prompt on either side - or, with ``admit_voice_groups``, on one side only."""
        if self.voice_groups:
            return (first.voice is None) != (r.voice is None)
        return first.voice is not None or r.voice is not None

    def _retire(self, s: int):
        self.eng.retire_row(s)
        self._slot[s] = None

    def _poll(self):
        """Admit, run the live slots up to the next boundary, hand out what is ready. The boundary: ``poll_steps``, or the nearest end by
        max_length - the host knows it and meets it exactly, so that its slot is refilled at once; EOS ends show at a poll - or, streaming,
        the nearest first chunk. Streaming then lists every slot that has a chunk ready or has finished for ONE codec pass."""
        self._admit()
        busy = [(s, r) for s, r in enumerate(self._slot) if r is not None]
        if not busy:
            return
        n = min(min(r.max_length - r.cols for _, r in busy), self.poll_steps)
        if self.chunk is not None:
            for _, r in busy:
                f = self._first_chunk_steps(r)
                if f is not None and f >= 1:
                    n = min(n, f)
                elif f is not None and r.voice is not None:
                    n = 0  # the prompt alone holds the first chunk: the codec pass comes before any further step
        if n > 0:
            self.eng.decode_steps(n)
            for _, r in busy:
                r.cols = min(r.cols + n, r.max_length)
        cur, live = self.eng.row_state()
        if self.chunk is None:
            whole = [(s, r) for s, r in busy if not live[s]]  # what finished at one poll is decoded whole, as one ragged batch
        else:
            rows, whole = self._stream_rows(busy, cur, live)
            while rows:  # more than once only under stream_voice_prompts: a finished slot that had more than max_emit frames ready is drained here
                rows = self._codec_pass(rows)
        group = [(r, self.eng.row_ids(s, cur[s])) for s, r in whole]
        for s, r in busy:
            if not live[s]:
                if r.records is not None:  # steps made = the slot's final clock - its given columns
                    steps = max(0, min(int(cur[s]), r.max_length) - 1 - r.T)
                    self._records[r.ticket] = {kind: buf[:steps] for kind, buf in r.records.items()}
                    r.records = None
                self._retire(s)
        if group:
            self._decode_group(group)
            if self.chunk is not None:
                self._whole_to_chunks(group)

    # -- streaming ----------------------------------------------------------------------------------------------------------------
    def _streams(self, r: _Request, cur: int) -> bool:
        """Whether r's frames can be named yet: below 2K - 1 columns build_delay_pattern_mask applies no pattern at all, and `cur` alone
        cannot tell which un-delay the finished request will get; a request whose max_length is below 2K - 1 never gets the pattern."""
        return r.max_length >= 2 * self.K - 1 and cur >= 2 * self.K - 1

    def _want(self, r: _Request) -> int:
        return self.first_chunk if r.first_out else self.chunk

    def _first_chunk_steps(self, r: _Request) -> Optional[int]:
        """Steps until r, whose first chunk is outstanding, can have it (no frame dropped from here on): kept + new raw frames - emitted
        - halo >= first_chunk with complete = columns - K, i.e. first_chunk + halo + K columns on a clean request."""
        if not r.first_out or r.max_length < 2 * self.K - 1:
            return None
        need = self.first_chunk + self.halo - (r.kept - r.emitted)  # raw frames still to absorb
        # the frames of a prompt that is not emitted do not count. A prompt that is emitted may hold the first chunk at admission: <= 0 then
        cols = max(2 * self.K - 1, max(r.absorbed, r.skipped) + need + self.K)
        return cols - r.cols

    def _stream_rows(self, busy, cur, live):
        """The rows ``(slot, complete, final, min_emit)`` of this poll's codec pass - a finished slot, and a live one that by the host's count
        has a chunk ready - and the ``(slot, request)`` pairs that ended below 2K - 1 columns: those go the whole-utterance way."""
        rows, whole = [], []
        for s, r in busy:
            done = not live[s]
            if not self._streams(r, cur[s]):
                if done:
                    whole.append((s, r))
                continue
            complete = min(cur[s], r.max_length) - self.K
            if done:
                rows.append((s, complete, 1, 0))
            elif r.kept + r.new_raw(complete) - r.emitted - self.halo >= self._want(r):
                rows.append((s, complete, 0, self._want(r)))
        return rows, whole

    def _codec_pass(self, rows):
        """ONE windowed codec pass over ``rows``: the requests' counts follow the pass's ``(emit, kept)`` pairs and the chunks go to ``_out``.
        Returns the rows to list again: final ones that a capped pass has not flushed yet."""
        ptr, ld = self.eng.ids_buffer()
        cap = {} if self.stream_voice is None else {"max_emit": self.max_emit}
        wave, out = self.model.audio_encoder.stream_decode(ptr, ld, rows, self.halo, col0=1, delay=1, **cap)
        self.codec_passes += 1
        self.codec_rows += len(rows)
        hop = self.model._codec_hop()
        pairs = out.tolist()  # the pass's one host read: (emit, kept) per row
        again = []
        for i, (s, complete, final, _) in enumerate(rows):
            r, emit, kept = self._slot[s], int(pairs[i][0]), int(pairs[i][1])
            pk = r.prompt_kept
            if pk is not None:  # the kept frames of a skipped prompt count as emitted when they are absorbed
                r.emitted += pk[min(len(pk) - 1, complete)] - pk[min(len(pk) - 1, r.absorbed)]
            r.absorbed, r.kept = complete, kept
            r.emitted += emit
            flushed = bool(final) and r.emitted >= kept  # a capped final pass may leave frames behind
            if final and not flushed:
                if emit == 0:
                    raise RuntimeError(f"stream table of slot {s}: {kept - r.emitted} frames left and none emitted")
                again.append(rows[i])
            if emit > 0:
                self._out.append((r.ticket, wave[i, : emit * hop].clone(), flushed))
                r.first_out = False
            elif final:  # nothing left to flush: the flag alone, or the reference's torch.zeros(1) for a request without any valid frame (:3641)
                self._out.append((r.ticket, torch.zeros(1 if r.emitted == 0 else 0, device=wave.device), True))
        return again

    def _whole_to_chunks(self, group):
        """The requests that ended below 2K - 1 columns went through the un-delay + filtered decode of the other mode (``_decode_group``):
        each waveform leaves as one last chunk."""
        self.whole_requests += len(group)
        # stream_voice_prompts="skip": the samples of the prompt's kept frames are dropped here, on the host
        drop = {r.ticket: self._whole_prompt_kept(r, ids) * self.model._codec_hop() for r, ids in group if r.prompt_kept is not None}
        while self._done:  # a streaming batcher keeps nothing else there
            t, w, _ = self._done.pop()
            self._out.append((t, w[drop[t]:] if drop.get(t) else w, True))

    def _valid_frames(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [K, frames] -> bool [frames]: the frames whose ids all lie in [0, codebook_size), the ones the special-id filter keeps."""
        cb = int(self.model.audio_encoder.config.codebook_size)
        return ((codes >= 0) & (codes < cb)).all(dim=0)

    def _whole_prompt_kept(self, r: _Request, ids: torch.Tensor) -> int:
        """Frames of r's prompt in the waveform of the whole-utterance path (a request that ended below 2K - 1 columns): there `_codes` strips
        nothing, a frame is a column, and the prompt's frames are columns 1 .. T (un-shifted where the request's max_length is below 2K - 1)."""
        return int(self._valid_frames(self._codes(ids, r.max_length, r.voice)[:, 1: 1 + r.T]).sum())

    def _drain(self, out: Deque):
        """Hands out what is in ``out`` (``_done`` or ``_out``: where the mode's polls put their results) until nothing is queued or running."""
        with torch.no_grad():
            while out or self.pending():
                if not out:
                    self._poll()
                while out:
                    yield out.popleft()

    def chunks(self) -> Iterator[Tuple[int, torch.Tensor, bool]]:
        """Streaming mode: yields (ticket, chunk, last) in the order chunks become available, until nothing is queued or running. The chunks of
        a ticket concatenate to the waveform the non-streaming mode yields for the same request; ``last`` is True exactly once per ticket."""
        if self.chunk is None:
            raise RuntimeError("chunks() needs streaming mode: construct the batcher with `stream_chunk_frames`")
        yield from self._drain(self._out)

    def cancel(self, ticket: int) -> bool:
        """Drops a request: a queued one leaves the queue, one in a slot is retired (``ptts_retire_row``: the slot is idle for the next
        admission), and nothing of it that is waiting to be handed out follows. False if the ticket is unknown or already finished."""
        queued = [r for r in self._queue if r.ticket == ticket]
        for r in queued:
            self._queue.remove(r)
        running = [s for s, r in enumerate(self._slot) if r is not None and r.ticket == ticket]
        for s in running:
            self._slot[s].records = None  # the slot's buffers go with it (retire_row clears the engine's record)
            self._retire(s)
        if queued or running:
            out = self._done if self.chunk is None else self._out  # in place: a generator of _drain holds on to it
            rest = [x for x in out if x[0] != ticket]
            out.clear()
            out.extend(rest)
        return bool(queued or running)

    def _codes(self, ids: torch.Tensor, max_length: int, voice: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Raw ids [K, columns] of one request -> its un-delayed audio codes [K, frames] (generate()'s tail, modeling_parler_tts.py:3585-3600).
        ``voice``: the request's voice prompt; the pattern is then built over BOS + prefix, as generate() builds it (:3523-3530), and the
        prompt's frames are part of the codes."""
        bos_col = ids[:, :1]
        given = bos_col if voice is None else torch.cat([bos_col, voice.to(ids.device)], dim=-1)
        _, pattern = build_delay_pattern_mask(given, self.bos, self.pad, max_length, self.K)
        out = apply_delay_pattern_mask(ids, pattern)
        _, m2 = build_delay_pattern_mask(bos_col, self.bos, self.pad, out.shape[1], self.K)
        keep = (m2 != self.bos) & (m2 != self.pad)
        return out[keep].reshape(self.K, -1)

    def _decode_group(self, group):
        """The requests that finished at the same poll go through the codec as ONE ragged batch (special-id filter + ragged decode); the shorter
        ones are padded with an id outside the codebook, which the filter drops like any special id."""
        codes = [self._codes(ids, r.max_length, r.voice) for r, ids in group]
        T = max(int(c.shape[1]) for c in codes)
        if T == 0:
            for r, _ in group:
                self._done.append((r.ticket, torch.zeros(1, device=codes[0].device), 1))  # the reference's torch.zeros(1) for no valid frame (:3641)
            return
        cb = int(self.model.audio_encoder.config.codebook_size)
        batch = torch.full((len(group), self.K, T), cb, dtype=torch.long, device=codes[0].device)
        for i, c in enumerate(codes):
            batch[i, :, : c.shape[1]] = c
        wav, frames = self.model.audio_encoder.decode_filtered(batch[None])
        hop = wav.shape[-1] // T
        kept = [int(x) for x in frames.tolist()]  # the one host read of the group: its kept-frame counts
        for i, (r, _) in enumerate(group):
            n = kept[i]
            if n > 0:
                self._done.append((r.ticket, wav[i, 0, : n * hop].clone(), n * hop))
            else:
                self._done.append((r.ticket, torch.zeros(1, device=wav.device), 1))

    def __iter__(self) -> Iterator[Tuple[int, torch.Tensor, int]]:
        """Yields (ticket, waveform, length) in the order requests finish, until nothing is queued or running."""
        if self.chunk is not None:
            raise RuntimeError("this batcher streams (`stream_chunk_frames`): iterate chunks() instead")
        yield from self._drain(self._done)

    def run(self, requests: Iterable[Dict]) -> List[Tuple[torch.Tensor, int]]:
        """``requests``: the keyword arguments of ``submit``, one dict per request. Returns (waveform, length) per request, in submission order."""
        tickets = [self.submit(**r) for r in requests]
        got = {t: (w, n) for t, w, n in self}
        return [got[t] for t in tickets]

    def close(self):
        """Retires every slot and drops the queue (the engine stays with the model; a later ``generate()`` ends the session by itself)."""
        self._queue.clear()
        for s in range(self.slots):
            if self._slot[s] is not None:
                self._retire(s)
        self._records.clear()  # step records nobody read
