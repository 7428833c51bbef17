"""Thin Python owners of the two native engines (libptts_hip.so). torch is used only for device memory,
streams and dtype plumbing: every FLOP of the hot path runs in the HIP library. No CPU fallback exists.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import _native as N
from .quant import is_fp8_matrix


def _stream_ptr(stream: Optional["torch.cuda.Stream"] = None, device=None) -> C.c_void_p:
    """Handle of the CURRENT stream of `device` (the engine's device, not torch's current device: a stream belongs to
    the device it was created on)."""
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return C.c_void_p(s.cuda_stream)


def _shape_arr(t: torch.Tensor):
    return (C.c_int64 * t.dim())(*t.shape)


def rope_tables(head_dim: int, theta: float, num_positions: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 cos/sin exactly as ParlerTTSRotaryEmbedding.forward builds them (modeling_parler_tts.py:373-406):
    inv_freq = theta^(-2i/d), freqs = inv_freq ⊗ position (fp32 matmul), emb = cat(freqs, freqs)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    pos = torch.arange(num_positions, dtype=torch.int64).float()
    freqs = (inv_freq[:, None] @ pos[None, :]).transpose(0, 1)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().contiguous(), emb.sin().contiguous()


class DecoderEngine:
    """Owner of a ``ptts_engine``: the autoregressive ParlerTTSDecoder step + sampler on MI355X."""

    def __init__(self, *, hidden_size: int, num_layers: int, num_heads: int, ffn_dim: int, num_codebooks: int,
                 vocab_size: int, max_positions: int, rope: bool = False, rope_theta: float = 10000.0,
                 pad_token_id: int = 1024, eos_token_id: int = 1024, bos_token_id: int = 1025,
                 dtype: torch.dtype = torch.bfloat16, max_batch: int = 1, max_ctx: int = 2700, max_enc: int = 256,
                 max_prompt: int = 128, device: Optional[torch.device] = None, num_kv_heads: int = 0, num_cross_kv_heads: int = 0,
                 weights_fp8: bool = False, kv_fp8: bool = False):
        if not torch.cuda.is_available():
            raise N.NativeLibraryError("DecoderEngine needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.lib = N.load_library()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"engine dtype must be float32 or bfloat16, got {dtype}")
        self.dtype = dtype
        self.K, self.V, self.H = num_codebooks, vocab_size, hidden_size
        self.rope, self.rope_theta, self.max_positions = rope, rope_theta, max_positions
        self.cfg = N.PttsConfig(hidden_size, num_layers, num_heads, ffn_dim, num_codebooks, vocab_size, max_positions, int(rope),
                                float(rope_theta), pad_token_id, eos_token_id, bos_token_id,
                                N.PTTS_BF16 if dtype == torch.bfloat16 else N.PTTS_F32, max_batch, max_ctx, max_enc, max_prompt,
                                self.device.index or 0, int(num_kv_heads or 0), int(num_cross_kv_heads or 0), int(bool(weights_fp8)), int(bool(kv_fp8)))
        self.weights_fp8 = bool(weights_fp8)
        self.kv_fp8 = bool(kv_fp8)
        if self.weights_fp8 and dtype != torch.bfloat16:
            raise ValueError("weights_fp8 needs the bfloat16 engine (e4m3 weights, bf16 activations)")
        self._h = C.c_void_p()
        N.check(self.lib.ptts_engine_create(C.byref(self.cfg), C.byref(self._h)), "ptts_engine_create")
        self.B = 0
        self.history_penalty = None  # (repetition_penalty, no_repeat_ngram_size) while the device node is on (set_history_penalty)
        self.sample_warp = None  # (min_p, typical_p, epsilon_cutoff, eta_cutoff) while the tail's WARP instances are on (set_sample_warp)
        self.logit_edits = None  # the engine-wide generation_extras.LogitEdits while the logit-edit node is on (set_logit_edits)
        self.step_records = None  # (scores, logits, cap_steps) while step records are on (set_step_records): the arenas of the next static call
        self._slot_records = {}  # slot -> (scores, logits) of set_slot_step_records: the engine writes into them until the slot is retired

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.ptts_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights ---------------------------------------------------------------------------------------
    def load_weight(self, name: str, tensor: torch.Tensor):
        t = tensor.detach()
        if t.dtype not in (torch.float32, torch.bfloat16):
            t = t.float()
        t = t.to(self.device).contiguous()
        dt = N.PTTS_BF16 if t.dtype == torch.bfloat16 else N.PTTS_F32
        N.check(self.lib.ptts_load_weight(self._h, name.encode(), C.c_void_p(t.data_ptr()), dt, _shape_arr(t), t.dim(), _stream_ptr(device=self.device)),
                f"ptts_load_weight({name})")
        # the engine re-packs asynchronously on the current stream; keep `t` alive until then
        torch.cuda.current_stream(self.device).synchronize()

    def load_weight_fp8(self, name: str, tensor: torch.Tensor):
        """weights_fp8 engines: quantise one projection matrix (``quant.quantize_rows_e4m3``), hand the exact dequantisation to
        the ordinary loader (MFMA-packed bf16 copy for prefill / batch > 4) and the e4m3 bytes + row scales to the GEMV step."""
        from .quant import quantize_rows_e4m3

        q, scale, deq = quantize_rows_e4m3(tensor.detach().to(self.device))
        self.load_weight(name, deq)
        q, scale = q.contiguous(), scale.contiguous()
        N.check(self.lib.ptts_load_weight_fp8(self._h, name.encode(), C.c_void_p(q.data_ptr()), C.c_void_p(scale.data_ptr()), _shape_arr(q), 2,
                                              _stream_ptr(device=self.device)), f"ptts_load_weight_fp8({name})")
        torch.cuda.current_stream(self.device).synchronize()

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = ""):
        """Accepts the reference's decoder state-dict names, optionally under `prefix`
        (e.g. ``"decoder."`` for a ParlerTTSForConditionalGeneration checkpoint)."""
        for k, v in sd.items():
            if not k.startswith(prefix):
                continue
            name = k[len(prefix):]
            if name.startswith("model.decoder.") or name.startswith("lm_heads."):
                if "rotary_emb" in name:
                    continue
                if self.weights_fp8 and name == "lm_heads.weight":  # fused heads (:1834-1840): quantise per codebook slice
                    for k in range(self.K):
                        self.load_weight_fp8(f"lm_heads.{k}.weight", v[k * self.V:(k + 1) * self.V])
                elif self.weights_fp8 and is_fp8_matrix(name):
                    self.load_weight_fp8(name, v)
                else:
                    self.load_weight(name, v)
        if self.rope:
            cos, sin = rope_tables(self.H // self.cfg.num_heads, self.rope_theta, max(self.max_positions, self.cfg.max_ctx))  # RoPE has no position limit (:373-406)
            self.load_weight("rope_cos", cos)
            self.load_weight("rope_sin", sin)
        N.check(self.lib.ptts_weights_ready(self._h), "ptts_weights_ready")

    # -- generation -------------------------------------------------------------------------------------
    def set_gen_params(self, *, max_length: int, min_new_tokens: int = 0, do_sample: bool = False, temperature: float = 1.0,
                       top_k: int = 0, top_p: float = 1.0, use_eos_gate: bool = True, seed: int = 0):
        gp = N.PttsGenParams(int(max_length), int(min_new_tokens), int(bool(do_sample)), float(temperature), int(top_k or 0), float(top_p),
                             int(bool(use_eos_gate)), int(seed) & (2 ** 64 - 1))
        N.check(self.lib.ptts_set_gen_params(self._h, C.byref(gp)), "ptts_set_gen_params")
        self.max_length = int(max_length)

    @staticmethod
    def _history_penalty(repetition_penalty, no_repeat_ngram_size):
        """The two options as a ``ptts_history_penalty`` (``None`` = the neutral value of that option); ``ValueError`` on values out of range."""
        p = 1.0 if repetition_penalty is None else float(repetition_penalty)
        n = 0 if no_repeat_ngram_size is None else int(no_repeat_ngram_size)
        if not (math.isfinite(p) and p > 0.0):
            raise ValueError(f"`repetition_penalty` must be a finite number > 0, got {repetition_penalty}")
        if n < 0 or (no_repeat_ngram_size is not None and n != no_repeat_ngram_size):
            raise ValueError(f"`no_repeat_ngram_size` must be an integer >= 0, got {no_repeat_ngram_size}")
        return N.PttsHistoryPenalty(p, n)

    def set_history_penalty(self, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None, enabled: bool = True):
        """transformers' ``repetition_penalty`` / ``no_repeat_ngram_size`` on the device (``ptts_set_history_penalty``): one kernel node in
        front of every sampler tail from the next ``prefill`` / ``begin_session`` on, with these values for every utterance (a session: for
        every request that brings none of its own). Neutral values (the defaults) keep the node and change no logit: how a session is
        opened when only some requests will bring penalties. ``enabled=False`` switches the node off (the state of a new engine).
        ``ValueError`` inside a session that holds a request."""
        if not enabled:
            N.check(self.lib.ptts_set_history_penalty(self._h, None, _stream_ptr(device=self.device)), "ptts_set_history_penalty")
            self.history_penalty = None
            return
        hp = self._history_penalty(repetition_penalty, no_repeat_ngram_size)
        N.check(self.lib.ptts_set_history_penalty(self._h, C.byref(hp), _stream_ptr(device=self.device)), "ptts_set_history_penalty")
        self.history_penalty = (float(hp.repetition_penalty), int(hp.no_repeat_ngram_size))

    def set_slot_history_penalty(self, slot: int, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                                 default: bool = False):
        """The record the next admission into the idle slot ``slot`` runs under (``ptts_set_slot_history_penalty``), its first token
        included; ``default=True`` restores the session's values, as ``retire_row`` does. Only in a session begun with the node on."""
        hp = None if default else self._history_penalty(repetition_penalty, no_repeat_ngram_size)
        N.check(self.lib.ptts_set_slot_history_penalty(self._h, int(slot), None if hp is None else C.byref(hp), _stream_ptr(device=self.device)),
                "ptts_set_slot_history_penalty")

    @staticmethod
    def _sample_warp(min_p, typical_p, epsilon_cutoff, eta_cutoff):
        """The four options as a ``ptts_sample_warp`` (``None`` = the neutral value of that option); ``ValueError`` on values out of range."""
        def number(name, v, neutral):
            if v is None:
                return neutral
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"`{name}` must be a number, got {v!r}") from None
            return f

        m, t = number("min_p", min_p, 0.0), number("typical_p", typical_p, 1.0)
        e, h = number("epsilon_cutoff", epsilon_cutoff, 0.0), number("eta_cutoff", eta_cutoff, 0.0)
        if not (math.isfinite(m) and 0.0 <= m <= 1.0):
            raise ValueError(f"`min_p` must lie in [0, 1], got {min_p}")
        if not (math.isfinite(t) and 0.0 < t <= 1.0):
            raise ValueError(f"`typical_p` must lie in (0, 1], got {typical_p}")
        if not (math.isfinite(e) and 0.0 <= e < 1.0):
            raise ValueError(f"`epsilon_cutoff` must lie in [0, 1), got {epsilon_cutoff}")
        if not (math.isfinite(h) and 0.0 <= h < 1.0):
            raise ValueError(f"`eta_cutoff` must lie in [0, 1), got {eta_cutoff}")
        return N.PttsSampleWarp(m, t, e, h)

    def set_sample_warp(self, min_p: Optional[float] = None, typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None,
                        eta_cutoff: Optional[float] = None, enabled: bool = True):
        """transformers' ``min_p`` / ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff`` on the device (``ptts_set_sample_warp``): from the next
        ``prefill`` / ``begin_session`` on every sampler tail is the instance that applies them behind top-p, with these values for every
        utterance (a session: for every request that brings none of its own). Neutral values (the defaults) change no draw: how a session is
        opened when only some requests will bring warpers. ``enabled=False`` switches the instances off (the state of a new engine).
        ``ValueError`` inside a session that holds a request."""
        if not enabled:
            N.check(self.lib.ptts_set_sample_warp(self._h, None, _stream_ptr(device=self.device)), "ptts_set_sample_warp")
            self.sample_warp = None
            return
        w = self._sample_warp(min_p, typical_p, epsilon_cutoff, eta_cutoff)
        N.check(self.lib.ptts_set_sample_warp(self._h, C.byref(w), _stream_ptr(device=self.device)), "ptts_set_sample_warp")
        self.sample_warp = (float(w.min_p), float(w.typical_p), float(w.epsilon_cutoff), float(w.eta_cutoff))

    def set_slot_sample_warp(self, slot: int, min_p: Optional[float] = None, typical_p: Optional[float] = None,
                             epsilon_cutoff: Optional[float] = None, eta_cutoff: Optional[float] = None, default: bool = False):
        """The record the next admission into the idle slot ``slot`` runs under (``ptts_set_slot_sample_warp``), its first token included;
        ``default=True`` restores the session's values, as ``retire_row`` does. Only in a session begun with the instances on."""
        w = None if default else self._sample_warp(min_p, typical_p, epsilon_cutoff, eta_cutoff)
        N.check(self.lib.ptts_set_slot_sample_warp(self._h, int(slot), None if w is None else C.byref(w), _stream_ptr(device=self.device)),
                "ptts_set_slot_sample_warp")

    @staticmethod
    def _logit_edits(edits):
        """A ``generation_extras.LogitEdits`` (``None``: the neutral record) as a ``ptts_logit_edits`` and the arrays it points to, which the
        caller keeps alive over the call."""
        from .generation_extras import LogitEdits

        ed = LogitEdits() if edits is None else edits
        I32 = C.c_int32
        arrays = [(I32 * len(ed.bias))(*[t for t, _ in ed.bias]), (C.c_float * len(ed.bias))(*[b for _, b in ed.bias]), (I32 * len(ed.bad))(*ed.bad),
                  (I32 * max(len(ed.suppress), 1))(*ed.suppress), (I32 * max(len(ed.begin_suppress), 1))(*ed.begin_suppress)]
        # a suppress list none of whose tokens lies in the vocabulary is still a stage: one token outside it, which the library ignores
        n_sup = len(ed.suppress) or (1 if ed.suppress_on else 0)
        n_beg = len(ed.begin_suppress) or (1 if ed.begin_suppress_on else 0)
        if not ed.suppress:
            arrays[3][0] = -1
        if not ed.begin_suppress:
            arrays[4][0] = -1
        start, factor = ed.decay if ed.decay is not None else (0, 1.0)
        rec = N.PttsLogitEdits(C.cast(arrays[0], C.POINTER(I32)), C.cast(arrays[1], C.POINTER(C.c_float)), C.cast(arrays[2], C.POINTER(I32)),
                               C.cast(arrays[3], C.POINTER(I32)), C.cast(arrays[4], C.POINTER(I32)), len(ed.bias), len(ed.bad), n_sup, n_beg,
                               int(ed.decay is not None), int(start), float(factor))
        return rec, arrays

    def set_logit_edits(self, edits=None, enabled: bool = True):
        """transformers' ``sequence_bias`` / ``bad_words_ids`` (single-token keys), ``exponential_decay_length_penalty``, ``suppress_tokens`` and
        ``begin_suppress_tokens`` on the device (``ptts_set_logit_edits``): one kernel node between the history-penalty node and every sampler
        tail from the next ``prefill`` / ``begin_session`` on, with ``edits`` (a ``generation_extras.LogitEdits``) for every utterance (a
        session: for every request that brings none of its own). ``None`` is the neutral record: the node is there and changes no logit, how a
        session is opened when only some requests will bring edits. ``enabled=False`` switches the node off (the state of a new engine).
        ``ValueError`` inside a session that holds a request."""
        if not enabled:
            N.check(self.lib.ptts_set_logit_edits(self._h, None, _stream_ptr(device=self.device)), "ptts_set_logit_edits")
            self.logit_edits = None
            return
        rec, keep = self._logit_edits(edits)
        N.check(self.lib.ptts_set_logit_edits(self._h, C.byref(rec), _stream_ptr(device=self.device)), "ptts_set_logit_edits")
        del keep
        from .generation_extras import LogitEdits

        self.logit_edits = LogitEdits() if edits is None else edits

    def set_slot_logit_edits(self, slot: int, edits=None, default: bool = False):
        """The record the next admission into the idle slot ``slot`` runs under (``ptts_set_slot_logit_edits``), its first token included;
        ``default=True`` restores the session's record, as ``retire_row`` does. Only in a session begun with the node on."""
        rec, keep = (None, None) if default else self._logit_edits(edits)
        N.check(self.lib.ptts_set_slot_logit_edits(self._h, int(slot), None if rec is None else C.byref(rec), _stream_ptr(device=self.device)),
                "ptts_set_slot_logit_edits")
        del keep

    def _step_records(self, scores, logits, cap_steps, lead):
        """The two arenas as a ``ptts_step_records``; each fp32, contiguous, on the engine's device, with room for ``cap_steps`` records of
        ``lead`` (a number of [K, V] blocks per step; ``None``: not checked, the batch is not known yet)."""
        for name, t in (("scores", scores), ("logits", logits)):
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"step records: `{name}` must be a contiguous float32 tensor on {self.device}")
            if lead is not None and t.numel() < int(cap_steps) * lead * self.K * self.V:
                raise ValueError(f"step records: `{name}` holds {t.numel()} values, {cap_steps} steps of {lead} x {self.K} x {self.V} need more")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()
        return N.PttsStepRecords(ptr(scores), ptr(logits), int(cap_steps))

    def set_step_records(self, scores: Optional[torch.Tensor] = None, logits: Optional[torch.Tensor] = None, cap_steps: int = 0, enabled: bool = True):
        """transformers' ``output_scores`` / ``output_logits`` on the device (``ptts_set_step_records``): from the next ``prefill`` on, step i of
        the call writes its processed scores into ``scores[i]`` and the raw logits of the heads into ``logits[i]`` - fp32 arenas
        ``[cap_steps, B*K, V]`` the caller allocates for that call's batch; ``None`` leaves a kind out. Both ``None`` with ``cap_steps=0`` is how a
        session is opened whose requests may bring records (``set_slot_step_records``). ``enabled=False`` switches the feature off (the state of
        a new engine). The engine holds a reference to the tensors until the next call of this function. ``ValueError`` inside a session that
        holds a request."""
        if not enabled:
            N.check(self.lib.ptts_set_step_records(self._h, None, _stream_ptr(device=self.device)), "ptts_set_step_records")
            self.step_records = None
            self._slot_records = {}
            return
        rec = self._step_records(scores, logits, cap_steps, None)
        N.check(self.lib.ptts_set_step_records(self._h, C.byref(rec), _stream_ptr(device=self.device)), "ptts_set_step_records")
        self.step_records = (scores, logits, int(cap_steps))

    def set_slot_step_records(self, slot: int, scores: Optional[torch.Tensor] = None, logits: Optional[torch.Tensor] = None, cap_steps: int = 0,
                              default: bool = False):
        """The record of the next admission into the idle slot ``slot`` (``ptts_set_slot_step_records``): fp32 ``[cap_steps, K, V]`` each, the
        admission's own first token is step 0. ``default=True`` clears it, as ``retire_row`` does. Only in a session begun with step records on.
        The engine holds a reference to the tensors until the slot's record is set again or the slot is retired."""
        rec = None if default else self._step_records(scores, logits, cap_steps, 1)
        N.check(self.lib.ptts_set_slot_step_records(self._h, int(slot), None if rec is None else C.byref(rec), _stream_ptr(device=self.device)),
                "ptts_set_slot_step_records")
        if default:
            self._slot_records.pop(int(slot), None)
        else:
            self._slot_records[int(slot)] = (scores, logits)

    def prefill(self, enc: torch.Tensor, enc_mask: Optional[torch.Tensor], prompt: Optional[torch.Tensor],
                prompt_mask: Optional[torch.Tensor], sample: bool = True):
        enc = enc.to(self.device, torch.float32).contiguous()
        B, Nn, H = enc.shape
        if H != self.H:
            raise ValueError(f"encoder_hidden_states width {H} != decoder hidden_size {self.H}")
        P = 0
        keep = [enc]
        pm = em = pr = None
        if prompt is not None and prompt.shape[1] > 0:
            pr = prompt.to(self.device, torch.float32).contiguous()
            P = pr.shape[1]
            keep.append(pr)
        if enc_mask is not None:
            em = enc_mask.to(self.device, torch.int32).contiguous()
            keep.append(em)
        if prompt_mask is not None and P > 0:
            pm = prompt_mask.to(self.device, torch.int32).contiguous()
            keep.append(pm)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()
        if getattr(self, "step_records", None) is not None:  # the batch is known now: the arenas of set_step_records must hold cap_steps x B x K x V
            scores, logits, cap = self.step_records
            self._step_records(scores, logits, cap, B)
        N.check(self.lib.ptts_prefill(self._h, ptr(enc), ptr(em), ptr(pr), ptr(pm), B, Nn, P, int(sample), _stream_ptr(device=self.device)), "ptts_prefill")
        self.B, self.P = B, P
        self._keep = keep  # inputs are consumed asynchronously by the enqueued kernels

    def score(self, enc: torch.Tensor, enc_mask: Optional[torch.Tensor], prompt: Optional[torch.Tensor], prompt_mask: Optional[torch.Tensor],
              input_ids: torch.Tensor, labels: Optional[torch.Tensor] = None, return_logits: bool = False):
        """One teacher-forced forward over the given decoder columns (``ptts_score``): ``input_ids`` int64 [B*K, T] (or [B, K, T]) exactly as the
        model is to see them, ``labels`` int64 [B, T, K] or None. Returns ``(nll, counted, logits)`` on the device: per-token negative
        log-likelihoods fp32 [B, T, K] (0 where a position does not count), int32 [B, T, K], and fp32 logits [B*K, P + T, V] - each None when not
        asked for. Without ``return_logits`` the logits are never materialised. The engine is left un-prefilled."""
        enc = enc.to(self.device, torch.float32).contiguous()
        B, Nn, H = enc.shape
        if H != self.H:
            raise ValueError(f"encoder_hidden_states width {H} != decoder hidden_size {self.H}")
        if labels is None and not return_logits:
            raise ValueError("score needs labels, return_logits=True, or both")
        ids = input_ids.to(self.device, torch.int64)
        if ids.dim() == 3:
            ids = ids.reshape(-1, ids.shape[-1])
        if ids.dim() != 2 or ids.shape[0] != B * self.K or ids.shape[1] < 1:
            raise ValueError(f"input_ids must be [B*K, T] or [B, K, T] with B = {B}, K = {self.K}, T >= 1; got {tuple(input_ids.shape)}")
        ids = ids.contiguous()
        T = ids.shape[1]
        if bool(((ids < 0) | (ids > self.V)).any()):
            raise ValueError(f"input_ids outside the embedding tables [0, {self.V}]")
        P = 0
        pm = em = pr = lab = nll = counted = logits = None
        if prompt is not None and prompt.shape[1] > 0:
            pr = prompt.to(self.device, torch.float32).contiguous()
            P = pr.shape[1]
            if pr.shape[0] != B or pr.shape[2] != H:
                raise ValueError(f"prompt must be [{B}, P, {H}], got {tuple(pr.shape)}")
        if enc_mask is not None:
            em = enc_mask.to(self.device, torch.int32).contiguous()
        if prompt_mask is not None and P > 0:
            pm = prompt_mask.to(self.device, torch.int32).contiguous()
        if labels is not None:
            lab = labels.to(self.device, torch.int64).contiguous()
            if tuple(lab.shape) != (B, T, self.K):
                raise ValueError(f"labels must be [B, T, K] = [{B}, {T}, {self.K}], got {tuple(lab.shape)}")
            # what torch's CrossEntropyLoss refuses: a target that takes part in the loss and is no class
            takes_part = (lab != -100) & (lab != int(self.cfg.bos_token_id)) & (ids.view(B, self.K, T).transpose(1, 2) != int(self.cfg.eos_token_id))
            if bool((takes_part & ((lab < 0) | (lab >= self.V))).any()):
                raise ValueError(f"labels outside [0, {self.V}) at positions that count towards the loss")
            nll = torch.empty(B, T, self.K, dtype=torch.float32, device=self.device)
            counted = torch.empty(B, T, self.K, dtype=torch.int32, device=self.device)
        if return_logits:
            logits = torch.empty(B * self.K, P + T, self.V, dtype=torch.float32, device=self.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()
        io = N.PttsScoreIO(ptr(ids), ptr(lab), ptr(nll), ptr(counted), ptr(logits))
        N.check(self.lib.ptts_score(self._h, ptr(enc), ptr(em), ptr(pr), ptr(pm), B, Nn, P, T, C.byref(io), _stream_ptr(device=self.device)), "ptts_score")
        self.B, self.P = B, P
        self._keep = [enc, pr, em, pm, ids, lab]  # inputs are consumed asynchronously by the enqueued kernels
        return nll, counted, logits

    def first_token_sync(self):
        """Blocks until the first token of the last sampling ``prefill`` exists on the device (``ptts_first_token_sync``): the end of
        time-to-first-token; work the prefill enqueued behind the sampler tail (cross-attention fold) is not waited for."""
        N.check(self.lib.ptts_first_token_sync(self._h), "ptts_first_token_sync")

    def first_token_times(self) -> Tuple[float, float]:
        """(prefill_ms, tail_ms): GPU time of the last sampling ``prefill`` as it ran in sequence on its stream - staging + forward up to
        the sampler tail, and the tail itself (``ptts_first_token_times``; synchronises on the first-token event)."""
        pre, tail = C.c_float(), C.c_float()
        N.check(self.lib.ptts_first_token_times(self._h, C.byref(pre), C.byref(tail)), "ptts_first_token_times")
        return float(pre.value), float(tail.value)

    def graph_nodes(self) -> int:
        """Kernel nodes per decode step of the step graph captured last (``ptts_debug_graph_nodes``)."""
        n = C.c_int32()
        N.check(self.lib.ptts_debug_graph_nodes(self._h, C.byref(n)), "ptts_debug_graph_nodes")
        return int(n.value)

    def set_audio_prefix(self, codes: Optional[torch.Tensor]):
        """Voice prompt for the NEXT ``prefill``: un-delayed audio codes int64 [B, K, T] (or [B*K, T]); ``None`` clears it."""
        if codes is None or codes.shape[-1] == 0:
            N.check(self.lib.ptts_set_audio_prefix(self._h, C.c_void_p(), 1, 0, _stream_ptr(device=self.device)), "ptts_set_audio_prefix")
            return
        codes = codes.to(self.device, torch.int64).reshape(-1, codes.shape[-1]).contiguous()
        if codes.shape[0] % self.K:
            raise ValueError(f"audio prefix rows {codes.shape[0]} not a multiple of num_codebooks {self.K}")
        N.check(self.lib.ptts_set_audio_prefix(self._h, C.c_void_p(codes.data_ptr()), codes.shape[0] // self.K, codes.shape[1], _stream_ptr(device=self.device)),
                "ptts_set_audio_prefix")
        self._keep_prefix = codes

    def decode_steps(self, n: int):
        N.check(self.lib.ptts_decode_steps(self._h, int(n), _stream_ptr(device=self.device)), "ptts_decode_steps")

    def state(self) -> Tuple[int, bool]:
        cur, fin = C.c_int32(), C.c_int32()
        N.check(self.lib.ptts_state(self._h, C.byref(cur), C.byref(fin), _stream_ptr(device=self.device)), "ptts_state")
        return cur.value, bool(fin.value)

    def _copy_out(self, ptr: int, shape, dtype, row_stride: Optional[int] = None) -> torch.Tensor:
        """Device-to-device copy of engine-owned memory into a fresh torch tensor (async on the current stream)."""
        out = torch.empty(tuple(shape), dtype=dtype, device=self.device)
        esz = out.element_size()
        hip = N.hip_runtime()
        if row_stride is None or row_stride == shape[-1]:
            rc = hip.hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(ptr), C.c_size_t(out.numel() * esz), 3, _stream_ptr(device=self.device))
        else:
            rc = hip.hipMemcpy2DAsync(C.c_void_p(out.data_ptr()), C.c_size_t(shape[-1] * esz), C.c_void_p(ptr), C.c_size_t(row_stride * esz),
                                      C.c_size_t(shape[-1] * esz), C.c_size_t(shape[0]), 3, _stream_ptr(device=self.device))
        if rc != 0:
            raise N.NativeLibraryError(f"hipMemcpy(D2D) failed with code {rc}")
        return out

    def ids(self, max_cols: Optional[int] = None) -> torch.Tensor:
        """Raw ids [B*K, cur_len] (a copy), exactly what `_sample` returns before the delay mask is applied. ``max_cols`` caps the
        columns returned: a caller reading while later steps are still in flight on another stream passes the number of columns it
        KNOWS to be complete (the device-side length may already count a column whose ids are not visible yet)."""
        p, ld = C.c_void_p(), C.c_int32()
        N.check(self.lib.ptts_ids(self._h, C.byref(p), C.byref(ld)), "ptts_ids")
        cur, _ = self.state()
        if max_cols is not None:
            cur = min(cur, int(max_cols))
        return self._copy_out(p.value, (self.B * self.K, cur), torch.int64, row_stride=ld.value)

    def step_forward(self):
        N.check(self.lib.ptts_step_forward(self._h, _stream_ptr(device=self.device)), "ptts_step_forward")

    def logits(self) -> torch.Tensor:
        """fp32 [B*K, V] logits of the last forward (a copy)."""
        p = C.c_void_p()
        N.check(self.lib.ptts_logits(self._h, C.byref(p)), "ptts_logits")
        return self._copy_out(p.value, (self.B * self.K, self.V), torch.float32)

    def push_tokens(self, tokens: torch.Tensor, finished: Optional[torch.Tensor] = None):
        tk = tokens.to(self.device, torch.int64).contiguous()
        fn = finished.to(self.device, torch.int32).contiguous() if finished is not None else None
        N.check(self.lib.ptts_push_tokens(self._h, C.c_void_p(tk.data_ptr()), C.c_void_p(fn.data_ptr()) if fn is not None else C.c_void_p(),
                                          _stream_ptr(device=self.device)), "ptts_push_tokens")
        self._keep2 = (tk, fn)

    # -- continuous batching (ptts_session_begin / ptts_admit_row / ptts_row_state / ptts_retire_row) -------------
    def begin_session(self, slots: int, enc_width: int, prompt_width: int, kv_fp8: bool = False):
        """Opens a continuous session: ``slots`` utterance slots, all idle; every request is padded to ``enc_width`` description and
        ``prompt_width`` prompt positions. Generation parameters are those of the last ``set_gen_params``, for every request that brings
        none of its own (``admit_row(..., gen=...)``).
        ``kv_fp8=True`` opens it on an engine created with ``kv_fp8`` (``ptts_session_begin_kv8``; a ``ValueError`` on any other engine);
        the default (``ptts_session_begin``) refuses such an engine with ``NotImplementedError``. The session is the same either way."""
        if kv_fp8:
            N.check(self.lib.ptts_session_begin_kv8(self._h, int(slots), int(enc_width), int(prompt_width), _stream_ptr(device=self.device)),
                    "ptts_session_begin_kv8")
        else:
            N.check(self.lib.ptts_session_begin(self._h, int(slots), int(enc_width), int(prompt_width), _stream_ptr(device=self.device)), "ptts_session_begin")
        self.B, self.P, self.session_N = int(slots), int(prompt_width), int(enc_width)

    def self_kv(self, layer: int):
        """Copies of one layer's self-attention K/V arena (``ptts_debug_self_kv``; for tests): ``(k, v, kscale, vscale)``. ``k`` / ``v``
        uint8 [max_batch, kv_heads, max_ctx, row_bytes] - 64 e4m3 bytes per row on a ``kv_fp8`` engine, else the 64 engine-dtype values
        of the row as bytes; ``kscale`` / ``vscale`` float32 [max_batch, kv_heads, max_ctx] on a ``kv_fp8`` engine, else ``None``."""
        k, v, ks, vs = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        rb, nkv, cap = C.c_int32(), C.c_int32(), C.c_int32()
        N.check(self.lib.ptts_debug_self_kv(self._h, int(layer), C.byref(k), C.byref(v), C.byref(ks), C.byref(vs), C.byref(rb), C.byref(nkv),
                                            C.byref(cap)), "ptts_debug_self_kv")
        shape = (self.cfg.max_batch, nkv.value, cap.value)
        rows = [self._copy_out(p.value, shape + (rb.value,), torch.uint8) for p in (k, v)]
        scales = [self._copy_out(p.value, shape, torch.float32) if p.value else None for p in (ks, vs)]
        return rows[0], rows[1], scales[0], scales[1]

    def admit_row(self, row: int, enc: torch.Tensor, enc_mask: Optional[torch.Tensor], prompt: Optional[torch.Tensor],
                  prompt_mask: Optional[torch.Tensor], max_length: int = 0, sample: bool = True, gen: Optional[dict] = None,
                  voice: Optional[torch.Tensor] = None):
        """Prefills ONE request (``enc`` [N, H], ``prompt`` [P, H] at the session's widths) into the idle slot ``row``; the other slots
        keep their state. ``max_length`` = the request's own 1 + max_new_tokens (0: the session's).
        ``gen``: the request's own sampler settings and seed (``ptts_admit_row_gen``) - keys ``min_new_tokens, do_sample, temperature, top_k,
        top_p, use_eos_gate, seed``, a key left out takes ``set_gen_params``'s default; the slot then draws from ``(seed, column, codebook)``,
        whichever slot it is. ``None``: the session's parameters and draw stream (``ptts_admit_row``).
        ``voice``: un-delayed audio codes int64 [K, T] the request continues (``ptts_admit_row_voice``): the slot starts with 1 + T given
        columns and ``max_length`` counts them, as ``set_audio_prefix`` + ``prefill`` do for a static batch. ``None`` or T == 0: the call made
        without it."""
        voice = None if voice is None else self._voice_codes([voice])[0]
        gp = None if gen is None else self._gen_params(gen)
        enc, em, pr, pm = self._session_inputs(None, enc, enc_mask, prompt, prompt_mask)
        ptr = self._ptr
        if voice is not None:
            N.check(self.lib.ptts_admit_row_voice(self._h, int(row), ptr(enc), ptr(em), ptr(pr), ptr(pm), ptr(voice), int(voice.shape[1]), int(max_length),
                                                  int(sample), C.byref(gp) if gp is not None else None, _stream_ptr(device=self.device)),
                    "ptts_admit_row_voice")
        elif gp is None:
            N.check(self.lib.ptts_admit_row(self._h, int(row), ptr(enc), ptr(em), ptr(pr), ptr(pm), int(max_length), int(sample),
                                            _stream_ptr(device=self.device)), "ptts_admit_row")
        else:
            N.check(self.lib.ptts_admit_row_gen(self._h, int(row), ptr(enc), ptr(em), ptr(pr), ptr(pm), int(max_length), int(sample), C.byref(gp),
                                                _stream_ptr(device=self.device)), "ptts_admit_row_gen")
        self._keep_admitted([int(row)], [enc, em, pr, pm, voice])

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()

    @staticmethod
    def _gen_params(gen: dict):
        """``admit_row``'s ``gen`` as a ``PttsGenParams``; its max_length 0: the admission's ``max_length`` argument rules the slot's end."""
        unknown = set(gen) - {"min_new_tokens", "do_sample", "temperature", "top_k", "top_p", "use_eos_gate", "seed"}
        if unknown:
            raise ValueError(f"unknown per-request generation parameters {sorted(unknown)}")
        return N.PttsGenParams(0, int(gen.get("min_new_tokens", 0)), int(bool(gen.get("do_sample", False))), float(gen.get("temperature", 1.0)),
                               int(gen.get("top_k", 0) or 0), float(gen.get("top_p", 1.0)), int(bool(gen.get("use_eos_gate", True))),
                               int(gen.get("seed", 0)) & (2 ** 64 - 1))

    def _voice_codes(self, voices):
        """Per request ``None`` or int64 [K, T] codes -> the same list on the device; a prompt of no frames is ``None``."""
        for v in voices:
            if v is not None and (v.dim() != 2 or v.shape[0] != self.K):
                raise ValueError(f"voice prompt codes {tuple(v.shape)}: expected [{self.K}, frames]")
        return [None if v is None or v.shape[1] == 0 else v.to(self.device, torch.int64).contiguous() for v in voices]

    def _session_inputs(self, n, enc, enc_mask, prompt, prompt_mask):
        """The inputs of ``n`` requests, [n, ...] at the session's widths (``n`` None: of one request, without the leading dimension), checked
        and on the device: ``(enc, enc_mask, prompt, prompt_mask)``, ``None`` where the admission passes a null pointer."""
        one = n is None
        shape = (lambda *w: w) if one else (lambda *w: (n,) + w)
        enc = enc.to(self.device, torch.float32).contiguous()
        if tuple(enc.shape) != shape(self.session_N, self.H):
            raise ValueError(f"encoder states {tuple(enc.shape)} do not match " + (f"the session's [{self.session_N}, {self.H}]" if one else
                             f"[{n}, {self.session_N}, {self.H}] ({n} slots at the session's widths)"))
        pr = em = pm = None
        if self.P > 0:
            if prompt is None or tuple(prompt.shape) != shape(self.P, self.H):
                raise ValueError(f"prompt embeddings {None if prompt is None else tuple(prompt.shape)} do not match " +
                                 (f"the session's [{self.P}, {self.H}]" if one else f"[{n}, {self.P}, {self.H}]"))
            pr = prompt.to(self.device, torch.float32).contiguous()
        if enc_mask is not None:
            em = enc_mask.to(self.device, torch.int32).contiguous()
            em = em.reshape(-1) if one else em
            if tuple(em.shape) != shape(self.session_N):
                raise ValueError(f"attention_mask of {em.numel()} positions does not match the session's {self.session_N}" if one else
                                 f"attention_mask {tuple(em.shape)} does not match [{n}, {self.session_N}]")
        if prompt_mask is not None and self.P > 0:
            pm = prompt_mask.to(self.device, torch.int32).contiguous()
            pm = pm.reshape(-1) if one else pm
            if tuple(pm.shape) != shape(self.P):
                raise ValueError(f"prompt_attention_mask of {pm.numel()} positions does not match the session's {self.P}" if one else
                                 f"prompt_attention_mask {tuple(pm.shape)} does not match [{n}, {self.P}]")
        return enc, em, pr, pm

    def _keep_admitted(self, rows, tensors):
        if not hasattr(self, "_keep_rows"):
            self._keep_rows = {}
        keep = [t for t in tensors if t is not None]
        for r in rows:
            self._keep_rows[r] = keep  # consumed asynchronously by the enqueued kernels

    def admit_rows(self, rows, enc: torch.Tensor, enc_mask: Optional[torch.Tensor], prompt: Optional[torch.Tensor],
                   prompt_mask: Optional[torch.Tensor], max_lengths=None, sample: bool = True, gens=None, voices=None):
        """Prefills ``n = len(rows)`` requests into ``n`` distinct idle slots with ONE prefill pass (``ptts_admit_rows``): request ``j``
        (``enc[j]`` [N, H], ``prompt[j]`` [P, H], ``max_lengths[j]``, ``gens[j]``) goes into slot ``rows[j]``, which afterwards is what
        ``admit_row`` makes of it. The engine needs ``n`` spare rows behind the session's slots (``max_batch >= slots + n``).
        ``max_lengths``: one per request (``None``: the session's for all); ``gens``: ``None``, or one entry per request, each ``None`` or
        ``admit_row``'s ``gen``.
        ``voices``: ``None``, or one entry per request, each ``None`` or ``admit_row``'s ``voice`` (int64 [K, T_j], ragged): the group runs
        ONE pass over ``P + 1 + max T_j`` positions per request (``ptts_admit_rows_voice``), a shorter request right-padded; slot ``rows[j]``
        afterwards is what ``admit_row(voice=voices[j])`` makes of it. Without the keyword, or with every entry ``None``: the call made without it."""
        rows = [int(r) for r in rows]
        n = len(rows)
        if voices is not None:
            if len(voices) != n:
                raise ValueError(f"{n} slots, {len(voices)} voices")
            voices = self._voice_codes(voices)
            if all(v is None for v in voices):
                voices = None
        max_lengths = [0] * n if max_lengths is None else [int(x) for x in max_lengths]
        if len(max_lengths) != n or (gens is not None and len(gens) != n):
            raise ValueError(f"{n} slots, {len(max_lengths)} max_lengths, {None if gens is None else len(gens)} gens")
        gp_arr = None
        if gens is not None:
            gps = [None if gen is None else self._gen_params(gen) for gen in gens]  # alive until the call returns: it copies the records
            gp_arr = (C.POINTER(N.PttsGenParams) * max(n, 1))(*[None if g is None else C.pointer(g) for g in gps])
        enc, em, pr, pm = self._session_inputs(n, enc, enc_mask, prompt, prompt_mask)
        ptr = self._ptr
        ints = lambda xs: (C.c_int32 * max(n, 1))(*xs)
        if voices is not None:
            codes = (C.c_void_p * max(n, 1))(*[None if v is None else v.data_ptr() for v in voices])
            N.check(self.lib.ptts_admit_rows_voice(self._h, n, ints(rows), ptr(enc), ptr(em), ptr(pr), ptr(pm), codes,
                                                   ints(0 if v is None else int(v.shape[1]) for v in voices), ints(max_lengths), int(sample), gp_arr,
                                                   _stream_ptr(device=self.device)), "ptts_admit_rows_voice")
        else:
            N.check(self.lib.ptts_admit_rows(self._h, n, ints(rows), ptr(enc), ptr(em), ptr(pr), ptr(pm), ints(max_lengths), int(sample), gp_arr,
                                             _stream_ptr(device=self.device)), "ptts_admit_rows")
        self._keep_admitted(rows, [enc, em, pr, pm] + (voices or []))

    def row_state(self) -> Tuple[list, list]:
        """(cur_len, live) per slot: columns written so far incl. BOS, and whether the slot is still generating. Synchronises."""
        cur, live = (C.c_int32 * self.B)(), (C.c_int32 * self.B)()
        N.check(self.lib.ptts_row_state(self._h, cur, live, _stream_ptr(device=self.device)), "ptts_row_state")
        return list(cur), [bool(v) for v in live]

    def retire_row(self, row: int):
        N.check(self.lib.ptts_retire_row(self._h, int(row), _stream_ptr(device=self.device)), "ptts_retire_row")
        self._slot_records.pop(int(row), None)  # the slot's step record is cleared with it

    def slot_voice(self) -> list:
        """Voice-prompt frames per slot as the device holds them (``ptts_debug_slot_voice``; for tests). Synchronises."""
        t = (C.c_int32 * self.B)()
        N.check(self.lib.ptts_debug_slot_voice(self._h, t, _stream_ptr(device=self.device)), "ptts_debug_slot_voice")
        return list(t)

    def row_ids(self, row: int, cols: int) -> torch.Tensor:
        """Raw ids [K, cols] of one slot (a copy)."""
        p, ld = C.c_void_p(), C.c_int32()
        N.check(self.lib.ptts_ids(self._h, C.byref(p), C.byref(ld)), "ptts_ids")
        return self._copy_out(p.value + int(row) * self.K * ld.value * 8, (self.K, int(cols)), torch.int64, row_stride=ld.value)

    def ids_buffer(self) -> Tuple[int, int]:
        """(device pointer, row stride in columns) of the engine's own raw id buffer int64 [B*K, stride] (``ptts_ids``), NOT a copy: what
        ``DacEngine.stream_decode`` reads in place (``col0=1, delay=1``), ordered behind the decode steps on the same stream."""
        p, ld = C.c_void_p(), C.c_int32()
        N.check(self.lib.ptts_ids(self._h, C.byref(p), C.byref(ld)), "ptts_ids")
        return int(p.value), int(ld.value)

    def generate_ids(self, enc, enc_mask, prompt, prompt_mask, poll_every: int = 64, audio_prefix: Optional[torch.Tensor] = None) -> torch.Tensor:
        """prefill + graph-replayed decode until every row finished; returns raw ids [B*K, Lout]. ``audio_prefix``:
        un-delayed voice-prompt codes [B, K, T] continued by the decoder."""
        self.set_audio_prefix(audio_prefix)
        self.prefill(enc, enc_mask, prompt, prompt_mask, sample=True)
        remaining = self.max_length - 2 - (0 if audio_prefix is None else int(audio_prefix.shape[-1]))
        while remaining > 0:
            n = min(poll_every, remaining)
            self.decode_steps(n)
            remaining -= n
            _, fin = self.state()
            if fin:
                break
        return self.ids()


class T5Engine:
    """Owner of a ``ptts_t5``: the description encoder (transformers ``T5EncoderModel``, gated-gelu, d_kv 64) on MI355X.
    Replaces the ``self.text_encoder(...)`` call of generate() (modeling_parler_tts.py:3048-3097) on the time-to-first-token path."""

    def __init__(self, *, vocab_size: int, d_model: int, d_kv: int, d_ff: int, num_layers: int, num_heads: int,
                 relative_attention_num_buckets: int = 32, relative_attention_max_distance: int = 128, layer_norm_epsilon: float = 1e-6,
                 dtype: torch.dtype = torch.bfloat16, max_batch: int = 1, max_len: int = 64, device: Optional[torch.device] = None):
        if not torch.cuda.is_available():
            raise N.NativeLibraryError("T5Engine needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.lib = N.load_library()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"engine dtype must be float32 or bfloat16, got {dtype}")
        self.dtype, self.d_model, self.max_batch, self.max_len = dtype, d_model, max_batch, max_len
        self.cfg = N.PttsT5Config(vocab_size, d_model, d_kv, d_ff, num_layers, num_heads, relative_attention_num_buckets,
                                  relative_attention_max_distance, float(layer_norm_epsilon),
                                  N.PTTS_BF16 if dtype == torch.bfloat16 else N.PTTS_F32, max_batch, max_len, self.device.index or 0)
        self._h = C.c_void_p()
        N.check(self.lib.ptts_t5_create(C.byref(self.cfg), C.byref(self._h)), "ptts_t5_create")

    @staticmethod
    def supports(config) -> bool:
        """True for the T5 configurations the HIP encoder implements (flan-t5 / T5 v1.1 shapes: gated gelu_new feed-forward, d_kv 64)."""
        return (getattr(config, "model_type", None) == "t5" and getattr(config, "d_kv", 0) == 64 and bool(getattr(config, "is_gated_act", False))
                and getattr(config, "dense_act_fn", None) == "gelu_new" and config.d_model % 32 == 0 and config.d_ff % 32 == 0)

    @classmethod
    def from_config(cls, config, **kw) -> "T5Engine":
        return cls(vocab_size=config.vocab_size, d_model=config.d_model, d_kv=config.d_kv, d_ff=config.d_ff, num_layers=config.num_layers,
                   num_heads=config.num_heads, relative_attention_num_buckets=config.relative_attention_num_buckets,
                   relative_attention_max_distance=getattr(config, "relative_attention_max_distance", 128),
                   layer_norm_epsilon=config.layer_norm_epsilon, **kw)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.ptts_t5_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = ""):
        """``sd``: transformers ``T5EncoderModel`` names (``shared.weight``, ``encoder.block.N....``), optionally under ``prefix``
        (``"text_encoder."`` for a ParlerTTSForConditionalGeneration checkpoint)."""
        for k, v in sd.items():
            if not k.startswith(prefix):
                continue
            name = k[len(prefix):]
            if not (name.startswith("encoder.") or name == "shared.weight"):
                continue
            t = v.detach()
            if t.dtype not in (torch.float32, torch.bfloat16):
                t = t.float()
            t = t.to(self.device).contiguous()
            dt = N.PTTS_BF16 if t.dtype == torch.bfloat16 else N.PTTS_F32
            N.check(self.lib.ptts_t5_load_weight(self._h, name.encode(), C.c_void_p(t.data_ptr()), dt, _shape_arr(t), t.dim(), _stream_ptr(device=self.device)),
                    f"ptts_t5_load_weight({name})")
            torch.cuda.current_stream(self.device).synchronize()  # the engine re-packs asynchronously; `t` must stay alive until then
        N.check(self.lib.ptts_t5_weights_ready(self._h), "ptts_t5_weights_ready")

    def graph_nodes(self) -> int:
        """Kernel nodes of the encoder graph captured last (``ptts_t5_debug_graph_nodes``; 0 before the first capture)."""
        n = C.c_int32(0)
        N.check(self.lib.ptts_t5_debug_graph_nodes(self._h, C.byref(n)), "ptts_t5_debug_graph_nodes")
        return int(n.value)

    def encode(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """input_ids int64 [B, N], attention_mask [B, N] or None -> float32 [B, N, d_model]: ``last_hidden_state`` with the masked
        positions zeroed (what generate() hands to the decoder, :3093-3097). Asynchronous on the current stream of the engine's device."""
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [batch, tokens], got {tuple(input_ids.shape)}")
        ids = input_ids.to(self.device, torch.int64).contiguous()
        B, Nn = ids.shape
        mk = attention_mask.to(self.device, torch.int32).contiguous() if attention_mask is not None else None
        if mk is not None and mk.shape != ids.shape:
            raise ValueError(f"attention_mask {tuple(mk.shape)} does not match input_ids {tuple(ids.shape)}")
        out = torch.empty(B, Nn, self.d_model, dtype=torch.float32, device=self.device)
        N.check(self.lib.ptts_t5_encode(self._h, C.c_void_p(ids.data_ptr()), C.c_void_p(mk.data_ptr()) if mk is not None else C.c_void_p(), B, Nn,
                                        C.c_void_p(out.data_ptr()), _stream_ptr(device=self.device)), "ptts_t5_encode")
        self._keep = (ids, mk)  # consumed asynchronously by the enqueued copies
        return out


class DacEngine:
    """Owner of a ``ptts_dac``: DAC codes → waveform (and, with ``encoder_dim`` > 0, waveform → codes for voice prompts)
    on MI355X (exact-f32 MFMA implicit-GEMM convolutions)."""

    def __init__(self, *, num_codebooks: int = 9, codebook_size: int = 1024, codebook_dim: int = 8, latent_dim: int = 1024,
                 decoder_dim: int = 1536, rates: Iterable[int] = (8, 8, 4, 2), max_batch: int = 1, max_frames: int = 2600,
                 device: Optional[torch.device] = None, encoder_dim: int = 0, compute_dtype: torch.dtype = torch.float32):
        if not torch.cuda.is_available():
            raise N.NativeLibraryError("DacEngine needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.lib = N.load_library()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        rates = tuple(int(r) for r in rates)
        arr = (C.c_int32 * 8)(*(list(rates) + [0] * (8 - len(rates))))
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"DAC compute dtype {compute_dtype} is not supported (float32: exact-f32 MFMA, bfloat16: bf16 MFMA operands)")
        self.compute_dtype = compute_dtype
        self.cfg = N.PttsDacConfig(num_codebooks, codebook_size, codebook_dim, latent_dim, decoder_dim, len(rates), arr,
                                   N.PTTS_BF16 if compute_dtype == torch.bfloat16 else N.PTTS_F32,
                                   max_batch, max_frames, self.device.index or 0, int(encoder_dim))
        self.encoder_dim = int(encoder_dim)
        self.latent_dim = latent_dim
        self.hop = math.prod(rates)
        self.K = num_codebooks
        self.codebook_size = codebook_size
        self.max_batch, self.max_frames = max_batch, max_frames
        self._h = C.c_void_p()
        N.check(self.lib.ptts_dac_create(C.byref(self.cfg), C.byref(self._h)), "ptts_dac_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.ptts_dac_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = ""):
        """`sd`: dac.model.DAC names with weight-norm in any of the three formats the reference may hold
        (folded ``.weight``, legacy ``.weight_g/.weight_v``, ``.parametrizations.weight.original0/1``;
        dac_wrapper/modeling_dac.py:148-164). Folded here on the host side once."""
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        for name, t in fold_weight_norm(sd).items():
            if not (name.startswith("quantizer.") or name.startswith("decoder.") or (self.encoder_dim > 0 and name.startswith("encoder."))):
                continue
            t = t.detach().to(self.device, torch.float32).contiguous()
            if name.endswith(".alpha"):
                t = t.reshape(-1).contiguous()
            N.check(self.lib.ptts_dac_load_weight(self._h, name.encode(), C.c_void_p(t.data_ptr()), _shape_arr(t), t.dim(), _stream_ptr(device=self.device)),
                    f"ptts_dac_load_weight({name})")
            torch.cuda.current_stream(self.device).synchronize()
        N.check(self.lib.ptts_dac_weights_ready(self._h), "ptts_dac_weights_ready")

    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        """codes int64 [B, K, T] → waveform float32 [B, 1, hop*T]."""
        if codes.dim() != 3 or codes.shape[1] != self.K:
            raise ValueError(f"audio_codes must be [batch, {self.K}, frames], got {tuple(codes.shape)}")
        codes = codes.to(self.device, torch.int64).contiguous()
        B, _, T = codes.shape
        out = torch.empty(B, 1, self.hop * T, dtype=torch.float32, device=self.device)
        N.check(self.lib.ptts_dac_decode(self._h, C.c_void_p(codes.data_ptr()), C.c_void_p(out.data_ptr()), B, T, _stream_ptr(device=self.device)), "ptts_dac_decode")
        self._keep = codes
        return out


    def compact_codes(self, codes: torch.Tensor):
        """codes int64 [B, K, T] → (codes with every frame holding an id outside [0, codebook_size) dropped, the kept ones in order
        [B, K, T]; kept-frame counts int32 [B]), both on the device (``ptts_dac_compact_codes``; modeling_parler_tts.py:3627-3636)."""
        if codes.dim() != 3 or codes.shape[1] != self.K:
            raise ValueError(f"audio_codes must be [batch, {self.K}, frames], got {tuple(codes.shape)}")
        codes = codes.to(self.device, torch.int64).contiguous()
        B, _, T = codes.shape
        out = torch.empty_like(codes)
        frames = torch.empty(B, dtype=torch.int32, device=self.device)
        N.check(self.lib.ptts_dac_compact_codes(self._h, C.c_void_p(codes.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(frames.data_ptr()), B, T,
                                                _stream_ptr(device=self.device)), "ptts_dac_compact_codes")
        self._keep = codes
        return out, frames

    def decode_ragged(self, codes: torch.Tensor, frames: torch.Tensor) -> torch.Tensor:
        """codes int64 [B, K, T], frames int32 [B] on the device → waveform float32 [B, 1, hop*T] in which utterance b is the decode of its
        first frames[b] frames and zero beyond (``ptts_dac_decode_ragged``: one pass, no per-utterance launches)."""
        if codes.dim() != 3 or codes.shape[1] != self.K:
            raise ValueError(f"audio_codes must be [batch, {self.K}, frames], got {tuple(codes.shape)}")
        codes = codes.to(self.device, torch.int64).contiguous()
        frames = frames.to(self.device, torch.int32).contiguous()
        B, _, T = codes.shape
        if frames.shape != (B,):
            raise ValueError(f"frames must be [batch], got {tuple(frames.shape)}")
        out = torch.empty(B, 1, self.hop * T, dtype=torch.float32, device=self.device)
        N.check(self.lib.ptts_dac_decode_ragged(self._h, C.c_void_p(codes.data_ptr()), C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr()), B, T,
                                                _stream_ptr(device=self.device)), "ptts_dac_decode_ragged")
        self._keep = (codes, frames)
        return out

    def decode_chunk(self, codes: torch.Tensor, first_frame: int, n_frames: int, halo: int, out: Optional[torch.Tensor] = None,
                     n_emit: Optional[int] = None) -> torch.Tensor:
        """codes int64 [B, K, T] (contiguous, on the device; read in place): decodes the window [first_frame - halo,
        first_frame + n_frames) and returns the samples of frames [first_frame, first_frame + n_emit) (default: all n_frames) as
        float32 [B, 1, hop*n_emit] (``ptts_dac_decode_chunk``). ``out``: a float32 [B, >= hop*(first_frame + n_emit)] waveform
        buffer to write into at sample offset hop*first_frame instead (chunked decode of a whole utterance). Enqueued on the
        CURRENT stream of the engine's device: a caller can run it on a side stream while the decoder graph replays."""
        if codes.dim() != 3 or codes.shape[1] != self.K:
            raise ValueError(f"audio_codes must be [batch, {self.K}, frames], got {tuple(codes.shape)}")
        if codes.device != self.device or codes.dtype != torch.int64 or not codes.is_contiguous():
            codes = codes.to(self.device, torch.int64).contiguous()
        B, _, T = codes.shape
        n_emit = n_frames if n_emit is None else int(n_emit)
        if out is None:
            dst = torch.empty(B, 1, self.hop * n_emit, dtype=torch.float32, device=self.device)
            ptr, ld = dst.data_ptr(), self.hop * n_emit
        else:
            if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1 or out.shape[1] < self.hop * (first_frame + n_emit):
                raise ValueError("out must be a float32 [batch, samples] buffer covering the emitted frames")
            dst, ptr, ld = out, out.data_ptr() + 4 * self.hop * first_frame, out.stride(0)
        N.check(self.lib.ptts_dac_decode_chunk(self._h, C.c_void_p(codes.data_ptr()), T, int(first_frame), int(n_frames), int(halo),
                                               C.c_void_p(ptr), int(ld), int(n_emit), B, _stream_ptr(device=self.device)), "ptts_dac_decode_chunk")
        self._keep = codes
        return dst

    # -- streaming out of a continuous session (ptts_dac_stream_open / _reset / _decode) ---------------------------
    def stream_open(self, slots: int, cap_frames: int, max_voice_frames: int = 0):
        """(Re)allocates and clears the per-slot stream table: kept codes [slots, K, cap_frames] and the counters, on the device.
        ``max_voice_frames > 0``: plus the slots' voice prompts [slots, K, max_voice_frames] (``ptts_dac_stream_open_voice``)."""
        if int(max_voice_frames):
            N.check(self.lib.ptts_dac_stream_open_voice(self._h, int(slots), int(cap_frames), int(max_voice_frames), _stream_ptr(device=self.device)),
                    "ptts_dac_stream_open_voice")
        else:
            N.check(self.lib.ptts_dac_stream_open(self._h, int(slots), int(cap_frames), _stream_ptr(device=self.device)), "ptts_dac_stream_open")
        self.stream_slots, self.stream_cap = int(slots), int(cap_frames)
        self._st_absorbed, self._st_ready_ub = [0] * int(slots), [0] * int(slots)  # the library's host-side bounds, mirrored to size `wave`
        self._st_voice = [0] * int(slots)  # prefix frames per slot, negative where the prompt is not emitted (the library's st_voice)

    def stream_reset(self, slot: int, voice: Optional[torch.Tensor] = None, emit_prompt: bool = True):
        """A new request enters ``slot``: its counters return to 0 (enqueued). ``voice``: the un-delayed codes int64 [K, T] of the voice prompt
        it continues (``ptts_dac_stream_reset_voice``); ``emit_prompt=False``: the prompt's frames are left context only."""
        T = 0
        if voice is None:
            N.check(self.lib.ptts_dac_stream_reset(self._h, int(slot), _stream_ptr(device=self.device)), "ptts_dac_stream_reset")
        else:
            if voice.dim() != 2 or voice.shape[0] != self.K:
                raise ValueError(f"voice must be [{self.K}, frames], got {tuple(voice.shape)}")
            voice = voice.to(self.device, torch.int64).contiguous()
            T = int(voice.shape[1])
            N.check(self.lib.ptts_dac_stream_reset_voice(self._h, int(slot), C.c_void_p(voice.data_ptr() if T else None), T, int(bool(emit_prompt)),
                                                         _stream_ptr(device=self.device)), "ptts_dac_stream_reset_voice")
            self._keep = voice
        self._st_absorbed[int(slot)] = self._st_ready_ub[int(slot)] = 0
        self._st_voice[int(slot)] = T if emit_prompt else -T

    def stream_decode(self, ids, ids_ld: Optional[int], rows, halo: int, col0: int = 0, delay: int = 0, max_emit: Optional[int] = None):
        """One windowed codec pass over the listed slots (``ptts_dac_stream_decode``). ``ids``: an int64 device tensor [slots, K, ld] of plain
        codes (``col0=0, delay=0``), or the pointer of ``DecoderEngine.ids_buffer()`` with its stride ``ids_ld`` (``col0=1, delay=1``), read in
        place. ``rows``: ``(slot, complete, final, min_emit)`` per listed slot. Returns ``(wave float32 [R, ld], out int32 [R, 2])`` on the
        device: row r holds ``hop * out[r, 0]`` samples (zero beyond), ``out[r] = (emit, kept)``. Enqueued on the current stream; no sync.
        ``max_emit``: no row emits more kept frames than this in one pass (``ptts_dac_stream_decode_capped``); a ``final`` row that had more
        ready is listed again until its emits add up."""
        if not getattr(self, "stream_slots", 0):
            raise ValueError("no stream table: call stream_open first")
        if isinstance(ids, torch.Tensor):
            if ids.device != self.device or ids.dtype != torch.int64 or not ids.is_contiguous():
                ids = ids.to(self.device, torch.int64).contiguous()
            ptr, ids_ld = ids.data_ptr(), int(ids.shape[-1])
            self._keep = ids
        else:
            ptr, ids_ld = int(ids), int(ids_ld)
        rows = [tuple(int(v) for v in r) for r in rows]
        R = len(rows)
        arr = (N.PttsDacStreamRow * max(R, 1))(*[N.PttsDacStreamRow(*r) for r in rows])
        emit_ub, bounds = 1, []
        for slot, complete, final, min_emit in rows:
            ub = 0
            if 0 <= slot < self.stream_slots:  # a bad descriptor is refused by the library with its own message
                v, a = self._st_voice[slot], self._st_absorbed[slot]
                # the frames of a prompt that is not emitted never become ready
                ub = self._st_ready_ub[slot] + (max(0, max(complete, -v) - max(a, -v)) if v < 0 else max(0, complete - a))
                emit_ub = max(emit_ub, ub if final else ub - int(halo))
            bounds.append(ub)
        if max_emit is not None:
            emit_ub = min(emit_ub, max(int(max_emit), 1))
        wave = torch.empty(max(R, 1), self.hop * emit_ub, dtype=torch.float32, device=self.device)
        out = torch.empty(max(R, 1), 2, dtype=torch.int32, device=self.device)
        if max_emit is None:
            N.check(self.lib.ptts_dac_stream_decode(self._h, C.c_void_p(ptr), ids_ld, int(col0), int(delay), arr, R, int(halo), C.c_void_p(wave.data_ptr()),
                                                    int(wave.shape[1]), C.c_void_p(out.data_ptr()), _stream_ptr(device=self.device)), "ptts_dac_stream_decode")
        else:
            N.check(self.lib.ptts_dac_stream_decode_capped(self._h, C.c_void_p(ptr), ids_ld, int(col0), int(delay), arr, R, int(halo),
                                                           C.c_void_p(wave.data_ptr()), int(wave.shape[1]), C.c_void_p(out.data_ptr()),
                                                           _stream_ptr(device=self.device), int(max_emit)), "ptts_dac_stream_decode_capped")
        for (slot, complete, final, min_emit), ub in zip(rows, bounds):
            left = 0 if final else min(ub, int(halo) + max(min_emit, 1) - 1)
            self._st_ready_ub[slot] = left if max_emit is None else max(left, ub - int(max_emit))  # a capped emit leaves ready - max_emit
            self._st_absorbed[slot] = complete
        return wave, out

    def encode(self, wave: torch.Tensor, n_quantizers: Optional[int] = None) -> torch.Tensor:
        """waveform float32 [B, 1, L] (L a multiple of the hop) → codes int64 [B, n_quantizers, L / hop]."""
        if self.encoder_dim <= 0:
            raise NotImplementedError("this DacEngine was built without the encoder (encoder_dim=0)")
        if wave.dim() != 3 or wave.shape[1] != 1:
            raise ValueError(f"input_values must be [batch, 1, samples], got {tuple(wave.shape)}")
        wave = wave.to(self.device, torch.float32).contiguous()
        B, _, L = wave.shape
        if L == 0 or L % self.hop:
            raise ValueError(f"waveform length {L} is not a positive multiple of the hop {self.hop} (apply the preprocess padding)")
        nq = self.K if n_quantizers is None else max(1, min(int(n_quantizers), self.K))
        codes = torch.empty(B, nq, L // self.hop, dtype=torch.int64, device=self.device)
        N.check(self.lib.ptts_dac_encode(self._h, C.c_void_p(wave.data_ptr()), C.c_void_p(codes.data_ptr()), B, L, nq, _stream_ptr(device=self.device)), "ptts_dac_encode")
        self._keep = wave
        return codes

    def debug_latents(self, B: int, T: int) -> torch.Tensor:
        """Latents z of the last ``encode`` as [B, latent, T] (parity probe)."""
        p = C.c_void_p()
        N.check(self.lib.ptts_dac_debug_latents(self._h, C.byref(p)), "ptts_dac_debug_latents")
        out = torch.empty(B, T, self.latent_dim, dtype=torch.float32, device=self.device)
        rc = N.hip_runtime().hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(p.value), C.c_size_t(out.numel() * 4), 3, _stream_ptr(device=self.device))
        if rc != 0:
            raise N.NativeLibraryError(f"hipMemcpy(D2D) failed with code {rc}")
        return out.transpose(1, 2).contiguous()
    def debug_stage(self, codes: torch.Tensor, stage: int):
        """Parity probe (``ptts_dac_debug_decode_upto``): decode stopped after `stage`; returns (act [B, C, rows] float32 - the exact values
        of the bf16 / fp32 activation buffer -, raw [B, C, rows] float32 residual stream or None)."""
        codes = codes.to(self.device, torch.int64).contiguous()
        B, _, T = codes.shape
        act, raw = C.c_void_p(), C.c_void_p()
        is_bf, rows, ch = C.c_int32(), C.c_int32(), C.c_int32()
        N.check(self.lib.ptts_dac_debug_decode_upto(self._h, C.c_void_p(codes.data_ptr()), B, T, int(stage), _stream_ptr(device=self.device), C.byref(act),
                                                    C.byref(is_bf), C.byref(raw), C.byref(rows), C.byref(ch)), "ptts_dac_debug_decode_upto")
        hip = N.hip_runtime()

        def grab(ptr, dtype):
            t = torch.empty(B, rows.value, ch.value, dtype=dtype, device=self.device)
            rc = hip.hipMemcpyAsync(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(t.numel() * t.element_size()), 3, _stream_ptr(device=self.device))
            if rc != 0:
                raise N.NativeLibraryError(f"hipMemcpy(D2D) failed with code {rc}")
            return t.float().transpose(1, 2).contiguous()

        a = grab(act.value, torch.bfloat16 if is_bf.value else torch.float32)
        r = grab(raw.value, torch.float32) if raw.value else None
        return a, r


def fold_weight_norm(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """w = g · v / ‖v‖ (norm over all dims but 0, torch weight_norm's default dim=0) for both key formats."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in sd.items():
        for g_suf, v_suf in ((".weight_g", ".weight_v"), (".parametrizations.weight.original0", ".parametrizations.weight.original1")):
            if k.endswith(g_suf):
                base = k[: -len(g_suf)]
                vv = sd[base + v_suf].float()
                norm = vv.flatten(1).norm(dim=1).view(-1, *([1] * (vv.dim() - 1)))
                out[base + ".weight"] = v.float() * vv / norm
                break
            if k.endswith(v_suf):
                break
        else:
            out[k] = v
    return out
