"""Restatements (numpy, no GPU) of what a voice admission into a continuous session writes and of what the session tail does behind it: the id
columns 1..T of the slot (``admit_voice_slots_kernel``), and ``tail_kernel<NV, true>`` over slots that each carry their own ``max_length`` and
voice-prompt length (``sampler_model.TailModel`` with a prefix length per slot). tests/test_session_voice_cpu.py checks both against
``build_delay_pattern_mask`` and ``sample_loop(decoder_input_ids=)``; tests/test_session_voice_gpu.py checks the kernels against them."""
import numpy as np
import torch

import sampler_model as SM


def prefix_id_columns(prefix, K, max_length, bos, pad):
    """[K, T] un-delayed codes -> the [K, T] values of id columns 1..T, cell by cell as the kernel computes them (one thread per cell)."""
    prefix = np.asarray(prefix, dtype=np.int64)
    T = prefix.shape[1]
    out = np.empty((K, T), dtype=np.int64)
    for i in range(K * T):
        k, j = i // T, 1 + i % T
        if max_length < 2 * K - 1:
            v = prefix[k, j - 1]
        elif j <= k:
            v = bos
        elif j - k >= max_length - K + 1:
            v = pad
        else:
            v = prefix[k, j - k - 1]
        out[k, j - 1] = v
    return out


class VoiceTailModel(SM.TailModel):
    """The session model with a voice-prompt length per slot (the device's slot_T beside row_maxlen). ``admit`` is what ptts_admit_row_voice
    leaves before its tail: reset, the id columns of the prefix, the clock at T + 1; ``retire`` what ptts_retire_row leaves. A launch over
    several slots is the per-slot step with that slot's own T: slots do not read each other's state."""

    def __init__(self, B, K, V, eos, pad, bos, ld, P=0, fill=0):
        super().__init__(B, K, V, eos, pad, bos, ld, session=True, P=P, fill=fill)
        self.slot_T = np.zeros(B, dtype=np.int32)
        self.prefix = np.zeros((B * K, ld), dtype=np.int64)

    def admit(self, b, max_length, prefix=None):
        K = self.K
        self.reset_row(b, 1, max_length)
        T = 0 if prefix is None else int(prefix.shape[-1])
        self.slot_T[b] = T
        if T:
            prefix = np.asarray(prefix, dtype=np.int64)
            self.prefix[b * K:(b + 1) * K, :T] = prefix
            seq = torch.cat([torch.full((K, 1), self.bos, dtype=torch.long), torch.from_numpy(prefix)], dim=-1)
            self._begin(b, seq, max_length)  # the pattern the model is fed through, the given columns, the clock
            # the given columns are exactly what the writer kernel computes
            assert np.array_equal(self.ids[b * K:(b + 1) * K, 1:1 + T], prefix_id_columns(prefix, K, max_length, self.bos, self.pad))
            assert self.cur_len[b] == T + 1

    def retire(self, b, session_max_length):
        self.reset_row(b, 0, session_max_length)
        self.slot_T[b] = 0

    def step(self, logits, gp, slots=None, **kw):
        live = []
        for b in (range(self.B) if slots is None else slots):
            self.T_prefix = int(self.slot_T[b])
            live += super().step(logits, gp, slots=[b], **kw)
        self.T_prefix = 0
        return live
