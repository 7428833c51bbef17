"""tests/stream_model.py extended to include/ptts_dac_stream_voice.h: a slot may hold a voice prompt (``reset(slot, voice, emit_prompt)``),
raw frame f comes from the prompt for f < T and from ``frames_of`` (the id buffer) otherwise, the special-id filter runs when a frame is
ABSORBED - prompt frames included, so a request whose ``complete`` stays below T has only that many -, the kept frames of a prompt that is
not emitted count as emitted at once, a pass emits at most ``max_emit`` frames per row and its window ends ``halo`` kept frames behind them.
A ``final`` row that had more ready is not flushed: the caller lists it again. ``max_emit=None`` on a slot without a prompt is
``StreamTableModel.decode`` to the letter."""
import numpy as np

from stream_model import StreamTableModel


class StreamVoiceTableModel(StreamTableModel):
    def __init__(self, slots, K, codebook_size, max_voice_frames=0):
        super().__init__(slots, K, codebook_size)
        self.max_voice_frames = max_voice_frames
        self.prefix = [np.zeros((K, 0), dtype=np.int64) for _ in range(slots)]
        self.skip_prompt = [False] * slots
        self.prompt_kept = [0] * slots  # kept frames that came out of the prompt

    def reset(self, slot, voice=None, emit_prompt=True):
        if not 0 <= slot < self.slots:
            raise ValueError(f"stream slot {slot} out of range")
        voice = np.zeros((self.K, 0), dtype=np.int64) if voice is None else np.asarray(voice, dtype=np.int64)
        if voice.shape[1] > self.max_voice_frames:
            raise ValueError(f"voice prompt of {voice.shape[1]} frames, the stream table was opened for {self.max_voice_frames}")
        super().reset(slot)
        self.prefix[slot], self.skip_prompt[slot], self.prompt_kept[slot] = voice, voice.shape[1] > 0 and not emit_prompt, 0

    def decode(self, frames_of, rows, halo, max_emit=None):
        """As ``StreamTableModel.decode``; ``frames_of`` is only asked for frames at or behind the slot's prompt. The window of a row is the kept
        frames [max(0, emitted - halo), min(kept, emitted + emit + halo))."""
        if max_emit is not None and max_emit < 1:
            raise ValueError(f"bad stream pass: max_emit {max_emit}")
        res = []
        for slot, complete, final, min_emit in rows:
            a, T = self.absorbed[slot], self.prefix[slot].shape[1]
            if complete > a:
                parts = []
                if a < T:
                    parts.append(self.prefix[slot][:, a:min(T, complete)])
                if complete > max(a, T):
                    parts.append(np.asarray(frames_of(slot, max(a, T), complete)))
                raw = np.concatenate(parts, axis=1)
                ok = ((raw >= 0) & (raw < self.cb)).all(axis=0)
                from_prompt = int(ok[: max(0, min(T, complete) - a)].sum())
                self.kept[slot] = np.concatenate([self.kept[slot], raw[:, ok]], axis=1)
                self.absorbed[slot] = complete
                self.prompt_kept[slot] += from_prompt
                if self.skip_prompt[slot]:
                    self.emitted[slot] += from_prompt
            kept, emitted = self.kept[slot].shape[1], self.emitted[slot]
            ready = kept - emitted
            emit = ready if final else (ready - halo if ready - halo >= max(min_emit, 1) else 0)
            if max_emit is not None:
                emit = min(emit, max_emit)
            w0, w1 = max(0, emitted - halo), min(kept, emitted + emit + halo)
            win = self.kept[slot][:, w0:w1] if emit > 0 else None
            res.append((emit, kept, emitted - w0, win))
            self.emitted[slot] += emit
        return res

    def flushed(self, slot):
        return self.emitted[slot] == self.kept[slot].shape[1]
