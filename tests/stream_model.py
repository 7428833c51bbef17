"""A host model of the per-slot stream table behind ``ptts_dac_stream_decode`` (include/ptts.h, "streaming out of a continuous session"):
absorb the raw frames [absorbed, complete) through the special-id filter, plan the emit, name the window of KEPT frames the codec runs on.
The GPU tests compare the library's ``out_dev`` pairs with it; the CPU tests put the oracle codec behind it as a stand-in for the engine."""
import numpy as np


class StreamTableModel:
    def __init__(self, slots, K, codebook_size):
        self.slots, self.K, self.cb = slots, K, codebook_size
        self.kept = [np.zeros((K, 0), dtype=np.int64) for _ in range(slots)]
        self.absorbed, self.emitted = [0] * slots, [0] * slots

    def reset(self, slot):
        self.kept[slot] = np.zeros((self.K, 0), dtype=np.int64)
        self.absorbed[slot] = self.emitted[slot] = 0

    def check(self, rows, cap):
        seen = set()
        for slot, complete, final, min_emit in rows:
            if not 0 <= slot < self.slots:
                raise ValueError(f"bad stream row: slot {slot} out of range")
            if slot in seen:
                raise ValueError(f"bad stream row: slot {slot} listed twice")
            seen.add(slot)
            if complete < self.absorbed[slot]:
                raise ValueError(f"bad stream row: complete {complete} decreases")
            if complete > cap:
                raise ValueError(f"bad stream row: complete {complete} beyond the table")

    def decode(self, frames_of, rows, halo):
        """``frames_of(slot, f0, f1)`` -> raw un-delayed frames int64 [K, f1 - f0]. Per listed row: (emit, kept, skip, window [K, n]) where
        ``window`` holds the kept frames [max(0, emitted - halo), kept) and the emitted ones start ``skip`` frames into it (emit == 0: no
        window)."""
        res = []
        for slot, complete, final, min_emit in rows:
            if complete > self.absorbed[slot]:
                raw = np.asarray(frames_of(slot, self.absorbed[slot], complete))
                ok = ((raw >= 0) & (raw < self.cb)).all(axis=0)
                self.kept[slot] = np.concatenate([self.kept[slot], raw[:, ok]], axis=1)
                self.absorbed[slot] = complete
            kept, emitted = self.kept[slot].shape[1], self.emitted[slot]
            ready = kept - emitted
            emit = ready if final else (ready - halo if ready - halo >= max(min_emit, 1) else 0)
            w0 = max(0, emitted - halo)
            win = self.kept[slot][:, w0:kept] if emit > 0 else None
            res.append((emit, kept, emitted - w0, win))
            self.emitted[slot] += emit
        return res
