"""Localized detection, host side (NOT in the reference's package API; its evaluation decodes this way, scripts/evaluate.py:442-516 with
the mask of model/watermarking.py:793-801): which frames count as watermarked, and how runs of them become segments.

The kernels (head_frames_kernel, head16_frames_kernel, wv_frames_reduce) give per FRAME the gated sigmoid sums and the gated sample
count; everything here is pure Python / numpy on those small arrays, so it runs without a GPU."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .watermark_id import WatermarkID


@dataclass(frozen=True)
class Segment:
    start_s: float                      # first sample of the segment, in seconds
    end_s: float                        # one past its last sample, in seconds
    watermark: WatermarkID              # decoded over the segment's gated samples only
    confidence: float                   # mean of the per-bit masked mean probabilities, as detect()'s confidence is
    coverage: float                     # gated samples / samples of the segment
    prob: Optional[np.ndarray] = None   # [nbits] float32, the masked mean probability of every bit
    frames: Tuple[int, int] = (0, 0)    # [f_lo, f_hi) in detector frames


def gate_threshold(p: float) -> float:
    """The locator-LOGIT threshold equivalent to sigmoid(logit) > p, in double: log(p / (1 - p))."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"threshold must lie strictly between 0 and 1, got {p}")
    return math.log(p / (1.0 - p))


def frame_valid(T: int, hop: int) -> np.ndarray:
    """Samples per frame of a T-sample clip: hop everywhere but the (possibly partial) last frame."""
    Fr = -(-int(T) // hop)
    v = np.full(Fr, hop, np.int64)
    v[-1] = int(T) - (Fr - 1) * hop
    return v


def segments_from_counts(count: Sequence[float], valid: Sequence[float], min_on: float = 0.5, min_gap_frames: int = 2,
                         min_len_frames: int = 5) -> List[Tuple[int, int]]:
    """Runs [f_lo, f_hi) of watermarked frames.  A frame is on when count / valid >= min_on (count = its gated samples, valid = its
    samples); gaps SHORTER than min_gap_frames are merged first, then runs shorter than min_len_frames are dropped.  With the default
    min_gap_frames = 2 two segments never touch the same frame or adjacent ones; min_len_frames = 5 is 100 ms at the default hop."""
    count, valid = np.asarray(count, np.float64).reshape(-1), np.asarray(valid, np.float64).reshape(-1)
    if count.shape != valid.shape:
        raise ValueError("count and valid need one entry per frame each")
    on = (valid > 0) & (count >= min_on * valid)
    runs: List[List[int]] = []
    f, n = 0, len(on)
    while f < n:
        if not on[f]:
            f += 1
            continue
        g = f
        while g < n and on[g]:
            g += 1
        if runs and f - runs[-1][1] < min_gap_frames:
            runs[-1][1] = g
        else:
            runs.append([f, g])
        f = g
    return [(lo, hi) for lo, hi in runs if hi - lo >= min_len_frames]


class SegmentTracker:
    """segments_from_counts + the f64 reduction of wv_frames_reduce as a STREAMING state machine over S lockstep streams: the host twin of
    wv_segment_track (csrc/wv_window.hip), the same decisions and the same order of additions, on numpy arrays.

    advance(fsum [S, nb + 1, Fr], f_lo, f_hi, last_valid, final) takes the next frames of every stream.  Per stream it holds the open run
    {lo, hi, f64 sums of every row over [lo, hi)} and the raw off frames after hi (fewer than min_gap_frames of them).  An on frame
    (valid > 0 and float64(count) >= min_on * valid) extends the open run: the held off frames are added first, one by one, then the frame,
    so the sums are those of one ascending pass over [lo, hi).  A run closes once min_gap_frames off frames have followed it, or on `final`;
    it is dropped if shorter than min_len_frames, else it becomes an event (lo, hi, count, prob [nb] float32) with
    prob = S / (float32(count) + float32(eps)) rounded once, 0 where count == 0.  poll() hands out the events closed since the last poll."""

    def __init__(self, S: int, nb: int, hop: int, min_on: float = 0.5, min_gap_frames: int = 2, min_len_frames: int = 5, eps: float = 1e-8,
                 dtype=np.float32):
        if S < 1 or nb < 1 or hop < 1 or min_gap_frames < 1 or min_len_frames < 0:
            raise ValueError("need S, nb, hop, min_gap_frames >= 1 and min_len_frames >= 0")
        self.S, self.nb, self.hop, self.min_on = int(S), int(nb), int(hop), float(min_on)
        self.G, self.min_len, self.eps, self.dtype = int(min_gap_frames), int(min_len_frames), np.float32(eps), dtype
        self.reset()

    def reset(self) -> None:
        self.frames_seen = 0
        self.closed = False
        self._open = [False] * self.S
        self._lo, self._hi = [0] * self.S, [0] * self.S
        self._acc = np.zeros((self.S, self.nb + 1), np.float64)
        self._gap: List[List[np.ndarray]] = [[] for _ in range(self.S)]         # the off frames after hi, oldest first
        self._events: List[list] = [[] for _ in range(self.S)]
        self.events_total = [0] * self.S

    def _prob(self, acc: np.ndarray) -> np.ndarray:
        cnt = acc[self.nb]
        if not cnt > 0.0:
            return np.zeros(self.nb, np.float32)
        return (acc[:self.nb] / np.float64(np.float32(cnt) + self.eps)).astype(np.float32)

    def _close(self, s: int) -> None:
        if self._hi[s] - self._lo[s] >= self.min_len:
            self._events[s].append((self._lo[s], self._hi[s], float(self._acc[s, self.nb]), self._prob(self._acc[s])))
            self.events_total[s] += 1
        self._open[s] = False
        self._gap[s] = []

    def advance(self, fsum, f_lo: int = 0, f_hi: Optional[int] = None, last_valid: Optional[int] = None, final: bool = False) -> None:
        if self.closed:
            raise RuntimeError("tracker saw its final frame; call reset() to start over")
        fsum = np.asarray(fsum, self.dtype)
        if fsum.ndim != 3 or fsum.shape[0] != self.S or fsum.shape[1] != self.nb + 1:
            raise ValueError(f"expected frame sums [{self.S}, {self.nb + 1}, Fr], got {fsum.shape}")
        f_hi = fsum.shape[2] if f_hi is None else int(f_hi)
        n = f_hi - int(f_lo)
        if n < 0 or f_lo < 0 or f_hi > fsum.shape[2]:
            raise ValueError("frames [f_lo, f_hi) lie outside fsum")
        last_valid = self.hop if last_valid is None else int(last_valid)
        cols = fsum[:, :, f_lo:f_hi].astype(np.float64)                          # exact: every value widens
        for s in range(self.S):
            for i in range(n):
                g = self.frames_seen + i
                col = cols[s, :, i]
                valid = last_valid if final and i == n - 1 else self.hop
                if valid > 0 and col[self.nb] >= self.min_on * valid:
                    if self._open[s]:
                        for off in self._gap[s]:
                            self._acc[s] += off
                    else:
                        self._open[s], self._lo[s] = True, g
                        self._acc[s] = 0.0
                    self._gap[s] = []
                    self._acc[s] += col
                    self._hi[s] = g + 1
                elif self._open[s]:
                    if g + 1 - self._hi[s] >= self.G:
                        self._close(s)
                    else:
                        self._gap[s].append(col)
            if final and self._open[s]:
                self._close(s)
        self.frames_seen += n
        self.closed = bool(final)

    def poll(self) -> List[list]:
        out, self._events = self._events, [[] for _ in range(self.S)]
        return out

    def open_runs(self) -> List[Optional[tuple]]:
        """Per stream the provisional open run (lo, hi, count, prob) over [lo, hi) as it stands (held off frames not included), or None."""
        return [(self._lo[s], self._hi[s], float(self._acc[s, self.nb]), self._prob(self._acc[s])) if self._open[s] else None
                for s in range(self.S)]


def bank_track_row_ok(row, capacity: int, nb: int, hop: int, n_fsum: int) -> bool:
    """Whether wv_bank_segment_track serves a descriptor row {slot, fsum_off, Fr_stride, f_lo, f_hi, frame0, last_valid, final} (it skips any
    other whole)."""
    slot, off, Fr, f_lo, f_hi, frame0, last_valid, _ = (int(v) for v in row)
    return (0 <= slot < capacity and 0 <= f_lo <= f_hi <= Fr <= 2 ** 31 - 1 and 0 <= off and off + (nb + 1) * Fr <= n_fsum
            and frame0 >= 0 and 0 <= last_valid <= hop)


class BankSegmentTracker:
    """`capacity` independent SegmentTracker states behind wv_bank_segment_track's descriptor interface: the host twin
    of that kernel, on numpy arrays.  advance(fsum, desc) takes fsum as ONE flat arena of frame sums and desc rows {slot, fsum_off, Fr_stride,
    f_lo, f_hi, frame0, last_valid, final}; row k of a stream's sums starts at fsum_off + k * Fr_stride, its frames this tick are columns
    [f_lo, f_hi), column f_lo being the slot's frame frame0.  A row that breaks the contract (bank_track_row_ok) is skipped whole, and so is a row
    without frames that is not final.  A slot whose state cannot follow from frame0 (an open run that does not end within min_gap_frames
    frames before it) is taken as closed, as the kernel takes it.  reset(slot) is what zeroing the slot's state and event sections is on the
    device.  `ring` is the event ring: poll() refuses, as session.HipSegmentTracker does, a slot on which more events closed since its last
    read than the ring holds."""

    def __init__(self, capacity: int, nb: int, hop: int, min_on: float = 0.5, min_gap_frames: int = 2, min_len_frames: int = 5, ring: int = 64,
                 eps: float = 1e-8, dtype=np.float32):
        if capacity < 1 or ring < 1:
            raise ValueError("need capacity, ring >= 1")
        self.capacity, self.nb, self.hop, self.ring, self.dtype = int(capacity), int(nb), int(hop), int(ring), dtype
        self.G = int(min_gap_frames)
        self._t = [SegmentTracker(1, nb, hop, min_on, min_gap_frames, min_len_frames, eps, dtype) for _ in range(self.capacity)]

    def reset(self, slot: int) -> None:
        self._t[slot].reset()

    def advance(self, fsum, desc) -> None:
        fsum = np.asarray(fsum, self.dtype).reshape(-1)
        for row in np.asarray(desc, np.int64).reshape(-1, 8):
            if not bank_track_row_ok(row, self.capacity, self.nb, self.hop, fsum.shape[0]):
                continue
            slot, off, Fr, f_lo, f_hi, frame0, last_valid, final = (int(v) for v in row)
            if f_hi == f_lo and not final:
                continue
            t = self._t[slot]
            if t._open[0] and not (0 <= t._lo[0] < t._hi[0] <= frame0 and frame0 - t._hi[0] < self.G):
                t._open[0], t._gap[0] = False, []
            t.frames_seen, t.closed = frame0, False
            t.advance(fsum[off: off + (self.nb + 1) * Fr].reshape(1, self.nb + 1, Fr), f_lo, f_hi, last_valid, bool(final))
            t.closed = False

    def frames_seen(self, slot: int) -> int:
        return self._t[slot].frames_seen

    def poll(self, slots) -> dict:
        """-> {slot: the events closed since the slot's last poll}."""
        out = {}
        for s in slots:
            evs = self._t[s].poll()[0]
            if len(evs) > self.ring:
                raise RuntimeError(f"slot {s}: {len(evs)} segments closed since the last read of a ring of {self.ring}: events were lost")
            out[s] = evs
        return out

    def open_runs(self, slots) -> dict:
        return {s: self._t[s].open_runs()[0] for s in slots}
