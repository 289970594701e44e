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
    change: Tuple[bool, bool] = (False, False)   # (start, end) is an id change found by a SplitRule, not an edge of the locator's run


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


WV_SPLIT_MAX_WINDOW = 256              # include/waveverify_hip.h


@dataclass(frozen=True)
class SplitRule:
    """Where a run of watermarked frames is cut because the decoded id changes inside it.  A frame boundary g with
    W = window_frames whole frames of the run's current piece on its left and W frames of the run on its right is a candidate; with L and R
    the per-row f64 sums of fsum over [g - W, g) and [g, g + W), S(g) = sum over the bits of |L_k / L_count - R_k / R_count| and d(g) = the
    bits whose two window means fall on different sides of 0.5.  g qualifies when S(g) >= threshold and d(g) >= min_bits; of qualifying
    candidates less than W apart the one with the largest S becomes the cut (the earliest of equals).
    The defaults are 0.5 s windows at the full-size detector's hop; they have NOT been measured on a trained detector."""
    window_frames: int = 25
    threshold: float = 0.5
    min_bits: int = 1

    def __post_init__(self):
        W, b = self.window_frames, self.min_bits
        if isinstance(W, bool) or not isinstance(W, (int, np.integer)) or not 2 <= W <= WV_SPLIT_MAX_WINDOW:
            raise ValueError(f"window_frames must be an integer in [2, {WV_SPLIT_MAX_WINDOW}], got {W!r}")
        if not float(self.threshold) > 0.0 or math.isinf(float(self.threshold)):
            raise ValueError(f"threshold must be a positive finite number, got {self.threshold!r}")
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 1:
            raise ValueError(f"min_bits must be an integer >= 1, got {b!r}")

    def check(self, nb: int, min_gap_frames: int, min_len_frames: int) -> "SplitRule":
        """The rule against the tracker it joins: max(2, min_gap_frames, min_len_frames) <= window_frames and min_bits <= nb, so that every
        piece of a run that is cut is itself long enough to be reported."""
        if self.window_frames < max(2, min_gap_frames, min_len_frames):
            raise ValueError(f"window_frames ({self.window_frames}) must be at least max(2, min_gap_frames, min_len_frames) = "
                             f"{max(2, min_gap_frames, min_len_frames)}")
        if self.min_bits > nb:
            raise ValueError(f"min_bits ({self.min_bits}) exceeds the detector's {nb} bits")
        return self


def _split_score(L: np.ndarray, R: np.ndarray):
    """Window sums [nb + 1] f64 -> (S, d, pL, pR), or None where a window has no gated sample.  S is added in ascending k."""
    nb = L.shape[0] - 1
    if not (L[nb] > 0.0 and R[nb] > 0.0):
        return None
    pL, pR = L[:nb] / L[nb], R[:nb] / R[nb]
    S = np.float64(0.0)
    for v in np.abs(pL - pR):
        S = S + v
    return S, int(((pL >= 0.5) != (pR >= 0.5)).sum()), pL, pR


def _note_margins(margins: Optional[dict], rule: SplitRule, S, d, pL, pR, cS) -> None:
    """How far the comparisons of one candidate are from going the other way (what a test of f32 sums against an f64 oracle needs)."""
    if margins is None:
        return
    m = margins.setdefault
    margins["threshold"] = min(m("threshold", np.inf), abs(float(S) - rule.threshold))
    if S >= rule.threshold:                                                      # only then does the vote decide anything
        # the vote's margin: how far from 0.5 the means are whose side would have to change before d crosses min_bits
        each = np.minimum(np.abs(pL - 0.5), np.abs(pR - 0.5))
        differ = (pL >= 0.5) != (pR >= 0.5)
        if d >= rule.min_bits:
            v = np.sort(each[differ])[::-1][rule.min_bits - 1]
        else:
            v = np.sort(each[~differ])[rule.min_bits - d - 1]
        margins["vote"] = min(m("vote", np.inf), float(v))
        if cS is not None and d >= rule.min_bits:
            margins["pending"] = min(m("pending", np.inf), abs(float(S) - float(cS)))


def split_scores(fsum_run, window_frames: int):
    """One whole run's frame sums [nb + 1, n] -> (g [m], S [m], d [m], ok [m], pL [nb, m], pR [nb, m]) for every boundary g in
    [W, n - W], relative to the run's first frame: window sums for every g at once, each an ascending f64 pass over its W frames; ok is False
    (and S is NaN) where a window holds no gated sample."""
    x = np.asarray(fsum_run)
    if x.ndim != 2 or x.shape[0] < 2:
        raise ValueError(f"expected one run's frame sums [nb + 1, n], got {x.shape}")
    x = x.astype(np.float64)
    nb, n, W = x.shape[0] - 1, x.shape[1], int(window_frames)
    gs = np.arange(W, n - W + 1)
    L, R = np.zeros((nb + 1, len(gs))), np.zeros((nb + 1, len(gs)))
    for t in range(W):
        L += x[:, gs - W + t]
        R += x[:, gs + t]
    ok = (L[nb] > 0.0) & (R[nb] > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        pL, pR = L[:nb] / L[nb], R[:nb] / R[nb]
        S = np.zeros(len(gs))
        for k in range(nb):
            S += np.abs(pL[k] - pR[k])
        d = ((pL >= 0.5) != (pR >= 0.5)).sum(0)
    return gs, S, d, ok, pL, pR


def split_points(fsum_run, rule: SplitRule, margins: Optional[dict] = None) -> List[int]:
    """The rule on ONE whole run: fsum_run [nb + 1, n] (the run's frames only, row nb the count row) -> the ascending boundaries g, relative
    to the run's first frame, at which it is cut: split_scores, then the one-pass scan.  margins: a dict that receives the smallest
    |S - threshold|, |S - pending S| and |p - 0.5| of the scan's comparisons."""
    gs, S, d, ok, pL, pR = split_scores(fsum_run, rule.window_frames)
    if rule.min_bits > pL.shape[0]:
        raise ValueError(f"min_bits ({rule.min_bits}) exceeds the {pL.shape[0]} bits")
    W = rule.window_frames
    out, plo, pend = [], 0, None
    for i, g in enumerate(int(v) for v in gs):
        if pend is not None and g - pend[0] >= W:
            out.append(pend[0])
            plo, pend = pend[0], None
        if g < plo + W or not ok[i]:
            continue
        _note_margins(margins, rule, S[i], d[i], pL[:, i], pR[:, i], None if pend is None else pend[1])
        if S[i] >= rule.threshold and d[i] >= rule.min_bits and (pend is None or S[i] > pend[1]):
            pend = (g, S[i])
    if pend is not None:
        out.append(pend[0])
    return out


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
                 dtype=np.float32, *, split: Optional[SplitRule] = None):
        if S < 1 or nb < 1 or hop < 1 or min_gap_frames < 1 or min_len_frames < 0:
            raise ValueError("need S, nb, hop, min_gap_frames >= 1 and min_len_frames >= 0")
        self.S, self.nb, self.hop, self.min_on = int(S), int(nb), int(hop), float(min_on)
        self.G, self.min_len, self.eps, self.dtype = int(min_gap_frames), int(min_len_frames), np.float32(eps), dtype
        self.split = None if split is None else split.check(self.nb, self.G, self.min_len)
        self.reset()

    def set_split(self, rule: Optional[SplitRule]) -> None:
        """Track under `rule` (None: plainly) from a fresh state."""
        self.split = None if rule is None else rule.check(self.nb, self.G, self.min_len)
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
        # with a rule: the current piece starts at _plo, _acc holds its rows over [_plo, _base), _cols the raw columns of the frames from
        # _base on (the held off frames after hi among them), _gn is the next boundary to evaluate, _pend the pending cut (g, S) or None
        self._plo, self._base, self._gn = [0] * self.S, [0] * self.S, [0] * self.S
        self._cols: List[List[np.ndarray]] = [[] for _ in range(self.S)]
        self._pend: List[Optional[tuple]] = [None] * self.S
        self.margins = {}                                                       # with a rule: the smallest margins of its comparisons so far

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
        if self.split is not None:
            for s in range(self.S):
                self._advance_split(s, cols[s], n, last_valid, final)
            self.frames_seen += n
            self.closed = bool(final)
            return
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

    # ---- with a SplitRule (the host twin of wv_segment_track_split): events carry a fifth entry (start is a change, end is a change)
    def _emit(self, s: int, end: int, end_is_change: bool) -> None:
        """The piece [plo, end): its remaining columns join the sums in ascending order, then it becomes an event."""
        while self._base[s] < end:
            self._acc[s] += self._cols[s].pop(0)
            self._base[s] += 1
        self._events[s].append((self._plo[s], end, float(self._acc[s, self.nb]), self._prob(self._acc[s]),
                                (self._plo[s] > self._lo[s], end_is_change)))
        self.events_total[s] += 1

    def _commit(self, s: int) -> None:
        cg = self._pend[s][0]
        self._emit(s, cg, True)
        self._plo[s], self._pend[s] = cg, None
        self._acc[s] = 0.0

    def _evaluate(self, s: int, g: int) -> None:
        W, cols, base = self.split.window_frames, self._cols[s], self._base[s]
        if self._pend[s] is not None and g - self._pend[s][0] >= W:
            self._commit(s)
            base = self._base[s]
        L, R = np.zeros(self.nb + 1), np.zeros(self.nb + 1)
        for j in range(g - W, g):
            L += cols[j - base]
        for j in range(g, g + W):
            R += cols[j - base]
        sc = _split_score(L, R)
        if sc is None:
            return
        S, d, pL, pR = sc
        pend = self._pend[s]
        _note_margins(self.margins, self.split, S, d, pL, pR, None if pend is None else pend[1])
        if S >= self.split.threshold and d >= self.split.min_bits and (pend is None or S > pend[1]):
            self._pend[s] = (g, S)

    def _scan(self, s: int) -> None:
        """Every boundary that has W frames of the run on its right by now, in ascending order; columns that can no longer lie after a cut
        (those before gn - W) leave the ring for the piece's sums."""
        W = self.split.window_frames
        while self._gn[s] + W <= self._hi[s]:
            self._evaluate(s, self._gn[s])
            self._gn[s] += 1
            while self._base[s] < max(self._plo[s], self._gn[s] - W):
                self._acc[s] += self._cols[s].pop(0)
                self._base[s] += 1

    def _close_split(self, s: int) -> None:
        if self._hi[s] - self._lo[s] >= self.min_len:
            if self._pend[s] is not None:
                self._commit(s)
            self._emit(s, self._hi[s], False)
        self._open[s], self._pend[s], self._cols[s] = False, None, []

    def _advance_split(self, s: int, cols: np.ndarray, n: int, last_valid: int, final: bool) -> None:
        for i in range(n):
            g = self.frames_seen + i
            col = cols[:, i]
            valid = last_valid if final and i == n - 1 else self.hop
            if valid > 0 and col[self.nb] >= self.min_on * valid:
                if not self._open[s]:
                    self._open[s], self._lo[s], self._plo[s], self._base[s] = True, g, g, g
                    self._gn[s], self._pend[s], self._cols[s] = g + self.split.window_frames, None, []
                    self._acc[s] = 0.0
                self._cols[s].append(col)
                self._hi[s] = g + 1
                self._scan(s)
            elif self._open[s]:
                if g + 1 - self._hi[s] >= self.G:
                    self._close_split(s)
                else:
                    self._cols[s].append(col)
        if final and self._open[s]:
            self._close_split(s)

    def poll(self) -> List[list]:
        out, self._events = self._events, [[] for _ in range(self.S)]
        return out

    def open_runs(self) -> List[Optional[tuple]]:
        """Per stream the provisional open run (lo, hi, count, prob) over [lo, hi) as it stands (held off frames not included), or None.
        With a rule: the current piece (plo, hi, count, prob, (its start is a change, False))."""
        if self.split is not None:
            return [self._open_piece(s) if self._open[s] else None for s in range(self.S)]
        return [(self._lo[s], self._hi[s], float(self._acc[s, self.nb]), self._prob(self._acc[s])) if self._open[s] else None
                for s in range(self.S)]

    def _open_piece(self, s: int) -> tuple:
        acc = self._acc[s].copy()
        for col in self._cols[s][:self._hi[s] - self._base[s]]:
            acc += col
        return self._plo[s], self._hi[s], float(acc[self.nb]), self._prob(acc), (self._plo[s] > self._lo[s], False)

    def split_state(self) -> List[Optional[tuple]]:
        """With a rule, per stream what wv_segment_track_split's state holds of an open run: (lo, hi, plo, pending boundary or -1, pending S,
        the piece's sums over [plo, max(plo, hi - 2 W + 1))), or None."""
        return [(self._lo[s], self._hi[s], self._plo[s], -1 if self._pend[s] is None else self._pend[s][0],
                 0.0 if self._pend[s] is None else float(self._pend[s][1]), self._acc[s].copy()) if self._open[s] else None
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
                 eps: float = 1e-8, dtype=np.float32, *, split: Optional[SplitRule] = None):
        if capacity < 1 or ring < 1:
            raise ValueError("need capacity, ring >= 1")
        self.capacity, self.nb, self.hop, self.ring, self.dtype = int(capacity), int(nb), int(hop), int(ring), dtype
        self.G, self.split = int(min_gap_frames), split
        self._t = [SegmentTracker(1, nb, hop, min_on, min_gap_frames, min_len_frames, eps, dtype, split=split) for _ in range(self.capacity)]

    def reset(self, slot: int) -> None:
        self._t[slot].reset()

    def set_split(self, rule: Optional[SplitRule]) -> None:
        for t in self._t:
            t.set_split(rule)
        self.split = rule

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
                t._open[0], t._gap[0], t._cols[0], t._pend[0] = False, [], [], None
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

    def split_state(self, slots) -> dict:
        return {s: self._t[s].split_state()[0] for s in slots}
