"""Live sessions: S audio streams watermarked, detected or located in lockstep as samples arrive.

Each push appends n >= 0 samples per stream.  The frames completed so far (a multiple of the net's hop) run as one window that
starts halo(cfg) samples before the first new frame (or at the stream's t = 0) and ends at the last completed frame; only the
new frames' columns are returned.  Incomplete-frame samples and the halo history stay on the device (wv_session_advance).
flush() runs the remaining partial frame as a final window ending at the true end, after which the concatenated outputs equal
the whole-clip forward on the concatenated input.  ("Session", not "stream", to keep clear of HIP streams.)

Segment sessions (SegmentSession, section 7d-5) run the locator and the detector's gated per-frame sums on one shared window per tick and
turn the frame sums into closed localize.Segments on the device (wv_segment_track); their push returns nothing, poll() reads.

Session banks (StreamBank, section 7d-6) drop the lockstep: `capacity` slots, each an independent stream with its own _Ticker that is opened,
pushed to (any number of samples, or not at all on a tick) and closed on its own.  The slots that complete frames on a tick become the rows of
one left-aligned, right-zero-padded window batch per pad_limit group (wv_bank_advance, the histories updated in place); per stream the
concatenated outputs are still the whole-clip forward on what it pushed.  A slot can be put into pass-through (section 7d-9): its history
still advances, it gets its input back bit for bit and joins no net launch; EmbedBank.set_message switches a stream's id, or its watermark
off, that way.

Segment banks (SegmentBank, section 7d-7) are the two together: per slot the segment session's tracker, fed by the bank's launches.  The frame
sums of a tick's launches lie in one arena, and one wv_bank_segment_track call takes a descriptor per slot with that slot's own frame range,
so the frames a short row computes on the batch's zero padding are never tracked.

The bookkeeping is independent of the backend: a session takes the net forward as a callable, the history update as another and its arrays
from NumpyArrays or TorchArrays, so the same state machine runs on the numpy oracle on a CPU.  What the lockstep and the bank classes share is
written once: _SegmentReader (tracker events -> Segments, and cut_rows, the rule that reads an event ring before it can overflow),
_HipTrackerState (the device trackers' buffers and read-backs) and _SegmentNets (the detector and the locator bound for frame sums).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from . import _lib, snr_floor
from .localize import bank_track_row_ok  # noqa: F401  (wv_bank_segment_track's row predicate, restated beside bank_row_ok)
from .window import halo as _halo

_CLOSED = "session was flushed; call reset() to start over"
_PRECISIONS = ("f32", "f16")


# ---------------------------------------------------------------------------------------------------------------- the array backends
class NumpyArrays:
    """The arrays of a session or bank on the host, in one float dtype (the float64 oracle runs pass theirs)."""

    def __init__(self, dtype=np.float32):
        self.dtype = dtype

    def zeros(self, *shape, dtype: Optional[str] = None):
        return np.zeros(shape, dtype or self.dtype)

    def cat(self, parts: list, *lead):
        """Along the last axis; no parts: an empty array [*lead, 0]."""
        return np.concatenate(parts, axis=-1) if parts else self.zeros(*lead, 0)

    def take(self, x):
        """x on this backend as a contiguous float array."""
        return np.ascontiguousarray(x, self.dtype)


class TorchArrays:
    """The same on a torch device in float32; torch is imported when the first of these is built.  dtype: what goes into a tick's table for it."""
    dtype = np.float32

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device

    def zeros(self, *shape, dtype: Optional[str] = None):
        return self.torch.zeros(shape, dtype=getattr(self.torch, dtype or "float32"), device=self.device)

    def cat(self, parts: list, *lead):
        return self.torch.cat(parts, dim=-1) if parts else self.zeros(*lead, 0)

    def take(self, x):
        return x.to(self.device, self.torch.float32).contiguous()


@dataclass
class Tick:
    """One push's plan: window = the first `wlen` samples of cat(history[:hv], new); keep its columns [keep, wlen);
    the next history = that sequence's samples [drop, drop + hv2)."""
    hv: int
    wlen: int
    keep: int
    drop: int
    hv2: int


class _Ticker:
    """Sample counts of lockstep sessions: t_in samples pushed, t_out samples emitted (a hop multiple until flush),
    history = input samples [h0, t_in) with h0 = max(0, t_out - H)."""

    def __init__(self, hop: int, H: int):
        self.hop, self.H = hop, H
        self.cap = H + hop
        self.reset()

    def reset(self):
        self.t_in = self.t_out = self.h0 = 0
        self.closed = False

    def push(self, n: int) -> Tick:
        if self.closed:
            raise RuntimeError(_CLOSED)
        hv = self.t_in - self.h0
        t_in = self.t_in + n
        t_new = t_in // self.hop * self.hop
        wlen = keep = 0
        h0 = self.h0
        if t_new > self.t_out:
            wlen, keep = t_new - self.h0, self.t_out - self.h0
            h0 = max(0, t_new - self.H)
            self.t_out = t_new
        tick = Tick(hv, wlen, keep, h0 - self.h0, t_in - h0)
        self.t_in, self.h0 = t_in, h0
        return tick

    def flush(self) -> Tick:
        if self.closed:
            raise RuntimeError(_CLOSED)
        hv = self.t_in - self.h0
        wlen = hv if self.t_in > self.t_out else 0
        tick = Tick(hv, wlen, self.t_out - self.h0, hv, 0)
        self.t_out = self.t_in
        self.closed = True
        return tick


def numpy_advance(hist: np.ndarray, x: np.ndarray, t: Tick):
    """Reference of wv_session_advance on host arrays: hist [S, cap], x [S, n] -> (window [S,1,wlen], next history [S, cap])."""
    seq = np.concatenate([hist[:, :t.hv], x], axis=1)
    nxt = np.zeros_like(hist)
    nxt[:, :t.hv2] = seq[:, t.drop:t.drop + t.hv2]
    return seq[:, None, :t.wlen].copy(), nxt


class StreamSession:
    """Lockstep state machine over S streams.  forward(window [S,1,L], keep) -> that window's result for its columns
    [keep, L); advance(history, x, Tick) -> (window, next history); arrays: the backend of the history (NumpyArrays() if None).
    Subclasses bind all three to a HipNet."""

    def __init__(self, S: int, hop: int, H: int, forward: Callable, advance: Callable = numpy_advance, arrays=None):
        if S < 1:
            raise ValueError("need at least one session")
        self.S = S
        self._t = _Ticker(hop, H)
        self._forward, self._advance = forward, advance
        self._arr = arrays or NumpyArrays()
        self.reset()

    @property
    def samples_seen(self) -> int:
        """Samples whose outputs have been produced."""
        return self._t.t_out

    def reset(self) -> None:
        self._t.reset()
        self._hist = self._arr.zeros(self.S, self._t.cap)
        self._on_reset()

    def _on_reset(self) -> None:
        pass

    def _step(self, x, t: Tick):
        win, self._hist = self._advance(self._hist, x, t)
        return self._forward(win, t.keep) if t.wlen > 0 else None

    def push(self, x):
        if x.shape[0] != self.S or len(x.shape) != 2:
            raise ValueError(f"expected new samples of shape [{self.S}, n], got {tuple(x.shape)}")
        return self._step(x, self._t.push(int(x.shape[1])))

    def flush(self):
        return self._step(self._arr.zeros(self.S, 0), self._t.flush())


class _HipSession(StreamSession):
    """StreamSession on a HipNet: history, window and outputs stay on the device."""

    def __init__(self, net, S: int, precision: str = "f32"):
        if precision not in _PRECISIONS:
            raise ValueError("precision must be 'f32' or 'f16'")
        arrays = TorchArrays(net.device)
        self.net, self.precision, self._torch = net, precision, arrays.torch
        super().__init__(S, net.cfg.hop_length, _halo(net.cfg), self._net_forward, self._hip_advance, arrays)

    def _hip_advance(self, hist, x, t: Tick):
        torch = self._torch
        x = self._arr.take(x)
        nxt = torch.empty_like(hist)
        win = torch.empty((self.S, 1, t.wlen), dtype=torch.float32, device=self.net.device)
        with torch.cuda.device(self.net.device):
            _lib.check(self.net._lib.wv_session_advance(
                hist.data_ptr(), hist.shape[1], t.hv, x.data_ptr() if x.numel() else None, x.shape[1],
                win.data_ptr() if t.wlen else None, t.wlen, nxt.data_ptr(), t.drop, t.hv2, self.S,
                _lib.stream()),
                "wv_session_advance")
        return win, nxt


class _ColumnsSession(_HipSession):
    """A _HipSession that returns the kept columns of _net(window [S, 1, L]) -> [S, 1, L]: [S, 1, k], k = 0 where no frame completed."""

    def _net_forward(self, win, keep):
        return self._net(win)[:, :, keep:].contiguous()

    def _step(self, x, t: Tick):
        y = super()._step(x, t)
        return self._arr.zeros(self.S, 1, 0) if y is None else y


class EmbedSession(_ColumnsSession):
    """Watermark S live streams: push(x [S, n]) -> watermarked samples of the frames completed by this push [S, 1, k].
    add_input=False: the generator's residual alone (what native_session.py brings back to a stream's own rate)."""

    def __init__(self, net, msg, precision: str = "f32", add_input: bool = True):
        import torch
        msg = torch.as_tensor(msg).to(net.device).float()
        if msg.dim() == 1:
            msg = msg.unsqueeze(0)
        self.msg, self.add_input = msg.contiguous(), bool(add_input)
        super().__init__(net, msg.shape[0], precision)

    def _net(self, win):
        return self.net.generator(win, self.msg, add_input=self.add_input, precision=self.precision)


class LocateSession(_ColumnsSession):
    """Locate the watermark in S live streams: push(x [S, n]) -> locator logits of the newly completed frames [S, 1, k]."""

    def _net(self, win):
        return self.net.locator(win, precision=self.precision)


@dataclass
class DetectState:
    mean_prob: object      # [S, nbits] time-averaged sigmoid over the samples seen
    bits: object           # [S, nbits] int32, mean_prob >= 0.5
    samples_seen: int


class DetectSession(_HipSession):
    """Detect the watermark in S live streams: push(x [S, n]) -> the running DetectState over every completed frame so far.
    Each window's sigmoid sum over its new columns (the head's windowed mode) is added to an f64 accumulator."""

    def _on_reset(self):
        self._acc = self._arr.zeros(self.S, self.net.cfg.head_bits, dtype="float64")

    def _net_forward(self, win, keep):
        L = win.shape[-1]
        return self.net.detector_window_psum(win, [keep] * self.S, [L] * self.S, precision=self.precision)

    def _step(self, x, t: Tick):
        psum = super()._step(x, t)
        if psum is not None:
            self._acc += psum.double()
        mp = (self._acc / max(self.samples_seen, 1)).float()
        return DetectState(mp, (mp >= 0.5).to(self._torch.int32), self.samples_seen)


# ---------------------------------------------------------------------------------------------------------------- live segment sessions
def segment_halo(detector_cfg, locator_cfg) -> int:
    """History of a session that runs both nets on ONE window per tick, in samples: the hop is the detector's, the locator's hop must divide
    it, and the halo is the larger of the detector's and the locator's rounded up to that hop."""
    hop, lhop = detector_cfg.hop_length, locator_cfg.hop_length
    if hop % lhop:
        raise ValueError(f"the locator's hop ({lhop}) does not divide the detector's ({hop}): the two nets cannot share one window")
    return max(_halo(detector_cfg), -(-_halo(locator_cfg) // hop) * hop)


def cut_rows(rows: list, unread: list, ring: int, period: int, hop: int):
    """The rule that reads an event ring before it can overflow.  rows: a tick's tracker descriptors {stream, fsum_off, Fr_stride, f_lo, f_hi,
    frame0, last_valid, final}; unread[stream]: frames tracked since the rings were last read, which bound the stream's waiting events by
    frames // period + 1 (two closes lie at least `period` frames apart).  -> ([(read the rings first, rows)], unread after them): the rows
    cut into pieces so that no stream's bound reaches `ring` between two reads.  A tick of ordinary pushes is one piece."""
    step = max(1, ring * period - 1)                                       # frames // period + 1 <= ring
    unread = list(unread)
    out, left = [], rows
    while left:
        m = [min(step, r[4] - r[3]) for r in left]
        drain = any(unread[r[0]] and (unread[r[0]] + k) // period + 1 >= ring for r, k in zip(left, m))
        if drain:
            unread = [0] * len(unread)
        piece, nxt = [], []
        for (s, off, Fr, lo, hi, f0, lv, fin), k in zip(left, m):
            last = lo + k == hi
            piece.append([s, off, Fr, lo, lo + k, f0, lv if last else hop, fin if last else 0])
            unread[s] += k
            if not last:
                nxt.append([s, off, Fr, lo + k, hi, f0 + k, lv, fin])
        out.append((drain, piece))
        left = nxt
    return out, unread


def _open_run_of(hdr, acc, nb: int, eps: float):
    """One stream's header and sums as ops.segment_state reads them -> its provisional open run (lo, hi, count, prob), or None."""
    if not hdr[0]:
        return None
    cnt = acc[nb]
    prob = (acc[:nb] / np.float64(np.float32(cnt) + np.float32(eps))).astype(np.float32) if cnt > 0.0 else np.zeros(nb, np.float32)
    return int(hdr[1]), int(hdr[2]), float(cnt), prob


def _open_piece_of(hdr, acc, ring, nb: int, W: int, eps: float):
    """One stream's header, sums and ring as ops.split_state reads them -> its current piece (plo, hi, count, prob, (start is a change,
    False)), or None: the ring's columns [sb, hi) join the sums in ascending order, as the kernel will add them."""
    if not hdr[0]:
        return None
    lo, hi, plo = int(hdr[1]), int(hdr[2]), int(hdr[4])
    acc = acc.copy()
    for j in range(max(plo, hi - 2 * W + 1), hi):
        acc += ring[j % ring.shape[0]].astype(np.float64)
    cnt = acc[nb]
    prob = (acc[:nb] / np.float64(np.float32(cnt) + np.float32(eps))).astype(np.float32) if cnt > 0.0 else np.zeros(nb, np.float32)
    return plo, hi, float(cnt), prob, (plo > lo, False)


class _SegmentReader:
    """What a segment session and a segment bank do with their tracker's events: hop, sample_rate, the event ring and the period of cut_rows,
    per stream the Segments closed and not yet handed out, per ring-reading unit the frames tracked since its last read (a lockstep session
    has ONE frame range, so one counter; a bank one per slot).  The class beside it says which streams exist:
    _streams(read) -> [(stream, samples it has pushed, what read() holds for it)], read being the tracker's poll or open_runs."""

    def _init_reader(self, hop: int, sample_rate: int, ring: int, min_gap_frames: int, min_len_frames: int) -> None:
        self.hop, self.sample_rate, self.ring = hop, int(sample_rate), int(ring)
        self._period = max(1, int(min_len_frames) + int(min_gap_frames))
        self._cut_ring = self.ring
        self.split = None

    def _set_split(self, rule) -> None:
        """The tracker takes the rule (and checks it against its own parameters).  Under a rule a stream can close more events over the same
        frames: cuts inside a run lie at least window_frames >= period / 2 frames apart and a close can emit two pieces at once, fewer than
        6 (frames // period + 1) events in all, so cut_rows works with a sixth of the ring."""
        if rule is not None and self.ring < 6:
            raise ValueError(f"a split rule needs an event ring of at least 6, got {self.ring}")
        self._tracker.set_split(rule)
        self.split, self._cut_ring = rule, self.ring if rule is None else self.ring // 6

    def _clear_reader(self, streams: int, counters: int) -> None:
        self._pending = [[] for _ in range(streams)]
        self._unread = [0] * counters

    def _confidence(self, prob: np.ndarray) -> float:
        return float(np.asarray(prob, np.float32).mean())

    def _segment_of(self, ev, t_in: int):
        """A tracker event (lo, hi, count, prob) of a stream that has pushed t_in samples -> localize.Segment.  t_in is the true length once
        the stream has ended and never short of a closed run before, so `end` is clipped only on the partial last frame."""
        from .localize import Segment
        from .watermark_id import WatermarkID
        lo, hi, count, prob = ev[:4]
        change = tuple(bool(c) for c in ev[4]) if len(ev) > 4 else (False, False)
        hop, fs = self.hop, self.sample_rate
        end = min(int(hi) * hop, t_in)
        prob = np.asarray(prob, np.float32)
        bits = "".join("1" if p >= np.float32(0.5) else "0" for p in prob)
        wid = WatermarkID.custom(bits) if len(bits) == 16 else None        # an id has 16 bits; a net of another width leaves prob to read
        return Segment(int(lo) * hop / fs, end / fs, wid, self._confidence(prob), float(count) / (end - int(lo) * hop), prob, (int(lo), int(hi)),
                       change)

    def _drain(self) -> None:
        """Read the rings (the one host synchronisation a push can make)."""
        for s, t_in, evs in self._streams(self._tracker.poll):
            if evs:
                self._pending[s] += [self._segment_of(ev, t_in) for ev in evs]
        self._unread = [0] * len(self._unread)

    def _taken(self, s: int) -> list:
        out, self._pending[s] = self._pending[s], []
        return out

    def _open_now(self) -> list:
        """-> [(stream, the run that is open now as a provisional Segment (its frames so far), or None)]."""
        return [(s, None if ev is None else self._segment_of(ev, t_in)) for s, t_in, ev in self._streams(self._tracker.open_runs)]

    def _cut(self, rows: list):
        return cut_rows(rows, self._unread, self._cut_ring, self._period, self.hop)


class SegmentStreamSession(_SegmentReader, StreamSession):
    """Localized detection of S live streams: push(x [S, n], gate=None) returns nothing; the watermarked stretches
    come out of poll() as localize.Segments once they have ended.  Backend independent: frame_sums(window [S,1,L], gate window [S,L] or
    None) -> the window's per-frame gated sums [S, nb + 1, ceil(L / hop)] (without a gate window it runs the locator itself), `tracker` has
    the interface of localize.SegmentTracker.  A tick hands the tracker the window's frames from keep / hop on.

    gate [S, n] (0 / 1) replaces the locator; its samples of an incomplete frame wait in a second history that goes through the same
    `advance`.  Whether a session is gated is settled by its first push and holds until reset().

    capacity is the tracker's event ring.  Before a tick would let cut_rows' bound on the events waiting there reach capacity the session reads
    the ring itself, and a long push is tracked in pieces that stay within it, so nothing is lost."""

    def __init__(self, S: int, hop: int, H: int, frame_sums: Callable, tracker, advance: Callable = numpy_advance, arrays=None,
                 sample_rate: int = 16000, capacity: int = 64, min_gap_frames: int = 2, min_len_frames: int = 5):
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        self._frame_sums, self._tracker = frame_sums, tracker
        self._init_reader(hop, sample_rate, capacity, min_gap_frames, min_len_frames)
        self.capacity = self.ring
        StreamSession.__init__(self, S, hop, H, None, advance, arrays)

    def _on_reset(self) -> None:
        self._ghist = None
        self._gated: Optional[bool] = None
        self._clear_reader(self.S, 1)
        self._tracker.reset()

    def _streams(self, read: Callable) -> list:
        t_in = self._t.t_in
        return [(s, t_in, v) for s, v in enumerate(read())]

    def poll(self):
        """-> per stream the Segments closed since the last poll, in stream order."""
        self._drain()
        return [self._taken(s) for s in range(self.S)]

    def open_segments(self):
        """-> per stream the run that is open now as a provisional Segment (its frames so far), or None.  Under a split rule: the run's
        current piece."""
        return [seg for _, seg in self._open_now()]

    def set_split(self, rule) -> None:
        """Cut runs where the decoded id changes (localize.SplitRule; None: off).  Only before the first push (or
        after reset()); poll(), flush() and open_segments() then deal in pieces, known 2 * window_frames frames after a change."""
        if self._gated is not None:
            raise RuntimeError("set_split is legal only before the first push; reset() first")
        self._set_split(rule)

    # ---- ticks
    def _track(self, fsum, f_lo: int, f_hi: int, last_valid: int, final: bool) -> None:
        pieces, unread = self._cut([[0, 0, 0, f_lo, f_hi, 0, last_valid, int(final)]])
        for drain, ((_, _, _, lo, hi, _, lv, fin),) in pieces:
            if drain:
                self._drain()
            self._tracker.advance(fsum, lo, hi, lv, bool(fin))
        self._unread = unread

    def _gate_window(self, gate, x, t: Tick):
        if self._gated is None:
            self._gated = gate is not None
            if self._gated:
                self._ghist = self._arr.zeros(self.S, self._t.cap)
        if self._gated != (gate is not None):
            raise ValueError("a session is gated on every push or on none; reset() to change")
        if not self._gated:
            return None
        if tuple(gate.shape) != tuple(x.shape):
            raise ValueError(f"gate must have the samples' shape {tuple(x.shape)}, got {tuple(gate.shape)}")
        gwin, self._ghist = self._advance(self._ghist, gate, t)
        return gwin.reshape(self.S, t.wlen)

    def _tick(self, x, gate, t: Tick, final: bool) -> None:
        gwin = self._gate_window(gate, x, t)
        win, self._hist = self._advance(self._hist, x, t)
        hop = self.hop
        if t.wlen > 0:
            fsum = self._frame_sums(win, gwin)
            f_hi = -(-t.wlen // hop)
            self._track(fsum, t.keep // hop, f_hi, t.wlen - (f_hi - 1) * hop, final)
        elif final:
            self._track(self._arr.zeros(self.S, self._tracker.nb + 1, 0), 0, 0, hop, True)

    def push(self, x, gate=None) -> None:
        if x.shape[0] != self.S or len(x.shape) != 2:
            raise ValueError(f"expected new samples of shape [{self.S}, n], got {tuple(x.shape)}")
        self._tick(x, gate, self._t.push(int(x.shape[1])), False)

    def flush(self):
        """The partial last frame, if any, runs with its true length, every open run closes -> the Segments not yet polled."""
        t = self._t.flush()
        if self._unread[0]:
            self._drain()                                                  # a close at `final` may follow the last one closely
        e = self._arr.zeros(self.S, 0)
        self._tick(e, e if self._gated else None, t, True)
        return self.poll()


class _HipTrackerState:
    """The state and the event rings of n streams on the device, in wv_segment_track's per-stream layouts, with the host's read cursors:
    what HipSegmentTracker and HipBankSegmentTracker hold, and their two read-backs (one device-to-host copy each)."""
    _what = "stream"

    def __init__(self, n: int, nb: int, hop: int, min_on: float, min_gap_frames: int, min_len_frames: int, ring: int, device, eps: float):
        import torch
        from . import ops
        self.nb, self.hop, self.min_on = int(nb), int(hop), float(min_on)
        self.G, self.min_len, self.eps, self.device = int(min_gap_frames), int(min_len_frames), float(eps), device
        self._n, self._ring, self._torch, self._ops = int(n), int(ring), torch, ops
        self._size(None)

    def _size(self, rule) -> None:
        """The buffers' sizes without or with a split rule (the two kernels have layouts of their own)."""
        ops = self._ops
        with self._torch.cuda.device(self.device):                                                # refuses what the kernel would
            self._bytes = (ops.segment_track_bytes(self._n, self.nb, self.G, self._ring) if rule is None else
                           ops.segment_split_bytes(self._n, self.nb, self.G, rule.window_frames, self._ring))
        self._strides = (self._bytes[0] // self._n, self._bytes[1] // self._n)
        self.split = rule

    def set_split(self, rule) -> None:
        """Track under `rule` (None: plainly) from zeroed buffers: the split kernels replace the plain ones."""
        if rule is not None:
            rule.check(self.nb, self.G, self.min_len)
        self._size(rule)
        self._clear()

    def _clear(self) -> None:
        torch = self._torch
        self.state = torch.zeros(self._bytes[0], dtype=torch.uint8, device=self.device)
        self.events = torch.zeros(self._bytes[1], dtype=torch.uint8, device=self.device)
        self._read = [0] * self._n

    def _new_events(self, streams) -> list:
        """-> [(stream, its events (lo, hi, count, prob) since the last read)]; refuses a ring that has been overrun."""
        rule = self.split
        n, recs = (self._ops.segment_events if rule is None else self._ops.split_events)(self.events, self._n, self.nb, self._ring)
        out = []
        for s in streams:
            new = int(n[s]) - self._read[s]
            if new > self._ring:
                raise RuntimeError(f"{self._what} {s}: {new} segments closed since the last read of a ring of {self._ring}: events were lost")
            new = [(int(r["lo"]), int(r["hi"]), float(r["count"]), r["prob"].copy()) +
                   (() if rule is None else ((bool(r["flags"] & 1), bool(r["flags"] & 2)),))
                   for r in (recs[s, e % self._ring] for e in range(self._read[s], int(n[s])))]
            out.append((s, new))
            self._read[s] = int(n[s])
        return out

    def _open_runs_of(self, streams) -> list:
        if self.split is not None:
            W = self.split.window_frames
            hdr, _, acc, ring = self._ops.split_state(self.state, self._n, self.nb, self.G, W)
            return [(s, _open_piece_of(hdr[s], acc[s], ring[s], self.nb, W, self.eps)) for s in streams]
        hdr, acc = self._ops.segment_state(self.state, self._n, self.nb)
        return [(s, _open_run_of(hdr[s], acc[s], self.nb, self.eps)) for s in streams]

    def split_state(self, streams) -> list:
        """-> [(stream, localize.SegmentTracker.split_state's tuple or None)], read from the device."""
        hdr, cS, acc, _ = self._ops.split_state(self.state, self._n, self.nb, self.G, self.split.window_frames)
        return [(s, (int(hdr[s][1]), int(hdr[s][2]), int(hdr[s][4]), int(hdr[s][6]) if hdr[s][5] else -1, float(cS[s]) if hdr[s][5] else 0.0,
                     acc[s].copy()) if hdr[s][0] else None) for s in streams]


class HipSegmentTracker(_HipTrackerState):
    """localize.SegmentTracker's interface on wv_segment_track: state and event ring stay on the device; advance() is one launch and no
    synchronisation, poll() and open_runs() are one device-to-host copy each."""

    def __init__(self, S: int, nb: int, hop: int, min_on: float, min_gap_frames: int, min_len_frames: int, capacity: int, device,
                 eps: float = 1e-8):
        super().__init__(S, nb, hop, min_on, min_gap_frames, min_len_frames, capacity, device, eps)
        self.S, self.capacity = self._n, self._ring
        self.reset()

    def reset(self) -> None:
        self._clear()
        self.frames_seen, self.closed = 0, False

    def set_split(self, rule) -> None:
        super().set_split(rule)
        self.frames_seen, self.closed = 0, False

    def advance(self, fsum, f_lo: int = 0, f_hi: Optional[int] = None, last_valid: Optional[int] = None, final: bool = False) -> None:
        if self.closed:
            raise RuntimeError("tracker saw its final frame; call reset() to start over")
        f_hi = int(fsum.shape[2]) if f_hi is None else int(f_hi)
        lv = self.hop if last_valid is None else last_valid
        with self._torch.cuda.device(self.device):
            if self.split is None:
                self._ops.segment_track(fsum, f_lo, f_hi, self.frames_seen, self.hop, lv, final, self.min_on, self.G, self.min_len, self.state,
                                        self.events, self.capacity, self.eps)
            else:
                self._ops.segment_track_split(fsum, f_lo, f_hi, self.frames_seen, self.hop, lv, final, self.min_on, self.G, self.min_len,
                                              self.split, self.state, self.events, self.capacity, self.eps)
        self.frames_seen += f_hi - int(f_lo)
        self.closed = bool(final)

    def poll(self):
        return [evs for _, evs in self._new_events(range(self.S))]

    def open_runs(self):
        return [run for _, run in self._open_runs_of(range(self.S))]


class _SegmentNets:
    """A detector and a locator HipNet bound for localized detection, as SegmentSession and SegmentBank use them: frame_sums(window batch,
    gate windows or None) is the detector's frames kernel gated by the caller's 0 / 1 gate or by the locator's logits on the same windows."""

    def _bind(self, detector, locator, threshold: float, precision: str, locator_precision: Optional[str], ring: int, ring_name: str):
        """Refuses what cannot work before anything is built on the device -> (hop, halo) of the one window the two nets share."""
        from .localize import gate_threshold
        locator_precision = precision if locator_precision is None else locator_precision
        if precision not in _PRECISIONS or locator_precision not in _PRECISIONS:
            raise ValueError("precision must be 'f32' or 'f16'")
        if detector.cfg.kind != "detector" or locator.cfg.kind != "locator":
            raise ValueError("need a detector and a locator")
        if ring < 1:
            raise ValueError(f"{ring_name} must be at least 1")
        self._arr = TorchArrays(detector.device)
        self.net, self.locator, self.precision, self.locator_precision, self._torch = detector, locator, precision, locator_precision, self._arr.torch
        self._logit_thr = gate_threshold(threshold)
        return detector.cfg.hop_length, segment_halo(detector.cfg, locator.cfg)

    def frame_sums(self, win, gwin, out=None):
        if gwin is not None:
            return self.net.detector_frame_sums(win, gwin, 0.5, self.precision, out=out)
        return self.net.detector_frame_sums(win, self.locator.locator(win, precision=self.locator_precision), self._logit_thr, self.precision,
                                            out=out)

    def _confidence(self, prob: np.ndarray) -> float:
        return float(self._torch.from_numpy(np.ascontiguousarray(prob, np.float32)).mean())      # as WaveVerify._segments takes it


class SegmentSession(_SegmentNets, SegmentStreamSession, _HipSession):
    """SegmentStreamSession on a detector and a locator HipNet: one history and one window per tick for both nets, the locator's logits (or
    the caller's gate) gating the detector's frames kernel, one wv_segment_track per tick.  Nothing comes back to the host in push()."""

    def __init__(self, detector, locator, S: int, threshold: float = 0.5, min_on: float = 0.5, min_gap_frames: int = 2,
                 min_len_frames: int = 5, precision: str = "f32", locator_precision: Optional[str] = None, sample_rate: int = 16000,
                 capacity: int = 64):
        hop, H = self._bind(detector, locator, threshold, precision, locator_precision, capacity, "capacity")
        tracker = HipSegmentTracker(S, detector.cfg.head_bits, hop, min_on, min_gap_frames, min_len_frames, capacity, detector.device)
        SegmentStreamSession.__init__(self, S, hop, H, self.frame_sums, tracker, self._hip_advance, self._arr, sample_rate, capacity,
                                      min_gap_frames, min_len_frames)


# ---------------------------------------------------------------------------------------------------------------- session banks
@dataclass
class BankLaunch:
    """One wv_bank_advance call and, where A > 0, one net forward on its [A, 1, Lmax] window batch: rows [p_lo, p_hi) of the tick's descriptor
    table, the first A of them the windows (row r of the batch is descriptor p_lo + r and window a_lo + r of the tick).  passthrough: the
    rows are slots in pass-through, and the launch's "forward" is the window batch itself."""
    p_lo: int
    p_hi: int
    a_lo: int
    A: int
    Lmax: int
    passthrough: bool = False


@dataclass
class BankPlan:
    """One tick of a bank, integers only.  desc [P, 8] int64 = {slot, hv, x_off, n, row, wlen, drop, hv2} as wv_bank_advance reads it; slots: the
    pushed slots in the order their samples are packed; windows: [(slot, Tick)] launch by launch, row by row; out: slot -> (offset, count) of
    its new columns in the tick's packed output of n_out samples; padded: samples the launches run only as right padding."""
    desc: np.ndarray
    launches: list
    slots: list
    n_x: int
    windows: list
    out: dict
    n_out: int
    padded: int


def plan_tick(ticks: dict, sizes: dict, pad_limit: float = 1.5, passthrough=frozenset()) -> BankPlan:
    """ticks {slot: Tick}, sizes {slot: samples pushed} -> the tick's launches.  The windows are sorted by (wlen, slot) and cut greedily
    wherever the next would be longer than pad_limit times the shortest of the launch, so a launch pads no row by more than that factor.
    Slots that complete no frame ride in the first launch (a launch of their own without windows if there is none); a slot with nothing to
    do at all has no descriptor.
    passthrough: slots whose windows go through no net.  Those that complete frames form ONE launch of their own after the others, whatever
    their lengths (its forward is the window batch itself, so padding costs a copy and no arithmetic); it counts nothing towards `padded`."""
    slots = sorted(ticks)
    x_off, n_x = {}, 0
    for s in slots:
        x_off[s] = n_x
        n_x += sizes[s]
    groups: list = []
    for s in sorted((s for s in slots if ticks[s].wlen > 0 and s not in passthrough), key=lambda s: (ticks[s].wlen, s)):
        if groups and ticks[s].wlen <= pad_limit * ticks[groups[-1][0]].wlen:
            groups[-1].append(s)
        else:
            groups.append([s])
    through = sorted((s for s in slots if ticks[s].wlen > 0 and s in passthrough), key=lambda s: (ticks[s].wlen, s))
    n_net = len(groups)                                                # the groups from here on are pass-through
    if through:
        groups.append(through)
    idle = [s for s in slots if ticks[s].wlen == 0 and sizes[s] > 0]
    if idle and not groups:
        groups.append([])
        n_net = 1
    rows, launches, windows, out, n_out, padded = [], [], [], {}, 0, 0
    for g, members in enumerate(groups):
        p_lo, a_lo = len(rows), len(windows)
        Lmax = ticks[members[-1]].wlen if members else 0
        for r, s in enumerate(members):
            t = ticks[s]
            rows.append([s, t.hv, x_off[s], sizes[s], r, t.wlen, t.drop, t.hv2])
            windows.append((s, t))
            out[s] = (n_out, t.wlen - t.keep)
            n_out += t.wlen - t.keep
            padded += Lmax - t.wlen if g < n_net else 0
        for s in (idle if g == 0 else ()):
            t = ticks[s]
            rows.append([s, t.hv, x_off[s], sizes[s], 0, 0, t.drop, t.hv2])
        launches.append(BankLaunch(p_lo, len(rows), a_lo, len(members), Lmax, g >= n_net))
    for s in slots:
        out.setdefault(s, (n_out, 0))
    return BankPlan(np.array(rows, np.int64).reshape(-1, 8), launches, slots, n_x, windows, out, n_out, padded)


def bank_row_ok(row, capacity: int, hcap: int, n_x: int, A: int, Lmax: int) -> bool:
    """Whether wv_bank_advance serves a descriptor row (it skips any other whole)."""
    slot, hv, x_off, n, r, wlen, drop, hv2 = (int(v) for v in row)
    return (0 <= slot < capacity and 0 <= hv <= hcap and 0 <= hv2 <= hcap and n >= 0 and drop >= 0 and drop + hv2 == hv + n
            and 0 <= wlen <= min(hv + n, Lmax) and 0 <= x_off and x_off + n <= n_x and (wlen == 0 or 0 <= r < A))


def numpy_bank_advance(hist: np.ndarray, x: np.ndarray, desc: np.ndarray, A: int, Lmax: int) -> np.ndarray:
    """Reference of wv_bank_advance on host arrays: hist [capacity, hcap] is updated IN PLACE (only the named slots, only [0, hv2)), x the
    packed new samples -> win [A, 1, Lmax], zeros beyond each row's wlen (and in rows no descriptor names, which the kernel leaves alone)."""
    capacity, hcap = hist.shape
    win = np.zeros((A, 1, Lmax), hist.dtype)
    for row in desc:
        if not bank_row_ok(row, capacity, hcap, int(x.shape[0]), A, Lmax):
            continue
        slot, hv, x_off, n, r, wlen, drop, hv2 = (int(v) for v in row)
        seq = np.concatenate([hist[slot, :hv], x[x_off:x_off + n]])
        if wlen:
            win[r, 0, :wlen] = seq[:wlen]
        hist[slot, :hv2] = seq[drop:drop + hv2]
    return win


class StreamBank:
    """`capacity` independent live streams: each slot has its own _Ticker, is opened, pushed to and closed on its own,
    and the slots that complete frames on a tick share one launch per net (per pad_limit group).  forward(window batch [A, 1, Lmax], slots)
    -> [A, C, Lmax]; advance(history, packed x, desc, A, Lmax) -> window batch, the history updated in place (numpy_bank_advance's contract);
    arrays: the backend of the histories (NumpyArrays() if None).
    A window batch is left-aligned: column 0 of row r is that stream's own h0, rows are zero beyond their wlen; the nets are causal and
    push-time wlen are hop multiples, so the padding changes no kept column.  close() runs its ragged window alone, at its true length.
    This base class runs on host arrays; push / close return per slot the kept columns [C, k], or None where nothing completed.
    A slot in PASS-THROUGH (set_passthrough; section 7d-9) still advances its history with every push, so that the net finds real context
    when it is switched back in, but takes part in no forward: it gets back the window's own columns [keep, wlen), its input bit for bit."""

    def __init__(self, capacity: int, hop: int, H: int, forward: Optional[Callable], advance: Optional[Callable] = numpy_bank_advance,
                 arrays=None, pad_limit: float = 1.5):
        if capacity < 1:
            raise ValueError("a bank needs at least one slot")
        if not pad_limit >= 1.0:
            raise ValueError("pad_limit must be at least 1 (float('inf'): one launch per tick)")
        self.capacity, self.pad_limit = int(capacity), float(pad_limit)
        self.hop, self.H, self.hcap = hop, H, H + hop
        self._tickers = [_Ticker(hop, H) for _ in range(self.capacity)]
        self._is_open = [False] * self.capacity
        self._through: set = set()                                         # the slots in pass-through
        self._forward, self._advance = forward, advance
        self._arr = arrays or NumpyArrays()
        self._hist = self._arr.zeros(self.capacity, self.hcap)
        self.stats = {"ticks": 0, "launches": 0, "window_samples": 0, "padded_samples": 0}

    # ---- slots
    def open(self, *args) -> int:
        """-> the lowest free slot, starting from nothing: its ticker is reset, so the history the slot's last stream left is never read."""
        for slot, taken in enumerate(self._is_open):
            if not taken:
                self._through.discard(slot)
                self._on_open(slot, *args)
                self._tickers[slot].reset()
                self._is_open[slot] = True
                return slot
        raise RuntimeError(f"all {self.capacity} slots of the bank are open")

    def _on_open(self, slot: int) -> None:
        pass

    def open_slots(self) -> list:
        return [s for s, taken in enumerate(self._is_open) if taken]

    def samples_seen(self, slot: int) -> int:
        """Samples of the slot's stream whose outputs have been produced."""
        self._check_slot(slot)
        return self._tickers[slot].t_out

    def set_passthrough(self, slot: int, on: bool) -> int:
        """Puts the slot into pass-through, or back under the net, from its next frame on -> that frame's first sample (samples_seen(slot), a
        hop multiple).  Samples already pushed towards that frame are emitted under the new setting."""
        self._check_slot(slot)
        (self._through.add if on else self._through.discard)(slot)
        return self._tickers[slot].t_out

    def _check_slot(self, slot) -> None:
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or not 0 <= slot < self.capacity or not self._is_open[slot]:
            raise ValueError(f"slot {slot!r} is not open")

    # ---- ticks
    def push(self, items: dict) -> dict:
        """{slot: 1-D samples, any length} -> {slot: this push's result}.  Everything is checked before any stream's state changes."""
        for slot, x in items.items():
            self._check_slot(slot)
            if len(x.shape) != 1:
                raise ValueError(f"slot {slot}: expected 1-D samples, got shape {tuple(x.shape)}")
        return self._tick(items, {slot: self._tickers[slot].push(int(x.shape[0])) for slot, x in items.items()})

    def close(self, slot: int):
        """The stream's partial last frame at its true length (what flush() is to a lockstep session) -> its last result; frees the slot."""
        self._check_slot(slot)
        out = self._tick({slot: self._arr.zeros(0)}, {slot: self._tickers[slot].flush()})[slot]
        self._is_open[slot] = False
        return out

    def _plan(self, xs: dict, ticks: dict) -> BankPlan:
        plan = plan_tick(ticks, {s: int(x.shape[0]) for s, x in xs.items()}, self.pad_limit, self._through)
        self.stats["ticks"] += 1
        self.stats["launches"] += sum(1 for ln in plan.launches if ln.A and not ln.passthrough)
        self.stats["window_samples"] += sum(ln.A * ln.Lmax for ln in plan.launches if not ln.passthrough)
        self.stats["padded_samples"] += plan.padded
        return plan

    def _tick(self, xs: dict, ticks: dict) -> dict:
        plan = self._plan(xs, ticks)
        x = self._arr.cat([xs[s] for s in plan.slots])
        res = {s: None for s in xs}
        for ln in plan.launches:
            win = self._advance(self._hist, x, plan.desc[ln.p_lo:ln.p_hi], ln.A, ln.Lmax)
            if ln.A:
                rows = plan.windows[ln.a_lo:ln.a_lo + ln.A]
                y = win if ln.passthrough else self._forward(win, [s for s, _ in rows])
                for r, (s, t) in enumerate(rows):
                    res[s] = y[r][..., t.keep:t.wlen]
        return res


class _HipBank(StreamBank):
    """StreamBank on a HipNet: histories, windows and outputs stay on the device.  A tick uploads ONE table (the wv_bank_advance descriptors and
    whatever else its launches read), then runs per launch wv_bank_advance and the net on the window batch."""

    def __init__(self, net, capacity: int = 64, precision: str = "f32", pad_limit: float = 1.5):
        if precision not in _PRECISIONS:
            raise ValueError("precision must be 'f32' or 'f16'")
        arrays = TorchArrays(net.device)
        self.net, self.precision, self._torch = net, precision, arrays.torch
        super().__init__(capacity, net.cfg.hop_length, _halo(net.cfg), None, None, arrays, pad_limit)

    def set_passthrough(self, slot: int, on: bool) -> int:
        raise ValueError(f"{type(self).__name__}: on the device pass-through is switched by set_message, on the banks that have it")

    def _upload(self, sections: list) -> dict:
        """[(name, host array)] -> {name: device tensor}: one buffer, every section on an 8-byte boundary, one copy."""
        torch = self._torch
        offs, total = [], 0
        for _, a in sections:
            offs.append(total)
            total += -(-a.nbytes // 8) * 8
        buf = np.zeros(total, np.uint8)
        for o, (_, a) in zip(offs, sections):
            buf[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        dev = torch.from_numpy(buf).to(self.net.device)
        return {name: dev[o:o + a.nbytes].view(getattr(torch, a.dtype.name)).view(a.shape)
                for o, (name, a) in zip(offs, sections)}

    def _packed(self, xs: dict, slots: list):
        """The tick's new samples (or gates) of `slots`, one after another in one device tensor; None where nobody brought any."""
        dev, f32 = self.net.device, self._torch.float32
        parts = [xs[s].to(dev, f32) for s in slots if xs[s].shape[0]]
        return self._torch.cat(parts) if parts else None

    def _bank_advance(self, hist, x, n_x: int, desc, ln: BankLaunch):
        """wv_bank_advance for one launch: desc the tick's uploaded descriptor table -> the window batch [A, 1, Lmax], None where A = 0."""
        win = self._torch.empty((ln.A, 1, ln.Lmax), dtype=self._torch.float32, device=self.net.device) if ln.A else None
        _lib.check(self.net._lib.wv_bank_advance(hist.data_ptr(), self.capacity, self.hcap, _lib.ptr(x), n_x, desc[ln.p_lo:].data_ptr(),
                                                 ln.p_hi - ln.p_lo, _lib.ptr(win), ln.A, ln.Lmax, _lib.stream()), "wv_bank_advance")
        return win

    def _sections(self, plan: BankPlan) -> list:
        return []

    def _begin(self, plan: BankPlan, tabs: dict) -> None:
        pass

    def _tick(self, xs: dict, ticks: dict) -> dict:
        plan = self._plan(xs, ticks)
        if plan.launches:
            with self._torch.cuda.device(self.net.device):
                x = self._packed(xs, plan.slots)
                tabs = self._upload([("desc", plan.desc)] + self._sections(plan))
                self._begin(plan, tabs)
                for ln in plan.launches:
                    win = self._bank_advance(self._hist, x, plan.n_x, tabs["desc"], ln)
                    if ln.A:
                        self._launch(win, tabs, plan, ln)
                return self._finish(plan, tabs)
        return self._finish(plan, None)


class _ColumnsBank(_HipBank):
    """A _HipBank that returns per slot the kept columns [k] of _net(window batch, tabs, launch) -> [A, 1, Lmax]: wv_window_scatter packs
    them into one tensor, and the values of a tick are views of it."""

    def _sections(self, plan: BankPlan) -> list:
        # wv_window_scatter's descriptor per window: {offset in `out` of the window's column 0, row stride (one row: unused), keep lo, keep hi}
        return [("scatter", np.array([[plan.out[s][0] - t.keep, plan.n_out, t.keep, t.wlen] for s, t in plan.windows], np.int64).reshape(-1, 4))]

    def _begin(self, plan: BankPlan, tabs: dict) -> None:
        self._out = self._torch.empty(plan.n_out, dtype=self._torch.float32, device=self.net.device)

    def _launch(self, win, tabs: dict, plan: BankPlan, ln: BankLaunch) -> None:
        y = win if ln.passthrough else self._net(win, tabs, ln)                # pass-through: the kept columns are the input's own
        _lib.check(self.net._lib.wv_window_scatter(y.data_ptr(), tabs["scatter"][ln.a_lo:].data_ptr(), self._out.data_ptr(), plan.n_out, ln.A, 1,
                                                   ln.Lmax, _lib.stream()), "wv_window_scatter")

    def _finish(self, plan: BankPlan, tabs) -> dict:
        out = self._out if tabs is not None else self._arr.zeros(0)
        self._out = None
        return {s: out[o:o + k] for s, (o, k) in plan.out.items()}


class EmbedBank(_ColumnsBank):
    """Watermark up to `capacity` live 16 kHz mono streams, each on its own clock: open(message) -> slot, push({slot: x [n]}) -> {slot: the
    watermarked samples of the frames that push completed [k]}, close(slot) -> the rest.
    messages: what turns open()'s argument into a [msg_dimension] bit tensor (WaveVerify passes its watermark-id table); without it open()
    takes the bits themselves.  The messages live on the host and travel in the tick's table, so open() touches no device memory.
    add_input=False: the generator's residual alone (what native_bank.py brings back to each slot's own rate).
    set_message(slot, message) changes a stream's id mid-stream and set_message(slot, None) switches its watermark off (pass-through: the
    input comes back bit for bit and the slot takes part in no generator launch), both from the slot's next frame on; open(None) opens in
    pass-through.  Per stream the concatenated output is span embedding (window.span_generator, hard cuts) of what it pushed, the span
    edges at the indices set_message returned.
    set_snr_floor(min_snr_db), before the first open(): the SNR floor of snr_floor.py.  The generator launches then
    return the residual alone and ONE wv_snr_floor call per launch turns (window batch, residual) into the rows wv_window_scatter packs; each
    row starts at its window's keep column, a frame boundary of its stream, and carries its slot's gain of the frame before in a [capacity]
    device array.  A slot's state is fresh at open() and on leaving pass-through; pass-through launches stay as they are.  Per stream the
    concatenated output is the file route's floor on the whole stream."""

    def __init__(self, net, capacity: int = 64, precision: str = "f32", pad_limit: float = 1.5, messages: Optional[Callable] = None,
                 add_input: bool = True):
        super().__init__(net, capacity, precision, pad_limit)
        self._messages, self.add_input = messages, bool(add_input)
        self._msg = np.zeros((self.capacity, net.cfg.msg_dimension), np.float32)
        self.snr_floor_db: Optional[float] = None
        self._opened = False
        self._strength = np.ones(self.capacity, np.float32)                # per slot, under a floor (native_bank sets each slot's own)
        self._fresh: set = set()                                           # slots whose next floor row ignores the stored gain

    def set_snr_floor(self, min_snr_db: Optional[float]) -> None:
        """The floor in dB for every slot (None: off).  Only before the bank's first open()."""
        if self._opened:
            raise RuntimeError("set_snr_floor is legal only before the bank's first open()")
        db = snr_floor.check_db(min_snr_db)
        if db is None:
            self.snr_floor_db = self._rho = self._ramp = self._gstate = None
            return
        rho, ramp = snr_floor.rho_of(db), snr_floor.floor_ramp(self.hop)
        self.snr_floor_db, self._rho = db, rho
        self._ramp = self._torch.from_numpy(ramp).to(self.net.device)
        self._gstate = self._arr.zeros(self.capacity)

    def _message_row(self, message) -> np.ndarray:
        m = self._messages(message) if self._messages is not None else message
        m = np.asarray(m.detach().cpu() if hasattr(m, "detach") else m, np.float32).reshape(-1)
        if m.shape[0] != self._msg.shape[1]:
            raise ValueError(f"a message has {self._msg.shape[1]} bits, got {m.shape[0]}")
        return m

    def _set(self, slot: int, message) -> None:
        """Everything is checked before the slot changes."""
        if message is None:
            if not self.add_input:
                raise ValueError("pass-through returns the input; a bank that returns the residual alone (add_input=False) has none")
            self._through.add(slot)
        else:
            self._msg[slot] = self._message_row(message)
            if slot in self._through:
                self._fresh.add(slot)                                      # leaving pass-through: no gain of a frame before
            self._through.discard(slot)

    def _on_open(self, slot: int, message) -> None:
        self._set(slot, message)
        self._opened = True
        self._fresh.add(slot)                                              # whatever gain the slot's last stream left is never read
        self._strength[slot] = 1.0

    def set_message(self, slot: int, message) -> int:
        """The slot's id from its next frame on (None: no watermark) -> that frame's first sample, samples_seen(slot)."""
        self._check_slot(slot)
        self._set(slot, message)
        return self._tickers[slot].t_out

    def _floor_rows(self, plan: BankPlan) -> np.ndarray:
        """wv_snr_floor's descriptor per window, launch by launch: the row's kept columns [keep, wlen) of its launch's window batch, in x, r
        and out alike; the slot's strength; its state, fresh where the slot has no frame before.  Pass-through rows are never read."""
        rows = np.zeros((len(plan.windows), snr_floor.DESC), np.int64)
        for ln in plan.launches:
            if ln.passthrough:
                continue
            for r in range(ln.A):
                s, t = plan.windows[ln.a_lo + r]
                at = r * ln.Lmax + t.keep
                rows[ln.a_lo + r] = [at, at, at, t.wlen - t.keep, snr_floor.strength_bits(self._strength[s]), s, int(s in self._fresh), -1]
                self._fresh.discard(s)
        return rows

    def _sections(self, plan: BankPlan) -> list:
        sec = super()._sections(plan) + [("msg", self._msg[[s for s, _ in plan.windows]])]
        if self.snr_floor_db is not None:
            sec.append(("floor", self._floor_rows(plan)))
        return sec

    def _net(self, win, tabs: dict, ln: BankLaunch):
        msg = tabs["msg"][ln.a_lo:ln.a_lo + ln.A]
        if self.snr_floor_db is None:
            return self.net.generator(win, msg, add_input=self.add_input, precision=self.precision)
        y = self.net.generator(win, msg, add_input=False, precision=self.precision)
        out = self._torch.empty_like(y)                                    # only the kept columns are written, and only they are read
        n = ln.A * ln.Lmax
        _lib.check(self.net._lib.wv_snr_floor(win.data_ptr(), n, y.data_ptr(), n, out.data_ptr(), n, tabs["floor"][ln.a_lo:].data_ptr(), ln.A, ln.Lmax,
                                              self._gstate.data_ptr(), self.capacity, None, 0, self._ramp.data_ptr(), self.hop, self._rho,
                                              int(self.add_input), _lib.stream()), "wv_snr_floor")
        return out


class LocateBank(_ColumnsBank):
    """Locate the watermark in up to `capacity` live streams: open() -> slot, push({slot: x [n]}) -> {slot: locator logits of the newly completed
    frames [k]}."""

    def _net(self, win, tabs: dict, ln: BankLaunch):
        return self.net.locator(win, precision=self.precision)


class DetectBank(_HipBank):
    """Detect the watermark in up to `capacity` live streams: push({slot: x [n]}) -> {slot: DetectState(mean_prob [nb], bits [nb], samples_seen)}
    over that stream's completed frames.  Each window's sigmoid sum over its own new columns [keep, wlen) goes into the slot's f64 accumulator
    (wv_bank_detect_update), in the order and the arithmetic of DetectSession."""

    def __init__(self, net, capacity: int = 64, precision: str = "f32", pad_limit: float = 1.5):
        super().__init__(net, capacity, precision, pad_limit)
        zeros, nb = self._arr.zeros, net.cfg.head_bits
        self._acc = zeros(self.capacity, nb, dtype="float64")
        self._seen = zeros(self.capacity, dtype="int64")
        self._zero = (zeros(nb), zeros(nb, dtype="int32"))
        self._last = [self._zero] * self.capacity

    def _on_open(self, slot: int) -> None:
        self._acc[slot].zero_()                                            # two fills on the stream; nothing waits for them
        self._seen[slot].zero_()
        self._last[slot] = self._zero

    def _sections(self, plan: BankPlan) -> list:
        w = plan.windows
        return [("det", np.array([[s, t.wlen - t.keep] for s, t in w], np.int64).reshape(-1, 2)),
                ("lo", np.array([t.keep for _, t in w], np.int32)), ("hi", np.array([t.wlen for _, t in w], np.int32))]

    def _begin(self, plan: BankPlan, tabs: dict) -> None:
        self._psum = self._torch.empty((len(plan.windows), self.net.cfg.head_bits), dtype=self._torch.float32, device=self.net.device)

    def _launch(self, win, tabs: dict, plan: BankPlan, ln: BankLaunch) -> None:
        a, b = ln.a_lo, ln.a_lo + ln.A
        self.net.detector_window_psum(win, tabs["lo"][a:b], tabs["hi"][a:b], psum=self._psum[a:b], precision=self.precision)

    def _finish(self, plan: BankPlan, tabs) -> dict:
        torch, A, nb = self._torch, len(plan.windows), self.net.cfg.head_bits
        if A:
            mp = torch.empty((A, nb), dtype=torch.float32, device=self.net.device)
            bits = torch.empty((A, nb), dtype=torch.int32, device=self.net.device)
            with torch.cuda.device(self.net.device):
                _lib.check(self.net._lib.wv_bank_detect_update(self._acc.data_ptr(), self._seen.data_ptr(), self.capacity, nb, self._psum.data_ptr(),
                                                               tabs["det"].data_ptr(), A, mp.data_ptr(), bits.data_ptr(), _lib.stream()),
                           "wv_bank_detect_update")
            for r, (s, _) in enumerate(plan.windows):
                self._last[s] = (mp[r], bits[r])
            self._psum = None
        return {s: DetectState(*self._last[s], self._tickers[s].t_out) for s in plan.slots}


# ---------------------------------------------------------------------------------------------------------------- segment banks
class SegmentStreamBank(_SegmentReader, StreamBank):
    """Localized detection of up to `capacity` live streams, each on its own clock: open() -> slot, push({slot: x [n]})
    returns nothing (a gated bank takes {slot: (x [n], gate [n])}, the 0 / 1 gate replacing the locator), poll() -> {slot: the Segments that
    closed since the last poll}, open_segments() -> {slot: the run still open, or None}, close(slot) -> the slot's Segments not yet polled.
    Backend independent: frame_sums(window batch [A, 1, Lmax], gate windows [A, Lmax] or None) -> the batch's per-frame gated sums
    [A, nb + 1, ceil(Lmax / hop)]; `tracker` has the interface of localize.BankSegmentTracker; `advance` is numpy_bank_advance's contract and
    serves the gate's histories with the same descriptor rows.

    The launches of a tick are plan_tick's.  Their frame sums lie one after another in ONE arena, and a descriptor per window tells the tracker
    where that stream's rows are and which of their frames are its own: [keep / hop, ceil(wlen / hop)).  The frames of a row beyond its wlen
    are computed on the batch's zero padding and belong to nobody; no descriptor reaches them.

    ring is the tracker's event ring per slot.  Before a tick would let cut_rows' bound on any slot's waiting events reach `ring` the bank reads
    the rings itself, and a long push is tracked in pieces that stay within the bound, so nothing is lost."""

    def __init__(self, capacity: int, hop: int, H: int, frame_sums: Callable, tracker, advance: Optional[Callable] = numpy_bank_advance,
                 arrays=None, pad_limit: float = 1.5, gated: bool = False, sample_rate: int = 16000, ring: int = 64,
                 min_gap_frames: int = 2, min_len_frames: int = 5):
        if ring < 1:
            raise ValueError("ring must be at least 1")
        StreamBank.__init__(self, capacity, hop, H, None, advance, arrays, pad_limit)
        self._frame_sums, self._tracker, self.gated = frame_sums, tracker, bool(gated)
        self._init_reader(hop, sample_rate, ring, min_gap_frames, min_len_frames)
        self._clear_reader(self.capacity, self.capacity)
        self._ghist = self._arr.zeros(self.capacity, self.hcap) if self.gated else None
        self._frames = [0] * self.capacity                                 # frames tracked so far: the next tick's frame0
        self._opened = False

    # ---- slots
    def set_split(self, rule) -> None:
        """Cut runs where the decoded id changes (localize.SplitRule; None: off), for every slot.  Only before the
        first open(); poll(), close() and open_segments() then deal in pieces, known 2 * window_frames frames after a change."""
        if self._opened:
            raise RuntimeError("set_split is legal only before the bank's first open()")
        self._set_split(rule)

    def _on_open(self, slot: int) -> None:
        self._opened = True
        self._tracker.reset(slot)                                          # whatever the slot's last stream left is never seen
        self._frames[slot] = self._unread[slot] = 0
        self._pending[slot] = []

    def _streams(self, read: Callable) -> list:
        tk = self._tickers
        return [(s, tk[s].t_in, v) for s, v in read(self.open_slots()).items()]

    def poll(self) -> dict:
        """-> {slot: the Segments closed since the last poll, in stream order} for every open slot."""
        self._drain()
        return {s: self._taken(s) for s in self.open_slots()}

    def open_segments(self) -> dict:
        """-> {slot: the run that is open now as a provisional Segment (its frames so far), or None} for every open slot."""
        return dict(self._open_now())

    # ---- ticks
    def push(self, items: dict) -> None:
        """{slot: samples [n]} ({slot: (samples [n], gate [n])} on a gated bank), any length per slot.  Everything is checked before any stream's
        state changes."""
        xs, gs = {}, {}
        for slot, item in items.items():
            self._check_slot(slot)
            pair = isinstance(item, (tuple, list))
            if self.gated and not (pair and len(item) == 2):
                raise ValueError(f"slot {slot}: a gated bank takes (samples, gate) on every push")
            if pair and not self.gated:
                raise ValueError(f"slot {slot}: this bank is not gated; it takes the samples alone")
            x, g = item if pair else (item, None)
            if len(x.shape) != 1:
                raise ValueError(f"slot {slot}: expected 1-D samples, got shape {tuple(x.shape)}")
            if g is not None and tuple(g.shape) != tuple(x.shape):
                raise ValueError(f"slot {slot}: gate must have the samples' shape {tuple(x.shape)}, got {tuple(g.shape)}")
            xs[slot], gs[slot] = x, g
        self._tick(xs, gs, {slot: self._tickers[slot].push(int(x.shape[0])) for slot, x in xs.items()}, False)

    def close(self, slot: int) -> list:
        """The stream's partial last frame alone at its true length, its open run closed -> the slot's Segments not yet polled; frees the slot."""
        self._check_slot(slot)
        if self._unread[slot]:
            self._drain()                                                  # a close at `final` may follow the last one closely
        e = self._arr.zeros(0)
        self._tick({slot: e}, {slot: e if self.gated else None}, {slot: self._tickers[slot].flush()}, True)
        self._drain()
        self._is_open[slot] = False
        return self._taken(slot)

    def _track_rows(self, plan: BankPlan, ticks: dict, final: bool):
        """-> (offset of every launch's frame sums in the tick's arena, the arena's length, the tracker's descriptor rows); the slots' frame
        counters move on to the tick's end."""
        hop, nb1 = self.hop, self._tracker.nb + 1
        offs, rows, n_fsum = [], [], 0
        for ln in plan.launches:
            Fr = -(-ln.Lmax // hop)
            offs.append(n_fsum)
            for r, (s, t) in enumerate(plan.windows[ln.a_lo:ln.a_lo + ln.A]):
                f_lo, f_hi = t.keep // hop, -(-t.wlen // hop)              # the frames from f_hi on are the batch's padding
                rows.append([s, n_fsum + r * nb1 * Fr, Fr, f_lo, f_hi, self._frames[s], t.wlen - (f_hi - 1) * hop, int(final)])
                self._frames[s] += f_hi - f_lo
            n_fsum += -(-ln.A * nb1 * Fr // 4) * 4                         # every launch's block starts on a 16-byte boundary
        if final:
            named = {r[0] for r in rows}
            rows += [[s, 0, 0, 0, 0, self._frames[s], hop, 1] for s in ticks if s not in named]     # no frame left: the open run still closes
        return offs, n_fsum, rows

    def _tick(self, xs: dict, gs: dict, ticks: dict, final: bool) -> None:
        plan = self._plan(xs, ticks)
        offs, n_fsum, rows = self._track_rows(plan, ticks, final)
        pieces, unread = self._cut(rows)
        self._run(plan, xs, gs, offs, n_fsum, [(drain, np.array(piece, np.int64).reshape(-1, 8)) for drain, piece in pieces])
        self._unread = unread

    def _run(self, plan: BankPlan, xs: dict, gs: dict, offs: list, n_fsum: int, pieces: list) -> None:
        x = self._arr.cat([xs[s] for s in plan.slots])
        g = self._arr.cat([gs[s] for s in plan.slots]) if self.gated else None
        arena = np.zeros(n_fsum, self._tracker.dtype)
        for ln, off in zip(plan.launches, offs):
            desc = plan.desc[ln.p_lo:ln.p_hi]
            win = self._advance(self._hist, x, desc, ln.A, ln.Lmax)
            gwin = self._advance(self._ghist, g, desc, ln.A, ln.Lmax).reshape(ln.A, ln.Lmax) if self.gated else None
            if ln.A:
                fs = np.asarray(self._frame_sums(win, gwin))
                arena[off:off + fs.size] = fs.reshape(-1)
        for drain, rows in pieces:
            if drain:
                self._drain()
            self._tracker.advance(arena, rows)


class HipBankSegmentTracker(_HipTrackerState):
    """localize.BankSegmentTracker's interface on wv_bank_segment_track: the slots' state and event rings stay on the device in
    wv_segment_track's per-stream layouts; advance() is one launch and no synchronisation, reset() two fills on the stream, poll() and
    open_runs() one device-to-host copy each."""
    _what = "slot"

    def __init__(self, capacity: int, nb: int, hop: int, min_on: float, min_gap_frames: int, min_len_frames: int, ring: int, device,
                 eps: float = 1e-8):
        super().__init__(capacity, nb, hop, min_on, min_gap_frames, min_len_frames, ring, device, eps)
        self.capacity, self.ring = self._n, self._ring
        self._clear()

    def reset(self, slot: int) -> None:
        ss, es = self._strides
        self.state[slot * ss:(slot + 1) * ss].zero_()                       # two fills on the stream; nothing waits for them
        self.events[slot * es:(slot + 1) * es].zero_()
        self._read[slot] = 0

    def advance(self, fsum, desc, P: Optional[int] = None) -> None:
        """fsum: the tick's arena (device float32, or None / empty); desc: int64 device tensor of rows [P, 8] (a host array is uploaded)."""
        torch = self._torch
        if not hasattr(desc, "data_ptr"):
            desc = torch.from_numpy(np.ascontiguousarray(desc, np.int64)).to(self.device)
        P = int(desc.numel() // 8) if P is None else int(P)
        fsum = fsum if fsum is not None and fsum.numel() else None
        with torch.cuda.device(self.device):
            if self.split is None:
                self._ops.bank_segment_track(fsum, desc, P, self.capacity, self.nb, self.hop, self.min_on, self.G, self.min_len, self.state,
                                             self.events, self.ring, self.eps)
            else:
                self._ops.bank_segment_track_split(fsum, desc, P, self.capacity, self.nb, self.hop, self.min_on, self.G, self.min_len,
                                                   self.split, self.state, self.events, self.ring, self.eps)

    def poll(self, slots) -> dict:
        return dict(self._new_events(slots))

    def open_runs(self, slots) -> dict:
        return dict(self._open_runs_of(slots))


class SegmentBank(_SegmentNets, SegmentStreamBank, _HipBank):
    """SegmentStreamBank on a detector and a locator HipNet: one history per slot for both nets (a gated bank has a second one for the gate,
    advanced by a second wv_bank_advance with the same rows), per launch the locator's logits (or the gate windows) gating the detector's
    frames kernel into that launch's block of the tick's arena, then ONE wv_bank_segment_track.  A tick uploads one table: the
    wv_bank_advance descriptors and the tracker's.  Nothing comes back to the host in push() but the ring read described above."""

    def __init__(self, detector, locator, capacity: int = 64, pad_limit: float = 1.5, threshold: float = 0.5, min_on: float = 0.5,
                 min_gap_frames: int = 2, min_len_frames: int = 5, ring: int = 64, gated: bool = False, precision: str = "f32",
                 locator_precision: Optional[str] = None, sample_rate: int = 16000):
        hop, H = self._bind(detector, locator, threshold, precision, locator_precision, ring, "ring")
        tracker = HipBankSegmentTracker(capacity, detector.cfg.head_bits, hop, min_on, min_gap_frames, min_len_frames, ring, detector.device)
        SegmentStreamBank.__init__(self, capacity, hop, H, None, tracker, None, self._arr, pad_limit, gated, sample_rate, ring, min_gap_frames,
                                   min_len_frames)

    def _run(self, plan: BankPlan, xs: dict, gs: dict, offs: list, n_fsum: int, pieces: list) -> None:
        torch, dev, nb1 = self._torch, self.net.device, self._tracker.nb + 1
        if not plan.launches and not pieces:
            return
        with torch.cuda.device(dev):
            x = self._packed(xs, plan.slots)
            g = self._packed(gs, plan.slots) if self.gated else None
            track = np.concatenate([rows for _, rows in pieces]) if pieces else np.zeros((0, 8), np.int64)
            tabs = self._upload([(name, a) for name, a in (("desc", plan.desc), ("track", track)) if a.size])
            arena = torch.empty(n_fsum, dtype=torch.float32, device=dev) if n_fsum else None
            for ln, off in zip(plan.launches, offs):
                win = self._bank_advance(self._hist, x, plan.n_x, tabs["desc"], ln)
                gwin = self._bank_advance(self._ghist, g, plan.n_x, tabs["desc"], ln) if self.gated else None
                if ln.A:
                    Fr = -(-ln.Lmax // self.hop)
                    self.frame_sums(win, gwin, out=arena[off:off + ln.A * nb1 * Fr].view(ln.A, nb1, Fr))
            p = 0
            for drain, rows in pieces:
                if drain:
                    self._drain()
                self._tracker.advance(arena, tabs["track"][p:], len(rows))
                p += len(rows)
