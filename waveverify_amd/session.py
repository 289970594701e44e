"""Live sessions: S audio streams watermarked, detected or located in lockstep as samples arrive.

Each push appends n >= 0 samples per stream.  The frames completed so far (a multiple of the net's hop) run as one window that
starts halo(cfg) samples before the first new frame (or at the stream's t = 0) and ends at the last completed frame; only the
new frames' columns are returned.  Incomplete-frame samples and the halo history stay on the device (wv_session_advance).
flush() runs the remaining partial frame as a final window ending at the true end, after which the concatenated outputs equal
the whole-clip forward on the concatenated input.  ("Session", not "stream", to keep clear of HIP streams.)

Segment sessions (SegmentSession, section 7d-5) run the locator and the detector's gated per-frame sums on one shared window per tick and
turn the frame sums into closed localize.Segments on the device (wv_segment_track); their push returns nothing, poll() reads.

The bookkeeping is independent of the backend: a session takes the net forward as a callable, and the history update as
another, so the same state machine runs on the numpy oracle on a CPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from .window import halo as _halo


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
            raise RuntimeError("session was flushed; call reset() to start over")
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
            raise RuntimeError("session was flushed; call reset() to start over")
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
    [keep, L); advance(history, x, Tick) -> (window, next history).  Subclasses bind both to a HipNet."""

    def __init__(self, S: int, hop: int, H: int, forward: Callable, advance: Callable = numpy_advance,
                 new_history: Optional[Callable] = None):
        if S < 1:
            raise ValueError("need at least one session")
        self.S = S
        self._t = _Ticker(hop, H)
        self._forward, self._advance = forward, advance
        self._new_history = new_history or (lambda S_, cap: np.zeros((S_, cap), np.float32))
        self._hist = self._new_history(S, self._t.cap)

    @property
    def samples_seen(self) -> int:
        """Samples whose outputs have been produced."""
        return self._t.t_out

    def reset(self) -> None:
        self._t.reset()
        self._hist = self._new_history(self.S, self._t.cap)
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
        return self._step(x=self._empty(), t=self._t.flush())

    def _empty(self):
        return np.zeros((self.S, 0), np.float32)


class _HipSession(StreamSession):
    """StreamSession on a HipNet: history, window and outputs stay on the device."""

    def __init__(self, net, S: int, precision: str):
        import torch
        if precision not in ("f32", "f16"):
            raise ValueError("precision must be 'f32' or 'f16'")
        self.net, self.precision, self._torch = net, precision, torch
        super().__init__(S, net.cfg.hop_length, _halo(net.cfg), self._net_forward, self._hip_advance,
                         lambda S_, cap: torch.zeros((S_, cap), dtype=torch.float32, device=net.device))

    def _empty(self):
        return self._torch.zeros((self.S, 0), dtype=self._torch.float32, device=self.net.device)

    def _hip_advance(self, hist, x, t: Tick):
        torch = self._torch
        from . import _lib
        x = x.to(self.net.device, torch.float32).contiguous()
        nxt = torch.empty_like(hist)
        win = torch.empty((self.S, 1, t.wlen), dtype=torch.float32, device=self.net.device)
        with torch.cuda.device(self.net.device):
            _lib.check(self.net._lib.wv_session_advance(
                hist.data_ptr(), hist.shape[1], t.hv, x.data_ptr() if x.numel() else None, x.shape[1],
                win.data_ptr() if t.wlen else None, t.wlen, nxt.data_ptr(), t.drop, t.hv2, self.S,
                _lib.stream()),
                "wv_session_advance")
        return win, nxt


class EmbedSession(_HipSession):
    """Watermark S live streams: push(x [S, n]) -> watermarked samples of the frames completed by this push [S, 1, k].
    add_input=False: the generator's residual alone (what native_session.py brings back to a stream's own rate)."""

    def __init__(self, net, msg, precision: str = "f32", add_input: bool = True):
        import torch
        msg = torch.as_tensor(msg).to(net.device).float()
        if msg.dim() == 1:
            msg = msg.unsqueeze(0)
        self.msg, self.add_input = msg.contiguous(), bool(add_input)
        super().__init__(net, msg.shape[0], precision)

    def _net_forward(self, win, keep):
        return self.net.generator(win, self.msg, add_input=self.add_input, precision=self.precision)[:, :, keep:].contiguous()

    def _no_output(self):
        return self._torch.zeros((self.S, 1, 0), dtype=self._torch.float32, device=self.net.device)

    def push(self, x):
        y = super().push(x)
        return self._no_output() if y is None else y

    def flush(self):
        y = super().flush()
        return self._no_output() if y is None else y


class LocateSession(EmbedSession):
    """Locate the watermark in S live streams: push(x [S, n]) -> locator logits of the newly completed frames [S, 1, k]."""

    def __init__(self, net, S: int, precision: str = "f32"):
        _HipSession.__init__(self, net, S, precision)

    def _net_forward(self, win, keep):
        return self.net.locator(win, precision=self.precision)[:, :, keep:].contiguous()


@dataclass
class DetectState:
    mean_prob: object      # [S, nbits] time-averaged sigmoid over the samples seen
    bits: object           # [S, nbits] int32, mean_prob >= 0.5
    samples_seen: int


class DetectSession(_HipSession):
    """Detect the watermark in S live streams: push(x [S, n]) -> the running DetectState over every completed frame so far.
    Each window's sigmoid sum over its new columns (the head's windowed mode) is added to an f64 accumulator."""

    def __init__(self, net, S: int, precision: str = "f32"):
        super().__init__(net, S, precision)
        self._on_reset()

    def _on_reset(self):
        self._acc = self._torch.zeros((self.S, self.net.cfg.head_bits), dtype=self._torch.float64, device=self.net.device)

    def _net_forward(self, win, keep):
        L = win.shape[-1]
        return self.net.detector_window_psum(win, [keep] * self.S, [L] * self.S, precision=self.precision)

    def _state(self, psum):
        if psum is not None:
            self._acc += psum.double()
        mp = (self._acc / max(self.samples_seen, 1)).float()
        return DetectState(mp, (mp >= 0.5).to(self._torch.int32), self.samples_seen)

    def push(self, x):
        return self._state(super().push(x))

    def flush(self):
        return self._state(super().flush())


# ---------------------------------------------------------------------------------------------------------------- live segment sessions
def segment_halo(detector_cfg, locator_cfg) -> int:
    """History of a session that runs both nets on ONE window per tick, in samples: the hop is the detector's, the locator's hop must divide
    it, and the halo is the larger of the detector's and the locator's rounded up to that hop."""
    hop, lhop = detector_cfg.hop_length, locator_cfg.hop_length
    if hop % lhop:
        raise ValueError(f"the locator's hop ({lhop}) does not divide the detector's ({hop}): the two nets cannot share one window")
    return max(_halo(detector_cfg), -(-_halo(locator_cfg) // hop) * hop)


class SegmentStreamSession(StreamSession):
    """Localized detection of S live streams: push(x [S, n], gate=None) returns nothing; the watermarked stretches
    come out of poll() as localize.Segments once they have ended.  Backend independent: frame_sums(window [S,1,L], gate window [S,L] or
    None) -> the window's per-frame gated sums [S, nb + 1, ceil(L / hop)] (without a gate window it runs the locator itself), `tracker` has
    the interface of localize.SegmentTracker.  A tick hands the tracker the window's frames from keep / hop on.

    gate [S, n] (0 / 1) replaces the locator; its samples of an incomplete frame wait in a second history that goes through the same
    `advance`.  Whether a session is gated is settled by its first push and holds until reset().

    capacity is the tracker's event ring.  The frames tracked since the last read bound the events waiting there by
    frames // max(1, min_len_frames + min_gap_frames) + 1 (two closes lie at least that many frames apart); before a tick would let that
    bound reach capacity the session reads the ring itself (the one host synchronisation a push can make), and a long push is tracked in
    pieces that stay within it, so nothing is lost."""

    def __init__(self, S: int, hop: int, H: int, frame_sums: Callable, tracker, advance: Callable = numpy_advance,
                 new_history: Optional[Callable] = None, sample_rate: int = 16000, capacity: int = 64, min_gap_frames: int = 2,
                 min_len_frames: int = 5):
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        StreamSession.__init__(self, S, hop, H, None, advance, new_history)
        self._frame_sums, self._tracker = frame_sums, tracker
        self.sample_rate, self.capacity = int(sample_rate), int(capacity)
        self._period = max(1, int(min_len_frames) + int(min_gap_frames))
        self._on_reset()

    def _on_reset(self) -> None:
        self._ghist = None
        self._gated: Optional[bool] = None
        self._unread = 0                                                   # frames tracked since the ring was last read
        self._pending = [[] for _ in range(self.S)]
        self._tracker.reset()

    # ---- events -> Segments
    def _confidence(self, prob: np.ndarray) -> float:
        return float(np.asarray(prob, np.float32).mean())

    def _segment(self, ev):
        from .localize import Segment
        from .watermark_id import WatermarkID
        lo, hi, count, prob = ev
        hop, end = self._t.hop, min(int(hi) * self._t.hop, self._t.t_in)   # t_in: the true length once flushed, never short before
        prob = np.asarray(prob, np.float32)
        bits = "".join("1" if p >= np.float32(0.5) else "0" for p in prob)
        wid = WatermarkID.custom(bits) if len(bits) == 16 else None       # an id has 16 bits; a net of another width leaves prob to read
        return Segment(int(lo) * hop / self.sample_rate, end / self.sample_rate, wid, self._confidence(prob),
                       float(count) / (end - int(lo) * hop), prob, (int(lo), int(hi)))

    def _drain(self) -> None:
        for s, evs in enumerate(self._tracker.poll()):
            self._pending[s] += [self._segment(ev) for ev in evs]
        self._unread = 0

    def poll(self):
        """-> per stream the Segments closed since the last poll, in stream order."""
        self._drain()
        out, self._pending = self._pending, [[] for _ in range(self.S)]
        return out

    def open_segments(self):
        """-> per stream the run that is open now as a provisional Segment (its frames so far), or None."""
        return [None if ev is None else self._segment(ev) for ev in self._tracker.open_runs()]

    # ---- ticks
    def _track(self, fsum, f_lo: int, f_hi: int, last_valid: int, final: bool) -> None:
        step = self.capacity * self._period - 1                            # frames // period + 1 <= capacity
        while True:
            m = min(step, f_hi - f_lo)
            last = f_lo + m == f_hi
            if self._unread and (self._unread + m) // self._period + 1 >= self.capacity:
                self._drain()
            self._tracker.advance(fsum, f_lo, f_lo + m, last_valid if last else self._t.hop, final and last)
            self._unread += m
            f_lo += m
            if last:
                return

    def _gate_window(self, gate, x, t: Tick):
        if self._gated is None:
            self._gated = gate is not None
            if self._gated:
                self._ghist = self._new_history(self.S, self._t.cap)
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
        hop = self._t.hop
        if t.wlen > 0:
            fsum = self._frame_sums(win, gwin)
            f_hi = -(-t.wlen // hop)
            self._track(fsum, t.keep // hop, f_hi, t.wlen - (f_hi - 1) * hop, final)
        elif final:
            self._track(self._no_frames(), 0, 0, hop, True)

    def _no_frames(self):
        return np.zeros((self.S, self._tracker.nb + 1, 0), np.float32)

    def push(self, x, gate=None) -> None:
        if x.shape[0] != self.S or len(x.shape) != 2:
            raise ValueError(f"expected new samples of shape [{self.S}, n], got {tuple(x.shape)}")
        self._tick(x, gate, self._t.push(int(x.shape[1])), False)

    def flush(self):
        """The partial last frame, if any, runs with its true length, every open run closes -> the Segments not yet polled."""
        t = self._t.flush()
        if self._unread:
            self._drain()                                                  # a close at `final` may follow the last one closely
        e = self._empty()
        self._tick(e, e if self._gated else None, t, True)
        return self.poll()


class HipSegmentTracker:
    """localize.SegmentTracker's interface on wv_segment_track: state and event ring stay on the device; advance() is one launch and no
    synchronisation, poll() and open_runs() are one device-to-host copy each."""

    def __init__(self, S: int, nb: int, hop: int, min_on: float, min_gap_frames: int, min_len_frames: int, capacity: int, device,
                 eps: float = 1e-8):
        import torch
        from . import ops
        self.S, self.nb, self.hop, self.min_on = int(S), int(nb), int(hop), float(min_on)
        self.G, self.min_len, self.capacity, self.eps, self.device = int(min_gap_frames), int(min_len_frames), int(capacity), float(eps), device
        self._torch, self._ops = torch, ops
        with torch.cuda.device(device):
            self._bytes = ops.segment_track_bytes(self.S, self.nb, self.G, self.capacity)       # refuses what the kernel would
        self.reset()

    def reset(self) -> None:
        torch = self._torch
        self.state = torch.zeros(self._bytes[0], dtype=torch.uint8, device=self.device)
        self.events = torch.zeros(self._bytes[1], dtype=torch.uint8, device=self.device)
        self.frames_seen, self.closed = 0, False
        self._read = [0] * self.S

    def advance(self, fsum, f_lo: int = 0, f_hi: Optional[int] = None, last_valid: Optional[int] = None, final: bool = False) -> None:
        if self.closed:
            raise RuntimeError("tracker saw its final frame; call reset() to start over")
        f_hi = int(fsum.shape[2]) if f_hi is None else int(f_hi)
        with self._torch.cuda.device(self.device):
            self._ops.segment_track(fsum, f_lo, f_hi, self.frames_seen, self.hop, self.hop if last_valid is None else last_valid, final,
                                    self.min_on, self.G, self.min_len, self.state, self.events, self.capacity, self.eps)
        self.frames_seen += f_hi - int(f_lo)
        self.closed = bool(final)

    def poll(self):
        n, recs = self._ops.segment_events(self.events, self.S, self.nb, self.capacity)
        out = []
        for s in range(self.S):
            new = int(n[s]) - self._read[s]
            if new > self.capacity:
                raise RuntimeError(f"stream {s}: {new} segments closed since the last read of a ring of {self.capacity}: events were lost")
            out.append([(int(r["lo"]), int(r["hi"]), float(r["count"]), r["prob"].copy())
                        for r in (recs[s, e % self.capacity] for e in range(self._read[s], int(n[s])))])
            self._read[s] = int(n[s])
        return out

    def open_runs(self):
        hdr, acc = self._ops.segment_state(self.state, self.S, self.nb)
        out = []
        for s in range(self.S):
            if not hdr[s, 0]:
                out.append(None)
                continue
            cnt = acc[s, self.nb]
            prob = (acc[s, :self.nb] / np.float64(np.float32(cnt) + np.float32(self.eps))).astype(np.float32) if cnt > 0.0 \
                else np.zeros(self.nb, np.float32)
            out.append((int(hdr[s, 1]), int(hdr[s, 2]), float(cnt), prob))
        return out


class SegmentSession(SegmentStreamSession, _HipSession):
    """SegmentStreamSession on a detector and a locator HipNet: one history and one window per tick for both nets, the locator's logits (or
    the caller's gate) gating the detector's frames kernel, one wv_segment_track per tick.  Nothing comes back to the host in push()."""

    def __init__(self, detector, locator, S: int, threshold: float = 0.5, min_on: float = 0.5, min_gap_frames: int = 2,
                 min_len_frames: int = 5, precision: str = "f32", locator_precision: Optional[str] = None, sample_rate: int = 16000,
                 capacity: int = 64):
        import torch
        from .localize import gate_threshold
        locator_precision = precision if locator_precision is None else locator_precision
        if precision not in ("f32", "f16") or locator_precision not in ("f32", "f16"):
            raise ValueError("precision must be 'f32' or 'f16'")
        if detector.cfg.kind != "detector" or locator.cfg.kind != "locator":
            raise ValueError("need a detector and a locator")
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        self.net, self.locator, self.precision, self.locator_precision, self._torch = detector, locator, precision, locator_precision, torch
        self._logit_thr = gate_threshold(threshold)
        hop, H = detector.cfg.hop_length, segment_halo(detector.cfg, locator.cfg)
        tracker = HipSegmentTracker(S, detector.cfg.head_bits, hop, min_on, min_gap_frames, min_len_frames, capacity, detector.device)
        SegmentStreamSession.__init__(self, S, hop, H, self._hip_frame_sums, tracker, self._hip_advance,
                                      lambda S_, cap: torch.zeros((S_, cap), dtype=torch.float32, device=detector.device), sample_rate,
                                      capacity, min_gap_frames, min_len_frames)

    def _hip_frame_sums(self, win, gwin):
        if gwin is not None:
            return self.net.detector_frame_sums(win, gwin, 0.5, self.precision)
        return self.net.detector_frame_sums(win, self.locator.locator(win, precision=self.locator_precision), self._logit_thr, self.precision)

    def _no_frames(self):
        return self._torch.zeros((self.S, self._tracker.nb + 1, 0), dtype=self._torch.float32, device=self.net.device)

    def _confidence(self, prob: np.ndarray) -> float:
        return float(self._torch.from_numpy(np.ascontiguousarray(prob, np.float32)).mean())      # as WaveVerify._segments takes it
