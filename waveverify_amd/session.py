"""Live sessions: S audio streams watermarked, detected or located in lockstep as samples arrive.

Each push appends n >= 0 samples per stream.  The frames completed so far (a multiple of the net's hop) run as one window that
starts halo(cfg) samples before the first new frame (or at the stream's t = 0) and ends at the last completed frame; only the
new frames' columns are returned.  Incomplete-frame samples and the halo history stay on the device (wv_session_advance).
flush() runs the remaining partial frame as a final window ending at the true end, after which the concatenated outputs equal
the whole-clip forward on the concatenated input.  ("Session", not "stream", to keep clear of HIP streams.)

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
