"""Live sessions at the stream's own sample rate and channel count.

`session.py` watermarks, detects and locates 16 kHz mono streams as samples arrive; `native.py` lets a FILE keep its rate and channels.  Here a
live stream does: S streams of C channels at `sample_rate` are pushed in lockstep, and come back watermarked at the same rate and channel count,

    front stage   new samples -> f32 channel mean -> 16 kHz (csrc/wv_native.hip, wv_native_session_down)
    inner session the 16 kHz windowed session of session.py, the generator returning its residual alone
    back stage    the residual -> `sample_rate`, strength times it added to the delayed originals (wv_native_session_up_add)

with both resamplers carrying state across pushes.  A stage emits only outputs that no future input can change: with orig : nw the two rates
over their gcd, L = 2 * width + orig, output m = g * nw + f reads inputs g * orig - width + j, j < L, so after t_in inputs the first
max(0, (t_in - width) // orig) * nw outputs are final; flush() emits the rest, ceil(nw * t_in / orig) in all, with zeros past the end as in the
file kernels.  Each output is the file kernels' fmaf chain over the same values, so the concatenated stream is `native.downmix_resample` /
`native.upsample_add` of the whole recording bit for bit.

The bookkeeping (StagePlan, EmbedPlan) is plain integer arithmetic: stream positions are Python ints and may pass 2^31; what a kernel is handed is
relative to the history's first sample and to the first phase group not yet emitted.  The sessions take the two stages as methods, stated here on
numpy arrays (any float dtype) so that the state machine runs on a CPU, and their arrays from the inner session's backend (session.NumpyArrays
/ TorchArrays); the Native*Session classes bind the stages to the HIP entry points and the HipNet sessions, where there is no CPU fallback."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib, native
from .native import MODEL_RATE
from .session import _CLOSED, DetectSession, EmbedSession, LocateSession, NumpyArrays, SegmentSession, Tick, _Ticker


# ---------------------------------------------------------------------------------------------------------------- the plan: integers only
@dataclass
class StageTick:
    """One push of one resampling stage.  Its sequence is cat(history[:hv], the n new samples); emit n_out outputs, output 0 being phase 0 of
    the first phase group not yet emitted, whose first tap is sequence sample -pad; the next history = sequence samples [drop, drop + hv2)."""
    hv: int
    n: int
    pad: int
    n_out: int
    drop: int
    hv2: int


class StagePlan:
    """Counts of one streaming resampler: t_in inputs received, n_done phase groups emitted, history = inputs [h0, t_in) with
    h0 = max(0, n_done * orig - width), fewer than L of them between pushes."""

    def __init__(self, orig: int, nw: int, L: int, width: int):
        self.orig, self.nw, self.L, self.width = int(orig), int(nw), int(L), int(width)
        self.cap = self.L
        self.reset()

    def reset(self) -> None:
        self.t_in = self.t_out = self.n_done = self.h0 = 0
        self.closed = False

    def _pad(self) -> int:
        return max(0, self.width - self.n_done * self.orig)

    def push(self, n: int) -> StageTick:
        if self.closed:
            raise RuntimeError(_CLOSED)
        hv, pad = self.t_in - self.h0, self._pad()
        t_in = self.t_in + n
        g = max(self.n_done, (t_in - self.width) // self.orig)          # every tap of groups < g has arrived
        h0 = max(0, g * self.orig - self.width)
        tick = StageTick(hv, n, pad, (g - self.n_done) * self.nw, h0 - self.h0, t_in - h0)
        self.t_in, self.n_done, self.h0 = t_in, g, h0
        self.t_out = g * self.nw
        return tick

    def total(self) -> int:
        """ceil(nw * t_in / orig): the whole-signal output length for what has been received."""
        return -(-self.nw * self.t_in // self.orig)

    def flush(self, n: int = 0, limit: Optional[int] = None) -> StageTick:
        """The last n inputs arrive and the stage closes: emit the rest, zeros past the end; limit: no more than this many outputs in all (the
        back stage cuts to the samples pushed)."""
        if self.closed:
            raise RuntimeError(_CLOSED)
        hv, pad = self.t_in - self.h0, self._pad()
        self.t_in += n
        end = self.total() if limit is None else min(self.total(), limit)
        tick = StageTick(hv, n, pad, max(0, end - self.t_out), hv + n, 0)
        self.t_out = max(self.t_out, end)
        self.closed = True
        return tick


@dataclass
class FloorTick:
    """The channel floor's part of one push: native frames f0 .. f0 + nf - 1 complete and their k samples leave; uv samples
    of u were held before the push, uv2 are held after it, so uv + back.n_out == k + uv2."""
    f0: int
    nf: int
    uv: int
    uv2: int
    k: int


@dataclass
class EmbedTick:
    """One push of a native embed session: the front stage's tick, the inner 16 kHz session's ticks (one; at flush its push and its flush) and the
    residual samples they return, the back stage's tick (back.n_out native samples come out) and the delay line's lengths before and after.
    Under a channel floor back.n_out counts the u formed, floor.k the samples that come out."""
    front: StageTick
    inner: tuple
    n_res: int
    back: StageTick
    pv: int
    pv2: int
    final: bool = False
    floor: Optional[FloorTick] = None


class EmbedPlan:
    """front StagePlan -> 16 kHz ticker of hop `hop` (halo H) -> back StagePlan, and the delay line of originals.
    channel_floor: the emission rule of the live per-channel SNR floor.  The back stage yields u up to t_u = back.t_out;
    a sample leaves only when its whole native frame has its u, so after a tick start(Fd) samples have left, Fd the largest f with
    start(f) <= t_u, start(f) = ceil(f * nw * hop / orig) (channel_floor.frame_starts), and the last t_u - start(Fd) < one frame of u are held.
    The frames counted as complete are those up to the one that holds sample start(Fd) - 1: an EMPTY frame (nw * hop < orig) behind it is counted
    with the next sample that leaves, so that a stream that ends there has the frames of its whole recording and no more.  flush() emits
    everything up to t_in, the last frame cut."""

    def __init__(self, sample_rate: int, hop: int, H: int = 0, channel_floor: bool = False):
        native.check_rate(sample_rate)
        self.sample_rate, self.hop = int(sample_rate), int(hop)
        self.front = StagePlan(*native.table_geometry(sample_rate, MODEL_RATE))
        self.back = StagePlan(*native.table_geometry(MODEL_RATE, sample_rate))
        self.ticker = _Ticker(hop, H)
        # the output lags the input by FEWER than this many native samples: fewer than L_front not yet through the front stage, fewer than hop
        # waiting for their frame, fewer than L_back residual samples not yet through the back stage
        self.latency_samples = self.front.L + -(-(self.hop + self.back.L) * self.sample_rate // MODEL_RATE)
        self.channel_floor = bool(channel_floor)
        if self.channel_floor:
            self.ucap = -(-self.back.nw * self.hop // self.back.orig)      # a nominal frame, ceil(nw * hop / orig): more than is ever held
            self.latency_samples += self.ucap
        self.pcap = self.latency_samples
        self.t_in = self.t_out = self.frames = 0

    def reset(self) -> None:
        self.front.reset()
        self.back.reset()
        self.ticker.reset()
        self.t_in = self.t_out = self.frames = 0

    @staticmethod
    def _res(t: Tick) -> int:
        return max(0, t.wlen - t.keep)

    def _tick(self, n: int, f: StageTick, inner: tuple, final: bool) -> EmbedTick:
        n_res = sum(self._res(t) for t in inner)
        pv = self.t_in - self.t_out
        self.t_in += n
        held = self.back.t_out - self.t_out                                 # u formed for samples not yet emitted: 0 without the floor
        b = self.back.flush(n_res, limit=self.t_in) if final else self.back.push(n_res)
        if not self.channel_floor:
            self.t_out += b.n_out
            return EmbedTick(f, inner, n_res, b, pv, self.t_in - self.t_out, final)
        M, orig, t_u, uv = self.back.nw * self.hop, self.back.orig, self.back.t_out, held
        end = t_u if final else -(-(t_u * orig // M) * M // orig)            # start(Fd)
        frames = ((end - 1) * orig) // M + 1 if end else 0                  # the frames of a recording of `end` samples
        fl = FloorTick(self.frames, frames - self.frames, uv, t_u - end, end - self.t_out)
        self.t_out, self.frames = end, frames
        return EmbedTick(f, inner, n_res, b, pv, self.t_in - self.t_out, final, fl)

    def push(self, n: int) -> EmbedTick:
        f = self.front.push(n)
        return self._tick(n, f, (self.ticker.push(f.n_out),), False)

    def flush(self) -> EmbedTick:
        f = self.front.flush()
        return self._tick(0, f, (self.ticker.push(f.n_out), self.ticker.flush()), True)


# ---------------------------------------------------------------------------------------------------------------- the stages on host arrays
def numpy_resample(seq: np.ndarray, pad: int, n_out: int, table) -> np.ndarray:
    """seq [S, len] -> [S, n_out] in seq's dtype: output m = g * nw + f is the sum over ascending j of K[f][j] * z[g * orig - pad + j], z = seq
    with zeros outside it.  One multiply and one add per tap in the arrays' own precision (the kernels make that one fmaf in f32), in the same
    order for every output, so it does not matter which call computes an output.  table = native.transposed_table(...)."""
    kt, orig, nw, L, _ = table
    S, n_seq = seq.shape
    acc = np.zeros((S, n_out), seq.dtype)
    if n_out == 0:
        return acc
    m = np.arange(n_out)
    g, f = m // nw, m % nw
    z = np.zeros((S, max(pad + n_seq, int(g[-1]) * orig + L)), seq.dtype)
    z[:, pad:pad + n_seq] = seq
    k = kt.astype(seq.dtype)
    for j in range(L):
        acc += k[j, f] * z[:, g * orig + j]
    return acc


def numpy_down(hist: np.ndarray, x: np.ndarray, t: StageTick, table):
    """Reference of wv_native_session_down: hist [S, cap] of channel means, x [S, C, n] -> (y [S, n_out], next history [S, cap])."""
    mono = x[:, 0].astype(hist.dtype)
    for c in range(1, x.shape[1]):
        mono = mono + x[:, c]
    mono = mono / hist.dtype.type(x.shape[1])
    seq = np.concatenate([hist[:, :t.hv], mono], axis=1)
    nxt = np.zeros_like(hist)
    nxt[:, :t.hv2] = seq[:, t.drop:t.drop + t.hv2]
    return numpy_resample(seq, t.pad, t.n_out, table), nxt


def numpy_up_add(rhist: np.ndarray, r: np.ndarray, pend: np.ndarray, x: np.ndarray, t: EmbedTick, table, gain: float):
    """Reference of wv_native_session_up_add: rhist [S, rcap], r [S, n_res], pend [S, C, pcap], x [S, C, n] -> (out [S, C, k], next pend, next
    rhist)."""
    b = t.back
    seq = np.concatenate([rhist[:, :b.hv], r.astype(rhist.dtype)], axis=1)
    u = numpy_resample(seq, b.pad, b.n_out, table)
    orig_ = np.concatenate([pend[:, :, :t.pv], x.astype(pend.dtype)], axis=2)
    out = orig_[:, :, :b.n_out] + pend.dtype.type(gain) * u[:, None, :]
    pnxt, rnxt = np.zeros_like(pend), np.zeros_like(rhist)
    pnxt[:, :, :t.pv2] = orig_[:, :, b.n_out:b.n_out + t.pv2]
    rnxt[:, :b.hv2] = seq[:, b.drop:b.drop + b.hv2]
    return out, pnxt, rnxt


# ---------------------------------------------------------------------------------------------------------------- the sessions
class _Stages:
    """The two stages and their state on host arrays of the backend's dtype; _HipStages states the same on the device."""

    def _table(self, of: int, nf: int):
        return native.transposed_table(of, nf)

    def _state(self, *shape):
        return self._arr.zeros(*shape)

    def _down(self, x, t: StageTick):
        y, self._hist = numpy_down(self._hist, x, t, self._ftab)
        return y

    def _up_add(self, r, x, t: EmbedTick):
        out, self._pend, self._rhist = numpy_up_add(self._rhist, r, self._pend, x, t, self._btab, self.strength)
        return out


class _HipStages(_Stages):
    """The stages as one launch each.  Every state buffer is a pair (current, next), the halves of one allocation: a launch reads the first,
    writes the next state into the second, and the pair swaps."""

    def _table(self, of: int, nf: int):
        front, back = native.tables(self.sample_rate, self._arr.device)
        return front if nf == MODEL_RATE else back

    def _state(self, *shape):
        return tuple(self._arr.zeros(2, *shape))

    def _down(self, x, t: StageTick):
        torch, dev = self._arr.torch, self._arr.device
        kt, orig, nw, L, width = self._ftab
        hist, nxt = self._hist
        y = torch.empty((self.S, t.n_out), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wv_native_session_down(
                hist.data_ptr(), hist.shape[1], t.hv, x.data_ptr() if t.n else None, t.n, kt.data_ptr(),
                y.data_ptr() if t.n_out else None, t.n_out, t.pad, nxt.data_ptr(), t.drop, t.hv2, self.S, self.channels, orig, nw, L, width,
                _lib.stream()), "wv_native_session_down")
        self._hist = (nxt, hist)
        return y

    def _up_add(self, r, x, t: EmbedTick):
        torch, dev = self._arr.torch, self._arr.device
        kt, orig, nw, L, width = self._btab
        b = t.back
        r = r.contiguous()
        (rhist, rnxt), (pend, pnxt) = self._rhist, self._pend
        out = torch.empty((self.S, self.channels, b.n_out), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wv_native_session_up_add(
                rhist.data_ptr(), rhist.shape[1], b.hv, r.data_ptr() if b.n else None, b.n, kt.data_ptr(),
                pend.data_ptr(), pend.shape[2], t.pv, x.data_ptr() if x.shape[2] else None, x.shape[2],
                out.data_ptr() if b.n_out else None, b.n_out, b.pad, float(self.strength), pnxt.data_ptr(), rnxt.data_ptr(), b.drop, b.hv2,
                self.S, self.channels, orig, nw, L, width, _lib.stream()), "wv_native_session_up_add")
        self._rhist, self._pend = (rnxt, rhist), (pnxt, pend)
        return out


class HostFrontSession(_Stages):
    """The front stage in front of a 16 kHz session `inner` (session.StreamSession or a subclass): push(x [S, C, n]) at `sample_rate` ->
    inner.push of the 16 kHz samples that became final; flush() -> the rest, then inner.flush().  Whatever the inner session returns stays on
    the 16 kHz time line.  The stage's arrays live on the inner session's backend; dtype: numpy arrays of that dtype instead."""

    def __init__(self, inner, sample_rate: int = MODEL_RATE, channels: int = 1, dtype=None):
        native.check_rate(sample_rate)
        if not 1 <= int(channels) <= 64:
            raise ValueError(f"channels must be within [1, 64], got {channels}")
        self.inner, self.S, self.sample_rate, self.channels = inner, inner.S, int(sample_rate), int(channels)
        self._arr = inner._arr if dtype is None else NumpyArrays(dtype)
        self._ftab, self._btab = self._table(self.sample_rate, MODEL_RATE), self._table(MODEL_RATE, self.sample_rate)
        self._plan = self._new_plan()
        self._new_state()

    def _new_plan(self):
        return StagePlan(*native.table_geometry(self.sample_rate, MODEL_RATE))

    def _new_state(self) -> None:
        self._hist = self._state(self.S, self._ftab[3])

    @property
    def samples_in(self) -> int:
        """Samples pushed per stream, at the stream's rate."""
        return self._plan.t_in

    def reset(self) -> None:
        self._plan.reset()
        self.inner.reset()
        self._new_state()

    def _checked(self, x):
        if len(x.shape) != 3 or x.shape[0] != self.S or x.shape[1] != self.channels:
            raise ValueError(f"expected new samples of shape [{self.S}, {self.channels}, n], got {tuple(x.shape)}")
        return self._arr.take(x)

    def _join(self, a, b):
        return b

    def push(self, x):
        x = self._checked(x)
        return self.inner.push(self._down(x, self._plan.push(int(x.shape[2]))))

    def flush(self):
        y = self._down(self._arr.zeros(self.S, self.channels, 0), self._plan.flush())
        first = self.inner.push(y)
        return self._join(first, self.inner.flush())


class HostEmbedSession(HostFrontSession):
    """Watermark S live streams of C channels at `sample_rate`: push(x [S, C, n]) -> the watermarked samples that became final [S, C, k], each
    x + strength * (the generator's residual brought to `sample_rate`) on every channel; flush() -> the rest, after which as many samples have
    come out as went in and their concatenation is embed_native_batch's arithmetic on the whole recording (the inner session's windows in place
    of one forward).  The output lags the input by fewer than `latency_samples`.  `inner` returns the RESIDUAL of its new frames, [S, 1, k]."""

    def __init__(self, inner, sample_rate: int = MODEL_RATE, channels: int = 1, strength: float = 1.0, dtype=None):
        self.strength = float(strength)
        super().__init__(inner, sample_rate, channels, dtype)

    def _new_plan(self):
        return EmbedPlan(self.sample_rate, self.inner._t.hop, self.inner._t.H)

    def _new_state(self) -> None:
        super()._new_state()
        self._rhist = self._state(self.S, self._btab[3])
        self._pend = self._state(self.S, self.channels, self._plan.pcap)

    @property
    def latency_samples(self) -> int:
        return self._plan.latency_samples

    @property
    def samples_out(self) -> int:
        """Samples emitted per stream, at the stream's rate."""
        return self._plan.t_out

    def _residual(self, y, t: EmbedTick):
        parts = []
        if y.shape[-1] or t.final:
            parts.append(self.inner.push(y))
        if t.final:
            parts.append(self.inner.flush())
        r = self._arr.cat([p.reshape(self.S, -1) for p in parts if p is not None], self.S)
        assert r.shape[-1] == t.n_res, (r.shape, t.n_res)
        return r

    def _run(self, x, t: EmbedTick):
        y = self._down(x, t.front)
        return self._up_add(self._residual(y, t), x, t)

    def push(self, x):
        x = self._checked(x)
        return self._run(x, self._plan.push(int(x.shape[2])))

    def flush(self):
        return self._run(self._arr.zeros(self.S, self.channels, 0), self._plan.flush())


class NativeEmbedSession(_HipStages, HostEmbedSession):
    """HostEmbedSession on a HipNet generator: msg [S, 16] (or [16]) the streams' messages; everything stays on the device."""

    def __init__(self, net, msg, sample_rate: int = MODEL_RATE, channels: int = 1, strength: float = 1.0, precision: str = "f32"):
        native.check_rate(sample_rate)                                  # refused before anything is built on the device
        HostEmbedSession.__init__(self, EmbedSession(net, msg, precision, add_input=False), sample_rate, channels, strength)


class NativeDetectSession(_HipStages, HostFrontSession):
    """Detect the watermark in S live streams of C channels at `sample_rate`: push(x [S, C, n]) -> session.DetectState over the 16 kHz frames
    completed so far (its samples_seen counts 16 kHz samples).  After flush() the state is that of a 16 kHz DetectSession given
    to_model_rate of the recording in the same pieces."""

    def __init__(self, net, S: int, sample_rate: int = MODEL_RATE, channels: int = 1, precision: str = "f32"):
        native.check_rate(sample_rate)                                  # refused before anything is built on the device
        HostFrontSession.__init__(self, DetectSession(net, S, precision), sample_rate, channels)


class NativeLocateSession(_HipStages, HostFrontSession):
    """Locate the watermark in S live streams: push(x [S, C, n]) -> the locator's logits of the 16 kHz frames completed by this push [S, 1, k].
    The logits stay on the 16 kHz time line: logit i of the concatenation belongs to the native samples around i * sample_rate / 16000."""

    def __init__(self, net, S: int, sample_rate: int = MODEL_RATE, channels: int = 1, precision: str = "f32"):
        native.check_rate(sample_rate)                                  # refused before anything is built on the device
        HostFrontSession.__init__(self, LocateSession(net, S, precision), sample_rate, channels)

    def _join(self, a, b):
        return self._arr.cat([a, b])


class NativeSegmentSession(_HipStages, HostFrontSession):
    """Watermarked segments of S live streams of C channels at `sample_rate`: push(x [S, C, n]) returns nothing; poll(), open_segments() and
    flush() are session.SegmentSession's on the 16 kHz samples the front stage has made final, so a Segment's frames count 16 kHz detector
    frames and its start_s / end_s are seconds on the stream's own clock.  After flush() the segments are those of a 16 kHz SegmentSession
    given to_model_rate of the recording in the same pieces.  A caller's gate has no native-rate form and is refused."""

    def __init__(self, detector, locator, S: int, sample_rate: int = MODEL_RATE, channels: int = 1, **kw):
        native.check_rate(sample_rate)                                  # refused before anything is built on the device
        HostFrontSession.__init__(self, SegmentSession(detector, locator, S, sample_rate=MODEL_RATE, **kw), sample_rate, channels)

    def push(self, x, gate=None) -> None:
        if gate is not None:
            raise ValueError("a gate is given per 16 kHz sample; a session at another rate or channel count takes none")
        HostFrontSession.push(self, x)

    def poll(self):
        return self.inner.poll()

    def open_segments(self):
        return self.inner.open_segments()

    def set_split(self, rule) -> None:
        """session.SegmentSession.set_split on the 16 kHz frames: only before the first push."""
        self.inner.set_split(rule)
