"""Windowed execution of the three nets: long clips, mixed-length batches.

All three nets are causal with a finite receptive field, so a clip can run as a batch of WINDOWS: a run of frames plus a left
halo at least as long as the receptive field.  Each window goes through the unchanged net forwards and only its kept columns
are written back.  The result equals the whole-clip forward up to f32 summation order provided that
  * window starts and keep edges sit on hop multiples counted from the clip's true t = 0,
  * every clip's first window starts at its true t = 0,
  * its last window ends at its true end (so the causal convs' extra right padding and the ConvTranspose trims match).
`halo` and `plan` are pure Python; the windowed forwards move data with csrc/wv_window.hip.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence

from . import _lib
from .config import NetConfig


# --------------------------------------------------------------------------- planner (no GPU, no torch)
def receptive_context(cfg: NetConfig) -> int:
    """Largest t - lo(t) over the net's outputs, lo(t) the earliest input sample output t depends on, walked analytically
    over the layer list.  A layer at cumulative stride st whose index i covers input samples [i*st - A, i*st + st - 1]:
      * stride-1 conv, k taps, dilation d:  A += (k-1)*d*st
      * causal strided conv (k = 2r, stride r, left pad k-1-(r-1)):  A += (k-1-(r-1))*st, then st *= r
      * STFT of n_fft points at hop st (left pad n_fft-1, frame i ends at sample i*st):  A = max(A, n_fft-1)  (added to the
        residual stream, so the two paths' maximum)
      * depth-wise ConvTranspose k = 2r, stride r, right trim r (the decoder): output j reads input floor(j/r)-1 and
        floor(j/r), so A += st_in + (r-1)*st_out
      * the head's ConvTranspose k = s = hop: output t reads frame floor(t/hop): A += hop-1."""
    rk = cfg.residual_kernel_size
    A = cfg.kernel_size - 1                                          # conv_pre
    st, mult = 1, 1
    for r in cfg.ratios_enc:
        for j in range(1, cfg.n_residual_enc + 1):                   # ResnetBlock: DW k dil base**j, DW k dil 1
            A += ((rk - 1) * cfg.dilation_base ** j + (rk - 1)) * st
        A = max(A, mult * cfg.n_fft_base - 1)                        # SpecBlock of this scale
        A += (2 * r - 1 - (r - 1)) * st                              # downsample DW conv k = 2r, stride r
        st *= r
        mult *= 2
    A = max(A, mult * cfg.n_fft_base - 1)                            # spec_post
    A += (cfg.last_kernel_size - 1) * st                             # conv_post DW
    if not cfg.has_decoder:
        return A + st - 1                                            # head ConvTranspose k = s = hop
    A += (cfg.kernel_size - 1) * st                                  # decoder's first DW conv
    for r in cfg.strides:
        sto = st // r
        A += st + (r - 1) * sto                                      # upsample ConvTranspose k = 2r
        st = sto
        for j in range(cfg.n_residual_dec):
            A += ((rk - 1) * cfg.dilation_base ** j + (rk - 1)) * st
    return A + cfg.last_kernel_size - 1                              # last conv


def halo(cfg: NetConfig) -> int:
    """Left context a window needs: the receptive context + 1, rounded up to the hop (5760 / 2880 / 416 samples for the
    default generator / detector / locator).  Perturbing input sample p changes no output at or beyond p + halo(cfg)."""
    hop = cfg.hop_length
    return -(-(receptive_context(cfg) + 1) // hop) * hop


def pipeline_hop(cfgs: Sequence[NetConfig]) -> int:
    """Window granularity for a combined embed -> detect -> locate pipeline: the lcm of the nets' hops (320 by default)."""
    h = 1
    for c in cfgs:
        h = h * c.hop_length // math.gcd(h, c.hop_length)
    return h


@dataclass(frozen=True)
class Window:
    clip: int        # index of the clip
    start: int       # first input sample, in the clip's coordinates
    length: int      # input samples
    keep_lo: int     # kept output columns [keep_lo, keep_hi), in the clip's coordinates
    keep_hi: int


def plan(lengths: Sequence[int], window: int, cfg: NetConfig, max_windows: int = 64) -> List[List[Window]]:
    """Windows for clips of the given lengths, grouped into launches of equal-length windows, at most max_windows each.
    `window` is rounded up to a multiple of the hop.  A clip no longer than the window runs whole; otherwise its first window
    is [0, L) and keeps all of it, each further window starts halo(cfg) before the first column it keeps, interior windows
    have length L, and the last one ends at the clip's end (the only ragged length).  Keep regions tile [0, T) once."""
    hop, H = cfg.hop_length, halo(cfg)
    if max_windows < 1:
        raise ValueError("max_windows must be >= 1")
    L = -(-int(window) // hop) * hop
    if L < H + hop:
        raise ValueError(f"window of {L} samples leaves nothing to keep after the {H}-sample halo; use at least {H + hop}")
    by_len = {}
    for b, T in enumerate(lengths):
        T = int(T)
        if T < 1:
            raise ValueError(f"clip {b} is empty")
        if T <= L:
            wins = [Window(b, 0, T, 0, T)]
        else:
            wins = [Window(b, 0, L, 0, L)]
            k = L
            while k + (L - H) < T:
                wins.append(Window(b, k - H, L, k, k + L - H))
                k += L - H
            wins.append(Window(b, k - H, T - (k - H), k, T))
        for w in wins:
            by_len.setdefault(w.length, []).append(w)
    out = []
    for n in sorted(by_len, reverse=True):
        ws = by_len[n]
        out += [ws[i:i + max_windows] for i in range(0, len(ws), max_windows)]
    return out


# --------------------------------------------------------------------------- windowed forwards on a HipNet
def _torch():
    import torch
    return torch


def _pack(clips, device):
    """-> (packed 1-D float32 tensor, lengths, base offsets, as_batch)."""
    torch = _torch()
    if isinstance(clips, torch.Tensor):
        x = clips
        if x.dim() == 2:
            x = x.unsqueeze(1)
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"expected audio of shape [B,1,T] or a list of 1-D clips, got {tuple(clips.shape)}")
        B, _, T = x.shape
        return x.to(device, torch.float32).contiguous().view(-1), [T] * B, [b * T for b in range(B)], True
    flat = []
    for i, c in enumerate(clips):
        c = c.to(device, torch.float32).reshape(-1)
        flat.append(c)
    if not flat:
        raise ValueError("no clips")
    lengths = [int(c.numel()) for c in flat]
    bases = [0]
    for n in lengths[:-1]:
        bases.append(bases[-1] + n)
    return torch.cat(flat).contiguous(), lengths, bases, False


def _unpack(out, lengths, bases, as_batch, C_=1):
    """out is the packed [C, T] outputs of every clip, one after the other."""
    if as_batch:
        return out.view(len(lengths), C_, lengths[0])
    return [out[C_ * b0: C_ * b0 + C_ * T].view(C_, T) if C_ > 1 else out[b0: b0 + T] for b0, T in zip(bases, lengths)]


def gather(net, packed, wins: Sequence[Window], bases):
    """[W, 1, L] window batch from the packed clips (wv_window_gather)."""
    torch = _torch()
    W, L = len(wins), wins[0].length
    offs = torch.tensor([bases[w.clip] + w.start for w in wins], dtype=torch.int64).to(packed.device)
    xw = torch.empty((W, 1, L), dtype=torch.float32, device=packed.device)
    _lib.check(net._lib.wv_window_gather(packed.data_ptr(), packed.numel(), offs.data_ptr(), xw.data_ptr(), W, L, _lib.stream()),
               "wv_window_gather")
    return xw


def scatter(net, y, wins: Sequence[Window], bases, lengths, out, C_=1):
    """Kept columns of y [W, C, L] into the packed [C, T] clip outputs `out` (wv_window_scatter)."""
    torch = _torch()
    W, L = len(wins), wins[0].length
    desc = torch.tensor([[C_ * bases[w.clip] + w.start, lengths[w.clip], w.keep_lo - w.start, w.keep_hi - w.start] for w in wins],
                        dtype=torch.int64).to(y.device)
    y = y.contiguous()
    _lib.check(net._lib.wv_window_scatter(y.data_ptr(), desc.data_ptr(), out.data_ptr(), out.numel(), W, C_, L, _lib.stream()),
               "wv_window_scatter")


def _run(net, clips, window, max_windows, fwd, C_=1):
    torch = _torch()
    with torch.cuda.device(net.device):
        packed, lengths, bases, as_batch = _pack(clips, net.device)
        out = torch.empty(C_ * packed.numel(), dtype=torch.float32, device=net.device)
        for wins in plan(lengths, window, net.cfg, max_windows):
            scatter(net, fwd(gather(net, packed, wins, bases), wins), wins, bases, lengths, out, C_)
        return _unpack(out, lengths, bases, as_batch, C_)


def windowed_generator(net, clips, msg, window: int = 480000, precision: str = "f32", max_windows: int = 64, add_input: bool = True):
    """Watermarked audio G(x, msg) + x of every clip, windowed.  clips: a list of 1-D device tensors of any lengths (-> a list
    of 1-D tensors) or [B,1,T] (-> [B,1,T]); msg [B|1, 16]: each window uses its clip's row.  add_input=False: the residual
    G(x, msg) alone (what the native-rate route brings back up to the file's rate)."""
    torch = _torch()
    msg = msg.to(net.device).float()
    if msg.dim() == 1:
        msg = msg.unsqueeze(0)

    def fwd(xw, wins):
        rows = torch.tensor([w.clip % msg.shape[0] for w in wins], dtype=torch.int64, device=net.device)
        return net.generator(xw, msg.index_select(0, rows).contiguous(), add_input=add_input, precision=precision)
    return _run(net, clips, window, max_windows, fwd)


def windowed_locator(net, clips, window: int = 480000, precision: str = "f32", max_windows: int = 64):
    """Locator logits of every clip, windowed: a list of 1-D tensors, or [B,1,T] for a [B,1,T] input."""
    return _run(net, clips, window, max_windows, lambda xw, wins: net.locator(xw, precision=precision))


def windowed_detector(net, clips, window: int = 480000, precision: str = "f32", max_windows: int = 64):
    """Detector logits of every clip, windowed: a list of [nbits, T] tensors, or [B, nbits, T]."""
    return _run(net, clips, window, max_windows, lambda xw, wins: net.detector(xw, precision=precision), net.cfg.head_bits)


def windowed_detector_mean_prob(net, clips, window: int = 480000, precision: str = "f32", max_windows: int = 64):
    """mean_t sigmoid(detector logits) of every clip, [B, nbits], without storing any logits: each window's sigmoid sum over its
    kept columns (the head kernels' windowed mode), then one fixed-order f64 reduction per clip (wv_window_reduce_mean)."""
    torch = _torch()
    nb = net.cfg.head_bits
    with torch.cuda.device(net.device):
        packed, lengths, bases, _ = _pack(clips, net.device)
        launches = plan(lengths, window, net.cfg, max_windows)
        n_rows = sum(len(w) for w in launches)
        psum = torch.empty((n_rows, nb), dtype=torch.float32, device=net.device)
        per_clip = [[] for _ in lengths]
        row = 0
        for wins in launches:
            xw = gather(net, packed, wins, bases)
            lo = [w.keep_lo - w.start for w in wins]
            hi = [w.keep_hi - w.start for w in wins]
            net.detector_window_psum(xw, lo, hi, psum[row: row + len(wins)], precision)
            for i, w in enumerate(wins):
                per_clip[w.clip].append((w.start, row + i))
            row += len(wins)
        ptr, rows = [0], []
        for lst in per_clip:
            rows += [r for _, r in sorted(lst)]
            ptr.append(len(rows))
        ptr_t = torch.tensor(ptr, dtype=torch.int32).to(net.device)
        rows_t = torch.tensor(rows, dtype=torch.int32).to(net.device)
        len_t = torch.tensor(lengths, dtype=torch.int64).to(net.device)
        mean = torch.empty((len(lengths), nb), dtype=torch.float32, device=net.device)
        _lib.check(net._lib.wv_window_reduce_mean(psum.data_ptr(), n_rows, ptr_t.data_ptr(), rows_t.data_ptr(), len_t.data_ptr(),
                                                  mean.data_ptr(), len(lengths), nb, _lib.stream()), "wv_window_reduce_mean")
        return mean


# --------------------------------------------------------------------------- localized detection: per-frame sums, windowed
def frame_scatter_desc(wins: Sequence[Window], frame_bases: Sequence[int], frames: Sequence[int], hop: int, C_: int) -> List[List[int]]:
    """wv_window_scatter descriptors in FRAME units for window outputs [W, C_, ceil(L / hop)]: per window {offset of its frame 0 in the
    packed [C_, Fr] clip outputs, the clip's Fr, kept frames lo, hi} (relative to the window).  Window starts and keep edges are hop
    multiples, so kept frames are whole; only a clip's last frame is partial (keep_hi == T there, rounded up).  Pure Python."""
    desc = []
    for w in wins:
        if w.start % hop or w.keep_lo % hop:
            raise ValueError("window start and keep edge must be hop multiples")
        desc.append([C_ * frame_bases[w.clip] + w.start // hop, frames[w.clip], (w.keep_lo - w.start) // hop, -(-(w.keep_hi - w.start) // hop)])
    return desc


def windowed_detector_frame_sums(net, clips, gates=None, gate_thr: float = 0.0, window: int = 480000, precision: str = "f32",
                                 max_windows: int = 64):
    """HipNet.detector_frame_sums of every clip, windowed: a list of [nbits + 1, Fr_b] tensors, or [B, nbits + 1, Fr] for a [B,1,T] input.
    gates: None, or the clips' gates in the same form as `clips` (per clip one value per sample).  Gate windows are gathered from the
    packed gates with the audio's own offsets, the frames kernel runs on the window batch and the kept frames are scattered in frame
    units, so no logits and no separate gate tensor are written."""
    torch = _torch()
    nb1, hop = net.cfg.head_bits + 1, net.cfg.hop_length
    with torch.cuda.device(net.device):
        packed, lengths, bases, as_batch = _pack(clips, net.device)
        gpacked = None
        if gates is not None:
            if isinstance(gates, torch.Tensor) and gates.dim() == 2:
                gates = gates.unsqueeze(1)
            gpacked, glen, _, _ = _pack(gates, net.device)
            if glen != lengths:
                raise ValueError("every clip's gate must have the clip's length")
        frames = [-(-T // hop) for T in lengths]
        fbases = [0]
        for n in frames[:-1]:
            fbases.append(fbases[-1] + n)
        out = torch.empty(nb1 * sum(frames), dtype=torch.float32, device=net.device)
        for wins in plan(lengths, window, net.cfg, max_windows):
            W, L = len(wins), wins[0].length
            xw = gather(net, packed, wins, bases)
            gw = None if gpacked is None else gather(net, gpacked, wins, bases).view(W, L)
            fs = net.detector_frame_sums(xw, gw, gate_thr, precision)
            desc = torch.tensor(frame_scatter_desc(wins, fbases, frames, hop, nb1), dtype=torch.int64).to(net.device)
            _lib.check(net._lib.wv_window_scatter(fs.data_ptr(), desc.data_ptr(), out.data_ptr(), out.numel(), W, nb1, fs.shape[2], _lib.stream()),
                       "wv_window_scatter")
        if as_batch:
            return out.view(len(lengths), nb1, frames[0])
        return [out[nb1 * f0: nb1 * (f0 + n)].view(nb1, n) for f0, n in zip(fbases, frames)]


# --------------------------------------------------------------------------- span embedding
# Watermark chosen stretches of a clip, each with its own id: out = x + w * G(x, msg(id)) inside a span, x bit for bit outside.  The
# generator is causal and halo(cfg) bounds how far back an output looks, so the residual over [s, e) needs the input from
# floor_hop(s) - H only: a span becomes one or more windows of its clip, the windows of all clips and spans share launches as a bank's
# rows do (left-aligned, right-zero-padded), and two data-movement kernels stand around each generator launch (wv_span_gather,
# wv_span_scatter_add).  plan_spans and the two numpy twins are integers and host arrays only.
@dataclass(frozen=True)
class SpanWindow:
    clip: int        # index of the clip
    start: int       # first input sample, in the clip's coordinates: a hop multiple
    length: int      # input samples; start + length is a hop multiple or the clip's true end
    keep_lo: int     # columns the window adds its residual to, [keep_lo, keep_hi) in the clip's coordinates: a piece of its span
    keep_hi: int
    span_lo: int     # the whole span [span_lo, span_hi) (the ramps count from its edges, not from the piece's)
    span_hi: int
    msg: object      # the span's third element: the window's message row


def span_ramp(fade_samples: int):
    """ramp[j] = float32(0.5 - 0.5 cos(pi (j + 0.5) / fade_samples)), formed in float64 and rounded once; None for a hard cut."""
    import numpy as np
    F = int(fade_samples)
    if F < 0 or F != fade_samples:
        raise ValueError("fade_samples must be a non-negative integer")
    if F == 0:
        return None
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(F, dtype=np.float64) + 0.5) / F)).astype(np.float32)


def check_spans(lengths: Sequence[int], spans) -> List[list]:
    """-> per clip its spans [(start, end, msg)] sorted by start, refusing what span embedding does not define: a span that is empty,
    inverted or outside its clip, and spans of one clip that overlap (abutting is allowed)."""
    if len(spans) != len(lengths):
        raise ValueError(f"{len(lengths)} clips but {len(spans)} span lists")
    out = []
    for b, (T, lst) in enumerate(zip(lengths, spans)):
        T = int(T)
        if T < 1:
            raise ValueError(f"clip {b} is empty")
        mine = sorted(((int(s), int(e), m) for s, e, m in lst), key=lambda v: v[:2])
        for s, e, _ in mine:
            if s >= e:
                raise ValueError(f"clip {b}: span [{s}, {e}) is empty or inverted")
            if s < 0 or e > T:
                raise ValueError(f"clip {b}: span [{s}, {e}) lies outside the clip's {T} samples")
        for (_, e0, _), (s1, _, _) in zip(mine, mine[1:]):
            if s1 < e0:
                raise ValueError(f"clip {b}: spans overlap at sample {s1}")
        out.append(mine)
    return out


def plan_spans(lengths: Sequence[int], spans, window: int, cfg: NetConfig, pad_limit: float = 1.5, max_windows: int = 64) -> List[List[SpanWindow]]:
    """Windows for the spans [(start, end, msg)] of clips of the given lengths, grouped into launches.
    A span [s, e) of a clip of T samples: its first window starts at max(0, floor_hop(s) - H) and, where that fits `window` (rounded up
    to the hop, at least H + hop), ends at min(ceil_hop(e), T) and keeps [s, e).  A longer one is cut as plan() cuts clips: the first
    piece is `window` long, each further piece starts H before the first column it keeps, the last ends at min(ceil_hop(e), T).  Keep
    ranges are the span's own samples (no hop multiples) and tile every span once.
    Launches: the windows of all clips and spans sorted by length, left-aligned, to be right-zero-padded to the launch's longest; a new
    launch starts where the next window would be longer than pad_limit times the launch's shortest or after max_windows rows.  A window
    that ends at a clip's ragged true end shares a launch only with windows of its own length (what StreamBank.close() does for it)."""
    hop, H = cfg.hop_length, halo(cfg)
    if max_windows < 1:
        raise ValueError("max_windows must be >= 1")
    if not pad_limit >= 1.0:
        raise ValueError("pad_limit must be at least 1 (float('inf'): as few launches as the ragged ends allow)")
    L = max(-(-int(window) // hop) * hop, H + hop)
    wins = []
    for b, mine in enumerate(check_spans(lengths, spans)):
        T = int(lengths[b])
        for s, e, m in mine:
            start = max(0, s // hop * hop - H)
            end = min(-(-e // hop) * hop, T)
            if end - start <= L:
                wins.append(SpanWindow(b, start, end - start, s, e, s, e, m))
                continue
            wins.append(SpanWindow(b, start, L, s, start + L, s, e, m))
            k = start + L
            while k + (L - H) < e:
                wins.append(SpanWindow(b, k - H, L, k, k + L - H, s, e, m))
                k += L - H
            wins.append(SpanWindow(b, k - H, end - (k - H), k, e, s, e, m))
    wins.sort(key=lambda w: (w.length, w.clip, w.start))
    ragged = lambda w: (w.start + w.length) % hop != 0                  # only a clip's true end is off the hop grid
    out: List[List[SpanWindow]] = []
    lone = False                                                        # the open launch holds a ragged window
    for w in wins:
        g = out[-1] if out else None
        fits = g is not None and len(g) < max_windows and w.length <= pad_limit * g[0].length
        if fits and (lone or ragged(w)) and w.length != g[0].length:
            fits = False
        if fits:
            g.append(w)
            lone = lone or ragged(w)
        else:
            out.append([w])
            lone = ragged(w)
    return out


def span_gather_desc(wins: Sequence[SpanWindow], bases: Sequence[int]) -> List[List[int]]:
    """wv_span_gather's rows {offset in the packed clips, wlen}."""
    return [[bases[w.clip] + w.start, w.length] for w in wins]


def span_scatter_desc(wins: Sequence[SpanWindow], bases: Sequence[int]) -> List[List[int]]:
    """wv_span_scatter_add's rows {offset in the packed output of the window's column 0, keep lo, keep hi, span start, span end}, the last
    four relative to the window's column 0."""
    return [[bases[w.clip] + w.start, w.keep_lo - w.start, w.keep_hi - w.start, w.span_lo - w.start, w.span_hi - w.start] for w in wins]


def span_gather_row_ok(row, n_src: int, Lmax: int) -> bool:
    """Whether wv_span_gather serves a descriptor row (it skips any other whole)."""
    off, wlen = (int(v) for v in row)
    return 0 <= off and 0 <= wlen <= Lmax and off + wlen <= n_src


def span_row_ok(row, n_out: int, Lmax: int) -> bool:
    """Whether wv_span_scatter_add serves a descriptor row (it skips any other whole)."""
    o, lo, hi, ss, se = (int(v) for v in row)
    return 0 <= lo < hi <= Lmax and ss <= lo and hi <= se and 0 <= o + lo and o + hi <= n_out


def numpy_span_gather(src, desc, A: int, Lmax: int, dst=None):
    """Reference of wv_span_gather on host arrays -> dst [A, 1, Lmax] (a fresh array of zeros if none is given: the kernel leaves a skipped
    row as it was)."""
    import numpy as np
    dst = np.zeros((A, 1, Lmax), src.dtype) if dst is None else dst
    for r, row in enumerate(np.asarray(desc, np.int64).reshape(-1, 2)[:A]):
        if span_gather_row_ok(row, int(src.shape[0]), Lmax):
            off, wlen = int(row[0]), int(row[1])
            dst[r, 0, :wlen] = src[off:off + wlen]
            dst[r, 0, wlen:] = 0
    return dst


def numpy_span_scatter_add(y, x, desc, ramp, gain, out):
    """Reference of wv_span_scatter_add on host arrays, in out's dtype with every rounding kept: w = gain * ramp[m] (gain alone beyond the
    ramp), v = w * y, out = x + v (v alone where x is None).  x may be out.  Only the served rows' keep ranges are written."""
    import numpy as np
    dt = out.dtype.type
    A, _, Lmax = y.shape
    F = 0 if ramp is None else int(len(ramp))
    g = dt(gain)
    for r, row in enumerate(np.asarray(desc, np.int64).reshape(-1, 5)[:A]):
        if not span_row_ok(row, int(out.shape[0]), Lmax):
            continue
        o, lo, hi, ss, se = (int(v) for v in row)
        j = np.arange(lo, hi, dtype=np.int64)
        m = np.minimum(j - ss, se - 1 - j)
        w = np.full(hi - lo, g, out.dtype)
        if F:
            inside = m < F
            w[inside] = g * np.asarray(ramp)[m[inside]].astype(out.dtype)
        v = w * y[r, 0, lo:hi].astype(out.dtype)
        out[o + lo:o + hi] = v if x is None else x[o + lo:o + hi].astype(out.dtype) + v
    return out


def _clip_lengths(clips) -> List[int]:
    if hasattr(clips, "dim"):
        if clips.dim() not in (2, 3) or (clips.dim() == 3 and clips.shape[1] != 1):
            raise ValueError(f"expected audio of shape [B,1,T] or a list of 1-D clips, got {tuple(clips.shape)}")
        return [int(clips.shape[-1])] * int(clips.shape[0])
    if not len(clips):
        raise ValueError("no clips")
    return [int(c.numel()) for c in clips]


def span_generator(net, clips, msgs, spans, window: int = 480000, precision: str = "f32", pad_limit: float = 1.5, max_windows: int = 64,
                   fade_samples: int = 0, gain: float = 1.0, add_input: bool = True):
    """Span embedding of every clip: out = x + w * G(x, msgs[m]) over each span (start, end, m) of spans[clip], x bit for bit elsewhere;
    w = gain * ramp(distance to the span's nearer edge), ramp = span_ramp(fade_samples).  clips as windowed_generator takes them, the
    result the same kind; msgs [M, msg_dimension]; spans: per clip a list of (start, end, row of msgs) in samples.
    add_input=False: the masked residual alone, zeros outside the spans (what the native-rate route brings up to the file's rate).
    Everything is planned and checked before anything touches the device; per launch wv_span_gather -> net.generator on the window batch
    with each row's own message -> wv_span_scatter_add."""
    import numpy as np
    torch = _torch()
    lengths = _clip_lengths(clips)
    ramp = span_ramp(fade_samples)
    if not gain == gain:
        raise ValueError("gain is not a number")
    n_msg = int(msgs.shape[0]) if msgs.dim() > 1 else 1
    launches = plan_spans(lengths, spans, window, net.cfg, pad_limit, max_windows)
    for w in (w for g in launches for w in g):
        if isinstance(w.msg, bool) or not isinstance(w.msg, (int, np.integer)) or not 0 <= w.msg < n_msg:
            raise ValueError(f"clip {w.clip}: span message row {w.msg!r} is not a row of the {n_msg} messages")
    with torch.cuda.device(net.device):
        packed, lengths, bases, as_batch = _pack(clips, net.device)
        out = packed.clone() if add_input else torch.zeros_like(packed)
        if launches:
            msgs = msgs.to(net.device).float().reshape(n_msg, -1)
            flat = [w for g in launches for w in g]
            table = np.concatenate([np.array(span_gather_desc(flat, bases), np.int64).reshape(-1), np.array(span_scatter_desc(flat, bases), np.int64).reshape(-1),
                                    np.array([w.msg for w in flat], np.int64)])
            table = torch.from_numpy(table).to(net.device)                 # one copy for every launch's descriptors
            N = len(flat)
            gdesc, sdesc, rows = table[:2 * N].view(N, 2), table[2 * N:7 * N].view(N, 5), table[7 * N:]
            ramp_t = None if ramp is None else torch.from_numpy(ramp).to(net.device)
            F = 0 if ramp is None else int(ramp.shape[0])
            a = 0
            for wins in launches:
                A, Lmax = len(wins), wins[-1].length
                xw = torch.empty((A, 1, Lmax), dtype=torch.float32, device=net.device)
                _lib.check(net._lib.wv_span_gather(packed.data_ptr(), packed.numel(), gdesc[a:].data_ptr(), xw.data_ptr(), A, Lmax, _lib.stream()),
                           "wv_span_gather")
                y = net.generator(xw, msgs.index_select(0, rows[a:a + A]).contiguous(), add_input=False, precision=precision).contiguous()
                _lib.check(net._lib.wv_span_scatter_add(y.data_ptr(), out.data_ptr() if add_input else None, sdesc[a:].data_ptr(), _lib.ptr(ramp_t), F,
                                                        float(gain), out.data_ptr(), out.numel(), A, Lmax, _lib.stream()), "wv_span_scatter_add")
                a += A
        return _unpack(out, lengths, bases, as_batch)
