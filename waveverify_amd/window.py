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
