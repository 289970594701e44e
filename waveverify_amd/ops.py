"""Single fused units of the hot path through the C ABI (wv_op_* of include/waveverify_hip.h).

Activations are CUDA tensors; weights are host arrays in the reference's layouts.  These are
test handles — the nets in nets.py run the same kernels with weights packed once."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib


def _w(a) -> Optional[np.ndarray]:
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, np.float32))


def _hp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


_ON_GPU = "activations must live on the GPU"


def _out(given: Optional[torch.Tensor], shape, dtype, device, what: str = "out") -> torch.Tensor:
    """An output buffer: the caller's (`out=` / `out_act=`: a test handle for guarded or misaligned placements; checked for shape,
    dtype, device and contiguity, never reallocated) or a fresh one."""
    shape = tuple(int(s) for s in shape)
    if given is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(given.shape) != shape or given.dtype != dtype or given.device != torch.device(device) or not given.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor {list(shape)} on {device}, got {given.dtype} "
                         f"{list(given.shape)} on {given.device}")
    return given


def pw_dw(X, w_pw, w_dw, dw_bias=None, film=None, resid=None, stride=1, dilation=1,
          pre_scale=1.0, pre_elu=True, out_scale=1.0, bands=1, act_scale: Optional[float] = None, out=None, out_act=None):
    """act_scale given: also returns the second output ELU(act_scale * y) -> (Y, Yact).  out / out_act: caller-owned outputs."""
    lib = _lib.load()
    X = _lib.dev(X, _ON_GPU)
    B, K, Tin = X.shape
    w_pw, w_dw, dw_bias = _w(w_pw), _w(w_dw), _w(dw_bias)
    M, ks = w_dw.shape[0], w_dw.shape[-1]
    w_pw = w_pw.reshape(M, K)
    Tout = -(-Tin // stride)
    Y = _out(out, (B, M, Tout), torch.float32, X.device)
    film = None if film is None else _lib.dev(film, _ON_GPU)
    resid = None if resid is None else _lib.dev(resid, _ON_GPU)
    Yact = _out(out_act, Y.shape, torch.float32, X.device, "out_act") if act_scale is not None else None
    _lib.check(lib.wv_op_pw_dw(X.data_ptr(), _hp(w_pw), _hp(w_dw), _hp(dw_bias), _lib.ptr(film), _lib.ptr(resid),
                               Y.data_ptr(), B, K, M, Tin, ks, stride, dilation, pre_scale,
                               int(pre_elu), out_scale, bands, _lib.ptr(Yact), float(act_scale or 0.0),
                               _lib.stream()), "wv_op_pw_dw")
    return Y if act_scale is None else (Y, Yact)


def resblock(X, w_pw1, w_dw1, b1, w_pw2, w_dw2, b2, pre_scale=1.0, out_scale=1.0, act_scale: Optional[float] = None,
             want_raw: bool = True, out=None, out_act=None):
    """Fused SEANetResnetBlock, raw in / raw out: y = X + out_scale * half2(half1(ELU(pre_scale * X))).
    -> Y, or (Y, Yact) with act_scale given, or Yact alone with want_raw=False."""
    lib = _lib.load()
    X = _lib.dev(X, _ON_GPU)
    B, Cc, T = X.shape
    ws = [_w(w_pw1).reshape(Cc, Cc), _w(w_dw1).reshape(Cc, -1), _w(b1), _w(w_pw2).reshape(Cc, Cc),
          _w(w_dw2).reshape(Cc, -1), _w(b2)]
    Y = _out(out, X.shape, torch.float32, X.device) if want_raw else None
    Yact = _out(out_act, X.shape, torch.float32, X.device, "out_act") if act_scale is not None else None
    _lib.check(lib.wv_op_resblock(X.data_ptr(), float(pre_scale), *[_hp(w) for w in ws], _lib.ptr(Y), _lib.ptr(Yact),
                                  B, Cc, T, out_scale, float(act_scale or 0.0), _lib.stream()), "wv_op_resblock")
    if Y is None:
        return Yact
    return Y if act_scale is None else (Y, Yact)


def dw_pw(X, w_pw, bias=None, w_dw=None, mode=0, ks_or_ratio=0, pre_scale=1.0, pre_elu=False,
          l2norm=False, accumulate_into: Optional[torch.Tensor] = None, out_scale=1.0,
          act_scale: Optional[float] = None, out=None, out_act=None):
    lib = _lib.load()
    X = _lib.dev(X, _ON_GPU)
    B, K, Tin = X.shape
    w_pw, bias, w_dw = _w(w_pw), _w(bias), _w(w_dw)
    M = w_pw.shape[0]
    w_pw = w_pw.reshape(M, K)
    Tout = Tin * ks_or_ratio if mode == 2 else Tin
    if accumulate_into is not None:
        Y = accumulate_into
        assert Y.is_cuda and Y.is_contiguous() and tuple(Y.shape) == (B, M, Tout)
    else:
        Y = _out(out, (B, M, Tout), torch.float32, X.device)
    Yact = _out(out_act, Y.shape, torch.float32, X.device, "out_act") if act_scale is not None else None
    _lib.check(lib.wv_op_dw_pw(X.data_ptr(), _hp(w_dw), _hp(w_pw), _hp(bias), Y.data_ptr(), B, K, M,
                               Tin, mode, ks_or_ratio, pre_scale, int(pre_elu), int(l2norm),
                               int(accumulate_into is not None), out_scale, _lib.ptr(Yact),
                               float(act_scale or 0.0), _lib.stream()), "wv_op_dw_pw")
    return Y if act_scale is None else (Y, Yact)


def stft_logmag(wav, n_fft, hop, mean=0.0, std=1.0, basis=None, out=None) -> torch.Tensor:
    lib = _lib.load()
    wav = _lib.dev(wav, _ON_GPU)
    B, T = wav.shape[0], wav.shape[-1]
    Tf = -(-T // hop)
    P = _out(out, (B, n_fft // 2 + 1, Tf), torch.float32, wav.device)
    basis = _w(basis)
    _lib.check(lib.wv_op_stft_logmag(wav.data_ptr(), _hp(basis), P.data_ptr(), B, T, n_fft, hop, mean,
                                     std, _lib.stream()), "wv_op_stft_logmag")
    return P


def spec_block(wav, w_pw, x, n_fft, hop, mean=0.0, std=1.0, out_scale=1.0, act_scale: Optional[float] = None, want_raw: bool = True,
               basis=None, out=None, out_act=None):
    """Whole SpecBlock in one launch: y = x + out_scale * (W @ logmag(STFT(wav))) -> Y, (Y, Yact) or Yact alone."""
    lib = _lib.load()
    wav, x = _lib.dev(wav, _ON_GPU), _lib.dev(x, _ON_GPU)
    B, T = wav.shape[0], wav.shape[-1]
    M = x.shape[1]
    w_pw = _w(w_pw).reshape(M, n_fft // 2 + 1)
    Y = _out(out, x.shape, torch.float32, x.device) if want_raw else None
    Yact = _out(out_act, x.shape, torch.float32, x.device, "out_act") if act_scale is not None else None
    _lib.check(lib.wv_op_spec_block(wav.data_ptr(), _hp(_w(basis)), _hp(w_pw), x.data_ptr(), _lib.ptr(Y), _lib.ptr(Yact), B, T, n_fft, hop, M,
                                    mean, std, out_scale, float(act_scale or 0.0), _lib.stream()), "wv_op_spec_block")
    if Y is None:
        return Yact
    return Y if act_scale is None else (Y, Yact)


def conv_pre(x, w, bias, in_scale, out=None) -> torch.Tensor:
    lib = _lib.load()
    x = _lib.dev(x, _ON_GPU)
    B, T = x.shape[0], x.shape[-1]
    w, bias = _w(w), _w(bias)
    Cc, ks = w.shape[0], w.shape[-1]
    Y = _out(out, (B, Cc, T), torch.float32, x.device)
    _lib.check(lib.wv_op_conv_pre(x.data_ptr(), _hp(w), _hp(bias), Y.data_ptr(), B, Cc, T, ks, in_scale,
                                  _lib.stream()), "wv_op_conv_pre")
    return Y


def tail(H, w, bias, x=None, T=None, pre_scale=1.0, out_scale=1.0, out=None) -> torch.Tensor:
    lib = _lib.load()
    H = _lib.dev(H, _ON_GPU)
    B, Cc, Tin = H.shape
    T = Tin if T is None else T
    w, bias = _w(w), _w(bias)
    ks = w.shape[-1]
    x = None if x is None else _lib.dev(x, _ON_GPU)
    out = _out(out, (B, 1, T), torch.float32, H.device)
    _lib.check(lib.wv_op_tail(H.data_ptr(), _hp(w), _hp(bias), _lib.ptr(x), out.data_ptr(), B, Cc, Tin, T, ks,
                              pre_scale, out_scale, _lib.stream()), "wv_op_tail")
    return out


def head(Z, w_rev, b_rev, w_last, b_last, T, want_logits=True, want_mean=True, out=None, out_mean=None):
    """-> (logits [B, nb, T] or None, mean probabilities [B, nb] or None); out / out_mean: caller-owned outputs."""
    lib = _lib.load()
    Z = _lib.dev(Z, _ON_GPU)
    B, D, Fr = Z.shape
    w_rev, b_rev, w_last, b_last = _w(w_rev), _w(b_rev), _w(w_last), _w(b_last)
    O, hop = w_rev.shape[1], w_rev.shape[2]
    nb = w_last.shape[0]
    w_last = w_last.reshape(nb, O)
    logits = _out(out, (B, nb, T), torch.float32, Z.device) if want_logits else None
    mean = _out(out_mean, (B, nb), torch.float32, Z.device, "out_mean") if want_mean else None
    _lib.check(lib.wv_op_head(Z.data_ptr(), _hp(w_rev), _hp(b_rev), _hp(w_last), _hp(b_last),
                              _lib.ptr(logits), _lib.ptr(mean), B, D, O, nb, hop, Fr, T, _lib.stream()), "wv_op_head")
    return logits, mean


def _gate(gate, B, T, device):
    if gate is None:
        return None
    gate = _lib.dev(gate, _ON_GPU)
    if gate.numel() != B * T:
        raise ValueError(f"gate must hold [B, T] = [{B}, {T}] values, got {tuple(gate.shape)}")
    return gate


def head_frames(Z, w_rev, b_rev, w_last, b_last, T, gate=None, gate_thr=0.0, out=None) -> torch.Tensor:
    """The head's gated per-frame form (head_frames_kernel): -> fsum [B, nb + 1, Fr]; row bit = per frame the sum of sigmoid(logit)
    over the samples with gate > gate_thr (all samples without a gate), row nb = their number."""
    lib = _lib.load()
    Z = _lib.dev(Z, _ON_GPU)
    B, D, Fr = Z.shape
    w_rev, b_rev, w_last, b_last = _w(w_rev), _w(b_rev), _w(w_last), _w(b_last)
    O, hop = w_rev.shape[1], w_rev.shape[2]
    nb = w_last.shape[0]
    w_last = w_last.reshape(nb, O)
    gate = _gate(gate, B, int(T), Z.device)
    fsum = _out(out, (B, nb + 1, Fr), torch.float32, Z.device)
    _lib.check(lib.wv_op_head_frames(Z.data_ptr(), _hp(w_rev), _hp(b_rev), _hp(w_last), _hp(b_last), _lib.ptr(gate), float(gate_thr),
                                     fsum.data_ptr(), B, D, O, nb, hop, Fr, int(T), _lib.stream()), "wv_op_head_frames")
    return fsum


def frames_reduce(fsum, segments, eps: float = 1e-8):
    """wv_frames_reduce: fsum [B, nb + 1, Fr], segments [n, 3] ints {clip, f_lo, f_hi} -> (prob [n, nb] float32, count [n] float64)."""
    lib = _lib.load()
    fsum = _lib.dev(fsum, _ON_GPU)
    B, nb1, Fr = fsum.shape
    seg = torch.as_tensor(segments, dtype=torch.int32).reshape(-1, 3).contiguous().to(fsum.device)
    n = seg.shape[0]
    prob = torch.empty((n, nb1 - 1), dtype=torch.float32, device=fsum.device)
    count = torch.empty(n, dtype=torch.float64, device=fsum.device)
    if n:
        _lib.check(lib.wv_frames_reduce(fsum.data_ptr(), B, nb1 - 1, Fr, seg.data_ptr(), n, float(eps), prob.data_ptr(), count.data_ptr(),
                                        _lib.stream()), "wv_frames_reduce")
    return prob, count


def segment_track_bytes(S: int, nb: int, min_gap_frames: int, capacity: int):
    """wv_segment_track_bytes -> (state bytes, event bytes) of S trackers."""
    import ctypes as C
    sb, eb = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.load().wv_segment_track_bytes(int(S), int(nb), int(min_gap_frames), int(capacity), C.byref(sb), C.byref(eb)),
               "wv_segment_track_bytes")
    return sb.value, eb.value


def segment_track(fsum, f_lo: int, f_hi: int, frame0: int, hop: int, last_valid: int, final: bool, min_on: float, min_gap_frames: int,
                  min_len_frames: int, state, events, capacity: int, eps: float = 1e-8) -> None:
    """wv_segment_track: one tick of S streaming segment trackers on fsum [S, nb + 1, Fr] (Fr may be 0 for a final tick without frames);
    state / events are uint8 device tensors of segment_track_bytes, all zeros before the first tick, updated in place."""
    lib = _lib.load()
    fsum = _lib.dev(fsum, _ON_GPU)
    S, nb1, Fr = fsum.shape
    if not (state.is_cuda and events.is_cuda and state.dtype == torch.uint8 and events.dtype == torch.uint8 and state.is_contiguous()
            and events.is_contiguous()):
        raise ValueError("state and events must be contiguous uint8 tensors on the GPU")
    _lib.check(lib.wv_segment_track(fsum.data_ptr() if Fr else None, S, nb1 - 1, max(Fr, 1), int(f_lo), int(f_hi), int(frame0), int(hop),
                                    int(last_valid), int(bool(final)), float(min_on), int(min_gap_frames), int(min_len_frames), float(eps),
                                    state.data_ptr(), state.numel(), events.data_ptr(), events.numel(), int(capacity), _lib.stream()),
               "wv_segment_track")


def bank_segment_track(fsum, desc, P: int, capacity: int, nb: int, hop: int, min_on: float, min_gap_frames: int, min_len_frames: int,
                       state, events, ring: int, eps: float = 1e-8) -> None:
    """wv_bank_segment_track: one tick of a segment bank.  fsum: the tick's arena of frame sums (a float32 device tensor, or None where no row
    has frames); desc: int64 device tensor, its first P rows of 8 are served; state / events: uint8 device tensors of
    segment_track_bytes(capacity, nb, min_gap_frames, ring), a fresh slot all zeros, updated in place."""
    lib = _lib.load()
    if fsum is not None and not (fsum.is_cuda and fsum.dtype == torch.float32 and fsum.is_contiguous()):
        raise ValueError("fsum must be a contiguous float32 tensor on the GPU")
    if not (desc.is_cuda and desc.dtype == torch.int64 and desc.is_contiguous() and desc.numel() >= 8 * int(P)):
        raise ValueError("desc must be a contiguous int64 tensor on the GPU with 8 values per row")
    if not (state.is_cuda and events.is_cuda and state.dtype == torch.uint8 and events.dtype == torch.uint8 and state.is_contiguous()
            and events.is_contiguous()):
        raise ValueError("state and events must be contiguous uint8 tensors on the GPU")
    n_fsum = 0 if fsum is None else fsum.numel()
    _lib.check(lib.wv_bank_segment_track(fsum.data_ptr() if n_fsum else None, n_fsum, desc.data_ptr(), int(P), int(capacity), int(nb), int(hop),
                                         float(min_on), int(min_gap_frames), int(min_len_frames), float(eps), state.data_ptr(), state.numel(),
                                         events.data_ptr(), events.numel(), int(ring), _lib.stream()), "wv_bank_segment_track")


def segment_event_dtype(nb: int) -> np.dtype:
    """One event record of wv_segment_track's `events` buffer as a numpy structured dtype."""
    return np.dtype({"names": ["lo", "hi", "count", "prob"], "formats": ["<i8", "<i8", "<f8", ("<f4", (int(nb),))], "offsets": [0, 8, 16, 24],
                     "itemsize": 24 + (4 * int(nb) + 7) // 8 * 8})


def segment_events(events, S: int, nb: int, capacity: int):
    """The `events` buffer read back (one device-to-host copy) -> (n [S] int64 events so far, records [S, capacity] of segment_event_dtype)."""
    raw = events.cpu().numpy().reshape(S, -1)
    rec = segment_event_dtype(nb)
    n = raw[:, :8].copy().view("<i8").reshape(S)
    recs = raw[:, 8:8 + capacity * rec.itemsize].copy().view(rec).reshape(S, capacity)
    return n, recs


def segment_state(state, S: int, nb: int):
    """The `state` buffer read back -> (header [S, 4] int64 {open, lo, hi, frames seen}, sums [S, nb + 1] float64 of the open runs)."""
    raw = state.cpu().numpy().reshape(S, -1)
    hdr = raw[:, :32].copy().view("<i8").reshape(S, 4)
    acc = raw[:, 32:32 + 8 * (nb + 1)].copy().view("<f8").reshape(S, nb + 1)
    return hdr, acc


# ---- the same two trackers under a split rule (localize.SplitRule) ------------------------------------
def segment_split_bytes(S: int, nb: int, min_gap_frames: int, window_frames: int, capacity: int):
    """wv_segment_split_bytes -> (state bytes, event bytes) of S split trackers."""
    import ctypes as C
    sb, eb = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.load().wv_segment_split_bytes(int(S), int(nb), int(min_gap_frames), int(window_frames), int(capacity), C.byref(sb),
                                                  C.byref(eb)), "wv_segment_split_bytes")
    return sb.value, eb.value


def _byte_buffers(state, events) -> None:
    if not (state.is_cuda and events.is_cuda and state.dtype == torch.uint8 and events.dtype == torch.uint8 and state.is_contiguous()
            and events.is_contiguous()):
        raise ValueError("state and events must be contiguous uint8 tensors on the GPU")


def segment_track_split(fsum, f_lo: int, f_hi: int, frame0: int, hop: int, last_valid: int, final: bool, min_on: float, min_gap_frames: int,
                        min_len_frames: int, rule, state, events, capacity: int, eps: float = 1e-8) -> None:
    """wv_segment_track_split: segment_track's tick under `rule` (a localize.SplitRule); state / events of segment_split_bytes."""
    lib = _lib.load()
    fsum = _lib.dev(fsum, _ON_GPU)
    S, nb1, Fr = fsum.shape
    _byte_buffers(state, events)
    _lib.check(lib.wv_segment_track_split(fsum.data_ptr() if Fr else None, S, nb1 - 1, max(Fr, 1), int(f_lo), int(f_hi), int(frame0), int(hop),
                                          int(last_valid), int(bool(final)), float(min_on), int(min_gap_frames), int(min_len_frames),
                                          float(eps), int(rule.window_frames), float(rule.threshold), int(rule.min_bits), state.data_ptr(),
                                          state.numel(), events.data_ptr(), events.numel(), int(capacity), _lib.stream()),
               "wv_segment_track_split")


def bank_segment_track_split(fsum, desc, P: int, capacity: int, nb: int, hop: int, min_on: float, min_gap_frames: int, min_len_frames: int,
                             rule, state, events, ring: int, eps: float = 1e-8) -> None:
    """wv_bank_segment_track_split: bank_segment_track's tick under `rule`; state / events of segment_split_bytes(capacity, ..., ring)."""
    lib = _lib.load()
    if fsum is not None and not (fsum.is_cuda and fsum.dtype == torch.float32 and fsum.is_contiguous()):
        raise ValueError("fsum must be a contiguous float32 tensor on the GPU")
    if not (desc.is_cuda and desc.dtype == torch.int64 and desc.is_contiguous() and desc.numel() >= 8 * int(P)):
        raise ValueError("desc must be a contiguous int64 tensor on the GPU with 8 values per row")
    _byte_buffers(state, events)
    n_fsum = 0 if fsum is None else fsum.numel()
    _lib.check(lib.wv_bank_segment_track_split(fsum.data_ptr() if n_fsum else None, n_fsum, desc.data_ptr(), int(P), int(capacity), int(nb),
                                               int(hop), float(min_on), int(min_gap_frames), int(min_len_frames), float(eps),
                                               int(rule.window_frames), float(rule.threshold), int(rule.min_bits), state.data_ptr(),
                                               state.numel(), events.data_ptr(), events.numel(), int(ring), _lib.stream()),
               "wv_bank_segment_track_split")


def split_event_dtype(nb: int) -> np.dtype:
    """One event record of the split trackers' `events` buffer; flags bit 0: the start is an id change, bit 1: the end is one."""
    return np.dtype({"names": ["lo", "hi", "count", "flags", "prob"], "formats": ["<i8", "<i8", "<f8", "<i8", ("<f4", (int(nb),))],
                     "offsets": [0, 8, 16, 24, 32], "itemsize": 32 + (4 * int(nb) + 7) // 8 * 8})


def split_events(events, S: int, nb: int, capacity: int):
    """segment_events for the split trackers -> (n [S] int64 events so far, records [S, capacity] of split_event_dtype)."""
    raw = events.cpu().numpy().reshape(S, -1)
    rec = split_event_dtype(nb)
    n = raw[:, :8].copy().view("<i8").reshape(S)
    recs = raw[:, 8:8 + capacity * rec.itemsize].copy().view(rec).reshape(S, capacity)
    return n, recs


def split_state(state, S: int, nb: int, min_gap_frames: int, window_frames: int):
    """The split trackers' `state` read back -> (header [S, 7] int64 {open, lo, hi, frames seen, plo, pending, cg}, cS [S] float64, sums
    [S, nb + 1] float64 of the current pieces over [plo, sb), ring [S, 2 W + G, nb + 1] float32)."""
    raw = state.cpu().numpy().reshape(S, -1)
    RC, a = 2 * int(window_frames) + int(min_gap_frames), 64 + 8 * (nb + 1)
    hdr = raw[:, :56].copy().view("<i8").reshape(S, 7)
    cS = raw[:, 56:64].copy().view("<f8").reshape(S)
    acc = raw[:, 64:a].copy().view("<f8").reshape(S, nb + 1)
    ring = raw[:, a:a + 4 * RC * (nb + 1)].copy().view("<f4").reshape(S, RC, nb + 1)
    return hdr, cS, acc, ring


# ---- the f16 mode's units (csrc/wv_h16.hip).  A "c8" tensor is torch.float16 [B, roundup(C,16)/8, T, 8] --------------------------
def _c8(t: torch.Tensor) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.float16 and t.dim() == 4 and t.shape[-1] == 8 and t.is_contiguous()):
        raise RuntimeError("expected a contiguous CUDA float16 tensor [B, C/8, T, 8]")
    return t


def h16_from_f32(X, scale: float = 1.0, elu: bool = False, out=None) -> torch.Tensor:
    lib = _lib.load()
    X = _lib.dev(X, _ON_GPU)
    B, Cc, T = X.shape
    Y = _out(out, (B, (Cc + 15) // 16 * 2, T, 8), torch.float16, X.device)
    _lib.check(lib.wv_h16_from_f32(X.data_ptr(), Y.data_ptr(), B, Cc, T, float(scale), int(elu), _lib.stream()), "wv_h16_from_f32")
    return Y


def h16_to_f32(X16, channels: int, out=None) -> torch.Tensor:
    lib = _lib.load()
    X16 = _c8(X16)
    B, G, T, _ = X16.shape
    if (channels + 15) // 16 * 2 != G:
        raise ValueError("channel count does not match the tensor's groups")
    Y = _out(out, (B, channels, T), torch.float32, X16.device)
    _lib.check(lib.wv_h16_to_f32(X16.data_ptr(), Y.data_ptr(), B, channels, T, _lib.stream()), "wv_h16_to_f32")
    return Y


def h16_conv_pre(x, w, bias, in_scale: float = 1.0, out=None) -> torch.Tensor:
    lib = _lib.load()
    x = _lib.dev(x, _ON_GPU)
    B, _, T = x.shape
    w, bias = _w(w), _w(bias)
    Cc, ks = w.shape[0], w.shape[-1]
    Y = _out(out, (B, Cc // 8, T, 8), torch.float16, x.device)
    _lib.check(lib.wv_h16_conv_pre(x.data_ptr(), _hp(w.reshape(Cc, ks)), _hp(bias), Y.data_ptr(), B, Cc, T, ks, float(in_scale), _lib.stream()),
               "wv_h16_conv_pre")
    return Y


def h16_resblock(X16, w_pw1, w_dw1, b1, w_pw2, w_dw2, b2, pre_scale=1.0, out_scale=1.0, act_scale: Optional[float] = None,
                 want_raw: bool = True, out=None, out_act=None):
    lib = _lib.load()
    X16 = _c8(X16)
    B, G, T, _ = X16.shape
    Cc = 8 * G
    ws = [_w(w_pw1).reshape(Cc, Cc), _w(w_dw1).reshape(Cc, -1), _w(b1), _w(w_pw2).reshape(Cc, Cc), _w(w_dw2).reshape(Cc, -1), _w(b2)]
    Y = _out(out, X16.shape, torch.float16, X16.device) if want_raw else None
    Yact = _out(out_act, X16.shape, torch.float16, X16.device, "out_act") if act_scale is not None else None
    _lib.check(lib.wv_h16_resblock(X16.data_ptr(), float(pre_scale), *[_hp(w) for w in ws], _lib.ptr(Y), _lib.ptr(Yact), B, Cc, T, float(out_scale),
                                   float(act_scale or 0.0), _lib.stream()), "wv_h16_resblock")
    if Y is None:
        return Yact
    return Y if act_scale is None else (Y, Yact)


def h16_conv(X16, w_pw, w_dw=None, bias=None, resid16=None, K: Optional[int] = None, ks=1, stride=1, pad=0, out_scale=1.0,
             act_scale: Optional[float] = None, want_raw: bool = True, want_f32: bool = False, out=None, out_act=None, out_f32=None):
    """y = out_scale * (bias + conv(x)) + resid.  -> dict with the requested outputs: "raw" (c8 f16), "act" (c8 f16), "f32" ([B,M,Tout]);
    out / out_act / out_f32: caller-owned buffers for them."""
    lib = _lib.load()
    X16 = _c8(X16)
    B, G, Tin, _ = X16.shape
    w_pw, w_dw, bias = _w(w_pw), _w(w_dw), _w(bias)
    M = w_pw.shape[0]
    K = int(K if K is not None else w_pw.reshape(M, -1).shape[1])
    if (K + 15) // 16 * 2 != G:
        raise ValueError("weight columns do not match the tensor's channel groups")
    w_pw = w_pw.reshape(M, K)
    Tout = (Tin + stride - 1) // stride
    Gm = (M + 15) // 16 * 2
    res = {}
    if want_raw:
        res["raw"] = _out(out, (B, Gm, Tout, 8), torch.float16, X16.device)
    if act_scale is not None:
        res["act"] = _out(out_act, (B, Gm, Tout, 8), torch.float16, X16.device, "out_act")
    if want_f32:
        res["f32"] = _out(out_f32, (B, M, Tout), torch.float32, X16.device, "out_f32")
    if resid16 is not None:
        _c8(resid16)
    _lib.check(lib.wv_h16_conv(X16.data_ptr(), _hp(w_pw), _hp(None if w_dw is None else w_dw.reshape(M, ks)), _hp(bias), _lib.ptr(resid16),
                               _lib.ptr(res.get("raw")), _lib.ptr(res.get("act")), _lib.ptr(res.get("f32")), B, K, M, Tin, ks, stride, pad, float(out_scale),
                               float(act_scale or 0.0), _lib.stream()), "wv_h16_conv")
    return res


def h16_spec_block(wav, w_pw, x16, n_fft, hop, mean=0.0, std=1.0, out_scale=1.0, act_scale: Optional[float] = None, want_raw: bool = True, basis=None,
                   out=None, out_act=None):
    """Whole SpecBlock on the f16 pipe: y = x + out_scale * (W @ logmag(STFT(wav))) -> Y16, (Y16, Yact16) or Yact16 alone (c8 f16)."""
    lib = _lib.load()
    wav, x16 = _lib.dev(wav, _ON_GPU), _c8(x16)
    B, T = wav.shape[0], wav.shape[-1]
    M = 8 * x16.shape[1]
    w_pw = _w(w_pw).reshape(M, n_fft // 2 + 1)
    Y = _out(out, x16.shape, torch.float16, x16.device) if want_raw else None
    Yact = _out(out_act, x16.shape, torch.float16, x16.device, "out_act") if act_scale is not None else None
    _lib.check(lib.wv_h16_spec_block(wav.data_ptr(), _hp(_w(basis)), _hp(w_pw), x16.data_ptr(), _lib.ptr(Y), _lib.ptr(Yact), B, T, n_fft, hop, M,
                                     mean, std, out_scale, float(act_scale or 0.0), _lib.stream()), "wv_h16_spec_block")
    if Y is None:
        return Yact
    return Y if act_scale is None else (Y, Yact)


def h16_upsample(X16, w_ct, w_pw, bias, ratio: int, act_scale: Optional[float] = None, want_raw: bool = True, out=None, out_act=None):
    """The decoder's upsample unit (ELU -> depth-wise ConvTranspose1d(2r, r), trimmed -> 1x1 + bias; seanet.py:1147-1170) as one conv on
    the f16 pipe.  X16 = the PRE-ACTIVATED input, c8 f16 [B, K/8, Tin, 8] -> c8 f16 [B, M/8, Tin * r, 8]."""
    lib = _lib.load()
    X16 = _c8(X16)
    B, G, Tin, _ = X16.shape
    K = 8 * G
    w_pw, w_ct, bias = _w(w_pw), _w(w_ct), _w(bias)
    M = w_pw.shape[0]
    w_pw, w_ct = w_pw.reshape(M, K), w_ct.reshape(K, 2 * ratio)
    Y = _out(out, (B, M // 8, Tin * ratio, 8), torch.float16, X16.device) if want_raw else None
    Yact = _out(out_act, (B, M // 8, Tin * ratio, 8), torch.float16, X16.device, "out_act") if act_scale is not None else None
    _lib.check(lib.wv_h16_upsample(X16.data_ptr(), _hp(w_ct), _hp(w_pw), _hp(bias), _lib.ptr(Y), _lib.ptr(Yact), B, K, M, Tin, int(ratio),
                                   float(act_scale or 0.0), _lib.stream()), "wv_h16_upsample")
    if Y is None:
        return Yact
    return Y if act_scale is None else (Y, Yact)


def h16_tail(A16, w, bias, T: int, out_scale: float, x=None, out=None) -> torch.Tensor:
    """Decoder tail on the pre-activated c8 stream: tanh(out_scale * (b + Conv1d(C -> 1, ks)(a))) (+ x) -> [B, 1, T] f32."""
    lib = _lib.load()
    A16 = _c8(A16)
    B, G, Tin, _ = A16.shape
    w, bias = _w(w), _w(bias)
    Cc, ks = w.shape[-2], w.shape[-1]
    if (Cc + 15) // 16 * 2 != G:
        raise ValueError("weight channels do not match the tensor's channel groups")
    xd = _lib.dev(x, _ON_GPU) if x is not None else None
    out = _out(out, (B, 1, T), torch.float32, A16.device)
    _lib.check(lib.wv_h16_tail(A16.data_ptr(), _hp(w.reshape(Cc, ks)), _hp(bias), _lib.ptr(xd), out.data_ptr(), B, Cc, Tin, T, ks, float(out_scale), _lib.stream()),
               "wv_h16_tail")
    return out


def h16_l2norm(lat, out=None) -> torch.Tensor:
    lib = _lib.load()
    lat = _lib.dev(lat, _ON_GPU)
    B, D, Fr = lat.shape
    Y = _out(out, (B, (D + 15) // 16 * 2, Fr, 8), torch.float16, lat.device)
    _lib.check(lib.wv_h16_l2norm(lat.data_ptr(), Y.data_ptr(), B, D, Fr, _lib.stream()), "wv_h16_l2norm")
    return Y


def h16_head(lat, wc, bc, T: int, keep_lo=None, keep_hi=None, out=None) -> torch.Tensor:
    """The f16 mode's mean-probability head (head16_kernel): lat [B, D, Fr] f32 latent before its L2Norm, wc [D, nb * hop] the composed
    head weight (column bit * hop + j), bc [nb].  -> mean over t < T of sigmoid(logits) [B, nb]; with keep_lo / keep_hi ([B] ints) the
    windowed mode instead: the SUM over t in [keep_lo[b], keep_hi[b]) [B, nb]."""
    lib = _lib.load()
    lat = _lib.dev(lat, _ON_GPU)
    B, D, Fr = lat.shape
    wc, bc = _w(wc), _w(bc)
    nb = bc.shape[0]
    hop = wc.shape[-1] // nb
    if wc.shape != (D, nb * hop):
        raise ValueError(f"wc must be [D, nb * hop] = [{D}, {nb} * hop], got {wc.shape}")
    if (keep_lo is None) != (keep_hi is None):
        raise ValueError("keep_lo and keep_hi go together")
    out = _out(out, (B, nb), torch.float32, lat.device)
    lo = hi = None
    if keep_lo is not None:
        lo = torch.as_tensor(keep_lo, dtype=torch.int32).reshape(-1).to(lat.device)
        hi = torch.as_tensor(keep_hi, dtype=torch.int32).reshape(-1).to(lat.device)
        if lo.numel() != B or hi.numel() != B:
            raise ValueError("keep_lo / keep_hi need one entry per clip")
    _lib.check(lib.wv_h16_head(lat.data_ptr(), _hp(wc), _hp(bc), None if lo is not None else out.data_ptr(), B, D, nb, hop, Fr, int(T),
                               _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(out) if lo is not None else None, _lib.stream()), "wv_h16_head")
    return out


def h16_head_frames(lat, wc, bc, T: int, gate=None, gate_thr=0.0, out=None) -> torch.Tensor:
    """h16_head in the gated per-frame form (head16_frames_kernel): -> fsum [B, nb + 1, Fr], as ops.head_frames."""
    lib = _lib.load()
    lat = _lib.dev(lat, _ON_GPU)
    B, D, Fr = lat.shape
    wc, bc = _w(wc), _w(bc)
    nb = bc.shape[0]
    hop = wc.shape[-1] // nb
    if wc.shape != (D, nb * hop):
        raise ValueError(f"wc must be [D, nb * hop] = [{D}, {nb} * hop], got {wc.shape}")
    gate = _gate(gate, B, int(T), lat.device)
    fsum = _out(out, (B, nb + 1, Fr), torch.float32, lat.device)
    _lib.check(lib.wv_h16_head_frames(lat.data_ptr(), _hp(wc), _hp(bc), _lib.ptr(gate), float(gate_thr), fsum.data_ptr(), B, D, nb, hop, Fr,
                                      int(T), _lib.stream()), "wv_h16_head_frames")
    return fsum


def h16_conv_film(X16, w_pw, w_dw, bias, film, ks, stride, pad, act_scale: Optional[float] = None, want_raw: bool = True, out=None,
                  out_act=None):
    """wv_h16_conv with FiLM behind the conv: film [B, bands, 2] (gamma, beta) on the device."""
    lib = _lib.load()
    X16, film = _c8(X16), _lib.dev(film, _ON_GPU)
    B, G, Tin, _ = X16.shape
    w_pw, w_dw, bias = _w(w_pw), _w(w_dw), _w(bias)
    M = w_pw.shape[0]
    K = w_pw.reshape(M, -1).shape[1]
    Tout = (Tin + stride - 1) // stride
    Gm = (M + 15) // 16 * 2
    Y = _out(out, (B, Gm, Tout, 8), torch.float16, X16.device) if want_raw else None
    Yact = _out(out_act, (B, Gm, Tout, 8), torch.float16, X16.device, "out_act") if act_scale is not None else None
    _lib.check(lib.wv_h16_conv_film(X16.data_ptr(), _hp(w_pw.reshape(M, K)), _hp(w_dw.reshape(M, ks) if w_dw is not None else None), _hp(bias), film.data_ptr(),
                                    int(film.shape[1]), _lib.ptr(Y), _lib.ptr(Yact), B, K, M, Tin, ks, stride, pad, float(act_scale or 0.0), _lib.stream()),
               "wv_h16_conv_film")
    if Y is None:
        return Yact
    return Y if act_scale is None else (Y, Yact)
