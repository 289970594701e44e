"""The two ends of the native-rate embed route (csrc/wv_native.hip).

A file keeps its own sample rate and channel count: the model runs at 16 kHz on a down-mixed, down-sampled copy (`downmix_resample`),
and its residual alone is brought back to the file's rate and added to every original channel (`upsample_add`).  Both directions use
torchaudio's polyphase table as `effects.resample_kernels` restates it (width 6, rolloff 0.99: the loader's filter, see `load_audio`),
handed to the kernels transposed; a 16 kHz file takes the same two kernels with the one-tap identity table.  There is no CPU fallback."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .effects import resample_kernels, resampled_length

_ON_GPU = "the native-rate route runs on the GPU (no CPU fallback)"

MODEL_RATE = 16000
MAX_TABLE_FLOATS = 4 * 1024 * 1024                  # 16 MB of taps: nw * L of a rate whose gcd with 16000 is not a few hertz


def table_geometry(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> Tuple[int, int, int, int]:
    """(orig, nw, L, width) of the table `resample_kernels(orig_freq, new_freq)` would build, from its published formula, without
    building it; (1, 1, 1, 0) for equal rates (the identity table)."""
    if int(orig_freq) <= 0 or int(new_freq) <= 0:
        raise ValueError(f"sample rates must be positive, got {orig_freq} -> {new_freq}")
    if int(orig_freq) == int(new_freq):
        return 1, 1, 1, 0
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, nw = int(orig_freq) // g, int(new_freq) // g
    width = math.ceil(lowpass_filter_width * orig / (min(orig, nw) * rolloff))
    return orig, nw, 2 * width + orig, width


def check_rate(sample_rate: int) -> None:
    """ValueError for a rate either of whose tables (to and from 16 kHz) would pass 16 MB."""
    for of, nf in ((sample_rate, MODEL_RATE), (MODEL_RATE, sample_rate)):
        _, nw, L, _ = table_geometry(of, nf)
        if nw * L > MAX_TABLE_FLOATS:
            raise ValueError(f"sample rate {sample_rate} Hz is not served: its {of} -> {nf} resampling table would hold {nw} x {L} taps "
                             f"({nw * L * 4 / 2 ** 20:.0f} MB, the limit is {MAX_TABLE_FLOATS * 4 // 2 ** 20} MB); resample the file to a "
                             f"standard rate first")


def transposed_table(orig_freq: int, new_freq: int) -> Tuple[np.ndarray, int, int, int, int]:
    """-> (kernels_t [L, nw] float32 contiguous, orig, nw, L, width): `resample_kernels(...)`'s table transposed, or [[1]] for equal rates."""
    orig, nw, L, width = table_geometry(orig_freq, new_freq)
    if int(orig_freq) == int(new_freq):
        return np.ones((1, 1), np.float32), orig, nw, L, width
    k, w, o, n = resample_kernels(orig_freq, new_freq)
    assert (o, n, k.shape[1], w) == (orig, nw, L, width)
    return np.ascontiguousarray(k.T), orig, nw, L, width


_tables: Dict[tuple, tuple] = {}


def tables(sample_rate: int, device) -> Tuple[tuple, tuple]:
    """-> (front, back) for one file rate on one device, cached: each (kernels_t device tensor, orig, nw, L, width); front is
    sample_rate -> 16000, back 16000 -> sample_rate."""
    sample_rate = int(sample_rate)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(_ON_GPU)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (sample_rate, device.index)
    if key not in _tables:
        check_rate(sample_rate)
        pair = []
        for of, nf in ((sample_rate, MODEL_RATE), (MODEL_RATE, sample_rate)):
            kt, orig, nw, L, width = transposed_table(of, nf)
            pair.append((torch.from_numpy(kt).to(device), orig, nw, L, width))
        _tables[key] = tuple(pair)
    return _tables[key]


def upsampled_length(T16: int, sample_rate: int) -> int:
    """ceil(nw * T16 / orig): what resampling T16 model-rate samples to `sample_rate` gives."""
    return resampled_length(T16, MODEL_RATE, sample_rate)


def _planar(audio: torch.Tensor) -> torch.Tensor:
    if audio.dim() == 2:
        audio = audio.unsqueeze(0)
    if audio.dim() != 3 or audio.shape[1] < 1 or audio.shape[2] < 1:
        raise ValueError(f"expected audio of shape [B,C,Tn] or [C,Tn], got {tuple(audio.shape)}")
    return _lib.dev(audio, _ON_GPU)


def downmix_resample(audio: torch.Tensor, sample_rate: int) -> torch.Tensor:
    """audio [B,C,Tn] (or [C,Tn]) at `sample_rate` -> the model's input [B,1,T16]: the channel mean resampled to 16 kHz in one kernel,
    T16 = effects.resampled_length(Tn, sample_rate, 16000)."""
    x = _planar(audio)
    B, C, Tn = x.shape
    with torch.cuda.device(x.device):
        (kt, orig, nw, L, width), _ = tables(sample_rate, x.device)
        T16 = resampled_length(Tn, sample_rate, MODEL_RATE)
        y = torch.empty((B, 1, T16), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().wv_native_downmix_resample(x.data_ptr(), kt.data_ptr(), y.data_ptr(), B, C, Tn, orig, nw, L, width, T16,
                                                         _lib.stream()), "wv_native_downmix_resample")
    return y


def upsample_add(audio: torch.Tensor, delta: torch.Tensor, sample_rate: int, gain: float = 1.0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """audio [B,C,Tn] at `sample_rate`, delta [B,1,T16] (or [B,T16]) at 16 kHz -> audio + gain * up(delta) on every channel, [B,C,Tn], in
    one kernel.  up(delta) is delta resampled to `sample_rate`, ceil(nw * T16 / orig) >= Tn samples cut to Tn.  out: where to write
    (float32, contiguous, audio's shape); `audio` itself works in place."""
    x = _planar(audio)
    B, C, Tn = x.shape
    d = _lib.dev(delta, _ON_GPU)
    if d.dim() == 3 and d.shape[1] == 1:
        d = d.squeeze(1)
    if d.dim() != 2 or d.shape[0] != B or d.shape[1] < 1:
        raise ValueError(f"expected delta of shape [{B},1,T16] or [{B},T16], got {tuple(delta.shape)}")
    T16 = int(d.shape[1])
    if upsampled_length(T16, sample_rate) < Tn:
        raise ValueError(f"delta of {T16} samples at 16 kHz gives {upsampled_length(T16, sample_rate)} samples at {sample_rate} Hz, fewer than the "
                         f"audio's {Tn}")
    if out is None:
        out = torch.empty_like(x)
    elif not (out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, C, Tn)):
        raise ValueError(f"out must be a contiguous float32 tensor of shape {(B, C, Tn)} on {x.device}")
    with torch.cuda.device(x.device):
        _, (kt, orig, nw, L, width) = tables(sample_rate, x.device)
        _lib.check(_lib.load().wv_native_upsample_add(x.data_ptr(), d.data_ptr(), kt.data_ptr(), out.data_ptr(), B, C, T16, Tn, orig, nw, L, width,
                                                     float(gain), _lib.stream()), "wv_native_upsample_add")
    return out


def floor_frames(Tn: int, sample_rate: int, hop: int = 320) -> int:
    """The frames of the per-channel floor in Tn native samples: frame(Tn - 1) + 1, frame(m) = (m * orig) // (nw * hop)."""
    orig, nw, _, _ = table_geometry(MODEL_RATE, sample_rate)
    return ((int(Tn) - 1) * orig) // (nw * int(hop)) + 1


def upsample_add_floor(audio: torch.Tensor, delta: torch.Tensor, sample_rate: int, min_snr_db: float, strength=1.0, hop: int = 320,
                       add: bool = True, return_gains: bool = False, out: Optional[torch.Tensor] = None):
    """upsample_add under the per-channel SNR floor (channel_floor.py): audio [B,C,Tn] at `sample_rate`, delta
    [B,1,T16] (or [B,T16]) at 16 kHz -> audio + w * up(delta), [B,C,Tn], w chosen per channel and native frame so that in no frame of any
    channel the watermark is louder than min_snr_db below that channel, and a silent channel comes back bit for bit.  strength: the cap of w,
    one number or one per row, finite and >= 0.  hop: the generator's hop_length (the frames are the 16 kHz floor's, seen from the native
    time line).  add=False: w * up(delta) alone.  return_gains: also the gains [B, C, F].  out: as in upsample_add; `audio` itself works."""
    from . import snr_floor
    rho = snr_floor.rho_of(min_snr_db)
    hop = int(hop)
    if hop < 1:
        raise ValueError(f"hop must be >= 1, got {hop}")
    rows = int(audio.shape[0]) if audio.dim() == 3 else 1
    s = np.broadcast_to(np.asarray(strength, np.float64), (rows,)) if np.ndim(strength) == 0 else np.asarray(strength, np.float64).reshape(-1)
    if s.shape[0] != rows or not (np.isfinite(s).all() and (s >= 0).all()):
        raise ValueError("strength must be finite and >= 0, one number or one per row")
    x = _planar(audio)
    B, C, Tn = x.shape
    d = _lib.dev(delta, _ON_GPU)
    if d.dim() == 3 and d.shape[1] == 1:
        d = d.squeeze(1)
    if d.dim() != 2 or d.shape[0] != B or d.shape[1] < 1:
        raise ValueError(f"expected delta of shape [{B},1,T16] or [{B},T16], got {tuple(delta.shape)}")
    T16 = int(d.shape[1])
    if upsampled_length(T16, sample_rate) < Tn:
        raise ValueError(f"delta of {T16} samples at 16 kHz gives {upsampled_length(T16, sample_rate)} samples at {sample_rate} Hz, fewer than the "
                         f"audio's {Tn}")
    if out is None:
        out = torch.empty_like(x)
    elif not (out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, C, Tn)):
        raise ValueError(f"out must be a contiguous float32 tensor of shape {(B, C, Tn)} on {x.device}")
    with torch.cuda.device(x.device):
        _, (kt, orig, nw, L, width) = tables(sample_rate, x.device)
        lib = _lib.load()
        need = ctypes.c_size_t(0)
        _lib.check(lib.wv_native_floor_up_add_bytes(B, C, T16, Tn, orig, nw, L, width, hop, ctypes.byref(need)), "wv_native_floor_up_add_bytes")
        ws = _lib.scratch(need.value, x.device)
        st = torch.from_numpy(s.astype(np.float32)).to(x.device)
        gains = torch.empty((B, C, floor_frames(Tn, sample_rate, hop)), dtype=torch.float32, device=x.device) if return_gains else None
        _lib.check(lib.wv_native_floor_up_add(x.data_ptr(), d.data_ptr(), kt.data_ptr(), out.data_ptr(), B, C, T16, Tn, orig, nw, L, width, hop, rho,
                                              st.data_ptr(), 1 if add else 0, _lib.ptr(gains), ws.data_ptr(), need.value, _lib.stream()),
                   "wv_native_floor_up_add")
    return (out, gains) if return_gains else out
