"""The reference's audio effects on the GPU: the sinc filters and the resampler (SURVEY.md section 8f-3 and the resample front-end of
8f-4, below) and its plain-arithmetic time-domain effects (second half of this file, csrc/wv_fx_time.hip).

Mirror of the four AudioEffects the reference implements with third-party arithmetic
(/root/reference/utils/effect_augmentation.py:1451-1501 resample, :1684-1870 high / low / band-pass) plus `identity` (:1364), with
the reference's own wrapper behaviour: cutoffs are clamped to [0, nyquist - 1e-5] and handed over as cutoff / NYQUIST, every method
returns (tensor, mask), low / high-pass return the input unchanged when the library would raise, band-pass raises ValueError.

PARITY UNPINNED: `julius` (0.2.7 in the reference's requirements) and `torchaudio` are not in this image and the reference holds no
output of theirs.  The filters are restated from the libraries' published algorithms --
  julius.lowpass.LowPassFilters: half_size = int(zeros / min_cutoff / 2), zeros = 8; filter = 2 c hann(2h+1) sinc(2 c pi t), t = -h..h,
      normalised to sum 1; replicate padding of h samples; cutoff in cycles per SAMPLE, must be <= 0.5; highpass = x - lowpass;
      bandpass = lowpass(high) - lowpass(low), both with the half_size of the lower cutoff;
  torchaudio.functional.resample (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): see `resample_kernels`
-- and checked here against an independent float64 restatement (oracle/wv_oracle_fx.py) only.  Note the reference's cutoff / nyquist
convention doubles the cutoff julius sees (3000 Hz at 16 kHz -> 0.375 cycles per sample = 6 kHz), and cutoffs above nyquist / 2 make the
library raise -- both are kept, not corrected.  The convolutions run in csrc/wv_fx.hip; there is no CPU fallback."""
from __future__ import annotations

import collections
import math
import random
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

_ON_GPU = "effects run on the GPU (no CPU fallback)"

DEFAULT_SAMPLE_RATE = 16000
EPSILON = 1e-5


# ---- taps, as the libraries publish them ----------------------------------------------------------------------------------------
def lowpass_taps(cutoffs, zeros: float = 8) -> Tuple[np.ndarray, int]:
    """julius.lowpass.LowPassFilters.__init__: one windowed-sinc filter per cutoff (cycles per sample), float32 arithmetic as torch's
    defaults give it.  -> (taps [n, 2h+1] float32, h)."""
    cutoffs = [float(c) for c in cutoffs]
    if min(cutoffs) < 0:
        raise ValueError("Minimum cutoff must be larger than zero.")
    if max(cutoffs) > 0.5:
        raise ValueError("A cutoff above 0.5 does not make sense.")
    half = int(zeros / min(c for c in cutoffs if c > 0) / 2)
    window = torch.hann_window(2 * half + 1, periodic=False)
    time = torch.arange(-half, half + 1)
    filters = []
    for c in cutoffs:
        if c == 0:
            f = torch.zeros_like(time).float()
        else:
            xx = 2 * c * math.pi * time
            sinc = torch.where(xx == 0, torch.tensor(1.0), torch.sin(xx) / xx)
            f = 2 * c * window * sinc
            f = f / f.sum()
        filters.append(f)
    return torch.stack(filters).numpy().astype(np.float32), half


def resample_kernels(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """torchaudio.functional.functional._get_sinc_resample_kernel (sinc_interp_hann): float64 index arithmetic, float32 kernels.
    -> (kernels [new, 2 width + orig] float32, width, orig, new) with orig / new divided by their gcd."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx
    t = np.clip(t * base, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0, 1.0, np.sin(t) / t)
    k = k * window * (base / orig)
    return k.astype(np.float32), width, orig, new


# ---- device convolutions -----------------------------------------------------------------------------------------------------------
def _fir(x: torch.Tensor, taps: np.ndarray, half: int) -> torch.Tensor:
    """x [..., T] -> [n_filters, ..., T]: julius' replicate-padded 'same' convolution."""
    lib = _lib.load()
    shape = list(x.shape)
    xr = _lib.dev(x, _ON_GPU).reshape(-1, shape[-1])
    nf, L = taps.shape
    td = torch.from_numpy(np.ascontiguousarray(taps)).to(xr.device)
    y = torch.empty(xr.shape[0], nf, shape[-1], device=xr.device)
    _lib.check(lib.wv_fx_fir_bank(xr.data_ptr(), td.data_ptr(), y.data_ptr(), xr.shape[0], shape[-1], nf, L, 1, half, half, 1, 0, _lib.stream()), "wv_fx_fir_bank")
    return y.permute(1, 0, 2).reshape([nf] + shape)


def lowpass(x: torch.Tensor, cutoff: float) -> torch.Tensor:
    """julius.lowpass_filter(x, cutoff)."""
    taps, half = lowpass_taps([cutoff])
    return _fir(x, taps, half)[0]


def highpass(x: torch.Tensor, cutoff: float) -> torch.Tensor:
    """julius.highpass_filter(x, cutoff) = x - lowpass(x)."""
    return _lib.dev(x, _ON_GPU) - lowpass(x, cutoff)


def bandpass(x: torch.Tensor, cutoff_low: float, cutoff_high: float) -> torch.Tensor:
    """julius.bandpass_filter: lowpass(high) - lowpass(low), one filter bank (the half width of the lower cutoff)."""
    if cutoff_low > cutoff_high:
        raise ValueError(f"Lower cutoff {cutoff_low} should be less than higher cutoff {cutoff_high}.")
    taps, half = lowpass_taps([cutoff_low, cutoff_high])
    lows = _fir(x, taps, half)
    return lows[1] - lows[0]


def resampled_length(T: int, orig_freq: int, new_freq: int) -> int:
    """Length of `resample_waveform`'s output: ceil(new * T / orig) with the two rates divided by their gcd."""
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(math.ceil((int(new_freq) // g) * T / (int(orig_freq) // g)))


def resample_waveform(x: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """torchaudio.transforms.Resample(orig_freq, new_freq)(x) on [..., T]."""
    if int(orig_freq) == int(new_freq):
        return _lib.dev(x, _ON_GPU)
    lib = _lib.load()
    k, width, orig, new = resample_kernels(orig_freq, new_freq)
    shape = list(x.shape)
    xr = _lib.dev(x, _ON_GPU).reshape(-1, shape[-1])
    T = shape[-1]
    t_out = int(math.ceil(new * T / orig))
    kd = torch.from_numpy(np.ascontiguousarray(k)).to(xr.device)
    y = torch.empty(xr.shape[0], t_out, device=xr.device)
    _lib.check(lib.wv_fx_resample(xr.data_ptr(), kd.data_ptr(), y.data_ptr(), xr.shape[0], T, orig, new, k.shape[1], width, t_out, _lib.stream()), "wv_fx_resample")
    return y.reshape(shape[:-1] + [t_out])


# ---- adjoints: the gradient of a loss through these effects -------------------------------------------------------------------------
# In the reference the four effects are plain differentiable torch ops (julius' FFT / direct convolutions, torchaudio's strided conv1d;
# effect_augmentation.py:1451-1501,1684-1870 -- not the straight-through Function classes of :462-500), so the generator's gradient
# crosses them through the TRANSPOSED filter.
def _fir_adjoint(dy: torch.Tensor, taps: np.ndarray, half: int) -> torch.Tensor:
    """Transpose of `_fir` for ONE filter: dy [..., T] -> dx [..., T] (time-reversed taps over the zero-padded gradient, then the
    transpose of the replicate padding)."""
    lib = _lib.load()
    shape = list(dy.shape)
    T = shape[-1]
    dr = _lib.dev(dy, _ON_GPU).reshape(-1, T)
    L = taps.shape[1]
    rev = torch.from_numpy(np.ascontiguousarray(taps[:1, ::-1])).to(dr.device)
    dxp = torch.empty(dr.shape[0], 1, T + L - 1, device=dr.device)               # gradient towards the replicate-padded signal
    _lib.check(lib.wv_fx_fir_bank(dr.data_ptr(), rev.data_ptr(), dxp.data_ptr(), dr.shape[0], T, 1, L, 1, L - 1, L - 1, 0, 0, _lib.stream()), "wv_fx_fir_bank")
    dx = torch.empty_like(dr)
    _lib.check(lib.wv_fx_fold_replicate(dxp.data_ptr(), dx.data_ptr(), dr.shape[0], T, half, half, _lib.stream()), "wv_fx_fold_replicate")
    return dx.reshape(shape)


def lowpass_adjoint(dy: torch.Tensor, cutoff: float) -> torch.Tensor:
    taps, half = lowpass_taps([cutoff])
    return _fir_adjoint(dy, taps, half)


def highpass_adjoint(dy: torch.Tensor, cutoff: float) -> torch.Tensor:
    return _lib.dev(dy, _ON_GPU) - lowpass_adjoint(dy, cutoff)


def bandpass_adjoint(dy: torch.Tensor, cutoff_low: float, cutoff_high: float) -> torch.Tensor:
    taps, half = lowpass_taps([cutoff_low, cutoff_high])
    return _fir_adjoint(dy, taps[1:2], half) - _fir_adjoint(dy, taps[0:1], half)


def resample_waveform_adjoint(dy: torch.Tensor, orig_freq: int, new_freq: int, t_in: int) -> torch.Tensor:
    """Transpose of `resample_waveform(x [..., t_in], orig_freq, new_freq)`: dy [..., t_out] -> dx [..., t_in]."""
    if int(orig_freq) == int(new_freq):
        return _lib.dev(dy, _ON_GPU)
    lib = _lib.load()
    k, width, orig, new = resample_kernels(orig_freq, new_freq)
    shape = list(dy.shape)
    dr = _lib.dev(dy, _ON_GPU).reshape(-1, shape[-1])
    kd = torch.from_numpy(np.ascontiguousarray(k)).to(dr.device)
    dx = torch.empty(dr.shape[0], t_in, device=dr.device)
    _lib.check(lib.wv_fx_resample_adjoint(dr.data_ptr(), kd.data_ptr(), dx.data_ptr(), dr.shape[0], t_in, orig, new, k.shape[1], width, shape[-1],
                                          _lib.stream()), "wv_fx_resample_adjoint")
    return dx.reshape(shape[:-1] + [t_in])


DIFFERENTIABLE = ("identity", "highpass_filter", "lowpass_filter", "bandpass_filter", "resample")


def apply_effect_backward(name: str, params: dict, d_out: torch.Tensor, sample_rate: int = DEFAULT_SAMPLE_RATE) -> torch.Tensor:
    """Gradient towards the input of `apply_effect(name, params, audio)` given the gradient towards its output (same length): the
    transposed operator for the effects the reference differentiates through (`DIFFERENTIABLE`); anything else is one of the
    reference's straight-through effects (effect_augmentation.py:462-500) and passes the gradient unchanged."""
    if name not in DIFFERENTIABLE or name == "identity":
        return d_out
    A = AudioEffects
    T = d_out.shape[-1]
    if name == "lowpass_filter" or name == "highpass_filter":
        c = A._cutoff(params.get("cutoff_freq", 3000 if name == "lowpass_filter" else 500), sample_rate)
        try:
            return (lowpass_adjoint if name == "lowpass_filter" else highpass_adjoint)(d_out, c)
        except ValueError:                                   # the forward passed the input through
            return d_out
    if name == "bandpass_filter":
        nyquist = sample_rate / 2.0
        lo = max(0.0, min(params.get("cutoff_freq_low", 300), nyquist - EPSILON)) / nyquist
        hi = max(0.0, min(params.get("cutoff_freq_high", 8000), nyquist - EPSILON)) / nyquist
        return bandpass_adjoint(d_out, lo, hi)
    new_sr = int(params["new_sample_rate"])                  # resample: down, up, then cropped / zero-padded back to T
    t_mid = resampled_length(T, sample_rate, new_sr)
    t_up = resampled_length(t_mid, new_sr, sample_rate)
    d_up = d_out[..., :t_up] if t_up <= T else torch.nn.functional.pad(d_out, (0, t_up - T))     # transpose of the crop / zero pad
    d_mid = resample_waveform_adjoint(d_up.contiguous(), new_sr, sample_rate, t_mid)
    return resample_waveform_adjoint(d_mid, sample_rate, new_sr, T)


# ---- the plain-arithmetic time-domain effects (csrc/wv_fx_time.hip) -------------------------------------------------------------------
# effect_augmentation.py:1081-1332 (the straight-through Functions), :1380-1448 speed, :1504-1681 echo / pink_noise, :1873-2132
# median_filter .. random_noise, :2338-2404 white_noise / shush.  PINNED to the reference (tests/golden/effects_time.npz, written by
# the reference's own apply_effect on the CPU) except `speed`, whose arithmetic is SoX's.  The random draws are made where the
# reference makes them -- torch's CPU generator, torch's device generator, numpy's and random's global generators -- so a seeded run
# reproduces; they are small pure functions here so that they can be checked without a GPU.
MIN_AUDIO_LENGTH = 2
MEDIAN_MAX_K = 255                      # WV_FX_MEDIAN_MAX_K
SMOOTH_MAX_W = 2048                     # WV_FX_SMOOTH_MAX_W
OP_SCALE, OP_ADD_NOISE, OP_QUANTIZE, OP_MUL = 0, 1, 2, 3


def echo_plan(T: int, sample_rate: int = DEFAULT_SAMPLE_RATE, volume_range=(0.1, 0.5), duration_range=(0.1, 0.5)) -> Tuple[int, float]:
    """echo's draws (effect_augmentation.py:1558-1567): duration then volume from torch's CPU generator, the duration capped at half the
    clip.  -> (n taps of the impulse response, volume)."""
    duration = torch.FloatTensor(1).uniform_(*duration_range).item()
    duration = min(duration, T / sample_rate * 0.5)
    volume = torch.FloatTensor(1).uniform_(*volume_range).item()
    return max(int(sample_rate * duration), MIN_AUDIO_LENGTH), volume


def smooth_window(window_size_range=(2, 10)) -> int:
    """smooth's draw (:1947)."""
    return int(torch.FloatTensor(1).uniform_(*window_size_range))


def suppression_indices(B: int, C: int, T: int, suppression_percentage: float) -> np.ndarray:
    """sample_suppression's draws (:2084-2091): one torch.randperm(T)[:num] per (b, c), in that loop order.  -> int32 [B * C, num]."""
    num = int(T * suppression_percentage)
    return np.stack([torch.randperm(T)[:num].numpy() for _ in range(B * C)]).astype(np.int32).reshape(B * C, num)


def pink_noise_host(size: int, depth: int = 16) -> np.ndarray:
    """pink_noise's generator (:1634-1663): the Voss-McCartney loop on numpy's global generator, normalised to a peak of 1, float32.
    The draws are data-dependent (the legacy randn caches and rejects), so the loop cannot be vectorised bit-exactly: it runs here as
    the reference runs it, one Python iteration per sample, and THAT is the cost of this effect (of the order of 0.1 s of host time
    per 16000-sample clip); the GPU only adds the result."""
    array = np.zeros(size)
    nums = np.zeros(depth)
    for i in range(size):
        nums[0] = np.random.randn()
        array[i] = nums.sum()
        nums[np.random.randint(0, depth)] = np.random.randn()
    max_val = np.max(np.abs(array)) if size else 0.0
    if max_val > 0:
        array = array / max_val
    return array.astype(np.float32)


def speed_ratio(speed: float) -> Tuple[int, int]:
    """speed s as the resampling ratio orig : new of SoX's `speed s` + `rate sr` chain (the clip is s times shorter): s itself as a
    fraction with a denominator of at most 100 (0.8 -> 4 : 5, T becomes ceil(5 T / 4))."""
    f = Fraction(float(speed)).limit_denominator(100)
    if f <= 0:
        raise ValueError(f"Speed must be positive, got {speed}")
    return f.numerator, f.denominator


def _rows(t: torch.Tensor) -> torch.Tensor:
    return _lib.dev(t, _ON_GPU).reshape(-1, t.shape[-1])


def pointwise(x: torch.Tensor, op: int, a: float, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wv_fx_pointwise: x * a, x + noise * a, rint(x * a) / a or x * noise (`noise` is the second operand of the two-tensor ops)."""
    xr = _rows(x)
    nr = _rows(noise) if noise is not None else None
    y = torch.empty_like(xr)
    _lib.check(_lib.load().wv_fx_pointwise(xr.data_ptr(), _lib.ptr(nr), y.data_ptr(), xr.shape[0], xr.shape[1], op, float(a),
                                           _lib.stream()), "wv_fx_pointwise")
    return y.reshape(x.shape)


def median(x: torch.Tensor, kernel_size: int) -> torch.Tensor:
    """scipy.signal.medfilt(x, kernel_size) along the last axis (zero padding; kernel_size odd, at most MEDIAN_MAX_K)."""
    xr = _rows(x)
    y = torch.empty_like(xr)
    _lib.check(_lib.load().wv_fx_median(xr.data_ptr(), y.data_ptr(), xr.shape[0], xr.shape[1], int(kernel_size), _lib.stream()), "wv_fx_median")
    return y.reshape(x.shape)


def shush_forward(x: torch.Tensor, k: int, mask: Optional[torch.Tensor] = None):
    """-> (y, keep, mask_out): the k quietest samples of every row zeroed (csrc/wv_fx_time.hip shush_kernel)."""
    xr = _rows(x)
    mr = _rows(mask) if mask is not None else None
    y, keep = torch.empty_like(xr), torch.empty_like(xr)
    mo = torch.empty_like(xr) if mr is not None else None
    _lib.check(_lib.load().wv_fx_shush(xr.data_ptr(), _lib.ptr(mr), y.data_ptr(), keep.data_ptr(),
                                       _lib.ptr(mo), xr.shape[0], xr.shape[1], int(k), _lib.stream()), "wv_fx_shush")
    return y.reshape(x.shape), keep.reshape(x.shape), (mo.reshape(mask.shape) if mo is not None else None)


def echo_forward(x: torch.Tensor, n: int, volume: float):
    """-> (y, record): the reference's echo with an impulse response of n taps; `record` (int64 [2], device) holds the two peaks
    (magnitude and earliest position; the backward reads the magnitudes)."""
    lib = _lib.load()
    xr = _rows(x)
    rec = torch.empty(2, dtype=torch.int64, device=xr.device)
    y = torch.empty_like(xr)
    _lib.check(lib.wv_fx_echo_peaks(xr.data_ptr(), rec.data_ptr(), xr.shape[0], xr.shape[1], int(n), float(volume), _lib.stream()), "wv_fx_echo_peaks")
    _lib.check(lib.wv_fx_echo_apply(xr.data_ptr(), rec.data_ptr(), y.data_ptr(), xr.shape[0], xr.shape[1], int(n), float(volume), _lib.stream()), "wv_fx_echo_apply")
    return y.reshape(x.shape), rec


def echo_backward(x: torch.Tensor, g: torch.Tensor, rec: torch.Tensor, n: int, volume: float) -> torch.Tensor:
    """Gradient towards x of echo_forward(x, n, volume) given g towards its output, through the correlation and both maxima.  Tied
    peaks (clipped audio) share a maximum's gradient evenly, as the reference's autograd of torch.max(torch.abs(.)) shares it."""
    lib = _lib.load()
    xr, gr = _rows(x), _rows(g)
    dx = torch.empty_like(xr)
    nbytes = int(lib.wv_fx_echo_backward_workspace_bytes())
    ws = _lib.scratch(nbytes, xr.device)
    _lib.check(lib.wv_fx_echo_backward(xr.data_ptr(), gr.data_ptr(), rec.data_ptr(), dx.data_ptr(), xr.shape[0], xr.shape[1], int(n), float(volume),
                                       ws.data_ptr(), nbytes, _lib.stream()), "wv_fx_echo_backward")
    return dx.reshape(g.shape)


def smooth_forward(x: torch.Tensor, w: int, mask: Optional[torch.Tensor] = None, valid_threshold: float = 0.5):
    """-> (y, mask_out): box filter of w taps over the reflect-padded signal; the mask from the zero-padded mask's window count."""
    xr = _rows(x)
    mr = _rows(mask) if mask is not None else None
    y = torch.empty_like(xr)
    mo = torch.empty_like(xr) if mr is not None else None
    _lib.check(_lib.load().wv_fx_smooth(xr.data_ptr(), _lib.ptr(mr), y.data_ptr(), _lib.ptr(mo),
                                        xr.shape[0], xr.shape[1], int(w), float(valid_threshold), _lib.stream()), "wv_fx_smooth")
    return y.reshape(x.shape), (mo.reshape(mask.shape) if mo is not None else None)


def smooth_backward(g: torch.Tensor, w: int) -> torch.Tensor:
    """Transpose of smooth_forward's audio path."""
    gr = _rows(g)
    dx = torch.empty_like(gr)
    _lib.check(_lib.load().wv_fx_smooth_backward(gr.data_ptr(), dx.data_ptr(), gr.shape[0], gr.shape[1], int(w), _lib.stream()), "wv_fx_smooth_backward")
    return dx.reshape(g.shape)


def scatter_zero(y: torch.Tensor, idx: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
    """y[row, idx[row, j]] = 0 IN PLACE (and on mask): y / mask contiguous float32 [..., T], idx int32 [rows, num] on the device."""
    for t in (y, mask):
        if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise RuntimeError("scatter_zero works in place on contiguous float32 GPU tensors")
    T = y.shape[-1]
    _lib.check(_lib.load().wv_fx_scatter_zero(y.data_ptr(), _lib.ptr(mask), idx.data_ptr(), y.numel() // T, T, int(idx.shape[-1]),
                                              _lib.stream()), "wv_fx_scatter_zero")


def stretch_linear(x: torch.Tensor, t_out: int) -> torch.Tensor:
    """torch.nn.functional.interpolate(x, size=t_out, mode='linear', align_corners=False) along the last axis (the source coordinate
    one fused multiply-add, as torch's CPU kernel forms it)."""
    xr = _rows(x)
    y = torch.empty(xr.shape[0], int(t_out), device=xr.device)
    _lib.check(_lib.load().wv_fx_stretch_linear(xr.data_ptr(), y.data_ptr(), xr.shape[0], xr.shape[1], int(t_out), _lib.stream()), "wv_fx_stretch_linear")
    return y.reshape(list(x.shape[:-1]) + [int(t_out)])


def _note(tape, **what) -> None:
    if tape is not None:
        tape.update(what)


# ---- the reference's effect wrappers -------------------------------------------------------------------------------------------------
class AudioEffects:
    """The reference's AudioEffects with its signatures, defaults and conventions: identity / highpass_filter / lowpass_filter /
    bandpass_filter / resample (effect_augmentation.py:1364-1379,1451-1501,1684-1870; parity unpinned, see the module docstring), and
    the time-domain effects added below the class.  Every method returns (tensor, mask); like the reference's, the time-domain ones
    are fail-safe: an invalid argument returns (tensor, mask) unchanged instead of raising.  What is NOT fail-safe: a CPU tensor
    (RuntimeError, there is no CPU fallback), a kernel that fails (RuntimeError) and a median window past the kernel's limit
    (ValueError naming it).  `_tape` is EffectTape's record of what the backward needs; callers leave it alone."""

    @staticmethod
    def identity(tensor, mask=None, **kwargs):
        return tensor, mask

    @staticmethod
    def _cutoff(freq: float, sample_rate: int) -> float:
        nyquist = sample_rate / 2
        return max(0.0, min(freq, nyquist - EPSILON)) / nyquist

    @staticmethod
    def highpass_filter(tensor, cutoff_freq: float = 500, sample_rate: int = DEFAULT_SAMPLE_RATE, mask=None, **kwargs):
        try:
            return highpass(tensor, AudioEffects._cutoff(cutoff_freq, sample_rate)), mask
        except ValueError:                                   # the reference catches the library's error and passes the input through
            return tensor, mask

    @staticmethod
    def lowpass_filter(tensor, cutoff_freq: float = 3000, sample_rate: int = DEFAULT_SAMPLE_RATE, mask=None, **kwargs):
        try:
            return lowpass(tensor, AudioEffects._cutoff(cutoff_freq, sample_rate)), mask
        except ValueError:
            return tensor, mask

    @staticmethod
    def bandpass_filter(tensor, cutoff_freq_low: float = 300, cutoff_freq_high: float = 8000, sample_rate: int = DEFAULT_SAMPLE_RATE,
                        mask=None, **kwargs):
        if cutoff_freq_low < 0:
            raise ValueError(f"Low cutoff frequency must be non-negative, got {cutoff_freq_low} Hz")
        if cutoff_freq_high < 0:
            raise ValueError(f"High cutoff frequency must be non-negative, got {cutoff_freq_high} Hz")
        nyquist = sample_rate / 2.0
        lo = max(0.0, min(cutoff_freq_low, nyquist - EPSILON))
        hi = max(0.0, min(cutoff_freq_high, nyquist - EPSILON))
        if lo >= hi:
            raise ValueError(f"Low cutoff {lo} Hz must be less than high cutoff {hi} Hz")
        nl, nh = lo / nyquist, hi / nyquist
        if not (0.0 < nl < 1.0) or not (0.0 < nh < 1.0):
            raise ValueError(f"Normalized cutoffs must be between 0 and 1. Got low: {nl}, high: {nh}")
        return bandpass(tensor, nl, nh), mask                # a cutoff above 0.5 cycles per sample raises ValueError, as in the reference

    @staticmethod
    def resample(tensor, new_sample_rate: int, sample_rate: int = DEFAULT_SAMPLE_RATE, mask=None, **kwargs):
        if not isinstance(new_sample_rate, int) or new_sample_rate <= 0:
            raise ValueError(f"new_sample_rate must be positive int, got {new_sample_rate}")
        down = resample_waveform(tensor, sample_rate, new_sample_rate)
        return resample_waveform(down, new_sample_rate, sample_rate), mask


    @staticmethod
    def speed(tensor, speed=1.0, sample_rate: int = DEFAULT_SAMPLE_RATE, mask=None, _tape=None, **kwargs):
        """PARITY UNPINNED, like the sinc filters: the reference runs SoX (`speed s`, `rate sr`) through torchaudio, absent here and from
        the reference's outputs.  Built as that chain: resample by the rational of 1 / s through the polyphase resampler (speed 0.8 ->
        4 : 5, T -> ceil(5 T / 4)), then the linear stretch back to T that _SoxEffectSTE(..., 'stretch') applies.  The mask comes back
        unchanged (adjust_mask_length to an equal length is the identity); the gradient is straight-through.  A tuple draws random.uniform."""
        x = _lib.dev(tensor, _ON_GPU)
        try:
            if isinstance(speed, tuple):
                speed = random.uniform(*speed)
            if speed <= 0:
                raise ValueError(f"Speed must be positive, got {speed}")
            orig, new = speed_ratio(speed)
        except (ValueError, TypeError, ZeroDivisionError):
            return tensor, mask
        return stretch_linear(resample_waveform(x, orig, new), x.shape[-1]), mask

    @staticmethod
    def echo(tensor, volume_range=(0.1, 0.5), duration_range=(0.1, 0.5), sample_rate: int = DEFAULT_SAMPLE_RATE, mask=None, _tape=None, **kwargs):
        """The delayed copy comes BEFORE the sound (the reference correlates with [1, 0, .., 0, volume]); peak-normalised over the whole
        tensor; the last n - 1 samples are 0.  Too short a clip (T < 2) comes back unchanged, before anything is drawn."""
        x = _lib.dev(tensor, _ON_GPU)
        T = x.shape[-1]
        try:
            if T / sample_rate <= 0 or T < MIN_AUDIO_LENGTH:
                return tensor, mask
            n, volume = echo_plan(T, sample_rate, volume_range, duration_range)
            if n > T:
                raise ValueError("impulse response longer than the clip")
        except (ValueError, TypeError, ZeroDivisionError, RuntimeError):
            return tensor, mask
        y, rec = echo_forward(x, n, volume)
        _note(_tape, x=x.clone(), n=n, volume=volume, rec=rec)
        return y, mask

    @staticmethod
    def pink_noise(tensor, noise_std: float = 0.01, mask=None, _tape=None, **kwargs):
        """The noise comes from `pink_noise_host` (the reference's Python loop on numpy's global generator: the host loop is the cost);
        the device only computes tensor + noise * noise_std."""
        x = _lib.dev(tensor, _ON_GPU)
        try:
            noise = torch.from_numpy(pink_noise_host(x.numel())).reshape(x.shape).to(x.device)
            a = float(noise_std)
        except (ValueError, TypeError):
            return tensor, mask
        return pointwise(x, OP_ADD_NOISE, a, noise), mask

    @staticmethod
    def median_filter(tensor, kernel_size: int = 3, mask=None, _tape=None, **kwargs):
        """scipy.signal.medfilt per row (ZERO padding, whatever the reference's comment says); an even kernel_size is bumped by 1."""
        x = _lib.dev(tensor, _ON_GPU)
        try:
            if kernel_size < 1:
                raise ValueError(f"Kernel size must be positive, got {kernel_size}")
            k = int(kernel_size) + (1 if int(kernel_size) % 2 == 0 else 0)
        except (ValueError, TypeError):
            return tensor, mask
        if k > MEDIAN_MAX_K:
            raise ValueError(f"median_filter: kernel_size {k} is past the kernel's limit of {MEDIAN_MAX_K} (WV_FX_MEDIAN_MAX_K)")
        return median(x, k), mask

    @staticmethod
    def smooth(tensor, window_size_range=(2, 10), mask=None, valid_threshold: float = 0.5, _tape=None, **kwargs):
        x = _lib.dev(tensor, _ON_GPU)
        if mask is not None and mask.device != tensor.device:
            raise RuntimeError(f"Device mismatch in smooth effect: tensor on {tensor.device}, mask on {mask.device}")
        try:
            w = smooth_window(window_size_range)
            if w < 1 or w > SMOOTH_MAX_W or w - 1 - (w - 1) // 2 >= x.shape[-1]:      # torch.ones(.., 0) / reflect padding would raise
                raise ValueError("window does not fit")
            thr = float(valid_threshold)
        except (ValueError, TypeError, RuntimeError):
            return tensor, mask
        y, m = smooth_forward(x, w, mask, thr)
        _note(_tape, w=w)
        return y, m

    @staticmethod
    def amplitude_scaling(tensor, scale: float = 1.0, mask=None, _tape=None, **kwargs):
        x = _lib.dev(tensor, _ON_GPU)
        try:
            a = float(scale)
        except (ValueError, TypeError):
            return tensor, mask
        y = pointwise(x, OP_SCALE, a)
        _note(_tape, scale=a)
        return y, mask

    @staticmethod
    def quantization(tensor, bit_depth: int = 16, mask=None, _tape=None, **kwargs):
        """(tensor * max_val).round() / max_val with max_val = 2^(bit_depth-1) - 1; bit_depth = 1 gives 0 / 0 = NaN, as in the reference."""
        x = _lib.dev(tensor, _ON_GPU)
        try:
            if not 1 <= bit_depth <= 32:
                raise ValueError(f"Bit depth must be between 1 and 32, got {bit_depth}")
            max_val = 2 ** (bit_depth - 1) - 1
        except (ValueError, TypeError):
            return tensor, mask
        return pointwise(x, OP_QUANTIZE, max_val), mask

    @staticmethod
    def sample_suppression(tensor, suppression_percentage: float = 0.1, mask=None, _tape=None, **kwargs):
        """Zeroes int(T * pct) random samples per (b, c) in a copy of the audio and of the mask (the reference writes into the mask it is
        given, which its dispatcher has cloned; here the clone is made in place of the write)."""
        x = _lib.dev(tensor, _ON_GPU)
        try:
            if not 0 <= suppression_percentage <= 1:
                raise ValueError(f"Suppression percentage must be between 0 and 1, got {suppression_percentage}")
            rows = x.numel() // x.shape[-1]
            idx = suppression_indices(rows, 1, x.shape[-1], suppression_percentage)
        except (ValueError, TypeError):
            return tensor, mask
        y = x.clone()
        m = _lib.dev(mask, _ON_GPU).clone() if mask is not None else None
        idx_d = torch.from_numpy(idx).to(x.device)
        scatter_zero(y, idx_d, m)
        _note(_tape, idx=idx_d)
        return y, m

    @staticmethod
    def _gaussian_noise(tensor, noise_std, mask):
        x = _lib.dev(tensor, _ON_GPU)
        try:
            if noise_std < 0:
                raise ValueError(f"Noise std must be non-negative, got {noise_std}")
            a = float(noise_std)
        except (ValueError, TypeError):
            return tensor, mask
        return pointwise(x, OP_ADD_NOISE, a, torch.randn_like(x)), mask      # the draw is torch's device generator, the scaled add the kernel

    @staticmethod
    def random_noise(tensor, noise_std: float = 0.001, mask=None, _tape=None, **kwargs):
        return AudioEffects._gaussian_noise(tensor, noise_std, mask)

    @staticmethod
    def white_noise(tensor, noise_std: float = 0.01, mask=None, _tape=None, **kwargs):
        return AudioEffects._gaussian_noise(tensor, noise_std, mask)

    @staticmethod
    def shush(tensor, fraction: float = 0.1, mask=None, _tape=None, **kwargs):
        """Zeroes the k = min(int(T * fraction), T - 1) quietest samples of each row; the mask is cleared where the OUTPUT is 0."""
        x = _lib.dev(tensor, _ON_GPU)
        try:
            if not 0 <= fraction <= 1:
                raise ValueError(f"Fraction must be between 0 and 1, got {fraction}")
            k = min(int(x.shape[-1] * fraction), x.shape[-1] - 1)
        except (ValueError, TypeError):
            return tensor, mask
        y, keep, m = shush_forward(x, k, mask)
        _note(_tape, keep=keep)
        return y, m



REFUSED = {"mp3_lossy_compression": "ffmpeg's codec", "aac_lossy_compression": "ffmpeg's codec", "encodec": "the transformers EnCodec model",
           "random_equalization": "SoX's biquad equaliser"}

# the reference's shipped evaluation list, in its order (conf/effects_config.yml `eval_effects`, model/watermarking.py:135-143): what a
# validation pass applies to the whole batch, one effect at a time.  tests/golden/eval_effects.json holds the same list as data.
EVAL_EFFECTS = (
    ("identity", {}),
    ("resample", {"new_sample_rate": 32000}),
    ("speed", {"speed": 0.8}),
    ("random_noise", {"noise_std": 0.001}),
    ("lowpass_filter", {"cutoff_freq": 2000}),
    ("highpass_filter", {"cutoff_freq": 3500}),
    ("bandpass_filter", {"cutoff_freq_low": 300, "cutoff_freq_high": 4000}),
)


def apply_effect(name: str, params: dict, audio: torch.Tensor, mask: Optional[torch.Tensor] = None, sample_rate: int = DEFAULT_SAMPLE_RATE):
    """Dispatcher with the (name, params, audio, mask) -> (audio, mask) shape WatermarkTrainer's `apply_effect` hook expects.  Effects
    that change the length (resample rounding) are cropped / zero-padded back to the input length, as the reference's
    AudioProcessor.adjust_audio_length does for its straight-through effects.  16 of the reference's 20 effect names run here; the other
    four raise NotImplementedError because their arithmetic is a third party's that this project does not have: mp3_lossy_compression
    and aac_lossy_compression (ffmpeg), encodec (transformers) and random_equalization (SoX's biquad) -- `REFUSED`.  Effects whose
    backward needs memory of the forward (shush, sample_suppression, echo, smooth, amplitude_scaling) get their gradient from
    `EffectTape`, not from the stateless `apply_effect_backward`."""
    fn = getattr(AudioEffects, name, None)
    if fn is None or name.startswith("_"):
        why = f" (needs {REFUSED[name]})" if name in REFUSED else ""
        raise NotImplementedError(f"effect '{name}' is not available on the GPU path{why}")
    out, mask = fn(audio, sample_rate=sample_rate, mask=mask, **params)
    T = audio.shape[-1]
    if out.shape[-1] > T:
        out = out[..., :T]
    elif out.shape[-1] < T:
        out = torch.nn.functional.pad(out, (0, T - out.shape[-1]))
    return out, mask


class EffectTape:
    """Memory between an effect's forward and its backward, with the shapes of WatermarkTrainer's two hooks:

        tape = EffectTape()
        WatermarkTrainer(..., effect_scheduler=s, apply_effect=tape.apply, effect_backward=tape.backward)

    `apply` runs `apply_effect` and records what that effect's backward needs (shush: the keep mask; sample_suppression: the indices;
    echo: the input, (n, volume) and the peak record; smooth: w; amplitude_scaling: the scale; nothing for the rest).  `backward` pops
    the records first in, first out -- the order WatermarkTrainer.step calls the two hooks in -- and applies that effect's gradient:
    masked (shush), scatter-zero (sample_suppression), the adjoints of echo and smooth, scale * g, the transposed filters of
    `apply_effect_backward` for the sinc / resample effects, and the identity for the straight-through ones (speed, quantization,
    median_filter), the additive noises and any effect whose forward fell back to returning its input.  A step that fails between
    the two hooks leaves records behind: call `reset()` before the next one."""

    def __init__(self, sample_rate: int = DEFAULT_SAMPLE_RATE):
        self.sample_rate = sample_rate
        self._records = collections.deque()

    def __len__(self) -> int:
        return len(self._records)

    def reset(self) -> None:
        self._records.clear()

    def apply(self, name: str, params: dict, audio: torch.Tensor, mask: Optional[torch.Tensor] = None):
        saved: dict = {}
        out = apply_effect(name, dict(params, _tape=saved), audio, mask, self.sample_rate)
        self._records.append((name, saved))
        return out

    def backward(self, name: str, params: dict, d_out: torch.Tensor) -> torch.Tensor:
        if not self._records:
            raise RuntimeError(f"EffectTape.backward('{name}'): nothing was applied")
        rec_name, saved = self._records.popleft()
        if rec_name != name:
            raise RuntimeError(f"EffectTape.backward('{name}') does not match the next record, '{rec_name}'")
        if name in DIFFERENTIABLE:
            return apply_effect_backward(name, params, d_out, self.sample_rate)
        if name == "shush" and "keep" in saved:
            return pointwise(d_out, OP_MUL, 0.0, saved["keep"])
        if name == "sample_suppression" and "idx" in saved:
            d = _lib.dev(d_out, _ON_GPU).clone()
            scatter_zero(d, saved["idx"])
            return d
        if name == "echo" and "rec" in saved:
            return echo_backward(saved["x"], d_out, saved["rec"], saved["n"], saved["volume"])
        if name == "smooth" and "w" in saved:
            return smooth_backward(d_out, saved["w"])
        if name == "amplitude_scaling" and "scale" in saved:
            return pointwise(d_out, OP_SCALE, saved["scale"])
        return d_out
