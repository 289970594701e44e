"""Multi-scale STFT and mel-spectrogram reconstruction losses of the reference's generator update, on HIP (csrc/wv_specloss.hip).

    stft = MultiScaleSTFTLoss();  loss, d_wm = stft(wm, x, grad_scale=10.0)
    mel = MelSpectrogramLoss();   loss, d_wm = mel(wm, x, grad_scale=20.0, want_grad=False)
    both = SpectralLosses(stft, mel);  l_stft, l_mel, d_wm = both(wm, x, stft_grad_scale=10.0, mel_grad_scale=20.0)

Composition (/root/reference/scripts/loss.py:449-731, `MultiScaleSTFTLoss.forward` and `MelSpectrogramLoss.forward`): for every scale,

    term = log_weight * mean|log10(clamp(S_wm, eps)^pow) - log10(clamp(S_x, eps)^pow)| + mag_weight * mean|S_wm - S_x|

with L1 means over [B, 1, bins or bands, frames] (nn.L1Loss), and the loss is the sum of the terms (weight 1).  A term whose weight is 0
is not computed, as in the reference (it contributes neither value nor gradient).

Configuration: what conf/base.yml binds through `argbind.bind_module(loss)` (scripts/train.py:232), the defaults of scripts/loss.py:48-60
where the file is silent:
  * MultiScaleSTFTLoss: window_lengths [2048, 512], hop = w // 4, mag_weight 1, log_weight 1, pow 2, clamp_eps 1e-5;
  * MelSpectrogramLoss: n_mels [5, 10, 20, 40, 80, 160, 320], window_lengths [32, 64, ..., 2048], hop = w // 4, fmin 0, fmax = sr / 2,
    pow 1, clamp_eps 1e-5, mag_weight 0, log_weight 1 (sample rate 16000).

Primitives.  They come from `audiotools.AudioSignal`, which the reference imports but does not vendor; nothing here holds audiotools or
librosa, so these are restatements and UNPINNED against those libraries (INTEGRATION.md lists them):
  * window: the periodic Hann window of length w, `scipy.signal.get_window("hann", w)` = 0.5 - 0.5 cos(2 pi n / w)   (`hann_window`);
  * transform: centred, reflect padding of w // 2 on each side (match_stride=False: no extra padding, no frames dropped), n_fft = w,
    hop = w // 4, one-sided: T // hop + 1 frames of w // 2 + 1 bins;
  * magnitude: S = |X|;
  * mel: |X| projected onto librosa's default `filters.mel` (Slaney mel scale, not HTK; Slaney area normalisation; float32 filters)
    restated in numpy (`mel_filters`), fmax None -> sr / 2.
Reflect padding is undefined for T <= w // 2: such clips raise ValueError.

The gradient (towards wm only; x is data): dL/dS = sign(difference) * pow / (S ln 10) where S >= eps (0 where the clamp binds), plus
mag_weight * sign(S_wm - S_x), divided by the element count; for a mel term it goes through the filters transposed; dX = dL/dS * X / |X|
(0 where |X| = 0); dwm = the overlap-add of Basis^T dX with the reflect padding's adjoint.  Shared scales (2048 and 512 of the default
configurations) compute their spectra once when both losses run through one `SpectralLosses`.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib

STFT_WINDOW_LENGTHS = [2048, 512]
MEL_N_MELS = [5, 10, 20, 40, 80, 160, 320]
MEL_WINDOW_LENGTHS = [32, 64, 128, 256, 512, 1024, 2048]


def hann_window(w: int) -> np.ndarray:
    """Periodic Hann window of length w (scipy.signal.get_window("hann", w)), float64."""
    n = np.arange(w, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / w)


def hz_to_mel(f):
    """Slaney mel scale (librosa.hz_to_mel, htk=False): linear below 1 kHz (200/3 Hz per mel), logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m):
    """Inverse of hz_to_mel (librosa.mel_to_hz, htk=False)."""
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filters(sr: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None) -> np.ndarray:
    """librosa.filters.mel(sr=sr, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax) with its defaults (htk=False, norm="slaney",
    dtype float32): triangles between n_mels + 2 points equally spaced in mel, each scaled by 2 / (its width in Hz).  [n_mels][n_fft//2+1]."""
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    weights = np.zeros((n_mels, 1 + n_fft // 2), dtype=np.float32)
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2: n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights


class _Plan:
    """One wv_specloss plan: the scales' packed bases, windows and mel bands resident on the device."""

    def __init__(self, scales):
        """scales: list of dicts {w, stft: (log_w, mag_w, pow, eps) or None, mel: (log_w, mag_w, pow, eps) or None, n_mels, fmin, fmax, sr}."""
        self.scales = scales
        n = len(scales)
        wl = (C.c_int * n)(*[s["w"] for s in scales])
        flags = (C.c_int * n)(*[(1 if s["stft"] else 0) | (2 if s["mel"] else 0) for s in scales])
        nm = (C.c_int * n)(*[s.get("n_mels", 0) if s["mel"] else 0 for s in scales])
        params = np.zeros((n, 8), np.float32)
        for i, s in enumerate(scales):
            if s["stft"]:
                params[i, :4] = s["stft"]
            if s["mel"]:
                params[i, 4:] = s["mel"]
        windows = np.concatenate([hann_window(s["w"]) for s in scales]).astype(np.float32)
        mels = [mel_filters(s["sr"], s["w"], s["n_mels"], s["fmin"], s["fmax"]).ravel() for s in scales if s["mel"]]
        melbuf = np.concatenate(mels).astype(np.float32) if mels else np.zeros(1, np.float32)
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.wv_specloss_plan_create(n, wl, flags, nm, params.ctypes.data, windows.ctypes.data, melbuf.ctypes.data, C.byref(h)),
                   "wv_specloss_plan_create")
        self._h, self._lib = h, lib

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.wv_specloss_plan_destroy(h)
            self._h = None

    def run(self, wm: torch.Tensor, x: torch.Tensor, stft_scale: float, mel_scale: float, want_grad: bool, out: Optional[torch.Tensor]):
        """-> (terms [n_scales][2], totals [2], d_wm or None)."""
        wm, x = _check(wm, x, [s["w"] for s in self.scales])
        B, T = wm.shape[0], wm.shape[-1]
        terms = torch.empty(len(self.scales), 2, device=wm.device)
        totals = torch.empty(2, device=wm.device)
        dwm = None
        if want_grad:
            if out is None:
                dwm = torch.zeros_like(wm)
            else:
                if out.shape != wm.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != wm.device:
                    raise ValueError("out must be a contiguous float32 tensor of wm's shape on wm's device")
                dwm = out
        ws = _lib.scratch(int(self._lib.wv_specloss_workspace_bytes(self._h, B, T)), wm.device)
        rc = self._lib.wv_specloss(self._h, wm.data_ptr(), x.data_ptr(), B, T, terms.data_ptr(), totals.data_ptr(),
                                   _lib.ptr(dwm), float(stft_scale), float(mel_scale), ws.data_ptr(), ws.numel(),
                                   _lib.stream(wm.device))
        _lib.check(rc, "wv_specloss")
        return terms, totals, dwm


def _check(wm: torch.Tensor, x: torch.Tensor, windows: Sequence[int]):
    if wm.shape != x.shape:
        raise ValueError(f"shape mismatch: {tuple(wm.shape)} vs {tuple(x.shape)}")
    if wm.dim() != 3 or wm.shape[1] != 1:
        raise ValueError(f"expected [B, 1, T] audio, got {tuple(wm.shape)}")
    T = wm.shape[-1]
    w = max(windows)
    if T <= w // 2:
        raise ValueError(f"clip length {T} <= window {w} // 2: reflect padding of the centred transform is undefined")
    if not (wm.is_cuda and x.is_cuda):
        raise RuntimeError("spectral losses run on the GPU: wm and x must be CUDA tensors")
    return wm.float().contiguous(), x.float().contiguous()


class MultiScaleSTFTLoss:
    """The reference's MultiScaleSTFTLoss (scripts/loss.py:449-561) as configured by conf/base.yml (see the module docstring)."""

    def __init__(self, window_lengths: Sequence[int] = STFT_WINDOW_LENGTHS, clamp_eps: float = 1e-5, mag_weight: float = 1.0,
                 log_weight: float = 1.0, pow: float = 2.0):
        self.window_lengths = [int(w) for w in window_lengths]
        self.term = (float(log_weight), float(mag_weight), float(pow), float(clamp_eps))
        self.scales = [{"w": w, "stft": self.term, "mel": None} for w in self.window_lengths]
        self._plan = None
        self.last_terms = None

    def __call__(self, wm: torch.Tensor, x: torch.Tensor, grad_scale: float = 1.0, want_grad: bool = True, out: Optional[torch.Tensor] = None):
        """-> (loss [1], grad_scale * dloss/dwm or None).  `out`: a [B,1,T] float32 tensor the gradient is ADDED to (and returned)."""
        _check(wm, x, self.window_lengths)
        if self._plan is None:
            self._plan = _Plan(self.scales)
        terms, totals, dwm = self._plan.run(wm, x, grad_scale, 0.0, want_grad, out)
        self.last_terms = terms[:, 0]
        return totals[:1], dwm


class MelSpectrogramLoss:
    """The reference's MelSpectrogramLoss (scripts/loss.py:564-731) as configured by conf/base.yml (see the module docstring)."""

    def __init__(self, n_mels: Sequence[int] = MEL_N_MELS, window_lengths: Sequence[int] = MEL_WINDOW_LENGTHS, sample_rate: int = 16000,
                 clamp_eps: float = 1e-5, mag_weight: float = 0.0, log_weight: float = 1.0, pow: float = 1.0,
                 mel_fmin: Optional[Sequence[float]] = None, mel_fmax: Optional[Sequence[Optional[float]]] = None):
        if len(n_mels) != len(window_lengths):
            raise ValueError(f"n_mels and window_lengths must have the same length, got {len(n_mels)} and {len(window_lengths)}")
        fmin = [0.0] * len(n_mels) if mel_fmin is None else [float(f) for f in mel_fmin]
        fmax = [None] * len(n_mels) if mel_fmax is None else list(mel_fmax)
        if len(fmin) != len(n_mels) or len(fmax) != len(n_mels):
            raise ValueError("mel_fmin and mel_fmax must match window_lengths in length")
        self.window_lengths, self.n_mels, self.sample_rate = [int(w) for w in window_lengths], [int(n) for n in n_mels], int(sample_rate)
        self.term = (float(log_weight), float(mag_weight), float(pow), float(clamp_eps))
        self.scales = [{"w": w, "stft": None, "mel": self.term, "n_mels": n, "fmin": lo, "fmax": hi, "sr": self.sample_rate}
                       for w, n, lo, hi in zip(self.window_lengths, self.n_mels, fmin, fmax)]
        self._plan = None
        self.last_terms = None

    def __call__(self, wm: torch.Tensor, x: torch.Tensor, grad_scale: float = 1.0, want_grad: bool = True, out: Optional[torch.Tensor] = None):
        """-> (loss [1], grad_scale * dloss/dwm or None).  `out`: a [B,1,T] float32 tensor the gradient is ADDED to (and returned)."""
        _check(wm, x, self.window_lengths)
        if self._plan is None:
            self._plan = _Plan(self.scales)
        terms, totals, dwm = self._plan.run(wm, x, 0.0, grad_scale, want_grad, out)
        self.last_terms = terms[:, 1]
        return totals[1:], dwm


class SpectralLosses:
    """Both losses in one plan: a window length the two share is transformed once per call and both terms read its spectra."""

    def __init__(self, stft: Optional[MultiScaleSTFTLoss] = None, mel: Optional[MelSpectrogramLoss] = None):
        self.stft = stft if stft is not None else MultiScaleSTFTLoss()
        self.mel = mel if mel is not None else MelSpectrogramLoss()
        scales: List[dict] = [dict(s) for s in self.mel.scales]
        self._stft_idx = []
        for s in self.stft.scales:
            j = next((i for i, q in enumerate(scales) if q["w"] == s["w"] and q["stft"] is None), None)
            if j is None:
                scales.append(dict(s))
                j = len(scales) - 1
            else:
                scales[j]["stft"] = s["stft"]
            self._stft_idx.append(j)
        self._mel_idx = list(range(len(self.mel.scales)))
        self.scales, self._plan = scales, None
        self.last_terms = None

    def __call__(self, wm: torch.Tensor, x: torch.Tensor, stft_grad_scale: float = 1.0, mel_grad_scale: float = 1.0, want_grad: bool = True,
                 out: Optional[torch.Tensor] = None):
        """-> (stft loss [1], mel loss [1], stft_grad_scale * dstft/dwm + mel_grad_scale * dmel/dwm or None)."""
        _check(wm, x, [s["w"] for s in self.scales])
        if self._plan is None:
            self._plan = _Plan(self.scales)
        terms, totals, dwm = self._plan.run(wm, x, stft_grad_scale, mel_grad_scale, want_grad, out)
        self.last_terms = {"stft": terms[self._stft_idx, 0], "mel": terms[self._mel_idx, 1]}
        return totals[:1], totals[1:], dwm
