"""Host side of the STOI metric (metrics.STOI): the constants of the published algorithm, the tables the kernels of csrc/wv_stoi.hip
read, and the float64 numpy route CPU tensors take.

Short-time objective intelligibility (Taal, Hendriks, Heusdens, Jensen 2011), non-extended, as the pystoi package states it and the
reference reports it on every validation batch (scripts/evaluate.py:65-144): resample to 10 kHz with Octave's `resample` filter, drop the
frames of the clean clip more than 40 dB under its loudest, 512-point DFT of 256-sample Hann frames, 15 third-octave bands from 150 Hz,
correlate 30-frame segments of the clean and the clipped, scaled estimate.  pystoi is not part of this project's environment: the
arithmetic below restates the publication, and parity with an installed `pystoi` stays unpinned.

The one place where published versions differ is the frame range.  Taal's MATLAB frames with `1:K/2:(length(x)-K)`, an EXCLUSIVE end:
a clip of exactly 256 + 128 k samples has k frames, not k + 1.  FRAME_END_EXCLUSIVE holds that convention for this route; csrc/wv_stoi.hip
holds the same switch under the name ST_FRAME_END_EXCLUSIVE (a CPU test reads both).  Whoever pins against a pystoi build flips it there.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

FS, N_FRAME, HOP, NFFT, NUMBAND, MINFREQ = 10000, 256, 128, 512, 15, 150
N_SEG, BETA, DYN_RANGE = 30, -15.0, 40.0
EPS = float(np.finfo(np.float64).eps)
FRAME_END_EXCLUSIVE = True                     # frame starts = range(0, len - 256, 128); False: range(0, len - 256 + 1, 128)
SHORT_VALUE = 1e-5                             # fewer than N_SEG frames after the silent ones left: pystoi's answer (with a warning)

BIN_LO, BIN_HI = 7, 219                        # DFT bins any band reads: [7, 219)
BASIS_ROWS = 512                               # 2 * 212 rows (re, im interleaved) padded to 16 tiles of 32
SHORT_MESSAGE = "Not enough STFT frames to compute intermediate intelligibility measure after removing silent frames. Returning 1e-5."


def window() -> np.ndarray:
    return np.hanning(N_FRAME + 2)[1:-1]


def n_frames(n: int) -> int:
    """Frames of an n-sample signal under the package's convention."""
    end = n - N_FRAME + (0 if FRAME_END_EXCLUSIVE else 1)
    return 0 if end <= 0 else -(-end // HOP)


def band_edges() -> np.ndarray:
    """[15, 2] first bin and one past the last bin of every third-octave band."""
    f = np.linspace(0, FS, NFFT + 1)[: NFFT // 2 + 1]
    k = np.arange(NUMBAND, dtype=np.float64)
    lo = MINFREQ * 2.0 ** ((2 * k - 1) / 6)
    hi = MINFREQ * 2.0 ** ((2 * k + 1) / 6)
    return np.stack([np.argmin(np.abs(f[None] - lo[:, None]), axis=1), np.argmin(np.abs(f[None] - hi[:, None]), axis=1)], axis=1)


def ratio(fs: int) -> Tuple[int, int]:
    g = math.gcd(FS, int(fs))
    return FS // g, int(fs) // g


def resample_filter(up: int, down: int) -> Tuple[np.ndarray, int]:
    """Octave's `resample` FIR for up / down -> (h [2 half + 1] float64 with unit sum, half)."""
    fc = 1.0 / (2 * max(up, down))
    roll = fc / 10
    half = int(math.ceil((60 - 8) / (28.714 * roll)))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60 - 8.7)) * 2 * up * fc * np.sinc(2 * fc * t)
    return h / h.sum(), half


def resample_kernels(fs: int) -> Tuple[np.ndarray, int, int, int, int]:
    """The filter as wv_fx_resample's table -> (kernels [up][L] float64, up, down, L, width):
    y10[n up + f] = sum_j kernels[f][j] x[n down + j - width], kernels[f][j] = up h[half + down f + up (width - j)], zero outside h."""
    up, down = ratio(fs)
    h, half = resample_filter(up, down)
    width = -(-half // up)
    L = 2 * width + down
    idx = half + down * np.arange(up)[:, None] + up * (width - np.arange(L)[None, :])
    ok = (idx >= 0) & (idx <= 2 * half)
    return np.where(ok, up * h[np.clip(idx, 0, 2 * half)], 0.0), up, down, L, width


def resampled_length(T: int, fs: int) -> int:
    up, down = ratio(fs)
    return -(-T * up // down)


def dft_basis() -> np.ndarray:
    """What the band-spectra kernel multiplies frames by, float64: [256 samples][512 rows] followed by the 256 window samples, flat.
    Row 2 i is w[n] cos(2 pi (7 + i) n / 512), row 2 i + 1 is -w[n] sin(...) for the 212 bins 7..218 (the frame's second window
    folded in); rows 424..511 are zero.  The angle is reduced modulo 512 in integers first."""
    w = window()
    n = np.arange(N_FRAME)
    k = np.arange(BIN_LO, BIN_HI)
    ang = 2 * np.pi * ((n[:, None] * k[None, :]) % NFFT) / NFFT
    b = np.zeros((N_FRAME, BASIS_ROWS), np.float64)
    b[:, 0: 2 * len(k): 2] = w[:, None] * np.cos(ang)
    b[:, 1: 2 * len(k): 2] = -w[:, None] * np.sin(ang)
    return np.concatenate([b.reshape(-1), w])


# ---- the float64 route ------------------------------------------------------------------------------------------------------------
def resample(x: np.ndarray, fs: int) -> np.ndarray:
    """[..., T] at fs -> [..., ceil(T up / down)] at 10 kHz through the kernel table, float64."""
    if int(fs) == FS:
        return np.asarray(x, np.float64)
    k, up, down, L, width = resample_kernels(fs)
    x = np.asarray(x, np.float64)
    T = x.shape[-1]
    t_out = resampled_length(T, fs)
    groups = -(-t_out // up)
    xp = np.zeros(x.shape[:-1] + (width + (groups - 1) * down + L,), np.float64)
    xp[..., width: width + T] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, L, axis=-1)[..., ::down, :][..., :groups, :]      # [..., groups, L]
    y = np.einsum("...gl,fl->...gf", win, k)
    return y.reshape(x.shape[:-1] + (groups * up,))[..., :t_out]


def kept_frames(x10: np.ndarray) -> Tuple[np.ndarray, int]:
    """Indices of the frames of the clean clip that stay (ascending), and the number of frames it has."""
    total = n_frames(x10.shape[-1])
    if total == 0:
        return np.zeros(0, np.int64), 0
    w = window()
    fr = np.lib.stride_tricks.sliding_window_view(x10, N_FRAME)[::HOP][:total] * w
    e = 20 * np.log10(np.sqrt((fr * fr).sum(axis=1)) + EPS)
    return np.nonzero((e.max() - DYN_RANGE - e) < 0)[0], total


def gathered_frames(x10: np.ndarray, kept: np.ndarray) -> np.ndarray:
    """[J, 256], J = len(kept) - 1: the frames of the clip with its dropped frames cut out, before their own window, by the gather the
    kernel uses -- frame j = F[kept[j]] + [j > 0] second half of F[kept[j-1]] onto the first 128 samples + first half of F[kept[j+1]]
    onto the last 128, F[i] = w * x10[128 i : 128 i + 256].  Exactly the overlap-add of the kept frames, framed again: every sample
    is a sum of two terms either way."""
    J = len(kept) - 1
    if J < 1:
        return np.zeros((0, N_FRAME), np.float64)
    w = window()
    F = np.stack([w * x10[HOP * i: HOP * i + N_FRAME] for i in kept])
    fr = F[:J].copy()
    fr[1:, :HOP] += F[: J - 1, HOP:]
    fr[:, HOP:] += F[1: J + 1, :HOP]
    return fr


def band_magnitudes(x10: np.ndarray, kept: np.ndarray) -> np.ndarray:
    """[15, J] third-octave magnitudes of the windowed gathered frames."""
    fr = gathered_frames(x10, kept)
    if not len(fr):
        return np.zeros((NUMBAND, 0), np.float64)
    spec = np.fft.rfft(fr * window(), NFFT, axis=1)
    p = spec.real ** 2 + spec.imag ** 2
    return np.stack([np.sqrt(p[:, lo:hi].sum(axis=1)) for lo, hi in band_edges()])


def correlate(x_tob: np.ndarray, y_tob: np.ndarray) -> float:
    """The segment stage on [15, J] band magnitudes, J >= 30."""
    J = x_tob.shape[1]
    xs = np.stack([x_tob[:, m - N_SEG: m] for m in range(N_SEG, J + 1)])
    ys = np.stack([y_tob[:, m - N_SEG: m] for m in range(N_SEG, J + 1)])
    alpha = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yp = np.minimum(ys * alpha, xs * (1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xs = xs - xs.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xs = xs / (np.linalg.norm(xs, axis=2, keepdims=True) + EPS)
    return float((yp * xs).sum() / (xs.shape[0] * NUMBAND))


def stoi_numpy(reference: np.ndarray, estimate: np.ndarray, fs: int) -> Tuple[float, int, int]:
    """One clip pair -> (d, kept frames, frames).  `reference` is the clean clip x: the silent frames are its, and d is not symmetric."""
    x10, y10 = resample(reference, fs), resample(estimate, fs)
    kept, total = kept_frames(x10)
    if len(kept) - 1 < N_SEG:
        return SHORT_VALUE, len(kept), total
    return correlate(band_magnitudes(x10, kept), band_magnitudes(y10, kept)), len(kept), total


_TABLES: Dict[tuple, tuple] = {}


def device_tables(fs: int, device):
    """(kernels [up][L] float32 or None at 10 kHz, up, down, L, width, basis float32) on `device`, built once per (fs, device)."""
    import torch
    key = (int(fs), str(device))
    if key not in _TABLES:
        basis = torch.from_numpy(dft_basis().astype(np.float32)).to(device)
        if int(fs) == FS:
            _TABLES[key] = (None, 1, 1, 0, 0, basis)
        else:
            k, up, down, L, width = resample_kernels(fs)
            _TABLES[key] = (torch.from_numpy(np.ascontiguousarray(k.astype(np.float32))).to(device), up, down, L, width, basis)
    return _TABLES[key]
