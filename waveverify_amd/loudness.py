"""Host side of the loudness measure (metrics.Loudness, data.ClipPool): the constants of ITU-R BS.1770-4, the tables the kernel of
csrc/wv_loudness.hip reads, and a float64 route for CPU tensors.  No kernels here.

The reference trains on excerpts its data loader re-draws until their loudness exceeds -40 LUFS (scripts/train.py:440-475 through
audiotools, there measured by pyloudnorm).  Neither package is part of this project's environment and the reference vendors neither:
the arithmetic below restates the published standard for ONE channel, and parity with audiotools' `Meter` stays unpinned.

K-weighting: two biquads per sample rate, derived in float64 from the analog prototypes by the bilinear transform with
K = tan(pi f0 / fs) -- at 48 kHz the standard's own table to all its printed digits.  Gating: 100 ms sub-blocks (fs / 10 samples, so
fs % 10 != 0 is refused; a trailing incomplete sub-block is dropped), blocks of 4 sub-blocks at hop 1, z_j the mean square of block j
and l_j = -0.691 + 10 log10 z_j, the absolute gate l_j > -70, the relative gate l_j > (-0.691 + 10 log10 mean z of the absolute-gated
blocks) - 10, loudness = -0.691 + 10 log10 mean z of the blocks past both.  Where no block passes the absolute gate the result is
MIN_LOUDNESS, this project's floor.  The filter state is zero at the first sample of every measured window: an excerpt is its own
signal."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np

SHELF_F0, SHELF_GAIN_DB, SHELF_Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
SHELF_VB_EXPONENT = 0.4996667741545416
HIGHPASS_F0, HIGHPASS_Q = 38.13547087602444, 0.5003270373238773
OFFSET = -0.691
ABSOLUTE_GATE = -70.0                          # LUFS
RELATIVE_GATE = -10.0                          # LU under the mean of the absolute-gated blocks
MIN_LOUDNESS = -70.0                           # no block past the absolute gate: this project's floor
BLOCK_SUBS = 4                                 # a 400 ms block = 4 sub-blocks of 100 ms, hop 1 sub-block (75 % overlap)


def sub_block(fs: int) -> int:
    """Samples of a 100 ms sub-block."""
    fs = int(fs)
    if fs < 1 or fs % 10 != 0:
        raise ValueError(f"loudness: sample rate {fs} is not a positive multiple of 10 (a sub-block is fs / 10 samples)")
    return fs // 10


def k_weighting(fs: int) -> np.ndarray:
    """[2, 6] float64 in scipy's sos layout [b0 b1 b2 1 a1 a2]: the shelf, then the high-pass."""
    fs = float(sub_block(fs) * 10)
    K = math.tan(math.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXPONENT
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = [(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0,
             1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0]
    K = math.tan(math.pi * HIGHPASS_F0 / fs)
    a0 = 1.0 + K / HIGHPASS_Q + K * K
    highpass = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HIGHPASS_Q + K * K) / a0]
    return np.array([shelf, highpass], np.float64)


_TABLES: Dict[tuple, "torch.Tensor"] = {}


def device_table(fs: int, device):
    """What wv_loudness reads as `table`: k_weighting(fs), 12 float64, on `device`; built once per (fs, device)."""
    import torch
    key = (int(fs), str(device))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(k_weighting(fs).reshape(-1).copy()).to(device)
    return _TABLES[key]


def _sosfilt_rows(sos: np.ndarray, x: np.ndarray) -> np.ndarray:
    """scipy.signal.sosfilt(sos, x, axis=-1) from a zero state, operation for operation, sample by sample over all rows at once."""
    y = np.array(x, np.float64)
    for b0, b1, b2, _, a1, a2 in sos:
        z1 = np.zeros(y.shape[:-1])
        z2 = np.zeros(y.shape[:-1])
        for t in range(y.shape[-1]):
            xn = y[..., t]
            yn = b0 * xn + z1
            z1 = b1 * xn - a1 * yn + z2
            z2 = b2 * xn - a2 * yn
            y[..., t] = yn
    return y


def k_filter(x: np.ndarray, fs: int) -> np.ndarray:
    """The K-weighted signal in float64 along the last axis, zero initial state: scipy's sosfilt where scipy is installed, else the same
    recurrence in numpy (equal bit for bit, slower)."""
    x = np.asarray(x, np.float64)
    try:
        from scipy.signal import sosfilt
    except ImportError:
        return _sosfilt_rows(k_weighting(fs), x)
    return sosfilt(k_weighting(fs), x, axis=-1)


def sub_block_energies(y: np.ndarray, fs: int) -> np.ndarray:
    """[..., T // h] sums of squares of the whole sub-blocks of a K-weighted signal."""
    h = sub_block(fs)
    n = y.shape[-1] // h
    if n < BLOCK_SUBS:
        raise ValueError(f"loudness: {y.shape[-1]} samples at {fs} Hz are fewer than one gating block of {BLOCK_SUBS} sub-blocks ({BLOCK_SUBS * h})")
    y = y[..., : n * h].reshape(y.shape[:-1] + (n, h))
    return (y * y).sum(axis=-1)


def gate(sub: np.ndarray, fs: int) -> float:
    """[S] sub-block energies of one window -> its gated loudness in LUFS."""
    h = sub_block(fs)
    z = (((sub[:-3] + sub[1:-2]) + sub[2:-1]) + sub[3:]) / (4.0 * h)
    with np.errstate(divide="ignore"):
        l = OFFSET + 10.0 * np.log10(z)
    keep = l > ABSOLUTE_GATE
    if not keep.any():
        return MIN_LOUDNESS
    keep &= l > (OFFSET + 10.0 * np.log10(z[keep].mean())) + RELATIVE_GATE
    return float(OFFSET + 10.0 * np.log10(z[keep].mean()))


def loudness_numpy(x: np.ndarray, fs: int, length: Optional[int] = None) -> float:
    """One window -> LUFS; with `length` the samples from there on count as zeros (the window keeps its size)."""
    x = np.array(x, np.float64).reshape(-1)
    if length is not None:
        x[max(int(length), 0):] = 0.0
    return gate(sub_block_energies(k_filter(x, fs), fs), fs)


def choose(lufs: np.ndarray, cutoff: float) -> np.ndarray:
    """[B, tries] loudness -> [B] the accepted try: the first strictly above the cutoff, else the last."""
    lufs = np.asarray(lufs, np.float64)
    above = lufs > cutoff
    return np.where(above.any(axis=1), above.argmax(axis=1), lufs.shape[1] - 1).astype(np.int64)


def draw(rng: np.random.Generator, clip_lengths: np.ndarray, batch: int, T: int, num_tries: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The draws of ClipPool.sample, in its documented order -> (clip [B], offset [B, tries], lens [B]), all int64:
    c = rng.integers(n_clips, size=B); u = rng.random((B, tries)); offset = floor(u (max(len_c - T, 0) + 1)); lens = min(len_c, T).
    (u < 1, so the offset leaves room for the excerpt; the minimum below only guards the product's rounding for u next to 1.)"""
    clip_lengths = np.asarray(clip_lengths, np.int64)
    c = rng.integers(len(clip_lengths), size=batch)
    u = rng.random((batch, num_tries))
    room = np.maximum(clip_lengths[c] - T, 0) + 1
    offset = np.minimum(np.floor(u * room[:, None]).astype(np.int64), room[:, None] - 1)
    return c.astype(np.int64), offset, np.minimum(clip_lengths[c], T)
