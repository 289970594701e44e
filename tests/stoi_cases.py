"""The float64 oracle of STOI (Taal et al. 2011, non-extended) and the case list the CPU and GPU tests share (a plain module:
`from stoi_cases import ...`).

The oracle is written from the published algorithm, stage by stage as pystoi lays it out -- resample, remove silent frames by
overlap-add, frame again, rfft, third-octave bands, 30-frame segments -- and shares no code with waveverify_amd/stoi.py, which uses the
gather form the kernels use.  pystoi itself is not available here, so parity with an installed `pystoi` stays unpinned; scipy, where
present, pins the resampler.  `dtype=np.float32` runs every stage but the DFT in float32 (what a float32 kernel can at best reach);
`bands=` and `n_seg=` exist so that a test can break the oracle and see the bars notice.

Cases: clips of tests/golden/speech_T16000.npz (`x`, three clips) against their own watermarked versions (`wm`) or against themselves
plus seeded white noise at a stated SNR, in batches of three clips of one length and rate.
"""
from __future__ import annotations

import math
import os
import warnings
from functools import lru_cache
from typing import Dict, List, NamedTuple, Optional

import numpy as np

FS, N_FRAME, HOP, NFFT, NUMBAND, MINFREQ = 10000, 256, 128, 512, 15, 150
N, BETA, DYN_RANGE = 30, -15.0, 40.0
EPS = np.finfo(np.float64).eps
FRAME_END_EXCLUSIVE = True          # Taal's MATLAB 1:K/2:(length(x)-K); for a pystoi build that ends at len - 256 + 1, flip this one switch
SHORT = 1e-5
W = np.hanning(N_FRAME + 2)[1:-1]

# inclusive bin ranges of the 15 bands on the 512-point grid at 10 kHz, written out
BAND_BINS = ((7, 8), (9, 10), (11, 13), (14, 16), (17, 21), (22, 26), (27, 33), (34, 42), (43, 54), (55, 68), (69, 86), (87, 108),
             (109, 137), (138, 173), (174, 218))


def frame_starts(n: int) -> range:
    return range(0, n - N_FRAME + (0 if FRAME_END_EXCLUSIVE else 1), HOP)


def thirdoct() -> np.ndarray:
    """[15, 257] 0 / 1 band matrix from the centre frequencies, as pystoi's utils.thirdoct builds it."""
    f = np.linspace(0, FS, NFFT + 1)[: NFFT // 2 + 1]
    obm = np.zeros((NUMBAND, len(f)))
    for i in range(NUMBAND):
        lo = int(np.argmin(np.abs(f - MINFREQ * 2.0 ** ((2 * i - 1) / 6))))
        hi = int(np.argmin(np.abs(f - MINFREQ * 2.0 ** ((2 * i + 1) / 6))))
        obm[i, lo:hi] = 1
    return obm


def resample_window(p: int, q: int):
    """Octave's `resample` filter -> (h, half)."""
    fc = 1 / (2 * max(p, q))
    roll = fc / 10
    half = int(math.ceil((60 - 8) / (28.714 * roll)))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60 - 8.7)) * 2 * p * fc * np.sinc(2 * fc * t)
    return h / h.sum(), half


def resample(x: np.ndarray, fs: int, dtype=np.float64) -> np.ndarray:
    """y10[k] = sum_j p h[half + k q - j p] x[j], k < ceil(len p / q): zero-stuff, convolve, take every q-th sample."""
    if fs == FS:
        return np.asarray(x, dtype)
    g = math.gcd(FS, fs)
    p, q = FS // g, fs // g
    h, half = resample_window(p, q)
    up = np.zeros(len(x) * p, dtype)
    up[::p] = x
    full = np.convolve(up, (p * h).astype(dtype))
    n_out = -(-len(x) * p // q)
    idx = half + q * np.arange(n_out)
    return np.where(idx < len(full), full[np.minimum(idx, len(full) - 1)], 0).astype(dtype)


def frame_energies(x10: np.ndarray) -> np.ndarray:
    fr = np.array([W * x10[s: s + N_FRAME] for s in frame_starts(len(x10))], np.float64).reshape(-1, N_FRAME)
    return 20 * np.log10(np.linalg.norm(fr, axis=1) + EPS)


def overlap_add(frames: np.ndarray, dtype) -> np.ndarray:
    out = np.zeros((len(frames) - 1) * HOP + N_FRAME, dtype)
    for i, f in enumerate(frames):
        out[i * HOP: i * HOP + N_FRAME] += f
    return out


def stoi_stages(x: np.ndarray, y: np.ndarray, fs: int, dtype=np.float64, bands: Optional[np.ndarray] = None, n_seg: int = N) -> Dict:
    """x = the clean clip, y = the estimate.  -> d, total / kept frame counts, kept_idx, margins (dB of every frame from the keep
    threshold), x_tob / y_tob [15, J] float64, frames_x / frames_y [J, 256] (the windowed frames the DFT sees), clipped (share of y'
    elements the clipping changes)."""
    obm = thirdoct() if bands is None else bands
    w = W.astype(dtype)
    x10, y10 = resample(np.asarray(x, dtype), fs, dtype), resample(np.asarray(y, dtype), fs, dtype)
    starts = list(frame_starts(len(x10)))
    out: Dict = {"total": len(starts), "x10": x10, "y10": y10}
    if not starts:
        out.update(d=SHORT, kept=0, kept_idx=np.zeros(0, np.int64), margins=np.zeros(0), J=-1)
        warnings.warn("Not enough STFT frames to compute intermediate intelligibility measure after removing silent frames. Returning 1e-5.", RuntimeWarning)
        return out
    e = frame_energies(np.asarray(x10, np.float64))
    margin = e.max() - DYN_RANGE - e
    keep = margin < 0
    kept_idx = np.nonzero(keep)[0]
    out.update(kept=int(keep.sum()), kept_idx=kept_idx, margins=margin)
    xf = np.array([w * x10[s: s + N_FRAME] for s in starts], dtype)[keep]
    yf = np.array([w * y10[s: s + N_FRAME] for s in starts], dtype)[keep]
    xs, ys = overlap_add(xf, dtype), overlap_add(yf, dtype)
    fx = np.array([w * xs[s: s + N_FRAME] for s in frame_starts(len(xs))], dtype).reshape(-1, N_FRAME)
    fy = np.array([w * ys[s: s + N_FRAME] for s in frame_starts(len(ys))], dtype).reshape(-1, N_FRAME)
    J = len(fx)
    out.update(J=J, frames_x=fx, frames_y=fy)
    X, Y = np.fft.rfft(fx.astype(np.float64), NFFT, axis=1).T, np.fft.rfft(fy.astype(np.float64), NFFT, axis=1).T      # [257, J]
    x_tob = np.sqrt(obm @ (np.abs(X) ** 2)).astype(dtype)
    y_tob = np.sqrt(obm @ (np.abs(Y) ** 2)).astype(dtype)
    out.update(x_tob=x_tob.astype(np.float64), y_tob=y_tob.astype(np.float64))
    if J < n_seg:
        warnings.warn("Not enough STFT frames to compute intermediate intelligibility measure after removing silent frames. Returning 1e-5.", RuntimeWarning)
        out.update(d=SHORT, clipped=0.0)
        return out
    x_seg = np.array([x_tob[:, m - n_seg: m] for m in range(n_seg, J + 1)])
    y_seg = np.array([y_tob[:, m - n_seg: m] for m in range(n_seg, J + 1)])
    alpha = np.linalg.norm(x_seg, axis=2, keepdims=True) / (np.linalg.norm(y_seg, axis=2, keepdims=True) + EPS)
    y_norm = y_seg * alpha
    ceiling = x_seg * (1 + 10 ** (-BETA / 20))
    y_prime = np.minimum(y_norm, ceiling)
    out["clipped"] = float((y_norm > ceiling).mean())
    y_prime = y_prime - y_prime.mean(axis=2, keepdims=True)
    x_seg = x_seg - x_seg.mean(axis=2, keepdims=True)
    y_prime = y_prime / (np.linalg.norm(y_prime, axis=2, keepdims=True) + EPS)
    x_seg = x_seg / (np.linalg.norm(x_seg, axis=2, keepdims=True) + EPS)
    out["d"] = float(np.sum(y_prime * x_seg, dtype=np.float64) / (x_seg.shape[0] * x_seg.shape[1]))
    return out


def stoi(x, y, fs, **kw) -> float:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return stoi_stages(x, y, fs, **kw)["d"]


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    fs: int
    x: np.ndarray            # [3, T] float32, the clean clips
    y: np.ndarray            # [3, T] float32, the estimates
    kinds: tuple             # per clip, what y is


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speech_T16000.npz")
QUIET = 1e-4
# per length: where each of the three clips starts in its 16000-sample fixture clip (chosen so that the short clips keep every frame)
SHORT_STARTS = {6553: (2400, 1500, 5200), 6554: (2400, 1500, 5200)}


def _noisy(x: np.ndarray, snr_db: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    n = rng.standard_normal(x.shape)
    n *= np.sqrt((x.astype(np.float64) ** 2).mean() / (n ** 2).mean()) * 10 ** (-snr_db / 20)
    return (x + n).astype(np.float32)


@lru_cache(maxsize=None)
def cases() -> List[Case]:
    g = np.load(GOLDEN)
    x0, wm0 = g["x"][:, 0].astype(np.float32), g["wm"][:, 0].astype(np.float32)
    out: List[Case] = []

    def add(name, fs, sl, kinds, x_src=x0):
        xs, ys = [], []
        for c, (kind, s) in enumerate(zip(kinds, sl)):
            xc = x_src[c][s]
            if kind == "wm":
                yc = xc + (wm0[c][s] - x0[c][s])                # the watermark of that stretch, on top of whatever x is here
            else:
                yc = _noisy(xc, float(kind[1:]), 100 * len(out) + c)
            xs.append(xc)
            ys.append(yc.astype(np.float32))
        out.append(Case(name, fs, np.stack(xs), np.stack(ys), tuple(kinds)))

    full = (slice(0, 16000),) * 3
    add("T16000", 16000, full, ("wm", "n20", "n0"))
    # 16001 samples: the clip and the first sample of the next one
    x1 = np.stack([np.concatenate([x0[c], x0[(c + 1) % 3][:1]]) for c in range(3)])
    add("T16001", 16000, (slice(0, 16001),) * 3, ("n20", "n5", "n0"), x_src=x1)
    add("T8000", 16000, (slice(4000, 12000),) * 3, ("wm", "n5", "n20"))
    for T in (6553, 6554):
        add(f"T{T}", 16000, tuple(slice(s, s + T) for s in SHORT_STARTS[T]), ("wm", "n20", "n0"))
    add("fs10000", 10000, (slice(2000, 10000),) * 3, ("wm", "n20", "n0"))
    add("fs8000", 8000, (slice(2000, 10000),) * 3, ("wm", "n5", "n0"))
    # a stretch scaled by 1e-4 at the start, in the middle, at the end: leading, interior (consecutive) and trailing frames go
    xq = x0.copy()
    xq[0, :3000] *= QUIET
    xq[1, 7000:10000] *= QUIET
    xq[2, 13000:] *= QUIET
    add("quiet", 16000, full, ("n20", "n20", "n20"), x_src=xq)
    return out


@lru_cache(maxsize=None)
def oracle(name: str):
    """The float64 stages of every clip of a case, computed once."""
    c = next(k for k in cases() if k.name == name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return [stoi_stages(c.x[b], c.y[b], c.fs) for b in range(3)]
