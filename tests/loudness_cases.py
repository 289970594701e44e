"""The float64 oracle of ITU-R BS.1770-4 gated loudness (one channel) and the case list the CPU and GPU tests share (a plain module:
`from loudness_cases import ...`).

The oracle restates the standard on its own -- the K-weighting table by the bilinear transform from the analog prototypes, the filter
by scipy.signal.sosfilt, the gating in numpy -- and shares no code with waveverify_amd/loudness.py.  audiotools and pyloudnorm are not
available here, so parity with audiotools' `Meter` stays unpinned.

Cases: for every (fs, T) of SHAPES one batch of windows of T samples -- seeded noise at rms 0.1; the same noise with its second half
scaled by 1e-3 (those blocks fall under the absolute gate) and by 1e-2 (they pass it and fall under the relative gate); a full-scale
997 Hz sine; zeros; the noise with only its first T // 2 samples valid; unit impulses at 0, chunk - 1, chunk, chunk + 1 for the
kernel's chunk length and at T - 1."""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Dict, List, NamedTuple, Optional

import numpy as np

SHAPES = ((16000, 6400), (16000, 6401), (16000, 7999), (16000, 8000), (16000, 16000), (16000, 16001), (16000, 48000), (48000, 19200),
          (44100, 22050))
MIN_LOUDNESS = -70.0


def sos(fs: int) -> np.ndarray:
    """[2, 6] K-weighting in scipy's sos layout, from the analog prototypes with K = tan(pi f0 / fs)."""
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 1.0, 2 * (K * K - 1) / a0,
             (1 - K / Q + K * K) / a0]
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1 + K / Q + K * K
    return np.array([shelf, [1.0, -2.0, 1.0, 1.0, 2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0]], np.float64)


def oracle(x: np.ndarray, fs: int, length: Optional[int] = None) -> Dict:
    """One window (samples from `length` on count as zeros) -> filtered [T], sub [T // h], l [blocks], gates (absolute, relative or
    None), lufs."""
    from scipy.signal import sosfilt
    if fs % 10:
        raise ValueError("fs % 10 != 0")
    h = fs // 10
    x = np.array(x, np.float64)
    if length is not None:
        x[length:] = 0.0
    nsub = len(x) // h
    if nsub < 4:
        raise ValueError("shorter than one block")
    y = sosfilt(sos(fs), x)
    sub = (y[: nsub * h].reshape(nsub, h) ** 2).sum(axis=1)
    z = np.array([sub[j: j + 4].sum() / (4 * h) for j in range(nsub - 3)])
    with np.errstate(divide="ignore"):
        l = -0.691 + 10 * np.log10(z)
    keep = l > -70.0
    out = {"filtered": y, "sub": sub, "l": l, "relative_gate": None}
    if not keep.any():
        out["lufs"] = MIN_LOUDNESS
        return out
    out["relative_gate"] = (-0.691 + 10 * np.log10(z[keep].mean())) - 10.0
    keep &= l > out["relative_gate"]
    out["lufs"] = float(-0.691 + 10 * np.log10(z[keep].mean()))
    return out


def loudness(x: np.ndarray, fs: int, length: Optional[int] = None) -> float:
    return oracle(x, fs, length)["lufs"]


class Case(NamedTuple):
    name: str
    fs: int
    T: int
    x: np.ndarray            # [N, T] float32
    lens: np.ndarray         # [N] int32
    labels: List[str]


def chunk() -> int:
    from waveverify_amd import _lib
    return int(_lib.load().wv_loudness_chunk())


@lru_cache(maxsize=None)
def cases() -> List[Case]:
    out = []
    c = chunk()
    for i, (fs, T) in enumerate(SHAPES):
        rng = np.random.default_rng(1000 + i)
        noise = (0.1 * rng.standard_normal(T)).astype(np.float32)
        rows, lens, labels = [], [], []

        def add(label, row, n=T):
            rows.append(np.asarray(row, np.float32))
            lens.append(n)
            labels.append(label)

        add("noise", noise)
        for label, scale in (("quiet_half_1e-3", 1e-3), ("quiet_half_1e-2", 1e-2)):
            q = noise.copy()
            q[T // 2:] *= np.float32(scale)
            add(label, q)
        add("sine997", np.sin(2 * np.pi * 997.0 * np.arange(T) / fs))
        add("zeros", np.zeros(T))
        add("half_valid", noise, T // 2)
        for at in sorted({0, c - 1, c, c + 1, T - 1}):
            if at < T:
                imp = np.zeros(T)
                imp[at] = 1.0
                add(f"impulse@{at}", imp)
        out.append(Case(f"fs{fs}_T{T}", fs, T, np.stack(rows), np.array(lens, np.int32), labels))
    return out


@lru_cache(maxsize=None)
def reference(name: str) -> List[Dict]:
    """The oracle on every window of a case, computed once."""
    k = next(k for k in cases() if k.name == name)
    return [oracle(k.x[n], k.fs, int(k.lens[n])) for n in range(len(k.x))]
