"""The cases of tests/test_gpu_native.py and tests/test_native_cpu.py (a plain module, like fx_contract_cases.py): file rates, channel
counts and clip lengths of the native-rate embed route, seeded inputs, and a float64 restatement of the whole route on the oracle's dense
resampling operator (oracle/wv_oracle_fx.resample_matrix) with the channel mean taken in float64."""
from __future__ import annotations

import functools

import numpy as np

from fx_contract_cases import BAR, resample_geometry, resample_t_max  # noqa: F401  (BAR: the project's filter bar, 2e-5 of the peak)
from oracle import wv_oracle_fx as OF
from waveverify_amd import effects as E

MODEL_RATE = 16000
RATES = [48000, 44100, 32000, 22050, 8000, 16000]           # 8000: the front end up-samples, the back end down-samples; 16000: identity
CHANNELS = [1, 2, 3]                                        # 3: the inexact divide
BATCH = 2
GAINS = [1.0, 0.37]
PEAK = 0.5                                                  # |input| <= 0.5: save_audio's clamp stays idle


def geometry(orig_freq: int, new_freq: int):
    """(orig, nw, L, width) of one direction's table; the one-tap identity for equal rates."""
    if orig_freq == new_freq:
        return 1, 1, 1, 0
    orig, nw, width = resample_geometry(orig_freq, new_freq)
    return orig, nw, 2 * width + orig, width


def lengths(sr: int):
    """Tn per rate: shorter than the filter, both sides of one phase group (of either direction's table), the 256-output tile's edge,
    several tiles, and a length whose 16 kHz copy spans several tiles too."""
    out = {1, 2, 255, 256, 257, 1001, 4801}
    for of, nf in ((sr, MODEL_RATE), (MODEL_RATE, sr)):
        orig, _, _, width = geometry(of, nf)
        out |= {width, orig - 1, orig + 1}
    return sorted(T for T in out if T >= 1)


def cases():
    return [(sr, Tn) for sr in RATES for Tn in lengths(sr)]


def t16(Tn: int, sr: int) -> int:
    return E.resampled_length(Tn, sr, MODEL_RATE)


def inputs(sr: int, C: int, Tn: int):
    """-> (x [BATCH, C, Tn], delta [BATCH, T16]) float32, uniform in [-PEAK, PEAK), seeded by the case."""
    rng = np.random.default_rng([sr, C, Tn])
    x = rng.uniform(-PEAK, PEAK, (BATCH, C, Tn)).astype(np.float32)
    delta = rng.uniform(-PEAK, PEAK, (BATCH, t16(Tn, sr))).astype(np.float32)
    return x, delta


def mono_f32(x: np.ndarray) -> np.ndarray:
    """The front end's channel mean as the kernel states it: f32, summed left to right, one true divide.  [B, C, T] -> [B, T]."""
    acc = x[:, 0].astype(np.float32).copy()
    for c in range(1, x.shape[1]):
        acc = (acc + x[:, c]).astype(np.float32)
    return (acc / np.float32(x.shape[1])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def table(orig_freq: int, new_freq: int):
    """-> (kernels [nw, L] float32, orig, nw, L, width); [[1]] for equal rates."""
    if orig_freq == new_freq:
        return np.ones((1, 1), np.float32), 1, 1, 1, 0
    k, width, orig, nw = E.resample_kernels(orig_freq, new_freq)
    return k, orig, nw, k.shape[1], width


@functools.lru_cache(maxsize=4)
def operator(orig_freq: int, new_freq: int, T_in: int, T_out: int) -> np.ndarray:
    """The dense float64 [T_out, T_in] operator of one direction (the identity's first T_out rows for equal rates)."""
    k, orig, nw, _, width = table(orig_freq, new_freq)
    return OF.resample_matrix(k, T_in, orig, nw, width, T_out)


def front64(x: np.ndarray, sr: int) -> np.ndarray:
    """[B, C, Tn] -> [B, T16] float64: the float64 channel mean through the dense operator."""
    Tn = x.shape[-1]
    return x.astype(np.float64).mean(axis=1) @ operator(sr, MODEL_RATE, Tn, t16(Tn, sr)).T


def up64(delta: np.ndarray, sr: int, Tn: int) -> np.ndarray:
    """[B, T16] -> [B, Tn] float64: the residual at the file's rate, cut to Tn."""
    return delta.astype(np.float64) @ operator(MODEL_RATE, sr, delta.shape[-1], Tn).T


def back64(x: np.ndarray, delta: np.ndarray, sr: int, gain: float) -> np.ndarray:
    """[B, C, Tn] float64: x + gain * up(delta) on every channel."""
    return x.astype(np.float64) + gain * up64(delta, sr, x.shape[-1])[:, None, :]
