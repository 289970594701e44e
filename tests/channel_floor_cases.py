"""Cases of the per-channel SNR floor tests (tests/test_channel_floor_cpu.py, tests/test_gpu_channel_floor.py): a plain module, fixed seeds,
importable without a GPU.

CASES            the raw geometries of wv_native_floor_up_add: rates chosen for their frame shapes (48000: 3:1, exact frames; 44100: 441:160,
                 exact 882; 11025: unequal frames 220 / 221; 8000: downward; 16000: the identity table), tiny hops so that frame edges are
                 cheap (hops 1, 3, 4, 7 at 8 kHz: frames of 0-1, 1-2, 2 and 3-4 samples), hop 320 once per rate, C in {1, 2, 3, 64}, B in
                 {1, 5}, Tn a whole number of frames, ending inside a frame, shorter than one frame, and 1
inputs(case)     x [B, C, Tn], delta [B, T16], strengths [B]: per-frame envelopes over 1e-3 .. 1 (well above the f32 denormal range), a silent
                 channel (all +0, in one case all -0), a stretch of delta == 0 wide enough that whole frames of u are exactly zero, frames loud
                 enough that the cap holds, rising and falling gains, per-row strengths including 0
up64 / route64   the float64 restatement of the back end and of the whole floored route"""
from __future__ import annotations

import math

import numpy as np

import native_cases as NC
import window_cases as W
from waveverify_amd import channel_floor as CF
from waveverify_amd import native

MIN_SNR_DB = 20.0
FLOORS = (10.0, 20.0, 40.0)
# The guarantee's bar.  Ex and Eu are float64 sums of exact products (relative error ~1e-16, nothing here); q = sqrt(rho Ex / Eu) likewise.
# The f32 roundings of the path: g = float32(q) <= q (1 + 2^-24); the weight never exceeds g; v = float32(w u), |v| <= g |u| (1 + 2^-24).  So
# sum v^2 <= q^2 Eu (1 + 2^-24)^4 = rho Ex (1 + 2^-24)^4, at most 4 * 10 log10(1 + 2^-24) = 1.04e-6 dB under the floor.  The issue allows a
# unit in the last place where this counts half of one: 4 * 10 log10(1 + 2^-23) = 2.07e-6 dB, and that is the bar held.
BOUND_DB = 4 * 10.0 * math.log10(1.0 + 2.0 ** -23)
STRENGTHS5 = (1.0, 0.75, 0.0, 0.5, 1.0)

# (name, sample rate, hop, C, B, Tn, silent channel or None, sign of the silence)
CASES = [
    ("8k.hop1", 8000, 1, 1, 1, 37, None, 0),
    ("8k.hop3.rows", 8000, 3, 2, 5, 50, 1, 0),                    # 34 frames of 1-2 samples: three tiles of 16 frames
    ("8k.hop4.whole", 8000, 4, 3, 1, 64, 2, 0),                   # 32 whole frames of 2
    ("8k.hop7.inside", 8000, 7, 2, 1, 45, 0, 1),                  # frames of 3-4, ends inside one; the silent channel is all -0
    ("8k.hop320", 8000, 320, 2, 1, 3 * 160 + 17, 1, 0),
    ("48k.hop320.rows", 48000, 320, 2, 5, 3 * 960 + 100, 1, 0),
    ("48k.hop320.tiles", 48000, 320, 2, 1, 9 * 960 + 3, None, 0),  # more frames than one tile holds
    ("48k.hop12.c64", 48000, 12, 64, 1, 20 * 36, 5, 0),           # a whole number of frames
    ("48k.short", 48000, 320, 1, 1, 500, None, 0),                # shorter than one frame
    ("48k.one", 48000, 320, 2, 1, 1, 1, 0),                       # Tn = 1
    ("44k.hop320", 44100, 320, 3, 1, 2 * 882 + 5, 1, 0),
    ("44k.hop4", 44100, 4, 2, 1, 300, None, 0),                   # frames of 11 and 12
    ("11k.hop320.rows", 11025, 320, 2, 5, 883, 0, 0),             # frames of 220 and 221, ends at a frame's edge
    ("11k.hop5", 11025, 5, 1, 1, 200, None, 0),                   # frames of 3 and 4
    ("16k.hop320", 16000, 320, 2, 1, 700, 1, 0),
    ("16k.hop12.rows", 16000, 12, 3, 5, 12 * 9 + 1, 2, 0),
]
IDS = [c[0] for c in CASES]


def case(name):
    return CASES[IDS.index(name)]


def geometry(sr: int):
    """(orig, nw, L, width) of the back end's table, 16 kHz -> sr."""
    return native.table_geometry(NC.MODEL_RATE, sr)


def _envelope(rng, F, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), F))


def inputs(c):
    """-> (x [B, C, Tn] float32, delta [B, T16] float32, strengths [B] float32)."""
    name, sr, hop, C, B, Tn, silent, sign = c
    rng = np.random.default_rng(W.seed_of("channel floor", name))
    orig, nw, _, _ = geometry(sr)
    T16 = NC.t16(Tn, sr)
    f16 = np.arange(T16) // hop
    st = CF.frame_starts(Tn, orig, nw, hop)
    F = len(st) - 1
    fn = CF.frame_of(np.arange(Tn), orig, nw, hop)
    x = np.empty((B, C, Tn), np.float32)
    for b in range(B):
        for ch in range(C):
            x[b, ch] = rng.standard_normal(Tn) * _envelope(rng, F, 1e-3, 1.0)[fn]
    delta = np.stack([rng.standard_normal(T16) * _envelope(rng, f16[-1] + 1, 1e-2, 0.3)[f16] for _ in range(B)]).astype(np.float32)
    a = hop * -(-(T16 // 3) // hop) - 30                          # u == 0 over a whole frame: delta is zero over the frame that starts 30
    if 0 <= a < T16:                                              # samples later and 30 past its end, more than the filter's reach
        delta[:, a:a + 2 * hop + 60] = 0.0
    if silent is not None:
        x[:, silent] = -0.0 if sign else 0.0
    s = np.array(STRENGTHS5[:B] if B > 1 else (1.0,), np.float32)
    return x, delta, s


def resample64(sig: np.ndarray, of: int, nf: int, Tout: int) -> np.ndarray:
    """[..., T] at `of` Hz -> [..., Tout] at `nf` Hz in float64: y[m] = sum_j K[m % nw][j] * sig_z[(m // nw) * orig - width + j], the signal
    zero outside its length (native_cases' dense operator, without building it)."""
    k, orig, nw, L, width = NC.table(of, nf)
    k = k.astype(np.float64)
    d = np.asarray(sig, np.float64)
    T = d.shape[-1]
    m = np.arange(Tout)
    idx = (m // nw)[:, None] * orig - width + np.arange(L)[None, :]
    ok = (idx >= 0) & (idx < T)
    dz = np.concatenate([d, np.zeros(d.shape[:-1] + (1,))], axis=-1)
    return (dz[..., np.where(ok, idx, T)] * k[m % nw]).sum(-1)


def up64(delta: np.ndarray, sr: int, Tn: int) -> np.ndarray:
    """[..., T16] -> [..., Tn] float64: the residual at the file's rate, cut to Tn."""
    return resample64(delta, NC.MODEL_RATE, sr, Tn)


def down64(x: np.ndarray, sr: int) -> np.ndarray:
    """[..., C, Tn] -> [..., T16] float64: the float64 channel mean at 16 kHz."""
    return resample64(np.asarray(x, np.float64).mean(axis=-2), sr, NC.MODEL_RATE, NC.t16(x.shape[-1], sr))


def floor64(x: np.ndarray, u: np.ndarray, sr: int, hop: int, s: float, rho: float, add: bool = True):
    """The twin's formula in float64 on a float64 residual: plain sums, no f32 rounding anywhere.  x [C, Tn], u [Tn] -> (out [C, Tn], g [C, F])."""
    x64, u64 = np.asarray(x, np.float64), np.asarray(u, np.float64)
    C, Tn = x64.shape
    orig, nw, _, _ = geometry(sr)
    st = CF.frame_starts(Tn, orig, nw, hop)
    cut = np.minimum(st, Tn)
    F = len(st) - 1
    Eu = np.array([np.sum(u64[a:b] ** 2) for a, b in zip(cut[:-1], cut[1:])])
    Ex = np.array([[np.sum(x64[c, a:b] ** 2) for a, b in zip(cut[:-1], cut[1:])] for c in range(C)])
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(Eu == 0, s, np.minimum(s, np.sqrt(rho * Ex / Eu)))
    f = CF.frame_of(np.arange(Tn), orig, nw, hop)
    k = np.arange(Tn) - st[f]
    ramp = (k + 1.0) / (st[1:] - st[:-1])[f]
    G, P = g[:, f], g[:, np.maximum(f - 1, 0)]
    w = np.where(P < G, np.minimum(G, P + (G - P) * ramp), G)
    v = w * u64
    assert F == g.shape[1]
    return (x64 + v if add else v), g


def kinds_of(g: np.ndarray, Eu: np.ndarray, s) -> set:
    """Which kinds of frames a gains trace [C, F] holds."""
    out = set()
    live = Eu > 0
    if (g[:, live] < s).any():
        out.add("capped")
    if s > 0 and (g[:, live] == s).any():
        out.add("uncapped")
    if (np.diff(g, axis=1) > 0).any():
        out.add("rising")
    if (np.diff(g, axis=1) < 0).any():
        out.add("falling")
    if (~live).any():
        out.add("u=0")
    return out
