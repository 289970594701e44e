"""The per-channel SNR floor at a file's own rate (csrc/wv_channel_floor.hip): the floor of snr_floor.py held on every
ORIGINAL channel of a native-rate file, on the native time line, where the residual is added.

x [C, Tn] are the original channels, u [Tn] the residual already brought to the native rate (wv_native_upsample_add's chain, cut to Tn),
orig : nw the resampler's reduced ratio 16 kHz -> native, hop the generator's hop.  Frames are the 16 kHz floor's frames seen from the native
time line: native sample m belongs to frame (m * orig) // (nw * hop), so frame f is [start(f), start(f + 1)) with start(f) =
ceil(f * nw * hop / orig); lengths differ by at most one and a short last frame occurs only at the true end.  Per frame and channel, in
float64 and in snr_floor.frame_energy's fixed order (k counted inside the native frame), Ex[c, f] = sum x[c]^2 and Eu[f] = sum u^2;
g[c, f] follows snr_floor.frame_gains' rule; the weight rises over one frame along ramp_f[k] = float32((k + 1) / L_f), L_f the frame's own
nominal length, and drops at once; v = w * u, out[c] = x[c] + v with x's own bits where v is +0 or -0.

numpy_channel_floor is the definition: the kernel matches it bit for bit.  There is no CPU path for the route itself (native.upsample_add_floor)."""
from __future__ import annotations

from typing import Tuple

import numpy as np

MAX_FRAME = 4096        # WV_CHANNEL_FLOOR_MAX_FRAME
LDS_FLOATS = 15360      # WV_CHANNEL_FLOOR_LDS_FLOATS


def frame_starts(Tn: int, orig: int, nw: int, hop: int) -> np.ndarray:
    """-> [F + 1] int64: start(f) = ceil(f * nw * hop / orig) for f = 0 .. F, F = ((Tn - 1) * orig) // (nw * hop) + 1 the frames a row of Tn
    native samples touches.  start(F) is the NOMINAL end of the last frame and may lie past Tn."""
    Tn, orig, nw, hop = int(Tn), int(orig), int(nw), int(hop)
    if Tn < 1 or orig < 1 or nw < 1 or hop < 1:
        raise ValueError("Tn, orig, nw and hop must be >= 1")
    M = nw * hop
    F = ((Tn - 1) * orig) // M + 1
    f = np.arange(F + 1, dtype=np.int64)
    return (f * M + orig - 1) // orig


def frame_of(m, orig: int, nw: int, hop: int) -> np.ndarray:
    """The frame of native sample m: (m * orig) // (nw * hop) in int64."""
    return (np.asarray(m, np.int64) * int(orig)) // (int(nw) * int(hop))


def frame_energy_var(a: np.ndarray, starts: np.ndarray) -> np.ndarray:
    """snr_floor.frame_energy for frames of unequal length: a [n] float32, frame f = a[starts[f] : min(starts[f + 1], n)] -> [F] float64,
    sample k of a frame to partial (k >> 2) & 15, each partial in ascending k from +0.0, folded ^8, ^4, ^2, ^1.  An empty frame gives 0."""
    n = int(a.shape[0])
    st = np.minimum(np.asarray(starts, np.int64), n)
    F = len(st) - 1
    if F <= 0:
        return np.zeros(0, np.float64)
    lens = st[1:] - st[:-1]
    m = max(-(-int(lens.max()) // 64), 1)
    k = np.arange(m * 64, dtype=np.int64)
    idx = st[:-1, None] + k[None, :]
    live = k[None, :] < lens[:, None]
    d = np.concatenate([a.astype(np.float64), [0.0]])
    sq = d[np.where(live, idx, n)]                                  # +0.0 past a frame's end: no bit of a non-negative sum changes
    sq = (sq * sq).reshape(F, m, 16, 4)
    p = np.zeros((F, 16), np.float64)
    for i in range(m):
        for q in range(4):
            p = p + sq[:, i, :, q]
    for h in (8, 4, 2, 1):
        p = p[:, :h] + p[:, h:2 * h]
    return p[:, 0]


def gains_of(Ex: np.ndarray, Eu: np.ndarray, s, rho: float) -> np.ndarray:
    """snr_floor.frame_gains' rule on energies: Ex [..., F], Eu [F] float64 -> g float32."""
    s = np.float32(s)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = np.sqrt((np.float64(rho) * Ex) / Eu)
        g = np.where(q < np.float64(s), q.astype(np.float32), s)
    return np.where(Eu == 0.0, s, g).astype(np.float32)


def numpy_channel_floor(x: np.ndarray, u: np.ndarray, orig: int, nw: int, hop: int, s, rho: float, add: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """The definition: x [C, Tn] float32, u [Tn] float32 -> (out [C, Tn] float32, g [C, F] float32)."""
    x = np.asarray(x, np.float32)
    u = np.asarray(u, np.float32)
    C, Tn = x.shape
    if u.shape != (Tn,):
        raise ValueError(f"u must have shape ({Tn},), got {u.shape}")
    st = frame_starts(Tn, orig, nw, hop)
    Eu = frame_energy_var(u, st)
    g = np.stack([gains_of(frame_energy_var(x[c], st), Eu, s, rho) for c in range(C)])
    m = np.arange(Tn, dtype=np.int64)
    f = frame_of(m, orig, nw, hop)
    k = m - st[f]
    Lf = (st[1:] - st[:-1])[f]
    ramp = ((k + 1).astype(np.float64) / Lf.astype(np.float64)).astype(np.float32)
    out = np.empty_like(x)
    for c in range(C):
        G = g[c][f]
        P = g[c][np.maximum(f - 1, 0)]
        with np.errstate(invalid="ignore", over="ignore"):
            up = P + (G - P) * ramp                                    # f32 throughout: three roundings
            w = np.where(P < G, np.where(up < G, up, G), G).astype(np.float32)
            v = (w * u).astype(np.float32)
            out[c] = np.where(v == 0, x[c], x[c] + v).astype(np.float32) if add else v
    return out, g


def numpy_floor_frames(x: np.ndarray, u: np.ndarray, starts: np.ndarray, s, rho: float, gprev=None) -> Tuple[np.ndarray, np.ndarray]:
    """numpy_channel_floor on a STRETCH of a stream that begins at a frame's start (the live route): x [C, n], u [n],
    starts [F + 1] the nominal starts of the stretch's frames counted from its sample 0 (the last frame is cut at n), gprev [C] the gains of the
    frame before the stretch, None where the stretch begins the stream (frame 0 takes its own) -> (out [C, n], g [C, F]).  Every sample and
    gain has the bits numpy_channel_floor gives it on the whole stream."""
    x = np.asarray(x, np.float32)
    u = np.asarray(u, np.float32)
    st = np.asarray(starts, np.int64)
    C, n = x.shape
    F = len(st) - 1
    if F <= 0:
        return np.empty((C, 0), np.float32), np.empty((C, 0), np.float32)
    Eu = frame_energy_var(u, st)
    g = np.stack([gains_of(frame_energy_var(x[c], st), Eu, s, rho) for c in range(C)])
    before = np.concatenate([g[:, :1] if gprev is None else np.asarray(gprev, np.float32).reshape(C, 1), g[:, :-1]], axis=1)
    m = np.arange(n, dtype=np.int64)
    f = np.searchsorted(st, m, side="right") - 1                           # the frame that holds m: empty frames hold nothing
    k = m - st[f]
    Lf = (st[1:] - st[:-1])[f]
    ramp = ((k + 1).astype(np.float64) / Lf.astype(np.float64)).astype(np.float32)
    out = np.empty_like(x)
    for c in range(C):
        G, P = g[c][f], before[c][f]
        with np.errstate(invalid="ignore", over="ignore"):
            up = P + (G - P) * ramp
            w = np.where(P < G, np.where(up < G, up, G), G).astype(np.float32)
            v = (w * u).astype(np.float32)
            out[c] = np.where(v == 0, x[c], x[c] + v).astype(np.float32)
    return out, g


def native_frame_snr_db(x: np.ndarray, v: np.ndarray, orig: int, nw: int, hop: int) -> np.ndarray:
    """10 log10(Ex / sum v^2) per native frame of ONE channel in float64 (plain sums); +inf where the frame carries no watermark."""
    Tn = len(x)
    st = np.minimum(frame_starts(Tn, orig, nw, hop), Tn)
    ex = np.array([np.sum(np.asarray(x[a:b], np.float64) ** 2) for a, b in zip(st[:-1], st[1:])])
    ev = np.array([np.sum(np.asarray(v[a:b], np.float64) ** 2) for a, b in zip(st[:-1], st[1:])])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ev == 0, np.inf, 10.0 * np.log10(ex / ev))
