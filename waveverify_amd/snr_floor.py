"""The SNR floor of embedding (csrc/wv_snr_floor.hip): in no frame of `frame` samples is the watermark louder than
min_snr_db below the programme, and silence stays silent.

x is the 16 kHz model input, r the generator's residual for it.  Frames of L samples are counted from the stream's sample 0 (a short last
frame only at its true end).  Per frame, in float64, Ex = sum x^2 and Er = sum r^2 IN ONE FIXED ORDER (frame_energy); the frame's gain is
g = s where Er == 0, else min(s, sqrt(rho * Ex / Er)) rounded to f32, rho = 10^(-min_snr_db / 10); it rises over one frame along
ramp[k] = float32((k + 1) / L) and drops at once, so the weight of a sample never exceeds its frame's gain; v = w * r, and with `add` the
output is x + v, x's own bits where v is +0 or -0.

numpy_snr_floor is the definition (the kernel's twin, bit for bit, skip rules included); apply runs the kernel, one launch for any mix of
rows.  There is no CPU fallback."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

DESC = 8            # int64 per descriptor row: {x offset, r offset, out offset, n, strength bits, state index or -1, fresh, gains offset or -1}
MAX_FRAME = 1048576  # WV_SNR_FLOOR_MAX_FRAME


def check_db(v) -> Optional[float]:
    """None (no floor) or a finite float; anything else raises ValueError."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"min_snr_db must be None or a finite number, got {v!r}")
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"min_snr_db must be None or a finite number, got {v!r}")
    return v


def rho_of(min_snr_db: float) -> float:
    """10^(-min_snr_db / 10) in float64."""
    db = check_db(min_snr_db)
    if db is None:
        raise ValueError("min_snr_db is None: there is no floor to apply")
    rho = 10.0 ** (-db / 10.0)
    if not (math.isfinite(rho) and rho > 0.0):
        raise ValueError(f"min_snr_db {db} dB is outside what float64 holds as a power ratio")
    return rho


def floor_ramp(frame: int) -> np.ndarray:
    """ramp[k] = float32((k + 1) / L), formed in float64 and rounded once."""
    L = int(frame)
    if L != frame or not 1 <= L <= MAX_FRAME:
        raise ValueError(f"frame must be an integer in [1, {MAX_FRAME}]")
    return ((np.arange(L, dtype=np.float64) + 1.0) / L).astype(np.float32)


def strength_bits(s) -> int:
    """The f32 bits of a strength as the descriptor carries them."""
    return int(np.array(s, np.float32).view(np.uint32))


def frame_energy(a: np.ndarray, L: int) -> np.ndarray:
    """a [n] float32 -> [ceil(n / L)] float64, the sum of squares of every frame in the kernel's order: sample k of a frame goes to partial
    (k >> 2) & 15, each partial adds its squares in ascending k from +0.0, and the 16 partials are folded p[j] += p[j ^ 8], ^ 4, ^ 2, ^ 1.
    (Padding a frame with zeros adds +0.0 to sums that are never negative: no bit changes.)"""
    n = int(a.shape[0])
    F = -(-n // L)
    if F == 0:
        return np.zeros(0, np.float64)
    m = -(-L // 64)
    sq = np.zeros((F, m * 64), np.float64)
    full = n // L
    d = a.astype(np.float64)
    sq[:full, :L] = d[:full * L].reshape(full, L)
    if full < F:
        sq[full, :n - full * L] = d[full * L:]
    sq = (sq * sq).reshape(F, m, 16, 4)
    p = np.zeros((F, 16), np.float64)
    for i in range(m):
        for q in range(4):
            p = p + sq[:, i, :, q]
    for h in (8, 4, 2, 1):
        p = p[:, :h] + p[:, h:2 * h]
    return p[:, 0]


def frame_gains(x: np.ndarray, r: np.ndarray, s, rho: float, L: int) -> np.ndarray:
    """-> g [F] float32: s where Er == 0, else q < s ? float32(q) : s with q = sqrt((rho * Ex) / Er) in float64."""
    s = np.float32(s)
    Ex, Er = frame_energy(x, L), frame_energy(r, L)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = np.sqrt((np.float64(rho) * Ex) / Er)
        g = np.where(q < np.float64(s), q.astype(np.float32), s)
    return np.where(Er == 0.0, s, g).astype(np.float32)


def floor_row(x: np.ndarray, r: np.ndarray, s, rho: float, ramp: np.ndarray, g_prev=None, add: bool = True):
    """One row of the twin: x, r [n] float32 -> (out [n] float32, g [F] float32).  g_prev: the gain of the stream's previous frame, None for
    none.  The row's last gain, g[-1], is what the next piece of the same stream takes as its g_prev."""
    L = int(ramp.shape[0])
    n = int(x.shape[0])
    g = frame_gains(x, r, s, rho, L)
    if n == 0:
        return np.zeros(0, np.float32), g
    gp = np.concatenate([[g[0] if g_prev is None else np.float32(g_prev)], g[:-1]]).astype(np.float32)
    f = np.arange(n) // L
    k = np.arange(n) - f * L
    G, P = g[f], gp[f]
    with np.errstate(invalid="ignore", over="ignore"):
        up = P + (G - P) * ramp[k]                                     # f32 throughout: three roundings
        w = np.where(P < G, np.where(up < G, up, G), G).astype(np.float32)
        v = w * r
        out = np.where(v == 0, x, x + v).astype(np.float32) if add else v.astype(np.float32)
    return out, g


def row_ok(row, n_x: int, n_r: int, n_out: int, n_max: int, n_state: int, n_gains: int, L: int) -> bool:
    """Whether wv_snr_floor serves a descriptor row (it skips any other whole)."""
    xo, ro, oo, n, sb, si, _, go = (int(v) for v in row)
    if not (0 <= sb <= 0xFFFFFFFF and 0 <= n <= n_max):
        return False
    s = np.array(sb, np.uint32).view(np.float32)
    if not (np.isfinite(s) and s >= 0):
        return False
    if not (0 <= xo <= n_x - n and 0 <= ro <= n_r - n and 0 <= oo <= n_out - n and -1 <= si < n_state):
        return False
    return go == -1 or (go >= 0 and go + -(-n // L) <= n_gains)


def numpy_snr_floor(x, r, out, desc, n_max: int, gstate, gains, ramp, rho: float, add: bool):
    """Reference of wv_snr_floor on host arrays: x, r, out flat float32; desc rows of DESC int64; gstate / gains float32 arrays or None.
    Writes out, gstate and gains in place as the kernel does (a skipped row and a row of n == 0 write nothing) and returns out."""
    L = int(ramp.shape[0])
    n_state = 0 if gstate is None else int(gstate.shape[0])
    n_gains = 0 if gains is None else int(gains.shape[0])
    for row in np.asarray(desc, np.int64).reshape(-1, DESC):
        if not row_ok(row, int(x.shape[0]), int(r.shape[0]), int(out.shape[0]), n_max, n_state, n_gains, L):
            continue
        xo, ro, oo, n, sb, si, fresh, go = (int(v) for v in row)
        if n == 0:
            continue
        s = np.array(sb, np.uint32).view(np.float32)
        g_prev = gstate[si] if si >= 0 and not fresh else None
        o, g = floor_row(x[xo:xo + n], r[ro:ro + n], s, rho, ramp, g_prev, add)
        out[oo:oo + n] = o
        if si >= 0:
            gstate[si] = g[-1]
        if go >= 0:
            gains[go:go + len(g)] = g
    return out


def frame_snr_db(x: np.ndarray, v: np.ndarray, L: int) -> np.ndarray:
    """10 log10(Ex / sum v^2) per frame in float64 (plain sums); +inf where the frame carries no watermark."""
    n = len(x)
    F = -(-n // L)
    pad = F * L - n
    ex = (np.pad(x.astype(np.float64), (0, pad)) ** 2).reshape(F, L).sum(1)
    ev = (np.pad(v.astype(np.float64), (0, pad)) ** 2).reshape(F, L).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ev == 0, np.inf, 10.0 * np.log10(ex / ev))


def _rows(x):
    """x [B,1,T] / [B,T] or a list of 1-D tensors -> (kind, list of 1-D views)."""
    if hasattr(x, "dim"):
        if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[1] != 1):
            raise ValueError(f"expected audio of shape [B,1,T] or a list of 1-D clips, got {tuple(x.shape)}")
        return "batch", [x[b].reshape(-1) for b in range(x.shape[0])]
    if not len(x):
        raise ValueError("no clips")
    return "list", [c.reshape(-1) for c in x]


def apply(x, residual, min_snr_db: float, strength=1.0, frame: int = 320, add: bool = True, return_gains: bool = False):
    """The floor on the device, one launch: x [B,1,T] (or [B,T]) or a list of 1-D tensors, residual the same kind and lengths -> the same
    kind: x + w * residual (add=False: w * residual alone).  strength: one number or one per row, finite and >= 0.  frame: the generator's
    hop_length.  Every row is a whole stream: frames from its sample 0, no state carried in.
    return_gains: also the gains, [B, F] for a batch or a list of [F_b], one per frame: where they are below `strength` the watermark was
    turned down."""
    import torch

    from . import _lib
    rho = rho_of(min_snr_db)
    ramp = floor_ramp(frame)
    L = int(frame)
    kind, xs = _rows(x)
    kind_r, rs = _rows(residual)
    if kind != kind_r or [int(a.numel()) for a in xs] != [int(a.numel()) for a in rs]:
        raise ValueError("x and residual must be the same kind and lengths")
    B = len(xs)
    if B > 65535:
        raise ValueError("at most 65535 rows per call")
    s = np.broadcast_to(np.asarray(strength, np.float64), (B,)) if np.ndim(strength) == 0 else np.asarray(strength, np.float64).reshape(-1)
    if s.shape[0] != B or not (np.isfinite(s).all() and (s >= 0).all()):
        raise ValueError("strength must be finite and >= 0, one number or one per row")
    if not xs[0].is_cuda:
        raise RuntimeError("waveverify_amd has no CPU path: x must be on the GPU")
    device = xs[0].device
    lengths = [int(a.numel()) for a in xs]
    with torch.cuda.device(device):
        if kind == "batch":
            xf = _lib.dev(x, "x must be on the GPU").reshape(-1)
            rf = _lib.dev(residual, "residual must be on the GPU").reshape(-1)
        else:
            xf = torch.cat([_lib.dev(a, "x must be on the GPU") for a in xs])
            rf = torch.cat([_lib.dev(a, "residual must be on the GPU") for a in rs])
        bases = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        frames = [-(-n // L) for n in lengths]
        gb = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
        table = np.empty((B, DESC), np.int64)
        table[:, 0] = table[:, 1] = table[:, 2] = bases[:-1]
        table[:, 3] = lengths
        table[:, 4] = s.astype(np.float32).view(np.uint32)
        table[:, 5] = -1
        table[:, 6] = 1
        table[:, 7] = gb[:-1] if return_gains else -1
        # the ramp rides behind the descriptors as raw bytes: ONE upload per call
        blob = np.concatenate([table.reshape(-1).view(np.uint8), ramp.view(np.uint8)])
        blob_t = torch.from_numpy(blob).to(device)
        desc_p = blob_t.data_ptr()
        ramp_p = desc_p + table.nbytes
        out = torch.empty_like(xf)
        gains = torch.zeros(max(int(gb[-1]), 1), dtype=torch.float32, device=device) if return_gains else None
        _lib.check(_lib.load().wv_snr_floor(xf.data_ptr(), xf.numel(), rf.data_ptr(), rf.numel(), out.data_ptr(), out.numel(), desc_p, B,
                                            max(lengths), None, 0, _lib.ptr(gains), int(gb[-1]) if return_gains else 0, ramp_p, L, rho,
                                            1 if add else 0, _lib.stream()), "wv_snr_floor")
        if kind == "batch":
            res = out.view(B, 1, lengths[0]) if x.dim() == 3 else out.view(B, lengths[0])
            g = gains[:int(gb[-1])].view(B, frames[0]) if return_gains else None
        else:
            res = [out[int(a):int(b)] for a, b in zip(bases, bases[1:])]
            g = [gains[int(a):int(b)] for a, b in zip(gb, gb[1:])] if return_gains else None
    return (res, g) if return_gains else res
