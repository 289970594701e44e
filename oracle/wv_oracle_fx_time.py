"""CPU restatement (numpy, float64 unless said otherwise) of the plain-arithmetic time-domain effects -- TEST INFRASTRUCTURE ONLY.

Only tests/ may import this file; the product (waveverify_amd/effects.py -> csrc/wv_fx_time.hip) never does.  One plain function per
operation, [rows, T] float32 in.  Pinned to the reference by tests/golden/effects_time.npz (tests/test_fx_time_cases_cpu.py), to
scipy.signal.medfilt and to torch's CPU interpolate; the GPU kernels are held to it case by case (tests/test_gpu_fx_time_fuzz.py).

The selections and the one-rounding-per-operation passes (pointwise, median, shush, scatter_zero, smooth's mask) are restated in the
kernel's own float32 and compare bit for bit; the float sums (echo, smooth, stretch's blend) are float64, and the tests' bars are the
float32 roundings a sample passes on the device."""
from __future__ import annotations

import numpy as np

OP_SCALE, OP_ADD_NOISE, OP_QUANTIZE, OP_MUL = 0, 1, 2, 3


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def pointwise(x, op, a, noise=None):
    """float32, bit for bit: x * a, x + fl(noise * a), rint(x * a) / a (half to even, IEEE divide, NaN for a = 0), x * noise."""
    x, a = _f32(x), np.float32(a)
    with np.errstate(all="ignore"):
        if op == OP_SCALE:
            return x * a
        if op == OP_ADD_NOISE:
            s = _f32(noise) * a
            return x + s
        if op == OP_MUL:
            return x * _f32(noise)
        if op == OP_QUANTIZE:
            return np.rint(x * a) / a
    raise ValueError(op)


def median(x, k):
    """scipy.signal.medfilt along the last axis: k // 2 zeros each side, every window sorted, element k // 2."""
    x = _f32(x)
    h = k // 2
    xp = np.pad(x, ((0, 0), (h, h)))
    win = np.lib.stride_tricks.sliding_window_view(xp, k, axis=1)
    return np.sort(win, axis=-1)[..., h].copy()


def shush(x, k, mask=None):
    """-> (y, keep, mask_out).  The k first samples of a stable ascending sort by the bit pattern of |x| go (the earliest first among
    equals); y = x * keep in float32, so a zeroed negative sample is -0; mask_out = mask * (y != 0)."""
    x = _f32(x)
    mag = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    order = np.argsort(mag, axis=1, kind="stable")
    keep = np.ones_like(x)
    np.put_along_axis(keep, order[:, :k], np.float32(0), axis=1)
    y = x * keep
    mo = None if mask is None else _f32(mask) * (y != 0).astype(np.float32)
    return y, keep, mo


def echo(x, n, volume):
    """c[t] = x[t] + v * x[t + n - 1] for t < T - n + 1, v = float64(float32(volume)); y = c / max|c| * max|x| over the whole tensor
    when both maxima are > 0, else c; the last n - 1 samples 0."""
    x = _f32(x).astype(np.float64)
    v = float(np.float32(volume))
    L = x.shape[1] - n + 1
    c = x[:, :L] + v * x[:, n - 1:]
    mo, mr = np.abs(x).max(), np.abs(c).max()
    y = np.zeros_like(x)
    y[:, :L] = c / mr * mo if (mo > 0 and mr > 0) else c
    return y


def echo_gradient(x, g, n, volume):
    """Gradient of (echo(x) * g).sum() towards x: torch's CPU float64 autograd through the formula of echo() written with
    torch.max(torch.abs(.)), as the reference writes it, so tied maxima share their gradient as the reference's autograd shares it."""
    import torch
    xt = torch.from_numpy(_f32(x).astype(np.float64)).requires_grad_(True)
    gt = torch.from_numpy(_f32(g).astype(np.float64))
    v = float(np.float32(volume))
    L = xt.shape[1] - n + 1
    c = xt[:, :L] + v * xt[:, n - 1:]
    mr, mo = torch.max(torch.abs(c)), torch.max(torch.abs(xt))
    if mr > 0 and mo > 0:
        c = c / mr * mo
    y = torch.zeros_like(xt)
    y[:, :L] = c
    (y * gt).sum().backward()
    return xt.grad.numpy()


def _box(xp, w):
    cs = np.concatenate([np.zeros((xp.shape[0], 1)), np.cumsum(xp, axis=1)], axis=1)      # float64 running sum: exact for the unit vectors
    return cs[:, w:] - cs[:, :-w]                                                         # and the dyadic cases, 2^-29 relative otherwise


def smooth(x, w, mask=None, thr=0.5):
    """-> (y, mask_out).  Box of w taps over the REFLECT-padded signal, pad_l = (w - 1) // 2; the mask from the ZERO-padded mask's
    integer window count, compared as float32(count) / float32(w) >= float32(thr)."""
    x = _f32(x).astype(np.float64)
    pl = (w - 1) // 2
    pr = w - 1 - pl
    y = _box(np.pad(x, ((0, 0), (pl, pr)), mode="reflect"), w) / w
    mo = None
    if mask is not None:
        cnt = np.rint(_box(np.pad(_f32(mask).astype(np.float64), ((0, 0), (pl, pr))), w)).astype(np.int64)
        mo = (cnt.astype(np.float32) / np.float32(w) >= np.float32(thr)).astype(np.float32)
    return y, mo


def smooth_transpose(g, w):
    """The dense [T, T] operator of smooth, built from unit vectors, transposed and applied to every row of g."""
    g = _f32(g).astype(np.float64)
    cols = smooth(np.eye(g.shape[1], dtype=np.float32), w)[0]         # cols[u] = A e_u, so cols[u, t] = A[t, u]
    return g @ cols.T


def scatter_zero(y, mask, idx):
    """-> (y', mask') with y'[r, idx[r, j]] = 0 and the same on the mask; an index outside [0, T) does nothing."""
    y = _f32(y).copy()
    mask = None if mask is None else _f32(mask).copy()
    T = y.shape[1]
    for r, row in enumerate(np.asarray(idx).reshape(y.shape[0], -1)):
        for t in row:
            if 0 <= int(t) < T:
                y[r, int(t)] = 0.0
                if mask is not None:
                    mask[r, int(t)] = 0.0
    return y, mask


def stretch_coords(t_in, t_out, fused=True):
    """-> (i0, i1, l0, l1) of interpolate(mode='linear', align_corners=False): the scale, the source coordinate and the weights in
    float32 as torch forms them, the coordinate the ONCE-rounded value of scale * (m + 0.5) - 0.5 (fused=False: rounded twice)."""
    scale = np.float32(t_in) / np.float32(t_out)
    m = np.arange(t_out, dtype=np.float32) + np.float32(0.5)
    if fused:
        src = (np.float64(scale) * m.astype(np.float64) - 0.5).astype(np.float32)        # the product of two float32 is exact in float64
    else:
        src = scale * m - np.float32(0.5)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int64), t_in - 1)
    i1 = i0 + (i0 < t_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1) - l1
    return i0, i1, l0, l1


def stretch(x, t_out, fused=True):
    """Linear stretch of every row to t_out samples: float32 index arithmetic (stretch_coords), the blend in float64."""
    x = _f32(x)
    i0, i1, l0, l1 = stretch_coords(x.shape[1], int(t_out), fused)
    x = x.astype(np.float64)
    return l0.astype(np.float64) * x[:, i0] + l1.astype(np.float64) * x[:, i1]
