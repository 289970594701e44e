"""References and bars of the f16-operand / f32-accumulate mode (csrc/wv_h16.hip), shared by tests/test_gpu_h16.py and
tests/test_gpu_h16_fuzz.py.

The mode is NOT the exact path: activations cross HBM as f16, weights are f16, sums are f32.  The references here restate the same
roundings (x, weights, ELU(c*x), u rounded to f16 where the packer and the kernels round them; float64 sums), so that what is left is
f32 summation order plus an occasional one-ulp flip of an f16 rounding: tolerance 3 f16 ulps of the result's magnitude
(3 * 2**-11 relative to max(1, |ref|max)) -- 75 times the f32 suite's bar, stated here because it is a different arithmetic.
Next to each restated reference stands the plain composition of the reference's own ops in float64, which the restatement is held to
on the CPU (4 f16 ulps for the composed convs, 6 for the block).  Importable without a GPU."""
import numpy as np
import torch

from oracle import wv_oracle as O

TOL = 3 * 2.0 ** -11
F32_TOL = 2e-4                                                    # the f32 output of the dense conv
COMPOSED_BOUND = 4 * 2.0 ** -11                                   # a restated composed conv against the reference's two ops
BLOCK_BOUND = 6 * 2.0 ** -11                                      # the restated block against the plain composition


def rnd(rng, *shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def h(a):
    """round to f16 and back (what the kernels store)"""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(got, ref, what="", tol=TOL):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    lim = tol * max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    assert err <= lim, f"{what}: max|d|={err:.3e} > {lim:.3e}"


L2E = 1.4426950408889634


def resblock16_ref(X, w1, d1, b1, w2, d2, b2, pre, s_out):
    """The block with the kernel's roundings restated (csrc/wv_h16.hip rh_kernel): both activations are kept TIMES log2(e) and rounded
    to f16 there, the 1x1 weights are packed DIVIDED by log2(e) and rounded to f16 (pack_rh_pw), sums in float64."""
    C = X.shape[1]
    w1s, w2s = h(w1.astype(np.float64) / L2E), h(w2.astype(np.float64) / L2E)
    xa = h(L2E * O.elu((X * np.float32(pre)).astype(np.float64)))
    y1 = O.sconv1d(O.sconv1d(xa.astype(np.float64), w1s.astype(np.float64), None), d1.astype(np.float64), b1.astype(np.float64), groups=C)
    u = h(L2E * O.elu(y1))
    y = X + np.float64(s_out) * O.sconv1d(O.sconv1d(u.astype(np.float64), w2s.astype(np.float64), None), d2.astype(np.float64), b2.astype(np.float64), groups=C)
    return y.astype(np.float32)


def resblock_plain(X, w1, d1, b1, w2, d2, b2, pre, s_out):
    """The block as the plain composition in float64 (f16 rounding of the operands only)."""
    C = X.shape[1]
    return X + s_out * O.sconv1d(O.sconv1d(O.elu(O.sconv1d(O.sconv1d(O.elu((X * pre).astype(np.float64)), w1.astype(np.float64), None), d1.astype(np.float64),
                                                                   b1.astype(np.float64), groups=C)), w2.astype(np.float64), None),
                                 d2.astype(np.float64), b2.astype(np.float64), groups=C)


def composed_weight(w_pw, w_dw):
    """[M][ks][K]: the 1x1 times the depth-wise taps, rounded as the packer rounds it (pack_h16)."""
    return h(w_pw[:, :, 0][:, None, :] * (w_dw[:, 0, :][:, :, None] if w_dw is not None else 1.0))


def dense_conv_ref(xa, wc, bias, stride, pad, Tout):
    """y[b][m][to] = bias[m] + sum_i sum_k wc[m][i][k] * xa[b][k][to * stride + i - pad], x = 0 outside (float64)."""
    B, K, Tin = xa.shape
    M, ks, _ = wc.shape
    xp = np.zeros((B, K, pad + Tout * stride + ks + stride), np.float64)
    xp[:, :, pad:pad + Tin] = xa
    ref = np.zeros((B, M, Tout), np.float64)
    for i in range(ks):
        ref += np.einsum("mk,bkt->bmt", wc[:, i, :].astype(np.float64), xp[:, :, i:i + Tout * stride:stride][:, :, :Tout])
    return ref + (0.0 if bias is None else bias[None, :, None])


def dense_conv_plain(xa, w_pw, w_dw, bias, stride, pad, Tout):
    """The same conv as its two ops in float64 with unrounded weights: the 1x1, then the depth-wise taps at the given stride and left pad."""
    B, K, Tin = xa.shape
    M = w_pw.shape[0]
    u = np.einsum("mk,bkt->bmt", w_pw[:, :, 0].astype(np.float64), xa.astype(np.float64))
    if w_dw is None:
        w_dw = np.ones((M, 1, 1))
    ks = w_dw.shape[-1]
    up = np.zeros((B, M, pad + Tout * stride + ks + stride), np.float64)
    up[:, :, pad:pad + Tin] = u
    ref = np.zeros((B, M, Tout), np.float64)
    for i in range(ks):
        ref += w_dw[None, :, 0, i, None].astype(np.float64) * up[:, :, i:i + Tout * stride:stride][:, :, :Tout]
    return ref + (0.0 if bias is None else bias[None, :, None])


def upsample16_ref(xa, w_ct, w_pw, b, r):
    """The upsample unit as the packer composes it (pack_up16): rows (p, m), tap 0 = frame l - 1 (ct[k][p + r]), tap 1 = frame l
    (ct[k][p]), each composed weight rounded to f16, float64 sums.  xa: the f16-rounded activated input [B, K, Tin]."""
    B, K, Tin = xa.shape
    M = w_pw.shape[0]
    ref = np.zeros((B, M, Tin * r), np.float64)
    xprev = np.concatenate([np.zeros((B, K, 1)), xa[:, :, :-1]], axis=2).astype(np.float64)
    for p in range(r):
        w0 = h(w_pw[:, :, 0] * w_ct[None, :, 0, p + r]).astype(np.float64)
        w1 = h(w_pw[:, :, 0] * w_ct[None, :, 0, p]).astype(np.float64)
        ref[:, :, p::r] = np.einsum("mk,bkt->bmt", w0, xprev) + np.einsum("mk,bkt->bmt", w1, xa.astype(np.float64))
    return (ref + b[None, :, None]).astype(np.float32)


def upsample_plain(xa, w_ct, w_pw, b, r):
    """The reference's two ops in float64 on the f16-rounded activated input."""
    return O.sconv1d(O.sconvtr1d_depthwise(xa.astype(np.float64), w_ct.astype(np.float64), r).astype(np.float64), w_pw.astype(np.float64), b.astype(np.float64))
