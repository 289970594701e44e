"""The three validation-metric kernels (csrc/wv_metrics.hip) on the GPU: against the reference's records (tests/golden/validation_metrics.npz,
tests/golden/metrics.npz) and the float64 restatements of validation_cases.py; and, called through the C ABI with guard bands around
every output, a poisoned workspace and inputs one float past an aligned boundary, for their contract: nothing else written, two runs
bit-equal, a clip's result independent of the batch it came in."""
import ctypes as C

import numpy as np
import pytest
import torch

from guard import Guards
from validation_cases import (MET_BER, MIOU_CASES, SI_BATCH, SI_BATCH_MEAN, SI_CASES, VAL_BER, ber_f64, check_decode, iou_counts_np, sisnr_bound,
                              sisnr_f64, ulp32)
from waveverify_amd import _lib, metrics

pytestmark = pytest.mark.gpu

SHAPES_T = (1, 63, 64, 65, 4097)          # shorter than a wave, one wave, one wave + 1, and one sample past the 4096-sample chunk
B3 = 3


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- against the reference's records ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", VAL_BER + MET_BER, ids=lambda c: c["name"])
def test_decode_equals_the_reference(case):
    errors, valid, avg = metrics.ber_per_clip(_cu(case["logits"]), _cu(case["bits"]), _cu(case["mask"]), threshold=case["thr"])
    assert errors.is_cuda and errors.dtype == torch.int32 and valid.dtype == torch.int32 and avg.dtype == torch.float32
    check_decode(case, errors.cpu().numpy(), valid.cpu().numpy(), avg.cpu().numpy())


@pytest.mark.parametrize("case", MIOU_CASES, ids=lambda c: c["name"])
def test_iou_equals_numpy_and_the_reference(case):
    p, g = _cu(case["p"]), _cu(case["g"])
    counts = metrics.iou_counts(p, g).cpu().numpy()
    assert counts.dtype == np.int32 and np.array_equal(counts, iou_counts_np(case["p"], case["g"]))
    assert float(metrics.miou_from_counts(counts.astype(np.int64).sum(axis=0))) == case["out"]
    per_clip = metrics.miou_per_clip(p, g)
    for b in range(p.shape[0]):
        assert per_clip[b] == metrics.MIOU()(case["p"][b:b + 1], case["g"][b:b + 1])


@pytest.mark.parametrize("c", SI_CASES, ids=lambda c: f"si{c['i']}-{c['kind']}-T{c['T']}")
def test_sisnr_against_float64_and_the_reference(c):
    """|gpu - f64| <= 1e-6 dB below 60 dB (sisnr_bound), |gpu - reference float32| <= d_i + that; the eps-driven values to 1e-9 dB."""
    m = metrics.SISNR()
    got = m(_cu(c["est"])[None, None], _cu(c["ref"])[None, None])
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (1,)
    v = float(got)
    print(f"si{c['i']:02d} {c['kind']:9s} T={c['T']:5d} gpu={v:+.9f} f64={c['f64']:+.9f} |gpu-f64|={abs(v - c['f64']):.2e} ref_f32={c['ref_f32']:+.6f} d={c['d']:.2e}")
    assert abs(v - c["f64"]) <= (1e-9 if c["kind"] in ("silent", "identical") else sisnr_bound(c["f64"]))
    assert abs(v - c["ref_f32"]) <= c["d"] + sisnr_bound(c["f64"])
    x, y = c["est"].astype(np.float64), c["ref"].astype(np.float64)
    want = np.array([x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()])
    assert np.allclose(m.last_moments.cpu().numpy()[0], want, rtol=1e-13, atol=0)


def test_sisnr_mean_is_the_reference_scalar():
    cs = [SI_CASES[i] for i in SI_BATCH]
    est, ref = (_cu(np.stack([c[k] for c in cs]))[:, None] for k in ("est", "ref"))
    m = metrics.SISNR()
    assert abs(float(m.mean(est, ref)) - SI_BATCH_MEAN) <= float(np.mean([c["d"] for c in cs])) + 1e-6
    assert torch.equal(m(est, ref), torch.cat([m(est[i:i + 1], ref[i:i + 1]) for i in range(len(cs))]))


# ---- the contract, through the C ABI ------------------------------------------------------------------------------------------------
def _decode_inputs(T, masked):
    rng = np.random.default_rng(100 + T)
    W = 16
    offs = rng.choice([-1.5, 1.5], size=(B3, W, 1))               # means well away from the threshold: the float64 decision is the answer
    logits = (rng.standard_normal((B3, W, T)) + offs).astype(np.float32)
    bits = rng.integers(0, 2, (B3, W)).astype(np.float32)
    mask = None
    if masked:
        mask = (rng.random((B3, 1, T)) < 0.6).astype(np.float32)
        mask[1] = 0.0                                             # a clip without a live sample
        mask[0, 0, 0] = 1.0
    return logits, bits, mask


def _run_decode(gin, lib, z, bits, mask, thr=0.5):
    """One call with output and workspace arenas of its own (fresh pattern, fresh poison); the inputs' arenas are checked with them."""
    B, W, T = z.t.shape
    g = Guards(offset=1)
    avg, err, val = g.output((B, W), torch.float32, "avg"), g.output((B,), torch.int32, "errors"), g.output((B,), torch.int32, "valid")
    ws = g.workspace(int(lib.wv_metrics_decode_workspace_bytes(B, W, T)))
    rc = lib.wv_metrics_decode(z.t.data_ptr(), bits.t.data_ptr(), None if mask is None else mask.t.data_ptr(), thr, 1e-8, B, W, T, avg.t.data_ptr(),
                               err.t.data_ptr(), val.t.data_ptr(), ws.t.data_ptr(), ws.n, _stream())
    assert rc == 0
    g.check()
    gin.check()
    return avg.t.clone(), err.t.clone(), val.t.clone()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("T", SHAPES_T)
def test_decode_contract(T, masked):
    lib = _lib.load()
    logits, bits, mask = _decode_inputs(T, masked)
    a64, ok64 = ber_f64(logits, mask)
    assert np.all((np.abs(a64 - 0.5) >= (np.log2(T) + 2) * 2.0 ** -24) | ~ok64)     # the cases are unambiguous by construction
    g = Guards(offset=1)                                                         # every tensor one element past a 256-byte boundary
    z, b, m = g.input(logits, "logits"), g.input(bits, "bits"), None if mask is None else g.input(mask, "mask")
    avg, err, val = _run_decode(g, lib, z, b, m)
    want_dec = (a64 >= 0.5) & ok64
    assert np.array_equal(val.cpu().numpy(), ok64.sum(axis=1))
    assert np.array_equal(err.cpu().numpy(), ((want_dec != (bits == 1)) & ok64).sum(axis=1))
    assert np.all(np.abs(avg.cpu().numpy().astype(np.float64) - a64) <= 2 * ulp32(a64))
    again = _run_decode(g, lib, z, b, m)                                        # a second run, on fresh poison: bit-equal
    assert all(torch.equal(p, q) for p, q in zip((avg, err, val), again))
    for i in range(B3):                                                          # and clip by clip, as B = 1 calls
        g1 = Guards(offset=1)
        one = _run_decode(g1, lib, g1.input(logits[i:i + 1]), g1.input(bits[i:i + 1]), None if mask is None else g1.input(mask[i:i + 1]))
        assert torch.equal(one[0], avg[i:i + 1]) and torch.equal(one[1], err[i:i + 1]) and torch.equal(one[2], val[i:i + 1])


def _run_iou(gin, lib, p, m):
    B, _, T = p.t.shape
    g = Guards(offset=1)
    counts = g.output((B, 4), torch.int32, "counts")
    ws = g.workspace(int(lib.wv_metrics_iou_workspace_bytes(B, T)))
    assert lib.wv_metrics_iou(p.t.data_ptr(), m.t.data_ptr(), B, T, counts.t.data_ptr(), ws.t.data_ptr(), ws.n, _stream()) == 0
    g.check()
    gin.check()
    return counts.t.clone()


@pytest.mark.parametrize("T", SHAPES_T)
def test_iou_contract(T):
    lib = _lib.load()
    rng = np.random.default_rng(200 + T)
    raw = rng.standard_normal((B3, 1, T)).astype(np.float32) + 0.5
    raw[0, 0, 0] = 0.5                                                          # exactly at the threshold: background
    mask = (rng.random((B3, 1, T)) < 0.5).astype(np.float32)
    mask[2] = 0.0
    g = Guards(offset=1)
    p, m = g.input(raw, "pred"), g.input(mask, "mask")
    counts = _run_iou(g, lib, p, m)
    assert np.array_equal(counts.cpu().numpy(), iou_counts_np(raw, mask))
    assert torch.equal(_run_iou(g, lib, p, m), counts)
    for i in range(B3):
        g1 = Guards(offset=1)
        assert torch.equal(_run_iou(g1, lib, g1.input(raw[i:i + 1]), g1.input(mask[i:i + 1])), counts[i:i + 1])


def _run_sisnr(gin, lib, x, y):
    B, _, T = x.t.shape
    g = Guards(offset=1)
    out, mom = g.output((B,), torch.int64, "sisnr"), g.output((B, 5), torch.int64, "moments")      # float64 outputs, guarded as 8-byte words
    ws = g.workspace(int(lib.wv_metrics_sisnr_workspace_bytes(B, T)))
    assert lib.wv_metrics_sisnr(x.t.data_ptr(), y.t.data_ptr(), B, T, 1e-8, out.t.data_ptr(), mom.t.data_ptr(), ws.t.data_ptr(), ws.n, _stream()) == 0
    g.check()
    gin.check()
    return out.t.clone().view(torch.float64), mom.t.clone().view(torch.float64)


@pytest.mark.parametrize("T", SHAPES_T)
def test_sisnr_contract(T):
    lib = _lib.load()
    rng = np.random.default_rng(300 + T)
    ref = (0.2 * rng.standard_normal((B3, 1, T))).astype(np.float32)
    est = (ref + 0.2 * 10 ** (-30 / 20) * rng.standard_normal((B3, 1, T))).astype(np.float32)
    est[1], ref[2] = ref[1], 0.0                                                 # an identical pair and a silent reference
    f64 = sisnr_f64(est[:, 0], ref[:, 0])
    g = Guards(offset=1)
    x, y = g.input(est, "estimate"), g.input(ref, "reference")
    out, mom = _run_sisnr(g, lib, x, y)
    got = out.cpu().numpy()
    for i in range(B3):
        assert abs(got[i] - f64[i]) <= (1e-9 if i > 0 else sisnr_bound(f64[i])), (i, got[i], f64[i])
    again = _run_sisnr(g, lib, x, y)
    assert torch.equal(again[0], out) and torch.equal(again[1], mom)
    for i in range(B3):
        g1 = Guards(offset=1)
        one = _run_sisnr(g1, lib, g1.input(est[i:i + 1]), g1.input(ref[i:i + 1]))
        assert torch.equal(one[0], out[i:i + 1]) and torch.equal(one[1], mom[i:i + 1])


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    z = torch.zeros(2, 4, 8, device="cuda")
    small = torch.empty(8, dtype=torch.uint8, device="cuda")
    out_f, out_i = torch.empty(2, 4, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda")
    args = (z.data_ptr(), out_f.data_ptr(), None, 0.5, 1e-8, 2, 4, 8, out_f.data_ptr(), out_i.data_ptr(), out_i.data_ptr())
    assert lib.wv_metrics_decode(*args, small.data_ptr(), small.numel(), _stream()) == -5             # WV_ENOMEM: workspace too small
    assert lib.wv_metrics_decode(*args[:5], 0, 4, 8, *args[8:], small.data_ptr(), 1 << 20, _stream()) == -1          # WV_EINVAL
    assert lib.wv_metrics_iou(z.data_ptr(), z.data_ptr(), 70000, 8, out_i.data_ptr(), small.data_ptr(), 1 << 30, _stream()) == -1
    assert lib.wv_metrics_sisnr(z.data_ptr(), z.data_ptr(), 2, 8, 1e-8, None, None, small.data_ptr(), 1 << 20, _stream()) == -1
    torch.cuda.synchronize()
