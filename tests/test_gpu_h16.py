"""The detector's f16-operand / f32-accumulate mode (csrc/wv_h16.hip), unit by unit through the C ABI against the numpy oracle.

The mode is NOT the exact path: activations cross HBM as f16, weights are f16, sums are f32.  The references below therefore
restate the same roundings (x, weights, ELU(c*x), u rounded to f16 where the kernel rounds them; float64 sums), so that what is left
is f32 summation order plus an occasional one-ulp flip of an f16 rounding: tolerance 3 f16 ulps of the result's magnitude
(3 * 2**-11 relative to max(1, |ref|max)) -- 75 times the f32 suite's bar, stated here because it is a different arithmetic."""
import numpy as np
import pytest
import torch

from oracle import wv_oracle as O

from h16_refs import (BLOCK_BOUND, COMPOSED_BOUND, L2E, TOL, close, cu, h, resblock16_ref, resblock_plain, rnd,  # noqa: F401  (other test files import these from here)
                      upsample16_ref, upsample_plain)
from h16_refs import dense_conv_ref as _dense_conv_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from waveverify_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _ops


def c8_to_np(ops, t, C):
    return ops.h16_to_f32(t, C).cpu().numpy()


@pytest.mark.parametrize("B,C,T", [(2, 64, 1000), (3, 33, 17), (1, 8, 1), (2, 129, 300)])
def test_layout_round_trip(ops, B, C, T):
    rng = np.random.default_rng(C + T)
    X = rnd(rng, B, C, T)
    t = ops.h16_from_f32(cu(X))
    assert t.dtype == torch.float16 and tuple(t.shape) == (B, (C + 15) // 16 * 2, T, 8)
    # the layout itself: element (b, c, t) sits at [b, c // 8, t, c % 8]; rows past C are zero
    ref = np.zeros((B, t.shape[1] * 8, T), np.float32)
    ref[:, :C] = h(X)
    lay = t.float().cpu().numpy().transpose(0, 1, 3, 2).reshape(B, -1, T)
    assert np.array_equal(lay, ref)
    assert np.array_equal(c8_to_np(ops, t, C), h(X))
    act = ops.h16_from_f32(cu(X), scale=0.7, elu=True)
    close(ops.h16_to_f32(act, C), h(O.elu(X * np.float32(0.7))), "ELU on the way", tol=2.0 ** -11)


@pytest.mark.parametrize("C,T,ks", [(64, 1000, 7), (64, 5, 7), (32, 300, 5)])
def test_conv_pre(ops, C, T, ks):
    rng = np.random.default_rng(C + T)
    x = rnd(rng, 3, 1, T, scale=0.1)
    w, b = rnd(rng, C, 1, ks, scale=0.4), rnd(rng, C, scale=0.1)
    s = np.float32(1.0 / 0.1122080159)
    ref = O.sconv1d(x * s, w, b)
    got = ops.h16_conv_pre(cu(x), w, b, in_scale=float(s))
    close(ops.h16_to_f32(got, C), h(ref), "conv_pre16")


# lengths around every tile edge: 244 outputs per tile at C = 64, 120 at C = 96 / 128 / 192, 56 at C = 256 / 384 / 512 / 768, 476 at C = 32;
# one-sample and sub-halo clips.  32: the locator's first stage; 96 / 192 / 384 / 768: the generator's decoder
@pytest.mark.parametrize("C,T", [(64, 16000), (64, 244), (64, 245), (64, 1), (64, 7), (64, 500), (128, 8000), (128, 120), (128, 121), (128, 3),
                                 (256, 2000), (256, 119), (256, 241), (512, 400), (512, 56), (512, 57), (512, 5),
                                 (32, 16000), (32, 476), (32, 477), (32, 2), (96, 16000), (96, 120), (96, 121), (96, 6), (192, 8000), (192, 241), (192, 1),
                                 (384, 2000), (384, 56), (384, 57), (384, 3), (768, 400), (768, 113), (768, 4)])
def test_resblock(ops, C, T):
    rng = np.random.default_rng(C * 3 + T)
    B = 3
    X = h(rnd(rng, B, C, T))
    w1, w2 = rnd(rng, C, C, 1, scale=C ** -0.5), rnd(rng, C, C, 1, scale=C ** -0.5)
    d1, d2 = rnd(rng, C, 1, 5, scale=0.45), rnd(rng, C, 1, 5, scale=0.45)
    b1, b2 = rnd(rng, C, scale=0.1), rnd(rng, C, scale=0.1)
    pre, s_out, s_act = np.float32(0.8660254), np.float32(0.41), np.float32(0.7071)
    y = resblock16_ref(X, w1, d1, b1, w2, d2, b2, pre, s_out)
    # ... and the restated roundings are the block itself: against the plain composition in float64 (f16 rounding of operands only)
    plain = resblock_plain(X, w1, d1, b1, w2, d2, b2, pre, s_out)
    assert np.abs(plain - y).max() <= BLOCK_BOUND * max(1.0, np.abs(plain).max())
    X16 = ops.h16_from_f32(cu(X))
    got, gact = ops.h16_resblock(X16, w1, d1, b1, w2, d2, b2, pre_scale=float(pre), out_scale=float(s_out), act_scale=float(s_act))
    close(ops.h16_to_f32(got, C), h(y), "resblock16")
    close(ops.h16_to_f32(gact, C), h(O.elu(y * s_act)), "resblock16 (activated copy)")
    only_raw = ops.h16_resblock(X16, w1, d1, b1, w2, d2, b2, pre_scale=float(pre), out_scale=float(s_out))
    only_act = ops.h16_resblock(X16, w1, d1, b1, w2, d2, b2, pre_scale=float(pre), out_scale=float(s_out), act_scale=float(s_act), want_raw=False)
    # the raw-only form rounds y = f16(v * s + x) in one instruction (v_fma_mixlo/hi_f16), the two-output form rounds the f32 sum: the same
    # value except where the f32 sum sits within its own rounding of an f16 tie
    assert float((ops.h16_to_f32(only_raw, C) - ops.h16_to_f32(got, C)).abs().max()) <= 2.0 ** -10 * max(1.0, float(np.abs(y).max()))
    close(ops.h16_to_f32(only_raw, C), h(y), "resblock16 (raw only)")
    assert torch.equal(only_act, gact)


@pytest.mark.parametrize("K,M,Tin,r", [(64, 128, 16000, 2), (64, 128, 1001, 2), (128, 256, 8000, 4), (128, 256, 501, 4), (256, 512, 2000, 5), (256, 512, 203, 5),
                                       (512, 1024, 400, 8), (512, 1024, 37, 8), (64, 128, 1, 2), (32, 64, 70, 8)])
def test_downsample_as_one_conv(ops, K, M, Tin, r):
    """ELU -> 1x1 -> depth-wise(2r, stride r) (seanet.py:739-760) with the two convolutions composed into one dense conv; c8 and f32 outputs."""
    rng = np.random.default_rng(K + M + Tin)
    B = 3
    X = rnd(rng, B, K, Tin)
    w_pw, w_dw, b = rnd(rng, M, K, 1, scale=K ** -0.5), rnd(rng, M, 1, 2 * r, scale=(2 * r) ** -0.5), rnd(rng, M, scale=0.1)
    pre = np.float32(0.7559)
    xa = h(O.elu(X * pre))
    wc = h(w_pw[:, :, 0][:, None, :] * w_dw[:, 0, :][:, :, None])          # [M][2r][K], rounded as the packer rounds it
    Tout = (Tin + r - 1) // r
    xp = np.zeros((B, K, r + Tout * r + r), np.float64)
    xp[:, :, r:r + Tin] = xa
    ref = np.zeros((B, M, Tout), np.float64)
    for i in range(2 * r):
        ref += np.einsum("mk,bkt->bmt", wc[:, i, :].astype(np.float64), xp[:, :, i:i + Tout * r:r])
    ref = (ref + b[None, :, None]).astype(np.float32)
    # the composition itself against the reference's two convs in float64 (f16 rounding of the composed weight: a few 1e-4 relative)
    two = O.sconv1d(O.sconv1d(xa.astype(np.float64), w_pw.astype(np.float64), None), w_dw.astype(np.float64), b.astype(np.float64), stride=r, groups=M)
    assert np.abs(two - ref).max() <= 4 * 2.0 ** -11 * max(1.0, np.abs(two).max())
    X16 = ops.h16_from_f32(cu(X), scale=float(pre), elu=True)
    out = ops.h16_conv(X16, w_pw, w_dw, b, ks=2 * r, stride=r, pad=r, act_scale=0.5, want_f32=True)
    close(out["f32"], ref, "downsample16 (f32 out)", tol=2e-4)
    close(ops.h16_to_f32(out["raw"], M), h(ref), "downsample16")
    close(ops.h16_to_f32(out["act"], M), h(O.elu(ref * np.float32(0.5))), "downsample16 (activated copy)")


@pytest.mark.parametrize("F,M,T", [(33, 64, 16000), (33, 64, 77), (65, 128, 8000), (129, 256, 2000), (257, 512, 400), (257, 512, 3)])
def test_spec_add(ops, F, M, T):
    """x' = x + scale * (W @ P) (seanet.py:500-502) with the spectrum rows zero-padded to a multiple of 16; only ELU(c * x') is written."""
    rng = np.random.default_rng(F + M + T)
    B = 3
    P, X = rnd(rng, B, F, T, scale=1.5), h(rnd(rng, B, M, T))
    w = h(rnd(rng, M, F, 1, scale=F ** -0.5))
    scale, c = np.float32(0.577), np.float32(0.7559)
    ref = (X + scale * np.einsum("mf,bft->bmt", w[:, :, 0].astype(np.float64), h(P).astype(np.float64))).astype(np.float32)
    P16, X16 = ops.h16_from_f32(cu(P)), ops.h16_from_f32(cu(X))
    out = ops.h16_conv(P16, w, None, None, resid16=X16, K=F, out_scale=float(scale), act_scale=float(c))
    close(ops.h16_to_f32(out["raw"], M), h(ref), "spec add16")
    close(ops.h16_to_f32(out["act"], M), h(O.elu(ref * c)), "spec add16 (activated copy)")


# ---- the whole detector in this mode, against the REFERENCE's own outputs (tests/golden, generated from the imported reference) ----
@pytest.fixture(scope="module")
def detector():
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    cfg = default_config("detector")
    return HipNet(cfg, random_state_dict(cfg, 0))


@pytest.mark.parametrize("fixture", ["full_T16000", "full_T16001", "full_T4800", "speech_T16000"])
def test_detector_f16_vs_reference_golden(golden_dir, detector, fixture):
    """Mean probabilities of the f16 mode against the reference's; every bit the reference decides with a margin above 4 x the measured
    |dp| must come out the same (VERDICT r2 item 5's bar), and on these fixtures that has to be every bit."""
    import os
    g = np.load(os.path.join(golden_dir, fixture + ".npz"))
    wm = torch.from_numpy(g["wm"]).cuda()
    mp = detector.detector_mean_prob(wm, precision="f16").cpu().numpy()
    ref = g["det_mean_prob"]
    err = float(np.abs(mp - ref).max())
    assert np.isfinite(mp).all() and err <= 2e-2, err
    margin = np.abs(ref - 0.5)
    decidable = margin > 4 * err
    assert ((mp >= 0.5).astype(np.int32) == g["det_bits"])[decidable].all()
    assert decidable.all(), f"{(~decidable).sum()} bits closer to the threshold than 4 x |dp| = {4 * err:.1e}"
    # and against the exact path of this library: the same order of magnitude
    mp32 = detector.detector_mean_prob(wm).cpu().numpy()
    assert float(np.abs(mp - mp32).max()) <= 2e-2
    if "det_logits_sub" in g.files:
        lg = detector.detector(wm, precision="f16")[..., ::37].cpu().numpy()
        assert np.abs(lg - g["det_logits_sub"]).max() <= 0.05 * max(1.0, np.abs(g["det_logits_sub"]).max())


def test_detector_f16_narrow_margin(golden_dir):
    """The narrow-margin fixture (margins 1e-3 .. 4e-2): bits are compared where the reference's margin exceeds 4 x the measured |dp|;
    the rest are reported, not asserted (an f16 mode cannot decide a 1e-3 margin)."""
    import os
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    g = np.load(os.path.join(golden_dir, "narrow_margin_T16000.npz"))
    cfg = default_config("detector")
    sd = random_state_dict(cfg, 0)
    sd["last_layer.bias"] = g["last_layer_bias"]
    D = HipNet(cfg, sd)
    mp = D.detector_mean_prob(torch.from_numpy(g["wm"]).cuda(), precision="f16").cpu().numpy()
    err = float(np.abs(mp - g["det_mean_prob"]).max())
    assert err <= 2e-2, err
    decidable = g["margin"] > 4 * err
    assert ((mp >= 0.5).astype(np.int32) == g["det_bits"])[decidable].all()
    print(f"narrow-margin fixture: |dp| max {err:.2e}, {int(decidable.sum())} of {decidable.size} bits decidable at 4 x |dp|, "
          f"{int(((mp >= 0.5).astype(np.int32) != g['det_bits']).sum())} differ in all")


def test_f16_mode_refuses_nets_without_a_plan():
    """Layer shapes outside the f16 kernels' set (here 16-channel first stages): the *_f16 entry points report WV_ESTATE -> RuntimeError; the
    exact path of the same nets runs."""
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    x = torch.zeros(1, 1, 800, device="cuda")
    for kind in ("locator", "detector"):
        cfg = default_config(kind, channels_enc=16)
        N = HipNet(cfg, random_state_dict(cfg, 0, parametrized=True))
        N._head(x, True, False)
        with pytest.raises(RuntimeError):
            N._head(x, True, False, precision="f16")
    cfg = default_config("generator", channels_enc=16)
    G = HipNet(cfg, random_state_dict(cfg, 0))
    with pytest.raises(RuntimeError):
        G.generator(x, torch.zeros(1, 16, device="cuda"), precision="f16")
    with pytest.raises(ValueError):
        G.generator(x, torch.zeros(1, 16, device="cuda"), precision="bf16")


@pytest.mark.parametrize("B,T", [(1, 16000), (5, 12345), (3, 333), (1, 1), (2, 5), (2, 321), (1, 48001)])
def test_detector_f16_shapes(detector, B, T):
    """Ragged lengths and batch sizes: finite, close to the exact path, and independent of the batch a clip sits in."""
    from waveverify_amd.init import synthetic_clips
    x = torch.from_numpy(synthetic_clips(B, T, seed=B + T)[0]).cuda()
    mp = detector.detector_mean_prob(x, precision="f16")
    mp32 = detector.detector_mean_prob(x)
    assert torch.isfinite(mp).all() and float((mp - mp32).abs().max()) <= 2e-2
    one = detector.detector_mean_prob(x[B - 1:B].contiguous(), precision="f16")
    assert torch.equal(one[0], mp[B - 1])


@pytest.mark.parametrize("n_fft,hop,T", [(64, 1, 16000), (64, 1, 300), (64, 1, 257), (64, 1, 5), (128, 2, 16000), (128, 2, 255), (128, 2, 3), (256, 8, 16000), (256, 8, 520),
                                         (256, 8, 7), (512, 40, 16000), (512, 40, 2600), (512, 40, 39), (1024, 320, 16000), (1024, 320, 20481), (1024, 320, 100)])
def test_spec_block_in_one_launch(ops, n_fft, hop, T):
    _spec_block_case(ops, n_fft, hop, T, n_fft)


# the locator's scales: half as many channels as DFT points (32 / 64 / 128 at n_fft 64 / 128 / 256, hops 1 / 4 / 32)
@pytest.mark.parametrize("n_fft,hop,T", [(64, 1, 16000), (64, 1, 257), (64, 1, 3), (128, 4, 16000), (128, 4, 1021), (128, 4, 5), (256, 32, 16000), (256, 32, 2081), (256, 32, 31)])
def test_spec_block_in_one_launch_half_channels(ops, n_fft, hop, T):
    _spec_block_case(ops, n_fft, hop, T, n_fft // 2)


def _spec_block_case(ops, n_fft, hop, T, C, basis=None, w_kind="random"):
    """STFT (waveform split in two f16 terms, f16 basis) -> log-magnitude -> 1x1 -> add in one launch, against the oracle's exact
    composition; silence in one clip (both clamps), a loud clip, tile-edge frame counts.  What separates the two: the basis rounded to
    f16 (leakage around the 1e-5 clamp level, visible only on near-silent bins), P and x' rounded to f16.  basis: [2F, n_fft] or None
    (the analytic one); w_kind "selector": W[m][f] = [m == f], so that bin 0 and the Nyquist bin each land in a channel of their own."""
    rng = np.random.default_rng(n_fft + hop + T + C)
    F, Tf = n_fft // 2 + 1, -(-T // hop)
    wav = np.clip(rnd(rng, 3, 1, T, scale=0.1), -1, 1)
    wav[1, 0, : T // 3] = 0.0
    wav[2] *= 8.0
    x = h(rnd(rng, 3, C, Tf))
    w = h(rnd(rng, C, F, 1, scale=F ** -0.5))
    if w_kind == "selector":
        w = np.zeros((C, F, 1), np.float32)
        w[np.arange(min(C, F)), np.arange(min(C, F)), 0] = 1.0
        if C < F:                                                # half-channel geometries: the Nyquist bin into the last channel
            w[C - 1, C - 1, 0], w[C - 1, F - 1, 0] = 0.0, 1.0
    s_out, s_act = np.float32(0.53), np.float32(0.7071)
    mag = O.causal_stft_mag(wav, n_fft, hop, basis)
    P = ((np.log(np.maximum(mag, np.float32(1e-5))) - np.float32(-4.3)) / np.float32(2.8)).astype(np.float32)
    ref = (x + s_out * O.sconv1d(P, w, None)).astype(np.float32)
    got, gact = ops.h16_spec_block(cu(wav), w, ops.h16_from_f32(cu(x)), n_fft, hop, mean=-4.3, std=2.8, out_scale=float(s_out), act_scale=float(s_act),
                                   basis=basis)
    g = ops.h16_to_f32(got, C).cpu().numpy()
    assert np.isfinite(g).all()
    # frames whose bins all sit clear of the clamp: the f16 bar; frames with near-silent bins (the silent third of clip 1): the clamp region's
    # log is steep (d log|X| = d|X| / |X|), the exact path's own test allows 5e-3 per unit of |w| there and so does this one
    quiet = (mag <= 1e-3).any(axis=1, keepdims=True)
    lim = TOL * max(1.0, float(np.abs(ref).max())) + np.where(quiet, 5e-3 * float(s_out) * float(np.abs(w).sum(1).max()), 0.0)
    print(f"MEASURE spec16 n_fft={n_fft} hop={hop} T={T} C={C} {w_kind}{'' if basis is None else ' (given basis)'}: "
          f"max|d| {float(np.abs(g - ref).max()):.2e}, over the bar {float((np.abs(g - ref) - lim).max()):.2e}")
    assert (np.abs(g - ref) <= lim).all(), float((np.abs(g - ref) - lim).max())
    ga = ops.h16_to_f32(gact, C).cpu().numpy()
    assert (np.abs(ga - O.elu(ref * s_act)) <= lim).all()
    only_act = ops.h16_spec_block(cu(wav), w, ops.h16_from_f32(cu(x)), n_fft, hop, mean=-4.3, std=2.8, out_scale=float(s_out), act_scale=float(s_act), want_raw=False,
                                  basis=basis)
    assert torch.equal(only_act, gact)


def test_detector_f16_captures_into_a_hip_graph(detector):
    """Like the exact path: plain launches on the caller's stream (no allocation, no sync), so the f16 forward captures into a HIP graph
    and replays bit-identically; and it is deterministic from run to run."""
    from waveverify_amd.init import synthetic_clips
    x = torch.from_numpy(synthetic_clips(3, 16000, seed=9)[0]).cuda()
    p0 = detector.detector_mean_prob(x, precision="f16")
    assert torch.equal(detector.detector_mean_prob(x, precision="f16"), p0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        detector.detector_mean_prob(x, precision="f16")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        p1 = detector.detector_mean_prob(x, precision="f16")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(p1, p0)
    p1.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(p1, p0)


def test_waveverify_api_opt_in():
    """WaveVerify.detect_batch through the f16 mode when the caller opts in (attribute `detector_precision`); the default stays exact."""
    from waveverify_amd.core import WaveVerify
    from waveverify_amd.init import synthetic_clips
    wv = WaveVerify.random_init(seed=0, device="cuda:0")
    assert wv.detector_precision == "f32"
    x_np, msg_np = synthetic_clips(4, 16000, seed=11)
    wm = wv.embed_batch(torch.from_numpy(x_np).cuda(), torch.from_numpy(msg_np).cuda())
    bits32, mp32 = wv.detect_batch(wm)
    wv.detector_precision = "f16"
    bits16, mp16 = wv.detect_batch(wm)
    assert torch.equal(bits16, bits32) and float((mp16 - mp32).abs().max()) <= 2e-2 and not torch.equal(mp16, mp32)
    wv.detector_precision = "bf16"
    with pytest.raises(ValueError):
        wv.detect_batch(wm)
    # all three nets at once: embed / locate through the mode as well; the exact outputs are the default again after set_precision("f32")
    x, msg = torch.from_numpy(x_np).cuda(), torch.from_numpy(msg_np).cuda()
    loc32 = wv.locate_batch(wm)
    wv.set_precision("f16")
    wm16 = wv.embed_batch(x, msg)
    assert not torch.equal(wm16, wm) and float((wm16 - wm).abs().max()) <= 1e-4
    assert torch.equal(wv.detect_batch(wm16)[0], bits32)
    assert float((wv.locate_batch(wm) - loc32).abs().max()) <= 0.02
    with pytest.raises(ValueError):
        wv.set_precision("bf16")
    wv.set_precision("f32")
    assert torch.equal(wv.embed_batch(x, msg), wm)


# ---- seeded sweep of geometries the detector does not use: the generic conv (any taps / stride / pad, ragged channel counts on the f32
# output, residual + both c8 outputs), the ResnetBlock at random lengths and batch sizes
def _generic_geometry(seed):
    """The shape draw of test_conv16_generic_geometries -> (rng, B, K, ks, stride, pad, Tin, c8_out, M); the test goes on drawing its data from rng."""
    rng = np.random.default_rng(1000 + seed)
    B = int(rng.integers(1, 6))
    K = int(rng.choice([8, 16, 24, 40, 64, 100, 144, 272]))
    ks = int(rng.choice([1, 2, 3, 5, 7, 8, 10, 16]))
    stride = int(rng.choice([1, 1, 2, 3, 4, 5, 8]))
    pad = int(rng.integers(0, ks))
    Tin = int(rng.choice([1, 2, 17, 50, 63, 64, 65, 200, 513, 1000]))
    c8_out = bool(rng.integers(0, 2))
    M = int(rng.choice([16, 32, 64, 96, 128, 320])) if c8_out else int(rng.choice([1, 7, 16, 33, 64, 130, 256]))
    return rng, B, K, ks, stride, pad, Tin, c8_out, M


@pytest.mark.parametrize("seed", range(24))
def test_conv16_generic_geometries(ops, seed):
    rng, B, K, ks, stride, pad, Tin, c8_out, M = _generic_geometry(seed)
    X = rnd(rng, B, K, Tin)
    w_pw, w_dw = rnd(rng, M, K, 1, scale=K ** -0.5), (rnd(rng, M, 1, ks, scale=ks ** -0.5) if ks > 1 else None)
    bias = rnd(rng, M, scale=0.1) if rng.integers(0, 2) else None
    Tout = (Tin + stride - 1) // stride
    wc = h(w_pw[:, :, 0][:, None, :] * (w_dw[:, 0, :][:, :, None] if w_dw is not None else 1.0))
    xa = h(X)
    s_out = np.float32(0.7)
    ref = _dense_conv_ref(xa, wc, bias, stride, pad, Tout) * s_out
    X16 = ops.h16_from_f32(cu(X))
    if c8_out:
        R = h(rnd(rng, B, M, Tout))
        ref = (ref + R).astype(np.float32)
        out = ops.h16_conv(X16, w_pw, w_dw, bias, resid16=ops.h16_from_f32(cu(R)), ks=ks, stride=stride, pad=pad, out_scale=float(s_out), act_scale=0.9,
                           want_f32=True)
        close(ops.h16_to_f32(out["raw"], M), h(ref), f"conv16 raw (K={K} M={M} ks={ks} s={stride} pad={pad} Tin={Tin})")
        close(ops.h16_to_f32(out["act"], M), h(O.elu(ref * np.float32(0.9))), "conv16 act")
        close(out["f32"], ref, "conv16 f32", tol=2e-4)
    else:
        out = ops.h16_conv(X16, w_pw, w_dw, bias, ks=ks, stride=stride, pad=pad, out_scale=float(s_out), want_raw=False, want_f32=True)
        close(out["f32"], ref.astype(np.float32), f"conv16 f32 (K={K} M={M} ks={ks} s={stride} pad={pad} Tin={Tin})", tol=2e-4)


def _random_block_shape(seed):
    """The shape draw of test_resblock16_random_lengths -> (rng, C, T, B)."""
    rng = np.random.default_rng(2000 + seed)
    C = int(rng.choice([32, 64, 96, 128, 192, 256, 384, 512, 768]))
    T = int(rng.integers(1, 700))
    B = int(rng.integers(1, 5))
    return rng, C, T, B


@pytest.mark.parametrize("seed", range(18))
def test_resblock16_random_lengths(ops, seed):
    rng, C, T, B = _random_block_shape(seed)
    X = h(rnd(rng, B, C, T))
    w1, w2 = rnd(rng, C, C, 1, scale=C ** -0.5), rnd(rng, C, C, 1, scale=C ** -0.5)
    d1, d2 = rnd(rng, C, 1, 5, scale=0.45), rnd(rng, C, 1, 5, scale=0.45)
    b1, b2 = rnd(rng, C, scale=0.1), rnd(rng, C, scale=0.1)
    pre, s_out = np.float32(rng.uniform(0.5, 1.0)), np.float32(rng.uniform(0.2, 0.6))
    y = resblock16_ref(X, w1, d1, b1, w2, d2, b2, pre, s_out)
    got = ops.h16_resblock(ops.h16_from_f32(cu(X)), w1, d1, b1, w2, d2, b2, pre_scale=float(pre), out_scale=float(s_out))
    close(ops.h16_to_f32(got, C), h(y), f"resblock16 C={C} T={T} B={B}")


@pytest.mark.parametrize("B,T", [(3, 16000), (2, 12345), (1, 333), (2, 48000)])
def test_detector_f16_mean_only_tail(detector, B, T):
    """Asked for the mean probabilities only, the f16 mode runs conv_post and the head on the f16 pipe too (L2Norm, head GEMM, sigmoid and
    the time mean in one kernel; the logits never exist).  Against the same mode's logits output (f32 conv_post + head): the same numbers
    to the f16 rounding of the latent."""
    from waveverify_amd.init import synthetic_clips
    x = torch.from_numpy(synthetic_clips(B, T, seed=3 * B + T)[0]).cuda()
    mp = detector.detector_mean_prob(x, precision="f16")
    lg = detector.detector(x, precision="f16")
    ref = torch.sigmoid(lg.double()).mean(dim=-1).float()
    assert float((mp - ref).abs().max()) <= 2e-4, float((mp - ref).abs().max())
    assert torch.equal(mp, detector.detector_mean_prob(x, precision="f16"))            # deterministic


# ================= round 4: the f16 mode through the Generator and the Locator =================
@pytest.mark.parametrize("K,M,Tin,r", [(1536, 768, 50, 8), (768, 384, 400, 5), (384, 192, 2000, 4), (192, 96, 8000, 2), (192, 96, 1, 2), (64, 32, 37, 3), (768, 384, 51, 5),
                                       (384, 192, 513, 4)])
def test_upsample_as_one_conv(ops, K, M, Tin, r):
    """The decoder's upsample unit ELU -> depth-wise ConvTranspose1d(2r, r), trimmed -> 1x1 + bias (seanet.py:1147-1170, conv.py:838-881)
    as ONE two-tap conv over (phase, channel) rows of the input frames: against the reference's two ops in float64 on the f16-rounded
    activated input (what the composed weight's f16 rounding costs: a few 1e-4 relative), and against the composition restated."""
    rng = np.random.default_rng(K + M + Tin + r)
    B = 2
    X = rnd(rng, B, K, Tin)
    w_ct, w_pw, b = rnd(rng, K, 1, 2 * r, scale=0.5), rnd(rng, M, K, 1, scale=K ** -0.5), rnd(rng, M, scale=0.1)
    pre = np.float32(0.7071)
    xa = h(O.elu(X * pre))
    two = upsample_plain(xa, w_ct, w_pw, b, r)
    # the composed weight as the packer rounds it: rows (p, m), tap 0 = frame l - 1 (ct[k][p + r]), tap 1 = frame l (ct[k][p])
    ref = upsample16_ref(xa, w_ct, w_pw, b, r)
    assert two.shape == ref.shape and np.abs(two - ref).max() <= COMPOSED_BOUND * max(1.0, np.abs(two).max())
    X16 = ops.h16_from_f32(cu(X), scale=float(pre), elu=True)
    got, gact = ops.h16_upsample(X16, w_ct, w_pw, b, r, act_scale=0.5)
    close(ops.h16_to_f32(got, M), h(ref), "upsample16")
    close(ops.h16_to_f32(gact, M), h(O.elu(ref * np.float32(0.5))), "upsample16 (activated copy)")
    assert torch.equal(ops.h16_upsample(X16, w_ct, w_pw, b, r), got)
    assert torch.equal(ops.h16_upsample(X16, w_ct, w_pw, b, r, act_scale=0.5, want_raw=False), gact)


@pytest.mark.parametrize("C,Tin,T,ks", [(96, 16000, 16000, 5), (96, 16320, 16001, 5), (96, 4, 3, 5), (96, 1000, 1000, 7), (48, 333, 330, 3), (8, 1, 1, 5)])
def test_tail16(ops, C, Tin, T, ks):
    rng = np.random.default_rng(C + Tin + ks)
    B = 3
    A = h(O.elu(rnd(rng, B, C, Tin)))
    w, b, x = rnd(rng, 1, C, ks, scale=(C * ks) ** -0.5), rnd(rng, 1, scale=0.1), rnd(rng, B, 1, T, scale=0.1)
    s = np.float32(0.1122080159)
    ref = np.tanh(O.sconv1d(A.astype(np.float64), w.astype(np.float64), b.astype(np.float64))[..., :T] * s).astype(np.float32)
    A16 = ops.h16_from_f32(cu(A))
    close(ops.h16_tail(A16, w, b, T, float(s)), ref, "tail16", tol=2e-6)
    close(ops.h16_tail(A16, w, b, T, float(s), x=cu(x)), ref + x, "tail16 + x", tol=2e-6)


@pytest.mark.parametrize("B,D,Fr", [(3, 128, 50), (2, 64, 500), (1, 128, 1), (2, 40, 7)])
def test_l2norm16(ops, B, D, Fr):
    rng = np.random.default_rng(D + Fr)
    X = rnd(rng, B, D, Fr)
    X[0, :, 0] = 0.0                                              # the eps branch (seanet.py:288-318)
    ref = X / np.maximum(np.sqrt((X.astype(np.float64) ** 2).sum(1, keepdims=True)), 1e-12) * np.sqrt(D)
    close(ops.h16_to_f32(ops.h16_l2norm(cu(X)), D), h(ref.astype(np.float32)), "l2norm16", tol=2.0 ** -11)


@pytest.mark.parametrize("K,M,Tin,r", [(64, 128, 16000, 2), (128, 256, 8000, 4), (256, 512, 2000, 5), (512, 1024, 400, 8), (512, 1024, 37, 8), (128, 256, 501, 4), (32, 64, 70, 4)])
def test_downsample_with_film(ops, K, M, Tin, r):
    """The generator's downsample unit: the composed conv with FiLM (seanet.py:928-966: per clip and band of M / 4 channels, y = gamma * y +
    beta) in its epilogue -- both conv kernels (x through LDS for stride >= 4 and M >= 256; straight from global memory else)."""
    rng = np.random.default_rng(K + M + Tin + 7)
    B, bands = 3, 4
    X = rnd(rng, B, K, Tin)
    w_pw, w_dw, b = rnd(rng, M, K, 1, scale=K ** -0.5), rnd(rng, M, 1, 2 * r, scale=(2 * r) ** -0.5), rnd(rng, M, scale=0.1)
    film = np.stack([rng.uniform(0.6, 1.4, (B, bands)), rng.normal(0, 0.3, (B, bands))], axis=-1).astype(np.float32)
    xa = h(O.elu(X * np.float32(0.7559)))
    wc = h(w_pw[:, :, 0][:, None, :] * w_dw[:, 0, :][:, :, None])
    Tout = (Tin + r - 1) // r
    ref = _dense_conv_ref(xa, wc, b, r, r, Tout)
    gam = np.repeat(film[:, :, 0], M // bands, axis=1)[:, :, None]
    bet = np.repeat(film[:, :, 1], M // bands, axis=1)[:, :, None]
    ref = (gam * ref + bet).astype(np.float32)
    X16 = ops.h16_from_f32(cu(X), scale=0.7559, elu=True)
    got, gact = ops.h16_conv_film(X16, w_pw, w_dw, b, cu(film), 2 * r, r, r, act_scale=0.8)
    close(ops.h16_to_f32(got, M), h(ref), "downsample16 + FiLM")
    close(ops.h16_to_f32(gact, M), h(O.elu(ref * np.float32(0.8))), "downsample16 + FiLM (activated copy)")


@pytest.fixture(scope="module")
def nets3():
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    out = {}
    for k in ("generator", "detector", "locator"):
        cfg = default_config(k)
        out[k] = HipNet(cfg, random_state_dict(cfg, 0))
    return out


WM_BAR = 1e-4        # north_star: watermarked-waveform samples within 1e-4 of the reference


@pytest.mark.parametrize("fixture", ["full_T16000", "full_T16001", "full_T4800", "speech_T16000"])
def test_generator_f16_vs_reference_golden(golden_dir, nets3, fixture):
    """wm of the f16 mode against the REFERENCE's own output: max|d| measured and held to north_star's 1e-4 (plain f16 storage of every
    stage suffices: tools/sim_f16.py predicted 5e-5, no stage needs the two-term split); the bits the reference's detector recovers from
    the reference's wm are recovered from this wm as well, by the exact detector and by the f16 one."""
    import os
    g = np.load(os.path.join(golden_dir, fixture + ".npz"))
    x, msg = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["msg"]).cuda()
    G, D = nets3["generator"], nets3["detector"]
    wm = G.generator(x, msg, add_input=True, precision="f16")
    err = float(np.abs(wm.cpu().numpy() - g["wm"]).max())
    print(f"{fixture}: f16-mode wm max|d| vs reference {err:.2e}")
    assert np.isfinite(wm.cpu().numpy()).all() and err <= WM_BAR, err
    delta = G.generator(x, msg, precision="f16")
    assert float((delta + x - wm).abs().max()) <= 1e-7
    for prec in ("f32", "f16"):
        mp = D.detector_mean_prob(wm, precision=prec).cpu().numpy()
        dp = float(np.abs(mp - g["det_mean_prob"]).max())
        decidable = np.abs(g["det_mean_prob"] - 0.5) > 4 * dp
        assert decidable.all() and ((mp >= 0.5).astype(np.int32) == g["det_bits"]).all(), (prec, dp)


@pytest.mark.parametrize("fixture", ["full_T16000", "full_T16001", "full_T4800", "speech_T16000"])
def test_locator_f16_vs_reference_golden(golden_dir, nets3, fixture):
    """Locator logits of the f16 mode against the reference's (sub-sampled in the fixture), and the binarised decisions (logit > 0.5,
    watermarking.py:717) wherever the reference's logit is further from the threshold than 4 x the measured error."""
    import os
    g = np.load(os.path.join(golden_dir, fixture + ".npz"))
    if "loc_logits_sub" not in g.files:
        pytest.skip("fixture holds no locator output")
    L = nets3["locator"]
    wm = torch.from_numpy(g["wm"]).cuda()
    lg = L.locator(wm, precision="f16").cpu().numpy()
    T = lg.shape[-1]
    step = -(-T // g["loc_logits_sub"].shape[-1])
    sub = lg[..., ::step]
    if sub.shape != g["loc_logits_sub"].shape:
        sub = lg[..., ::7]
    assert sub.shape == g["loc_logits_sub"].shape, (sub.shape, g["loc_logits_sub"].shape)
    ref = g["loc_logits_sub"]
    err = float(np.abs(sub - ref).max())
    print(f"{fixture}: f16-mode locator logits max|d| {err:.2e} (|logit| max {np.abs(ref).max():.2f})")
    assert err <= 0.03 * max(1.0, float(np.abs(ref).max())), err
    far = np.abs(ref - 0.5) > 4 * err
    assert ((sub > 0.5) == (ref > 0.5))[far].all() and far.mean() > 0.9
    lg32 = L.locator(wm).cpu().numpy()
    assert float(np.abs(lg - lg32).max()) <= 0.03 * max(1.0, float(np.abs(lg32).max()))


@pytest.mark.parametrize("B,T", [(1, 16000), (3, 12345), (2, 333), (1, 1), (2, 321), (1, 48001)])
def test_generator_locator_f16_shapes(nets3, B, T):
    """Ragged lengths and batch sizes through the whole f16 embed + locate: finite, within the wm bar of the exact path, independent of
    the batch a clip sits in, deterministic."""
    from waveverify_amd.init import synthetic_clips
    x_np, msg_np = synthetic_clips(B, T, seed=B + T)
    x, msg = torch.from_numpy(x_np).cuda(), torch.from_numpy(msg_np).cuda()
    G, L = nets3["generator"], nets3["locator"]
    wm = G.generator(x, msg, add_input=True, precision="f16")
    wm32 = G.generator(x, msg, add_input=True)
    assert torch.isfinite(wm).all() and float((wm - wm32).abs().max()) <= WM_BAR
    assert torch.equal(G.generator(x, msg, add_input=True, precision="f16"), wm)
    one = G.generator(x[B - 1:B].contiguous(), msg[B - 1:B].contiguous(), add_input=True, precision="f16")
    assert torch.equal(one[0], wm[B - 1])
    assert torch.equal(G.generator(x, msg[:1].contiguous().repeat(B, 1), add_input=True, precision="f16"),
                       G.generator(x, msg[:1].contiguous(), add_input=True, precision="f16"))          # one message for the batch (watermarking.py:320-329)
    lg = L.locator(wm, precision="f16")
    lg32 = L.locator(wm)
    assert torch.isfinite(lg).all() and float((lg - lg32).abs().max()) <= 0.03 * max(1.0, float(lg32.abs().max()))
    assert torch.equal(L.locator(wm[B - 1:B].contiguous(), precision="f16")[0], lg[B - 1])


def test_generator_f16_against_the_oracle_at_batch_8(nets3):
    """Eight synthetic clips (SURVEY 8d's inputs): wm of the f16 mode against the numpy oracle, max|d| <= 1e-4, BER 0 through both detectors."""
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict, synthetic_clips
    x_np, msg_np = synthetic_clips(8, 16000)
    cfg_g, cfg_d = default_config("generator"), default_config("detector")
    wm_ref = O.embed(cfg_g, random_state_dict(cfg_g, 0), x_np, msg_np)
    mp_ref = O.mean_probabilities(O.detector_forward(cfg_d, random_state_dict(cfg_d, 0), wm_ref))
    wm = nets3["generator"].generator(torch.from_numpy(x_np).cuda(), torch.from_numpy(msg_np).cuda(), add_input=True, precision="f16")
    err = float(np.abs(wm.cpu().numpy() - wm_ref).max())
    print(f"f16-mode wm max|d| vs oracle, 8 clips: {err:.2e}")
    assert err <= WM_BAR
    for prec in ("f32", "f16"):
        mp = nets3["detector"].detector_mean_prob(wm, precision=prec).cpu().numpy()
        assert ((mp >= 0.5) == (mp_ref >= 0.5)).all()


def test_f16_batch_1024_rows_equal_a_small_batch(nets3):
    """configs[4] at full size in the f16 mode (the c8 tensors cross 2 GiB there): rows {0, 512, 1016 ..} of a 1024-clip run are bit-equal to
    the same clips in an 8-clip run (mirror of test_detector_batch_1024 for the exact path)."""
    from waveverify_amd.init import synthetic_clips
    x_np, _ = synthetic_clips(8, 16000, seed=77)
    x8 = torch.from_numpy(x_np).cuda()
    big = x8.repeat(128, 1, 1).contiguous()                       # row i = clip i % 8
    D = nets3["detector"]
    mp8 = D.detector_mean_prob(x8, precision="f16")
    mp = D.detector_mean_prob(big, precision="f16")
    assert torch.isfinite(mp).all()
    for row in (0, 1, 511, 512, 1016, 1023):
        assert torch.equal(mp[row], mp8[row % 8]), row
    del big, mp
    torch.cuda.empty_cache()


def test_generator_f16_batch_256_rows_equal_a_small_batch(nets3):
    """The headline batch through the f16 generator: rows of a 256-clip run bit-equal to an 8-clip run (which the golden / oracle tests hold)."""
    from waveverify_amd.init import synthetic_clips
    x_np, msg_np = synthetic_clips(8, 16000, seed=78)
    x8, m8 = torch.from_numpy(x_np).cuda(), torch.from_numpy(msg_np).cuda()
    G = nets3["generator"]
    wm8 = G.generator(x8, m8, add_input=True, precision="f16")
    wm = G.generator(x8.repeat(32, 1, 1).contiguous(), m8.repeat(32, 1).contiguous(), add_input=True, precision="f16")
    for row in (0, 17, 128, 255):
        assert torch.equal(wm[row], wm8[row % 8]), row
    del wm
    torch.cuda.empty_cache()


def test_generator_f16_captures_into_a_hip_graph(nets3):
    from waveverify_amd.init import synthetic_clips
    x_np, msg_np = synthetic_clips(2, 8000, seed=5)
    x, msg = torch.from_numpy(x_np).cuda(), torch.from_numpy(msg_np).cuda()
    G = nets3["generator"]
    w0 = G.generator(x, msg, add_input=True, precision="f16")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        G.generator(x, msg, add_input=True, precision="f16")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        w1 = G.generator(x, msg, add_input=True, precision="f16")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(w1, w0)


def _other_configuration(seed):
    """Configuration `seed` (0 .. 5) of the sweep below -> (generator kwargs, detector / locator kwargs, T)."""
    from waveverify_amd.config import default_config
    rng = np.random.default_rng(4000 + seed)
    strides = [[8, 5, 4, 2], [8, 4, 2], [5, 4, 2], [8, 5, 4, 2], [4, 4, 2], [8, 5, 2]][seed]
    ce = [64, 32, 64, 32, 96, 64][seed]
    cd = 96                                                      # decoder stages 768 / 384 / 192 / 96 (four strides) or 384 / 192 / 96
    kw = dict(channels_enc=ce, strides=strides, n_residual_enc=int(rng.integers(1, 3)))
    gkw = dict(channels_dec=cd, n_residual_dec=int(rng.integers(1, 4)), freq_bands=int(rng.choice([2, 4])), **kw)
    return gkw, kw, int(rng.choice([16000, 8000, 12345]))


@pytest.mark.parametrize("seed", range(6))
def test_f16_mode_on_other_configurations(seed):
    """The mode on configurations OTHER than the defaults, inside the f16 kernels' coverage (stage widths 32 ... 768, k = 5, dilation 1):
    other base widths (so that the SpecBlocks take the fallback path or the half-channel kernel), other block counts, strides and FiLM
    band counts.  Against the exact path of this library on the same weights (which tests/test_gpu_fuzz.py holds to the oracle): wm within
    the 1e-4 bar, bits equal, locator logits within 3 % of their range."""
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict, synthetic_clips
    from waveverify_amd.nets import HipNet
    gkw, kw, T = _other_configuration(seed)
    cg = default_config("generator", **gkw)
    cdt = default_config("detector", **kw)
    cl = default_config("locator", **kw)
    G, D, L = (HipNet(c, random_state_dict(c, 10 + seed)) for c in (cg, cdt, cl))
    x_np, msg_np = synthetic_clips(3, T, seed=seed)
    x, msg = torch.from_numpy(x_np).cuda(), torch.from_numpy(msg_np).cuda()
    try:
        wm16 = G.generator(x, msg, add_input=True, precision="f16")
    except RuntimeError as e:                                    # a stage outside the kernels' set: the mode says so, the exact path runs
        assert "f16" in str(e)
        G.generator(x, msg, add_input=True)
        pytest.skip(f"configuration outside the f16 plan: {e}")
    wm = G.generator(x, msg, add_input=True)
    assert torch.isfinite(wm16).all() and float((wm16 - wm).abs().max()) <= 1e-4, float((wm16 - wm).abs().max())
    mp, mp16 = D.detector_mean_prob(wm), D.detector_mean_prob(wm16, precision="f16")
    dp = float((mp - mp16).abs().max())
    far = (mp - 0.5).abs() > 4 * dp
    assert dp <= 2e-2 and torch.equal((mp16 >= 0.5)[far], (mp >= 0.5)[far])
    lg, lg16 = L.locator(wm), L.locator(wm, precision="f16")
    assert float((lg - lg16).abs().max()) <= 0.03 * max(1.0, float(lg.abs().max()))


def test_generator_f16_against_the_oracle_of_its_own_arithmetic(nets3):
    """oracle/wv_oracle_h16.py restates the MODE's arithmetic on the CPU: the pinned torch port of the reference path with a round-to-f16
    at every point where a kernel of the mode rounds (and float64 sums).  A whole net in f16 storage is its own noise amplifier -- one
    activation that lands on the other side of a rounding boundary (f32 vs f64 sums) moves the output as much as the rounding noise itself
    -- so GPU and oracle agree at the level at which both agree with the exact path (measured 3.7e-5 / 3.2e-5 / 3.6e-5), not tighter; a
    rounding point in the wrong place or a misplaced log2(e) shows up at 1e-3 and more.  All three distances are held to north_star's 1e-4."""
    from oracle import wv_oracle_h16 as O16
    from oracle import wv_oracle_torch as OT
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict, synthetic_clips
    cfg = default_config("generator")
    net = OT.Net(cfg, random_state_dict(cfg, 0))
    x_np, msg_np = synthetic_clips(2, 8000, seed=21)
    ref16 = O16.embed(net, x_np, msg_np).numpy()
    exact = OT.embed(net, x_np, msg_np).numpy()
    got = nets3["generator"].generator(torch.from_numpy(x_np).cuda(), torch.from_numpy(msg_np).cuda(), add_input=True, precision="f16").cpu().numpy()
    d_or, d_ex, o_ex = float(np.abs(got - ref16).max()), float(np.abs(got - exact).max()), float(np.abs(ref16 - exact).max())
    print(f"f16 mode: GPU vs its oracle {d_or:.2e}; GPU vs exact {d_ex:.2e}; oracle vs exact {o_ex:.2e}")
    assert d_ex <= 1e-4 and o_ex <= 1e-4 and d_or <= 1e-4, (d_or, d_ex, o_ex)


# ---- the detector and the locator against the oracle of the mode's own arithmetic (oracle/wv_oracle_h16.py: detect_mean_prob, the head16
# tail; detect_logits / locate, the f32 tail).  Bars from the MI355X, far under the 2e-2 / 3 % the comparisons above allow.
# What sets them is the encoder's f16 stream ahead of the tails (an f16 activation that rounds the other way, f32 vs float64 sums, in
# any stage): the rounding points of spec_post / conv_post move the logits by less than the measured distance (oracle variants: 1.3e-4 ..
# 1.6e-4 relative), so these bars cannot see one misplaced rounding in the tails -- tests/test_gpu_h16_head.py does that for head16 --
# but they do see a wrong length in the time mean (T rounded up to whole frames: 3.4e-4 at T = 12345) or spec_post normalised with the
# previous scale's mean and std (logits 2.9e-2, mean 4.3e-4).
# Measured: mean probabilities 1.7e-6 (T >= 8000), 1.2e-5 (T = 333), 6.4e-5 (T = 1: one sample is the mean); logits 2.1e-4 of
# max(1, |logits|max) on the default nets, 4.4e-4 on the configuration sweep.
LOGIT_BAR = 1e-3


def det_mean_bar(T: int) -> float:
    """2e-5 plus the per-sample noise (~2e-4 in probability) averaged over the clip: 2.2e-4 at T = 1, 3.1e-5 at T = 333, 2.2e-5 at 16000."""
    return 2e-5 + 2e-4 / T ** 0.5


def _oracle_net(cfg, seed):
    from oracle import wv_oracle_torch as OT
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    sd = random_state_dict(cfg, seed)
    return HipNet(cfg, sd), OT.Net(cfg, sd)


def _vs_oracle(what, got, ref, bar, scale=1.0):
    got, ref = got.detach().double().cpu().numpy(), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) / scale
    print(f"MEASURE {what}: {err:.2e}")
    assert np.isfinite(got).all() and err <= bar, (what, err)


@pytest.fixture(scope="module")
def oracle_nets():
    from waveverify_amd.config import default_config
    return {k: _oracle_net(default_config(k), 0) for k in ("detector", "locator")}


@pytest.mark.parametrize("B,T", [(2, 16000), (1, 12345), (3, 333), (1, 1)])
def test_detector_f16_mean_prob_vs_its_oracle(oracle_nets, B, T):
    """Mean probabilities of the f16 mode (the head16 tail: f16 conv_post, head16_kernel) against oracle/wv_oracle_h16.detect_mean_prob,
    held to det_mean_bar(T) (measured 1.7e-6 / 1.7e-6 / 1.2e-5 / 6.4e-5 at these shapes)."""
    from oracle import wv_oracle_h16 as O16
    from waveverify_amd.init import synthetic_clips
    hip, net = oracle_nets["detector"]
    x = synthetic_clips(B, T, seed=B + T)[0]
    _vs_oracle(f"detector f16 mean B={B} T={T}", hip.detector_mean_prob(torch.from_numpy(x).cuda(), precision="f16"),
               O16.detect_mean_prob(net, x), det_mean_bar(T))


@pytest.mark.parametrize("kind", ["detector", "locator"])
@pytest.mark.parametrize("B,T", [(2, 16000), (1, 12345), (3, 333), (1, 1)])
def test_f16_logits_vs_the_f32_tail_oracle(oracle_nets, kind, B, T):
    """Detector and locator logits of the f16 mode, element by element, against the f32-tail oracle (spec_post on the f16 pipe with its
    x' in f32, then the exact conv_post / L2Norm / head), relative to max(1, |logits|max): measured 2.1e-4 at most, bar LOGIT_BAR."""
    from oracle import wv_oracle_h16 as O16
    from waveverify_amd.init import synthetic_clips
    hip, net = oracle_nets[kind]
    x = synthetic_clips(B, T, seed=B + T)[0]
    ref = O16.detect_logits(net, x).numpy()
    got = hip.detector(torch.from_numpy(x).cuda(), precision="f16") if kind == "detector" else hip.locator(torch.from_numpy(x).cuda(), precision="f16")
    _vs_oracle(f"{kind} f16 logits B={B} T={T}", got, ref, LOGIT_BAR, max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("case", [f"sweep{s}" for s in range(6)] + ["nbits8", "nbits20", "nbits36"])
def test_f16_detector_and_locator_on_other_configurations_vs_the_oracle(case):
    """The six configurations of test_f16_mode_on_other_configurations (SpecBlocks on the fallback path or the half-channel kernel, other
    strides and block counts) and detectors of 8, 20 and 36 bits (36: more than head16_kernel takes, so the mean output runs the f32 tail):
    mean probabilities and logits against the oracle, with the tail head16_gate picks."""
    from oracle import wv_oracle_h16 as O16
    from waveverify_amd.config import default_config
    from waveverify_amd.init import synthetic_clips
    if case.startswith("sweep"):
        _, kw, T = _other_configuration(int(case[5:]))
        cfgs = [default_config("detector", **kw), default_config("locator", **kw)]
    else:
        cfgs, T = [default_config("detector", nbits=int(case[5:]))], 16000
    x = synthetic_clips(3, T, seed=len(case) + T)[0]
    xt = torch.from_numpy(x).cuda()
    for cfg in cfgs:
        hip, net = _oracle_net(cfg, 7)
        ref = O16.detect_logits(net, x).numpy()
        scale = max(1.0, float(np.abs(ref).max()))
        if cfg.kind == "detector":
            _vs_oracle(f"{case} detector f16 mean (head16 tail: {O16.head16_gate(cfg)})", hip.detector_mean_prob(xt, precision="f16"),
                       O16.detect_mean_prob(net, x), det_mean_bar(T))
            _vs_oracle(f"{case} detector f16 logits", hip.detector(xt, precision="f16"), ref, LOGIT_BAR, scale)
        else:
            _vs_oracle(f"{case} locator f16 logits", hip.locator(xt, precision="f16"), ref, LOGIT_BAR, scale)
