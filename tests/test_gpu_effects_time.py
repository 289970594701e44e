"""The reference's plain-arithmetic time-domain effects on the GPU (csrc/wv_fx_time.hip, waveverify_amd/effects.py) against
tests/golden/effects_time.npz: the REFERENCE's own apply_effect run on the CPU, forward and autograd, under fixed seeds
(tests/golden/make_golden_effects_time.py).  One substitution was made there: julius.fft_conv1d is absent and
torch.nn.functional.conv1d stood in for it, which computes the same cross-correlation without the FFT's rounding.

Bit for bit (np.array_equal: -0.0 equals 0.0; NaN-aware for the 1-bit quantisation): median_filter, quantization, amplitude_scaling,
shush (audio, keep mask through its gradient, mask), sample_suppression, pink_noise, the noise adds given the noise, smooth's mask,
and every straight-through gradient.  Within the project's filter bar, 2e-5 of the output's peak (test_gpu_effects.py): echo,
smooth's audio, the linear stretch and the echo / smooth gradients -- float sums whose order is not the CPU's.  The echo gradient
needs no wider bar: the reference's own float32-versus-float64 autograd difference on these cases, stored in the fixture as
<case>_grad_f32_f64, is 5e-8 .. 5e-7 of the gradient's peak.  `speed` is PARITY UNPINNED (SoX is absent) and is held to the
resampler's round-trip bar only."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from guard import Guards
from waveverify_amd import _lib
from waveverify_amd import effects as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "effects_time.npz"))
CASES = json.loads(str(GOLD["cases"]))
SR = 16000
BAR = 2e-5
BIT_EXACT = ("median_filter", "quantization", "amplitude_scaling", "shush", "sample_suppression", "pink_noise")
GRID = {"identity": {}, "highpass_filter": {"cutoff_freq": {"choices": [500, 3500]}}, "lowpass_filter": {"cutoff_freq": {"choices": [1000, 2000]}},
        "bandpass_filter": {"cutoff_freq_low": {"choices": [300]}, "cutoff_freq_high": {"choices": [4000]}}, "speed": {"speed": {"choices": [0.8]}},
        "resample": {"new_sample_rate": {"choices": [32000]}}, "random_noise": {"noise_std": {"choices": [0.001]}}}       # model/watermarking.py:146-167


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def rel(got, ref):
    g = got.detach().cpu().numpy().astype(np.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    return float(np.abs(g - ref).max() / max(1e-12, np.abs(ref).max()))


def same(got, ref):
    return np.array_equal(got.detach().cpu().numpy(), ref, equal_nan=True)


def ids(names):
    return [c["key"] + "-" + c["name"] for c in CASES if c["name"] in names]


def pick(names):
    return [c for c in CASES if c["name"] in names]


def inputs(c):
    T = c["T"]
    return GOLD[f"x_{T}"], GOLD[f"mask_{T}"], GOLD[f"r_{T}"]


def want_grad(c, r):
    return r if f"{c['key']}_grad_is_r" in GOLD.files else GOLD[c["key"] + "_grad"]


@pytest.mark.parametrize("c", pick(BIT_EXACT), ids=ids(BIT_EXACT))
def test_bit_exact_effects_match_the_reference(c):
    x, mask, r = inputs(c)
    tape = E.EffectTape(SR)
    seed_all(c["seed"])
    y, m = tape.apply(c["name"], c["params"], cu(x), cu(mask))
    dx = tape.backward(c["name"], c["params"], cu(r))
    print(c["key"], c["name"], c["params"], "audio differs at", int((y.cpu().numpy() != GOLD[c["key"] + "_y"]).sum()), "samples")
    assert same(y, GOLD[c["key"] + "_y"]), "audio"
    assert same(m, GOLD[c["key"] + "_m"]), "mask"
    assert same(dx, want_grad(c, r)), "gradient"
    if c["name"] == "median_filter":
        assert c["params"]["kernel_size"] in (3, 5, 31, 4, 33) and E.MEDIAN_MAX_K >= 33 > 31        # both routes of the kernel are in the fixture
    if c["name"] == "shush":
        k = min(int(c["T"] * c["params"]["fraction"]), c["T"] - 1)
        _, keep, _ = E.shush_forward(cu(x), k)
        kz = keep.cpu().numpy()
        assert set(np.unique(kz)) <= {0.0, 1.0} and ((kz == 0).sum(-1) == k).all()


@pytest.mark.parametrize("c", pick(("random_noise", "white_noise")), ids=ids(("random_noise", "white_noise")))
def test_noise_add_matches_the_reference_given_the_noise(c):
    x, mask, r = inputs(c)
    y = E.pointwise(cu(x), E.OP_ADD_NOISE, c["params"]["noise_std"], cu(GOLD[c["key"] + "_noise"]))
    assert same(y, GOLD[c["key"] + "_y"])
    assert f"{c['key']}_grad_is_r" in GOLD.files and np.array_equal(GOLD[c["key"] + "_m"], mask)       # identity gradient, mask untouched


@pytest.mark.parametrize("c", pick(("echo", "smooth")), ids=ids(("echo", "smooth")))
def test_echo_and_smooth_match_the_reference(c):
    x, mask, r = inputs(c)
    tape = E.EffectTape(SR)
    seed_all(c["seed"])
    y, m = tape.apply(c["name"], c["params"], cu(x), cu(mask))
    dx = tape.backward(c["name"], c["params"], cu(r))
    ey, eg = rel(y, GOLD[c["key"] + "_y"].astype(np.float64)), rel(dx, GOLD[c["key"] + "_grad"].astype(np.float64))
    print(c["key"], c["name"], c["params"], f"audio {ey:.3g} gradient {eg:.3g} of the peak")
    assert same(m, GOLD[c["key"] + "_m"]), "mask"
    assert ey <= BAR, ey
    assert eg <= BAR, eg
    if c["name"] == "echo":
        n = int(GOLD[c["key"] + "_n"])
        assert float(GOLD[c["key"] + "_grad_f32_f64"]) <= BAR / 2           # the reference's own f32 error leaves the bar where it is
        assert not y[..., c["T"] - n + 1:].any() and m.data_ptr() != 0
    else:
        assert int(GOLD[c["key"] + "_w"]) >= 2


def test_linear_stretch_matches_interpolate():
    for tin, tout in GOLD["stretch"]:
        x = GOLD[f"stretch_{tin}_{tout}_x"]
        y = E.stretch_linear(cu(x), int(tout))
        e = rel(y, GOLD[f"stretch_{tin}_{tout}_y"].astype(np.float64))
        print("stretch", tin, tout, f"{e:.3g}")
        assert e <= BAR, (tin, tout, e)


def _dot(a, b):
    return float((a.double() * b.double()).sum())


@pytest.mark.parametrize("T", [1001, 37])
@pytest.mark.parametrize("w", [2, 3, 7, 10])
def test_smooth_backward_is_the_transposed_operator(w, T):
    g = torch.Generator(device="cuda").manual_seed(T + w)
    x = torch.randn(2, 1, T, device="cuda", generator=g) * 0.1
    d = torch.randn(2, 1, T, device="cuda", generator=g)
    y, _ = E.smooth_forward(x, w)
    dx = E.smooth_backward(d, w)
    lhs, rhs = _dot(y, d), _dot(x, dx)
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), float(y.norm() * d.norm()) * 1e-2, 1e-6), (lhs, rhs)


def test_shush_with_ties_zeroes_exactly_k_and_nothing_above_the_threshold():
    rng = np.random.default_rng(5)
    x = (np.round(rng.standard_normal((3, 1, 4001)) * 4) / 4).astype(np.float32)          # a handful of distinct magnitudes, zeros among them
    T = x.shape[-1]
    for fraction in (0.3, 0.05, 0.7):
        k = min(int(T * fraction), T - 1)
        y, keep, _ = E.shush_forward(cu(x), k)
        y, keep = y.cpu().numpy().reshape(3, T), keep.cpu().numpy().reshape(3, T)
        for row, yr, kr in zip(x.reshape(3, T), y, keep):
            a = np.abs(row)
            thr = np.sort(a)[k - 1]
            gone = kr == 0
            assert gone.sum() == k and np.array_equal(yr, row * kr)
            assert (a[gone] <= thr).all() and gone[a < thr].all()                       # none above the threshold, all below it
            at = np.flatnonzero(a == thr)
            n_at = int(gone[at].sum())
            assert gone[at[:n_at]].all() and not gone[at[n_at:]].any()                  # of the equal ones, the earliest


def test_random_noise_on_the_device():
    x = torch.zeros(1, 1, 16000, device="cuda")
    mask = torch.ones_like(x)
    torch.manual_seed(7)
    y, m = E.AudioEffects.random_noise(x + 0.25, noise_std=0.01, mask=mask)
    assert y.shape == x.shape and m is mask
    d = (y - 0.25).cpu().numpy().astype(np.float64)
    assert abs(d.std() - 0.01) <= 0.05 * 0.01, d.std()
    torch.manual_seed(7)
    y2, _ = E.AudioEffects.random_noise(x + 0.25, noise_std=0.01, mask=mask)
    assert torch.equal(y, y2)
    y3, _ = E.AudioEffects.white_noise(x, noise_std=-1.0)                                    # fail-safe: an invalid argument returns the input
    assert y3 is x


def test_speed_keeps_length_mask_and_a_tone():
    T = 16000
    t = np.arange(T) / SR
    tone = cu((0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)[None, None])
    mask = torch.ones_like(tone)
    y, m = E.apply_effect("speed", {"speed": 0.8}, tone, mask)
    assert y.shape == tone.shape and m is mask
    mid = slice(T // 4, 3 * T // 4)
    assert float((y[..., mid] - tone[..., mid]).abs().max()) <= 2e-2
    random.seed(3)
    y2, _ = E.AudioEffects.speed(tone, speed=(0.9, 1.1))
    assert y2.shape == tone.shape
    assert E.AudioEffects.speed(tone, speed=-1.0)[0] is tone


def test_wrappers_keep_the_reference_conventions():
    x = torch.randn(2, 1, 400, device="cuda") * 0.1
    mask = torch.ones_like(x)
    assert E.AudioEffects.median_filter(x, kernel_size=0, mask=mask)[0] is x                # the reference catches its own ValueError
    with pytest.raises(ValueError, match=str(E.MEDIAN_MAX_K)):
        E.AudioEffects.median_filter(x, kernel_size=E.MEDIAN_MAX_K + 2)
    assert E.AudioEffects.quantization(x, bit_depth=33)[0] is x
    assert E.AudioEffects.shush(x, fraction=1.5)[0] is x
    assert E.AudioEffects.sample_suppression(x, suppression_percentage=2.0, mask=mask)[1] is mask
    assert E.AudioEffects.echo(x[..., :1])[0].shape[-1] == 1                                 # too short: unchanged
    y, m = E.AudioEffects.sample_suppression(x, 0.25, mask=mask)
    assert int((y == 0).sum()) >= 2 * 100 and torch.equal(m == 0, y == 0) and bool(mask.all())   # the caller's mask is not written
    with pytest.raises(NotImplementedError, match="biquad"):
        E.apply_effect("random_equalization", {}, x, mask)


def test_effect_tape_pairs_each_backward_with_its_forward():
    x = torch.randn(1, 1, 2000, device="cuda") * 0.1
    d = torch.randn(1, 1, 2000, device="cuda")
    tape = E.EffectTape()
    torch.manual_seed(11)
    plan = [("shush", {"fraction": 0.2}), ("amplitude_scaling", {"scale": 0.5}), ("sample_suppression", {"suppression_percentage": 0.1}),
            ("lowpass_filter", {"cutoff_freq": 2000}), ("smooth", {"window_size_range": (4, 5)}), ("quantization", {"bit_depth": 8}),
            ("echo", {"duration_range": (0.01, 0.02)})]
    outs = [tape.apply(n, p, x, None)[0] for n, p in plan]
    assert len(tape) == len(plan)
    grads = [tape.backward(n, p, d) for n, p in plan]
    assert len(tape) == 0
    assert torch.equal(grads[0], d * (outs[0] != 0)) and int((grads[0] == 0).sum()) == 400
    assert torch.equal(grads[1], d * 0.5)
    assert torch.equal(grads[2], d * (outs[2] != 0)) and int((grads[2] == 0).sum()) == 200
    assert torch.equal(grads[3], E.lowpass_adjoint(d, 0.25))
    assert torch.equal(grads[4], E.smooth_backward(d, 4))
    assert grads[5] is d
    assert not torch.equal(grads[6], d) and torch.isfinite(grads[6]).all()
    tape.apply("shush", {"fraction": 0.2}, x, None)
    with pytest.raises(RuntimeError, match="does not match"):
        tape.backward("smooth", {}, d)
    with pytest.raises(RuntimeError, match="nothing was applied"):
        tape.backward("shush", {}, d)


def test_trainer_runs_the_shipped_effect_schedule():
    """THE HEADLINE: a WatermarkTrainer with an EffectScheduler over the reference's shipped grid (model/watermarking.py:146-167: nine
    effect settings of seven names, `speed` and `random_noise` among them) and EffectTape hooks runs three steps with finite losses,
    and effect_update_count advances by the number selected.  Seed 42 makes the first selection lowpass, random_noise, resample, speed,
    highpass, highpass, identity."""
    from waveverify_amd.config import default_config
    from waveverify_amd.effect_scheduler import EffectScheduler
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import WatermarkTrainer
    small = dict(channels_enc=8, dimension=16, strides=[2, 2], n_fft_base=16)
    cg = default_config("generator", channels_dec=8, n_residual_dec=1, **small)
    cd, cl = default_config("detector", output_dim=8, **small), default_config("locator", output_dim=8, **small)
    np.random.seed(42)
    torch.manual_seed(42)
    sched, tape = EffectScheduler(GRID), E.EffectTape(SR)
    tr = WatermarkTrainer(cg, random_state_dict(cg, 1, parametrized=True), cd, random_state_dict(cd, 1, parametrized=True), cl,
                          random_state_dict(cl, 1, parametrized=True), effect_scheduler=sched, apply_effect=tape.apply, effect_backward=tape.backward)
    x = torch.randn(8, 1, 1600, device="cuda") * 0.1
    msg = torch.randint(0, 2, (8, 16), device="cuda").float()
    for step in range(3):
        before = tr.effect_update_count
        out = tr.step(x, msg, augment=False)
        assert np.isfinite(float(out["loss"].item())), step
        assert tr.effect_update_count - before == 7 and len(tape) == 0
    assert sched.total_effects == 21
    assert {"speed", "random_noise"} <= {n for n, c in sched.effect_usage_stats.items() if c > 0}


# ---- guard bands: every new entry point between NaN guards, ragged T, one element past a 16-byte boundary ----------------------------
def _p(a):
    return C.c_void_p(a.t.data_ptr()) if a is not None else None


def bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


@pytest.mark.parametrize("offset", [0, 1])
def test_time_effects_guarded(offset):
    """Every entry point of csrc/wv_fx_time.hip through the C ABI on guarded ragged clips (rows * T % 4 != 0; offset = 1 puts every
    operand one element past a 16-byte boundary): inputs bitwise unchanged, guards intact, every promised element written (median's and
    smooth's edge windows and echo's zero tail included), results bit-equal to the wrappers on fresh tensors, which the tests above
    hold to the reference."""
    lib = _lib.load()
    rng = np.random.default_rng(23)
    R, T = 3, 1003
    x = (0.3 * rng.standard_normal((R, T))).astype(np.float32)
    z = rng.standard_normal((R, T)).astype(np.float32)
    mk = (rng.random((R, T)) > 0.3).astype(np.float32)
    xf, zf, mf = cu(x), cu(z), cu(mk)
    s = None

    def fresh():
        g = Guards(offset=offset)
        return g, g.input(x, "x"), g.input(z, "z"), g.input(mk, "mask")

    for op, a in ((E.OP_SCALE, 0.7), (E.OP_ADD_NOISE, 0.01), (E.OP_QUANTIZE, 127.0), (E.OP_MUL, 0.0)):
        g, xg, zg, _ = fresh()
        y = g.output((R, T), name=f"pointwise{op}")
        assert lib.wv_fx_pointwise(_p(xg), _p(zg), _p(y), R, T, op, a, s) == 0
        g.check()
        assert torch.equal(bits(y.t), bits(E.pointwise(xf, op, a, zf)))
    for k in (5, 31, 33):
        g, xg, _, _ = fresh()
        y = g.output((R, T), name=f"median{k}")
        assert lib.wv_fx_median(_p(xg), _p(y), R, T, k, s) == 0
        g.check()
        assert torch.isfinite(y.t).all() and torch.equal(bits(y.t), bits(E.median(xf, k)))
    assert lib.wv_fx_median(_p(xg), _p(y), R, T, 4, s) != 0 and lib.wv_fx_median(_p(xg), _p(y), R, T, E.MEDIAN_MAX_K + 2, s) != 0
    for k in (0, 100, T - 1):
        g, xg, _, mg = fresh()
        y, keep, mo = g.output((R, T), name="shush y"), g.output((R, T), name="keep"), g.output((R, T), name="shush mask")
        assert lib.wv_fx_shush(_p(xg), _p(mg), _p(y), _p(keep), _p(mo), R, T, k, s) == 0
        g.check()
        ry, rk, rm = E.shush_forward(xf, k, mf)
        assert torch.equal(bits(y.t), bits(ry)) and torch.equal(bits(keep.t), bits(rk)) and torch.equal(bits(mo.t), bits(rm))
        assert int((keep.t == 0).sum()) == R * k
    assert lib.wv_fx_shush(_p(xg), _p(mg), _p(y), _p(keep), _p(mo), R, T, T, s) != 0
    n, vol = 301, 0.4
    g, xg, zg, _ = fresh()
    rec, y = g.output((2,), torch.int64, name="echo record"), g.output((R, T), name="echo y")
    assert lib.wv_fx_echo_peaks(_p(xg), _p(rec), R, T, n, vol, s) == 0 and lib.wv_fx_echo_apply(_p(xg), _p(rec), _p(y), R, T, n, vol, s) == 0
    g.check()
    ry, rrec = E.echo_forward(xf, n, vol)
    assert torch.equal(rec.t, rrec) and torch.equal(bits(y.t), bits(ry)) and not y.t[:, T - n + 1:].any() and y.t[:, : T - n + 1].all()
    assert abs(float(y.t.abs().max()) - float(np.abs(x).max())) <= 1e-6
    g = Guards(offset=offset)
    xg, zg, rg = g.input(x, "x"), g.input(z, "g"), g.input(rrec, "echo record")
    dx = g.output((R, T), name="echo dx")
    nbytes = int(lib.wv_fx_echo_backward_workspace_bytes())
    ws = g.workspace(nbytes, "echo workspace")
    runs = []
    for _ in range(2):
        g.repoison()
        assert lib.wv_fx_echo_backward(_p(xg), _p(zg), _p(rg), _p(dx), R, T, n, vol, _p(ws), nbytes, s) == 0
        g.check()
        runs.append(bits(dx.t))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], bits(E.echo_backward(xf, zf, rrec, n, vol)))
    assert lib.wv_fx_echo_backward(_p(xg), _p(zg), _p(rg), _p(dx), R, T, n, vol, _p(ws), nbytes - 4, s) != 0
    for w in (2, 7, 10):
        g, xg, zg, mg = fresh()
        y, mo, dx = g.output((R, T), name="smooth y"), g.output((R, T), name="smooth mask"), g.output((R, T), name="smooth dx")
        assert lib.wv_fx_smooth(_p(xg), _p(mg), _p(y), _p(mo), R, T, w, 0.5, s) == 0
        assert lib.wv_fx_smooth_backward(_p(zg), _p(dx), R, T, w, s) == 0
        g.check()
        ry, rm = E.smooth_forward(xf, w, mf, 0.5)
        assert torch.equal(bits(y.t), bits(ry)) and torch.equal(bits(mo.t), bits(rm)) and torch.equal(bits(dx.t), bits(E.smooth_backward(zf, w)))
    idx = np.stack([rng.permutation(T)[:100] for _ in range(R)]).astype(np.int32)
    g = Guards(offset=offset)
    ig = g.input(idx, "idx")
    y, mo = g.output((R, T), name="scatter y"), g.output((R, T), name="scatter mask")
    y.t.copy_(xf)
    mo.t.copy_(mf)
    assert lib.wv_fx_scatter_zero(_p(y), _p(mo), _p(ig), R, T, 100, s) == 0
    g.check()
    want, wantm = x.copy(), mk.copy()
    np.put_along_axis(want, idx.astype(np.int64), 0.0, axis=1)
    np.put_along_axis(wantm, idx.astype(np.int64), 0.0, axis=1)
    assert np.array_equal(y.t.cpu().numpy(), want) and np.array_equal(mo.t.cpu().numpy(), wantm)
    for tout in (801, 1254):
        g, xg, _, _ = fresh()
        y = g.output((R, tout), name=f"stretch {tout}")
        assert lib.wv_fx_stretch_linear(_p(xg), _p(y), R, T, tout, s) == 0
        g.check()
        assert torch.isfinite(y.t).all() and torch.equal(bits(y.t), bits(E.stretch_linear(xf, tout)))
