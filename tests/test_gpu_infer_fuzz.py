"""Geometry fuzz of the exact f32 inference kernels, route by route, against the float64 oracle (oracle/wv_oracle.py with dtype=float64).

Every kernel-level case of tests/infer_fuzz_cases.py runs through waveverify_amd.ops with the library's profiler on: the kernel name it
collected must be the one the restated launcher predicted (so tests/test_infer_fuzz_cases_cpu.py's route counts are facts about the
library), every output is held to the float64 oracle at 2e-5 of the reference tensor's largest magnitude -- no floor at 1.0 -- and a
second call must be bit-equal.  Where the project holds a route bit-equal to a two-kernel form, that is asserted too.  Whole nets run
against the float64 oracle at 5e-5 (generator) / 1e-4 (detector, locator), and their profile must be the restated launch plan.
Each figure is printed before it is asserted (pytest -s)."""
import zlib

import numpy as np
import pytest
import torch

import infer_fuzz_cases as C
from oracle import wv_oracle as O

pytestmark = pytest.mark.gpu

D = np.float64
BAR = 2e-5                                                        # forward, of the reference tensor's largest magnitude


@pytest.fixture(scope="module")
def ops():
    from waveverify_amd import ops as _ops
    from waveverify_amd import profile
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    profile.enable(True)
    yield _ops
    profile.enable(False)


def launched(fn):
    """Run fn with a fresh profile -> (its result, {kernel name: launches}, {(role, kernel): launches})."""
    from waveverify_amd import profile
    profile.reset()
    out = fn()
    by_kernel, by_role = {}, {}
    for e in profile.collect():
        by_kernel[e["kernel"]] = by_kernel.get(e["kernel"], 0) + e["launches"]
        by_role[(e["role"], e["kernel"])] = by_role.get((e["role"], e["kernel"]), 0) + e["launches"]
    return out, by_kernel, by_role


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def rnd(rng, *shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hold(got, ref, what, bar=BAR, extra=None):
    """|got - ref| <= bar * |ref|max (+ extra, an element-wise allowance the caller derives), printed before it is asserted."""
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    mag = float(np.abs(ref).max()) if ref.size else 0.0
    d = np.abs(got.astype(D) - ref)
    err = float(d.max()) if ref.size else 0.0
    print(f"FIG {what}: err {err:.3e} |ref|max {mag:.3e} rel {err / mag if mag else 0.0:.3e} bar {bar:.1e}")
    lim = bar * mag + (extra if extra is not None else 0.0)
    assert (d <= lim).all(), f"{what}: max|d| = {err:.3e}, bar {bar:.1e} x |ref|max {mag:.3e}"


def same(a, b, what):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), f"{what}: a second call is not bit-equal"


def ids(cases):
    return ["-".join(str(int(v) if isinstance(v, (bool, np.bool_)) else v) for v in c) for c in cases]


# ---- pw_dw -------------------------------------------------------------------------------------------------------------------------------
PW_DW = C.pw_dw_cases()


@pytest.mark.parametrize("case", PW_DW, ids=ids(PW_DW))
def test_pw_dw_fuzz(ops, case):
    B, K, M, T, ks, stride, dil, pre, epi, act = case
    a = C.pw_dw_args(case)
    name, _ = C.launch_pw_dw(a)
    rng = np.random.default_rng(seed_of(case))
    X = rnd(rng, B, K, T)
    w_pw, w_dw, b_dw = rnd(rng, M, K, 1, scale=K ** -0.5), rnd(rng, M, 1, ks, scale=ks ** -0.5), rnd(rng, M, scale=0.1)
    xin = X.astype(D) * D(np.float32(a.pre_scale))
    h = O.sconv1d(O.elu(xin, D) if a.pre_elu else xin, w_pw, None, dtype=D)
    ref = O.sconv1d(h, w_dw, b_dw, stride=stride, dilation=dil, groups=M, dtype=D)
    kw = {}
    if a.resid:
        R = rnd(rng, *ref.shape)
        ref = ref * D(np.float32(0.61)) + R
        kw.update(resid=cu(R), out_scale=0.61)
    if a.film:
        film = rnd(rng, B, a.bands, 2)
        bw = M // a.bands
        ref = ref * np.repeat(film[:, :, 0], bw, 1)[:, :, None].astype(D) + np.repeat(film[:, :, 1], bw, 1)[:, :, None].astype(D)
        kw.update(film=cu(film), bands=a.bands)
    if act:
        kw.update(act_scale=0.7071)
    Xd = cu(X)
    run = lambda: ops.pw_dw(Xd, w_pw, w_dw, b_dw, stride=stride, dilation=dil, pre_scale=a.pre_scale, pre_elu=a.pre_elu, **kw)
    got, kernels, _ = launched(run)
    assert kernels == {name: 1}, f"the launcher took {kernels}, the restatement says {name}"
    what = f"pw_dw {name}"
    if act:
        hold(got[0], ref, what)
        hold(got[1], O.elu(ref * D(np.float32(0.7071)), D), what + " (activated copy)")
    else:
        hold(got, ref, what)
    same(run(), got, what)


# ---- upsample ----------------------------------------------------------------------------------------------------------------------------
UP = C.up_cases()


@pytest.mark.parametrize("case", UP, ids=ids(UP))
def test_upsample_fuzz(ops, case):
    B, K, M, Tin, r, pre, act = case
    a = C.up_args(case)
    name, _ = C.launch_pw_dw(a)
    rng = np.random.default_rng(seed_of(case))
    X = rnd(rng, B, K, Tin)
    w_ct, w_pw, b = rnd(rng, K, 1, 2 * r, scale=(2 * r) ** -0.5), rnd(rng, M, K, 1, scale=K ** -0.5), rnd(rng, M, scale=0.1)
    xin = X.astype(D) * D(np.float32(a.pre_scale))
    ref = O.sconv1d(O.sconvtr1d_depthwise(O.elu(xin, D) if a.pre_elu else xin, w_ct, r, dtype=D), w_pw, b, dtype=D)
    Xd = cu(X)
    run = lambda: ops.dw_pw(Xd, w_pw, b, w_ct, mode=2, ks_or_ratio=r, pre_scale=a.pre_scale, pre_elu=a.pre_elu, act_scale=0.9 if act else None)
    got, kernels, _ = launched(run)
    assert kernels == {name: 1}, f"the launcher took {kernels}, the restatement says {name}"
    what = f"upsample {name}"
    if act:
        hold(got[0], ref, what)
        hold(got[1], O.elu(ref * D(np.float32(0.9)), D), what + " (activated copy)")
    else:
        hold(got, ref, what)
    same(run(), got, what)


# ---- conv_post and the SpecBlock add -------------------------------------------------------------------------------------------------------
POST = C.convpost_cases()


@pytest.mark.parametrize("case", POST, ids=ids(POST))
def test_convpost_fuzz(ops, case):
    B, K, M, T, ks, l2 = case
    name = C.launch_dw_pw(M, T, 1, l2)
    rng = np.random.default_rng(seed_of(case))
    X = rnd(rng, B, K, T)
    w_dw, w_pw, b = rnd(rng, K, 1, ks, scale=ks ** -0.5), rnd(rng, M, K, 1, scale=K ** -0.5), rnd(rng, M)
    ref = O.sconv1d(O.sconv1d(O.elu(X, D), w_dw, None, groups=K, dtype=D), w_pw, b, dtype=D)
    if l2:
        ref = ref / np.maximum(np.sqrt((ref ** 2).sum(1, keepdims=True)), 1e-12) * D(M ** 0.5)
    Xd = cu(X)
    run = lambda: ops.dw_pw(Xd, w_pw, b, w_dw, mode=1, ks_or_ratio=ks, pre_elu=True, l2norm=l2)
    got, kernels, _ = launched(run)
    assert kernels == {name: 1}, f"the launcher took {kernels}, the restatement says {name}"
    hold(got, ref, f"conv_post {name}")
    same(run(), got, "conv_post")


ADD = C.specadd_cases()


@pytest.mark.parametrize("case", ADD, ids=ids(ADD))
def test_specadd_fuzz(ops, case):
    B, F, Cc, T, act = case
    name, _ = C.specadd_route(case)
    rng = np.random.default_rng(seed_of(case))
    P, Xa, w = rnd(rng, B, F, T), rnd(rng, B, Cc, T), rnd(rng, Cc, F, 1, scale=F ** -0.5)
    ref = Xa.astype(D) + D(np.float32(0.61)) * O.sconv1d(P, w, None, dtype=D)
    Pd = cu(P)

    def run():
        acc = cu(Xa)
        r = ops.dw_pw(Pd, w, None, None, mode=0, accumulate_into=acc, out_scale=0.61, act_scale=0.7071 if act else None)
        return r if act else acc
    got, kernels, _ = launched(run)
    assert kernels == {name: 1}, f"the launcher took {kernels}, the restatement says {name}"
    what = f"spec add {name}"
    if act:
        hold(got[0], ref, what)
        hold(got[1], O.elu(ref * D(np.float32(0.7071)), D), what + " (activated copy)")
    else:
        hold(got, ref, what)
    same(run(), got, what)


# ---- STFT and the one-launch SpecBlock -----------------------------------------------------------------------------------------------------
def _logmag(wav, n_fft, hop, mean, std):
    mag = O.causal_stft_mag(wav, n_fft, hop, dtype=D)
    return mag, (np.log(np.maximum(mag, 1e-5)) - D(np.float32(mean))) / D(np.float32(std))


def _bands(mag, ref):
    """test_stft_logmag's three magnitude bands as an element-wise bound on the normalised log-magnitude: 2e-5 of |ref|max (no floor) where
    mag > 1e-2, 1e-4 down to 1e-3, 5e-3 below (|d log m| = |dm| / m)."""
    return np.where(mag > 1e-2, BAR * np.abs(ref).max(), np.where(mag > 1e-3, 1e-4, 5e-3))


def _wave(rng, B, T):
    wav = np.clip(rnd(rng, B, 1, T, scale=0.1), -1, 1)
    wav[B - 1, 0, : T // 3] = 0.0                                 # silence: both clamps
    return wav


STFT = C.stft_cases()


@pytest.mark.parametrize("case", STFT, ids=ids(STFT))
def test_stft_fuzz(ops, case):
    B, n_fft, hop, T = case
    name = C.launch_stft_logmag(n_fft, hop, T)
    rng = np.random.default_rng(seed_of(case))
    wav = _wave(rng, B, T)
    mag, ref = _logmag(wav, n_fft, hop, -4.3, 2.8)
    wd = cu(wav)
    run = lambda: ops.stft_logmag(wd, n_fft, hop, mean=-4.3, std=2.8)
    got, kernels, _ = launched(run)
    assert kernels == {name: 1}, f"the launcher took {kernels}, the restatement says {name}"
    g = got.cpu().numpy()
    assert g.shape == ref.shape and np.isfinite(g).all()
    d = np.abs(g - ref)
    for band, sel in (("mag > 1e-2", mag > 1e-2), ("1e-3 < mag <= 1e-2", (mag > 1e-3) & (mag <= 1e-2)), ("mag <= 1e-3", mag <= 1e-3)):
        print(f"FIG stft {name} {band}: err {d[sel].max(initial=0):.3e} |ref|max {np.abs(ref).max():.3e}")
    assert (d <= _bands(mag, ref)).all(), f"stft {name}: {float((d / _bands(mag, ref)).max()):.2f} of its band's bound"
    same(run(), got, "stft")


SPEC = C.specblock_cases()


@pytest.mark.parametrize("case", SPEC, ids=ids(SPEC))
def test_specblock_fuzz(ops, case):
    B, n_fft, hop, T = case
    Cc, F, Tf = n_fft, n_fft // 2 + 1, -(-T // hop)
    name = C.launch_stft_spec(n_fft, hop, T, Cc)
    rng = np.random.default_rng(seed_of(case))
    wav = _wave(rng, B, T)
    if B > 1:
        wav[0] *= 8.0
    x, w = rnd(rng, B, Cc, Tf), rnd(rng, Cc, F, 1, scale=F ** -0.5)
    s_out, s_act = np.float32(0.53), np.float32(0.7071)
    mag, P = _logmag(wav, n_fft, hop, -4.3, 2.8)
    ref = x.astype(D) + D(s_out) * O.sconv1d(P, w, None, dtype=D)
    # the spectrogram's own bound, band by band, through the 1x1: |W| @ bound
    extra = D(s_out) * np.matmul(np.abs(w[:, :, 0]).astype(D), _bands(mag, P))
    wd, xd = cu(wav), cu(x)
    run = lambda: ops.spec_block(wd, w, xd, n_fft, hop, mean=-4.3, std=2.8, out_scale=float(s_out), act_scale=float(s_act))
    (got, gact), kernels, _ = launched(run)
    assert kernels == {name: 1}, f"the launcher took {kernels}, the restatement says {name}"
    hold(got, ref, f"spec block {name}", extra=extra)
    hold(gact, O.elu(ref * D(s_act), D), f"spec block {name} (activated copy)", extra=extra * D(s_act))
    same(run(), (got, gact), "spec block")
    assert torch.equal(ops.spec_block(wd, w, xd, n_fft, hop, mean=-4.3, std=2.8, out_scale=float(s_out)), got)
    assert torch.equal(ops.spec_block(wd, w, xd, n_fft, hop, mean=-4.3, std=2.8, out_scale=float(s_out), act_scale=float(s_act), want_raw=False), gact)
    if Cc >= 128:                                                  # the two kernels it replaces, held bit-equal from 128 rows (K1 add)
        two = xd.clone()
        Pd = ops.stft_logmag(wd, n_fft, hop, mean=-4.3, std=2.8)
        _, two_act = ops.dw_pw(Pd, w, None, None, mode=0, accumulate_into=two, out_scale=float(s_out), act_scale=float(s_act))
        assert torch.equal(two, got) and torch.equal(two_act, gact), "the one-launch SpecBlock differs from STFT + add"
    else:                                                          # below 128 rows the add is the plain 1x1 kernel: the same 33 products per output in
        two = xd.clone()                                           # another order, 2e-6 of the result's largest magnitude (test_spec_block_in_one_launch's bound, no floor)
        ops.dw_pw(ops.stft_logmag(wd, n_fft, hop, mean=-4.3, std=2.8), w, None, None, mode=0, accumulate_into=two, out_scale=float(s_out))
        twin = float((two - got).abs().max())
        print(f"FIG spec block {name} against STFT + add: {twin:.3e} |got|max {float(got.abs().max()):.3e}")
        assert twin <= 2e-6 * float(got.abs().max()), f"the one-launch SpecBlock is {twin:.3e} from STFT + add"


# ---- the one-launch ResnetBlock ------------------------------------------------------------------------------------------------------------
def _block(rng, B, Cc, T):
    X = rnd(rng, B, Cc, T)
    w1, w2 = rnd(rng, Cc, Cc, 1, scale=Cc ** -0.5), rnd(rng, Cc, Cc, 1, scale=Cc ** -0.5)
    d1, d2 = rnd(rng, Cc, 1, 5, scale=0.45), rnd(rng, Cc, 1, 5, scale=0.45)
    b1, b2 = rnd(rng, Cc, scale=0.1), rnd(rng, Cc, scale=0.1)
    return X, (w1, d1, b1, w2, d2, b2)


PRE, S_OUT, S_ACT = np.float32(0.8660254), np.float32(0.41), np.float32(0.7071)


def _block_ref(X, ws):
    w1, d1, b1, w2, d2, b2 = ws
    Cc = X.shape[1]
    u = O.sconv1d(O.sconv1d(O.elu(X.astype(D) * D(PRE), D), w1, None, dtype=D), d1, b1, groups=Cc, dtype=D)
    return X.astype(D) + D(S_OUT) * O.sconv1d(O.sconv1d(O.elu(u, D), w2, None, dtype=D), d2, b2, groups=Cc, dtype=D)


def _run_block(ops, Xd, ws, outs, name, what):
    kw = dict(pre_scale=float(PRE), out_scale=float(S_OUT))
    if outs != "raw":
        kw.update(act_scale=float(S_ACT), want_raw=outs == "both")
    run = lambda: ops.resblock(Xd, *ws, **kw)
    got, kernels, _ = launched(run)
    assert kernels == {name: 1}, f"the launcher took {kernels}, the restatement says {name}"
    same(run(), got, what)
    # the same block as two K1 launches (self-activating first unit): the project holds the fused kernel bit-equal to them
    w1, d1, b1, w2, d2, b2 = ws
    _, ua = ops.pw_dw(Xd, w1, d1, b1, pre_scale=float(PRE), pre_elu=True, act_scale=1.0)
    two, two_act = ops.pw_dw(ua, w2, d2, b2, resid=Xd, pre_elu=False, out_scale=float(S_OUT), act_scale=float(S_ACT))
    y, yact = (got, None) if outs == "raw" else (None, got) if outs == "act" else got
    assert y is None or torch.equal(two, y), f"{what}: the one-launch block differs from two launches by {float((two - y).abs().max()):.3e}"
    assert yact is None or torch.equal(two_act, yact), f"{what}: the activated copy differs from two launches"
    return y, yact


RB = C.resblock_cases()


@pytest.mark.parametrize("case", RB, ids=ids(RB))
def test_resblock_fuzz(ops, case):
    B, Cc, T, outs = case
    rng = np.random.default_rng(seed_of(case))
    X, ws = _block(rng, B, Cc, T)
    ref = _block_ref(X, ws)
    name = C.rb_geometry(Cc)["name"]
    y, yact = _run_block(ops, cu(X), ws, outs, name, f"resblock {name}")
    if y is not None:
        hold(y, ref, f"resblock {name}")
    if yact is not None:
        hold(yact, O.elu(ref * D(S_ACT), D), f"resblock {name} (activated copy)")


@pytest.mark.parametrize("Cc", [64, 96, 128, 192])
def test_resblock_persistent_walk(ops, Cc):
    """rb_kernel is persistent: grid = min(tiles, CUs * per_cu) and a workgroup walks tile += grid, refilling the next window under GEMM 2
    and rewriting the u zero padding only at a clip's first tile.  The smallest case with more tiles than the cap: three tiles per clip (a
    workgroup's consecutive tiles differ in their place in the clip, both ways) and a tile count that is no multiple of the grid.
    Outside the 6e6 size bound: at 256 CUs (B, C, T) = (172, 64, 508) 22 MB, (87, 96, 492) 16 MB, (87, 128, 508) 23 MB, (87, 192, 252) 17 MB."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    geo = C.rb_geometry(Cc)
    B, T = C.persistent_walk_case(geo, cus)
    tiles, grid = C.persistent_grid(geo, B, T, cus)
    assert tiles > cus * geo["per_cu"] and tiles % grid and tiles == 3 * B
    rng = np.random.default_rng(seed_of("walk", Cc))
    X, ws = _block(rng, B, Cc, T)
    ref = _block_ref(X, ws)
    y, yact = _run_block(ops, cu(X), ws, "both", geo["name"], f"resblock walk C={Cc} B={B} T={T}")
    hold(y, ref, f"resblock walk {geo['name']} B={B} T={T} tiles={tiles} grid={grid}")
    hold(yact, O.elu(ref * D(S_ACT), D), f"resblock walk {geo['name']} (activated copy)")


@pytest.mark.parametrize("Cc", [64, 96, 128, 192])
def test_resblock16_persistent_walk(ops, Cc):
    """The f16 rh_kernel walks the same way (per_cu 2 / 5 / 2 / 1 at C = 64 / 96 / 128 / 192).  Its yardstick is the f16 mode's own: the
    kernel's roundings restated with float64 sums (tests/test_gpu_h16.py resblock16_ref), 3 f16 ulps of the result's largest magnitude.
    At 256 CUs: (B, C, T) = (172, 64, 492), (428, 96, 132), (172, 128, 252), (87, 192, 252), 11 MB at the most."""
    from test_gpu_h16 import TOL, h, resblock16_ref
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    geo = C.rh_geometry(Cc)
    B, T = C.persistent_walk_case(geo, cus)
    tiles, grid = C.persistent_grid(geo, B, T, cus)
    assert tiles > cus * geo["per_cu"] and tiles % grid and tiles == 3 * B
    rng = np.random.default_rng(seed_of("walk16", Cc))
    X, ws = _block(rng, B, Cc, T)
    X = h(X)
    y = resblock16_ref(X, *ws, PRE, S_OUT)
    X16 = ops.h16_from_f32(cu(X))
    run = lambda: ops.h16_resblock(X16, *ws, pre_scale=float(PRE), out_scale=float(S_OUT), act_scale=float(S_ACT))
    (got, gact), kernels, _ = launched(run)
    assert kernels == {geo["name"]: 1}, f"the launcher took {kernels}, the restatement says {geo['name']}"
    hold(ops.h16_to_f32(got, Cc), h(y).astype(D), f"resblock16 walk {geo['name']} B={B} T={T} tiles={tiles} grid={grid}", bar=TOL)
    hold(ops.h16_to_f32(gact, Cc), h(O.elu(y * S_ACT)).astype(D), f"resblock16 walk {geo['name']} (activated copy)", bar=TOL)
    same(run(), (got, gact), "resblock16 walk")


# ---- whole nets ----------------------------------------------------------------------------------------------------------------------------
NETS = C.net_cases()


def _plan_counts(plan):
    c = {}
    for key in plan["launches"]:
        c[key] = c.get(key, 0) + 1
    return c


@pytest.mark.parametrize("idx,cfgkw,T,B", NETS, ids=[f"{i}-T{T}-B{B}" for i, _, T, B in NETS])
def test_whole_nets_fuzz(ops, idx, cfgkw, T, B):
    """Generator, detector and locator of a drawn configuration against the float64 oracle, and their profile against the restated plan."""
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict, synthetic_clips
    from waveverify_amd.nets import HipNet
    kw = dict(cfgkw)
    nspec = len(kw["strides"]) + 1
    kw["spec_means"] = [-4.0 + 0.1 * i for i in range(nspec)]
    kw["spec_stds"] = [2.5 + 0.05 * i for i in range(nspec)]
    x, msg = synthetic_clips(B, T, seed=2000 + idx)
    xt, mt = torch.from_numpy(x).cuda(), torch.from_numpy(msg).cuda()
    cg = default_config("generator", **kw)
    sdg = random_state_dict(cg, 131 + idx, parametrized=bool(idx & 1))
    ref = O.generator_forward(cg, sdg, x, msg, dtype=D)
    net = HipNet(cg, sdg)
    got, _, by_role = launched(lambda: net.generator(xt, mt))
    plan = C.net_plan(C.net_cfg_dict(cfgkw), B, T, True)
    assert by_role == _plan_counts(plan), f"generator #{idx}: profile {sorted(by_role.items())} != plan {sorted(_plan_counts(plan).items())}"
    hold(got, ref, f"generator #{idx}", bar=5e-5)
    assert torch.equal(net.generator(xt, mt), got)
    for kind in ("detector", "locator"):
        dk = {k: v for k, v in kw.items() if k not in ("channels_dec", "n_residual_dec", "embedding_dim", "embedding_layers")}
        cd = default_config(kind, **dk)
        sdd = random_state_dict(cd, 157 + idx)
        refl = (O.detector_forward if kind == "detector" else O.locator_forward)(cd, sdd, x, dtype=D)
        netd = HipNet(cd, sdd)
        gotl, _, by_role = launched(lambda: netd.detector(xt) if kind == "detector" else netd.locator(xt))
        plan = C.net_plan(C.net_cfg_dict(cfgkw), B, T, False)
        assert by_role == _plan_counts(plan), f"{kind} #{idx}: profile {sorted(by_role.items())} != plan {sorted(_plan_counts(plan).items())}"
        hold(gotl, refl, f"{kind} #{idx}", bar=1e-4)
