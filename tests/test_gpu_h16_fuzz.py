"""Geometry fuzz of the f16 mode's conv and ResnetBlock kernels (csrc/wv_h16.hip), route by route, against the oracle of the mode's own
arithmetic (tests/h16_refs.py: inputs, composed weights and stored activations rounded to f16 where the packer and the kernels round
them, float64 sums).

Every case of tests/h16_fuzz_cases.py runs through ops.h16_conv / h16_conv_film / h16_upsample / h16_resblock with the library's profiler
on: the kernel name it collected must be the one the restated launcher predicted (so tests/test_h16_fuzz_cases_cpu.py's route counts are
facts about the library).  The bars are tests/test_gpu_h16.py's: c8 outputs 3 f16 ulps of |ref|max, the f32 output 2e-4; inputs are scaled as
there and |ref|max >= 1 is asserted, so the floor in `close` never acts.  Before any launch the restated reference is held to the plain
composition of the reference's two ops in float64 (4 f16 ulps; the block 6).  Every call runs twice and must be bit-equal, and on every
route whose tiles hold columns of several clips (the flat run, both two-clip SHORT forms) row b of the batch must equal the same clip run
alone, bit for bit.  Each figure is printed before it is asserted (pytest -s)."""
import zlib

import numpy as np
import pytest
import torch

import h16_fuzz_cases as H
from h16_refs import (BLOCK_BOUND, COMPOSED_BOUND, F32_TOL, TOL, close, composed_weight, cu, dense_conv_plain, dense_conv_ref, h, resblock16_ref,
                      resblock_plain, rnd, upsample16_ref, upsample_plain)
from oracle import wv_oracle as O

pytestmark = pytest.mark.gpu

S_OUT, S_ACT = np.float32(0.7), np.float32(0.9)                   # test_conv16_generic_geometries' scales
UP_PRE, UP_ACT = np.float32(0.7071), np.float32(0.5)              # test_upsample_as_one_conv's


@pytest.fixture(scope="module")
def ops():
    from waveverify_amd import ops as _ops
    from waveverify_amd import profile
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    profile.enable(True)
    yield _ops
    profile.enable(False)


def launched(fn):
    """Run fn with a fresh profile -> (its result, {kernel name: launches})."""
    from waveverify_amd import profile
    profile.reset()
    out = fn()
    by_kernel = {}
    for e in profile.collect():
        by_kernel[e["kernel"]] = by_kernel.get(e["kernel"], 0) + e["launches"]
    return out, by_kernel


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def hold(got, ref, what, tol=TOL, activated=False):
    """The figure, then tests/test_gpu_h16.py's `close` at its bar.  The raw and f32 references reach 1, so the floor in `close` is idle; an
    activated copy ELU(s * y) with s < 1 need not, and is held to the bar times its own largest magnitude (no floor: the tighter reading)."""
    g = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    mag = float(np.abs(ref).max())
    err = float(np.abs(g - ref).max()) if g.shape == ref.shape else float("nan")
    print(f"FIG {what}: err {err:.3e} |ref|max {mag:.3e} rel {err / mag:.3e} bar {tol:.2e}")
    assert activated or mag >= 1.0, f"{what}: |ref|max = {mag:.3e} < 1, the floor of the bar would act"
    close(got, ref, what, tol)
    assert err <= tol * mag, f"{what}: max|d|={err:.3e} > {tol:.2e} x |ref|max {mag:.3e}"


def same(a, b, what):
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), f"{what}: a second call is not bit-equal"


def drawn(build, case):
    """build(rng) -> (problem, reference) on the case's own seed; the reference must reach 1 (it does for every case of the lists: the
    smallest, 256 outputs of one tap, reach 1.003)."""
    prob, ref = build(np.random.default_rng(seed_of(case, 0)))
    assert float(np.abs(ref).max()) >= 1.0, f"{case}: |ref|max = {float(np.abs(ref).max()):.3e} < 1, the floor of the bar would act"
    return prob, ref


# ---- the problems: everything the CPU can do before a launch -------------------------------------------------------------------------------
def dense_problem(case):
    """-> dict(X, w_pw, w_dw, bias, film, R, ref): inputs and the restated reference of a dense-conv case; weights are seeded by (K, M, taps)
    alone, so that cases which differ in their lengths share them.  Asserts the restated reference against the plain two ops."""
    B, K, M, Tin, ks, stride, pad, epi, outs = case
    a = H.dense_args(case)
    wr = np.random.default_rng(seed_of("weights", K, M, ks))
    w_pw, w_dw = rnd(wr, M, K, 1, scale=K ** -0.5), (rnd(wr, M, 1, ks, scale=ks ** -0.5) if ks > 1 else None)
    bias = rnd(wr, M, scale=0.1)
    wc = composed_weight(w_pw, w_dw)

    def build(rng):
        X = rnd(rng, B, K, Tin)
        xa = h(X)
        ref = dense_conv_ref(xa, wc, bias, stride, pad, a.Tout)
        plain = dense_conv_plain(xa, w_pw, w_dw, bias, stride, pad, a.Tout)
        d = float(np.abs(plain - ref).max())
        assert d <= COMPOSED_BOUND * max(1.0, float(np.abs(plain).max())), f"{case}: the restated conv is {d:.3e} from its two ops"
        film = R = None
        if a.film:
            film = np.stack([rng.uniform(0.6, 1.4, (B, a.bands)), rng.normal(0, 0.3, (B, a.bands))], axis=-1).astype(np.float32)
            bw = M // a.bands
            ref = np.repeat(film[:, :, 0], bw, axis=1)[:, :, None] * ref + np.repeat(film[:, :, 1], bw, axis=1)[:, :, None]
        else:
            ref = ref * S_OUT
            if a.resid:
                R = h(rnd(rng, B, M, a.Tout))
                ref = ref + R
        return dict(X=X, film=film, R=R), ref.astype(np.float32)
    prob, ref = drawn(build, case)
    prob.update(w_pw=w_pw, w_dw=w_dw, bias=bias, ref=ref, a=a)
    return prob


def up_problem(case):
    B, K, Mo, Tin, r, outs = case
    wr = np.random.default_rng(seed_of("weights", K, Mo, r))
    w_ct, w_pw, b = rnd(wr, K, 1, 2 * r, scale=0.5), rnd(wr, Mo, K, 1, scale=K ** -0.5), rnd(wr, Mo, scale=0.1)

    def build(rng):
        X = rnd(rng, B, K, Tin)
        xa = h(O.elu(X * UP_PRE))
        ref = upsample16_ref(xa, w_ct, w_pw, b, r)
        two = upsample_plain(xa, w_ct, w_pw, b, r)
        d = float(np.abs(two - ref).max())
        assert two.shape == ref.shape and d <= COMPOSED_BOUND * max(1.0, float(np.abs(two).max())), f"{case}: the restated unit is {d:.3e} from its two ops"
        return dict(X=X), ref
    prob, ref = drawn(build, case)
    prob.update(w_ct=w_ct, w_pw=w_pw, b=b, ref=ref, a=H.up_args(case))
    return prob


# ---- the launches ----------------------------------------------------------------------------------------------------------------------------
def dense_run(ops, p, X16, R16, filmd):
    """-> [raw, act, f32] (None where not asked for)"""
    a = p["a"]
    act = float(S_ACT) if a.Yact else None
    if a.film:
        r = ops.h16_conv_film(X16, p["w_pw"], p["w_dw"], p["bias"], filmd, a.ks, a.stride, a.pad, act_scale=act, want_raw=a.Y)
        raw, ya = (r if a.Y and a.Yact else (r, None) if a.Y else (None, r))
        return [raw, ya, None]
    r = ops.h16_conv(X16, p["w_pw"], p["w_dw"], p["bias"], resid16=R16, ks=a.ks, stride=a.stride, pad=a.pad, out_scale=float(S_OUT), act_scale=act,
                     want_raw=a.Y, want_f32=a.Yf32)
    return [r.get("raw"), r.get("act"), r.get("f32")]


def present(outs):
    return [o for o in outs if o is not None]


def clip_alone_equal(B, run_clip, batch, what):
    """Row b of the batch against the same clip run alone, bit for bit, every clip."""
    for b in range(B):
        for o, s in zip(present(batch), present(run_clip(b))):
            if not torch.equal(o[b], s[0]):
                d = float((o[b].float() - s[0].float()).abs().max())
                raise AssertionError(f"{what}: clip {b} of {B} differs from the same clip run alone by {d:.3e}")


def _dense(ops, case):
    p = dense_problem(case)
    a, ref = p["a"], p["ref"]
    B, K, M = case[:3]
    name, info = H.launch_conv16(a)
    X16 = ops.h16_from_f32(cu(p["X"]))
    R16 = ops.h16_from_f32(cu(p["R"])) if p["R"] is not None else None
    filmd = cu(p["film"]) if p["film"] is not None else None
    got, kernels = launched(lambda: dense_run(ops, p, X16, R16, filmd))
    assert kernels == {name: 1}, f"the launcher took {kernels}, the restatement says {name} ({info['route']})"
    what = f"{info['route']} {name}"
    if got[0] is not None:
        hold(ops.h16_to_f32(got[0], M), h(ref), what + " raw")
    if got[1] is not None:
        hold(ops.h16_to_f32(got[1], M), h(O.elu(ref * S_ACT)), what + " act", activated=True)
    if got[2] is not None:
        hold(got[2], ref, what + " f32", F32_TOL)
    same(present(dense_run(ops, p, X16, R16, filmd)), present(got), what)
    if H.spans_clips(info) and B > 1:
        clip_alone_equal(B, lambda b: dense_run(ops, p, X16[b:b + 1].contiguous(), None if R16 is None else R16[b:b + 1].contiguous(),
                                                None if filmd is None else filmd[b:b + 1].contiguous()), got, what)


DENSE = H.dense_cases()


@pytest.mark.parametrize("case", DENSE, ids=ids(DENSE))
def test_conv16_fuzz(ops, case):
    _dense(ops, case)


@pytest.mark.parametrize("case", H.DENSE_EXPLICIT, ids=ids(H.DENSE_EXPLICIT))
def test_conv16_placed(ops, case):
    _dense(ops, case)


def up_run(ops, p, X16):
    a = p["a"]
    r = ops.h16_upsample(X16, p["w_ct"], p["w_pw"], p["b"], a.up, act_scale=float(UP_ACT) if a.Yact else None, want_raw=a.Y)
    return list(r) if a.Y and a.Yact else [r, None] if a.Y else [None, r]


def _up(ops, case):
    p = up_problem(case)
    a, ref = p["a"], p["ref"]
    B, K, Mo = case[:3]
    name, info = H.launch_conv16(a)
    X16 = ops.h16_from_f32(cu(p["X"]), scale=float(UP_PRE), elu=True)
    got, kernels = launched(lambda: up_run(ops, p, X16))
    assert kernels == {name: 1}, f"the launcher took {kernels}, the restatement says {name} ({info['route']})"
    what = f"up {info['route']} {name}"
    if got[0] is not None:
        hold(ops.h16_to_f32(got[0], Mo), h(ref), what + " raw")
    if got[1] is not None:
        hold(ops.h16_to_f32(got[1], Mo), h(O.elu(ref * UP_ACT)), what + " act", activated=True)
    same(present(up_run(ops, p, X16)), present(got), what)
    if H.spans_clips(info) and B > 1:
        clip_alone_equal(B, lambda b: up_run(ops, p, X16[b:b + 1].contiguous()), got, what)


UP = H.up_cases()


@pytest.mark.parametrize("case", UP, ids=ids(UP))
def test_upsample16_fuzz(ops, case):
    _up(ops, case)


@pytest.mark.parametrize("case", H.UP_EXPLICIT, ids=ids(H.UP_EXPLICIT))
def test_upsample16_placed(ops, case):
    _up(ops, case)


# ---- the persistent ResnetBlock kernel at the widths whose older cases never give a workgroup a second tile -------------------------------
PRE, RB_OUT, RB_ACT = np.float32(0.8660254), np.float32(0.41), np.float32(0.7071)     # test_resblock's scales


@pytest.mark.parametrize("Cc", H.WALK_WIDTHS)
def test_resblock16_persistent_walk_other_widths(ops, Cc):
    """rh_kernel is persistent: grid = min(tiles, CUs * per_cu) and a workgroup walks tile += grid (per_cu 2 / 2 / 1 / 1 / 1 at C = 32 /
    256 / 384 / 512 / 768).  The smallest (B, T) with three tiles per clip, more tiles than the grid and a tile count that is no multiple
    of the grid; at 256 CUs (B, C, T) = (172, 32, 972), (172, 256, 132), (87, 384, 132), (87, 512, 132), (87, 768, 132): 18 MB at the most."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    geo = H.rh_geometry(Cc)
    B, T = H.persistent_walk_case(geo, cus)
    tiles, grid = H.persistent_grid(geo, B, T, cus)
    assert tiles == 3 * B and tiles > cus * geo["per_cu"] and tiles % grid
    rng = np.random.default_rng(seed_of("walk16", Cc))
    X = h(rnd(rng, B, Cc, T))
    ws = (rnd(rng, Cc, Cc, 1, scale=Cc ** -0.5), rnd(rng, Cc, 1, 5, scale=0.45), rnd(rng, Cc, scale=0.1),
          rnd(rng, Cc, Cc, 1, scale=Cc ** -0.5), rnd(rng, Cc, 1, 5, scale=0.45), rnd(rng, Cc, scale=0.1))
    y = resblock16_ref(X, *ws, PRE, RB_OUT)
    plain = resblock_plain(X, *ws, PRE, RB_OUT)
    assert np.abs(plain - y).max() <= BLOCK_BOUND * max(1.0, np.abs(plain).max())
    X16 = ops.h16_from_f32(cu(X))
    run = lambda: ops.h16_resblock(X16, *ws, pre_scale=float(PRE), out_scale=float(RB_OUT), act_scale=float(RB_ACT))
    (got, gact), kernels = launched(run)
    assert kernels == {geo["name"]: 1}, f"the launcher took {kernels}, the restatement says {geo['name']}"
    what = f"resblock16 walk {geo['name']} B={B} T={T} tiles={tiles} grid={grid}"
    hold(ops.h16_to_f32(got, Cc), h(y), what)
    hold(ops.h16_to_f32(gact, Cc), h(O.elu(y * RB_ACT)), what + " act", activated=True)
    same(run(), (got, gact), what)
