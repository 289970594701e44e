"""The one-launch ResnetBlock kernel's window walk (wv_rb.hip): stencil edges carried from group to group and from window to window
through LDS, runs of consecutive windows per workgroup, masked stores where a run starts mid-clip, carries reset at a clip's start.

Every case holds `ops.resblock` in its four forms (raw + activated, raw only, activated only) BIT FOR BIT to the same block run as two
`ops.pw_dw` launches, as tests/test_gpu_ops.py::test_fused_resblock does; the cases with small tensors also to the float64 oracle at
that test's tolerance.  A = the columns a carried-edge window advances by (256; 128 at C = 192), G = CU count x workgroups per CU = the
grid the launcher fills.  C = 96 and 192 run the carried-edge kernel; C = 64 and 128 kept the halo kernel (where a window yields
A - 12 outputs) and run the same shapes:

  (a)  B = 3, T around every multiple of A: one window per run, so every window after a clip's first starts mid-clip (masked stores);
  (b)  B = 1, T = (2G + 3) A + 4: runs of three windows that start mid-clip -- the carry crosses windows, masked starts meet run ends;
  (c)  B = G + 7, T = 8: a workgroup takes a second clip -- the carries reset at a clip's start;
  (c2) B = G + 7, T = 2A + 4: the same with three-window runs -- the window parity of the doubled edge slot runs on across runs;
  (d)  the training form's four saved tensors against the two-launch route: u and v from the two halves run as units, and the 1x1
       outputs h0 / h1 from the same units with the identity stencil (taps 0 0 0 0 1, gain 1, no bias: the weight-normed taps are
       exactly those, and 1 * h + 0 is exact), which fold the 1x1 weights with the same kernel the block does.
"""
import numpy as np
import pytest
import torch

from oracle import wv_oracle as O

pytestmark = pytest.mark.gpu

WINDOW = {64: 256, 96: 256, 128: 256, 192: 128}                   # A: columns per window
PER_CU = {64: 2, 96: 1, 128: 1, 192: 1}                           # workgroups per CU (LDS-limited)
PRE, S_OUT, S_ACT = np.float32(0.8660254), np.float32(0.41), np.float32(0.7071)


@pytest.fixture(scope="module")
def ops():
    from waveverify_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _ops


def grid(C):
    return torch.cuda.get_device_properties(0).multi_processor_count * PER_CU[C]


def rnd(rng, *shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def weights(C, seed):
    rng = np.random.default_rng(seed)
    return (rnd(rng, C, C, 1, scale=C ** -0.5), rnd(rng, C, 1, 5, scale=0.45), rnd(rng, C, scale=0.1),
            rnd(rng, C, C, 1, scale=C ** -0.5), rnd(rng, C, 1, 5, scale=0.45), rnd(rng, C, scale=0.1))


def close(got, ref, what, tol=2e-5):
    got = got.detach().cpu().numpy()
    err, lim = float(np.abs(got - ref).max()), tol * float(np.abs(ref).max())
    assert np.isfinite(got).all(), what
    assert err <= lim, f"{what}: max|d|={err:.3e} > {lim:.3e}"


def first_diff(a, b):
    d = (a != b).nonzero()
    return "equal" if d.numel() == 0 else f"{d.shape[0]} differ, first at (clip, channel, t) = {tuple(d[0].tolist())}"


def check_block(ops, Xd, C, seed, oracle):
    w1, d1, b1, w2, d2, b2 = weights(C, seed)
    kw = dict(pre_scale=float(PRE), out_scale=float(S_OUT))
    got, gact = ops.resblock(Xd, w1, d1, b1, w2, d2, b2, act_scale=float(S_ACT), **kw)
    only_raw = ops.resblock(Xd, w1, d1, b1, w2, d2, b2, **kw)
    only_act = ops.resblock(Xd, w1, d1, b1, w2, d2, b2, act_scale=float(S_ACT), want_raw=False, **kw)
    _, ua = ops.pw_dw(Xd, w1, d1, b1, pre_scale=float(PRE), pre_elu=True, act_scale=1.0)
    two, two_act = ops.pw_dw(ua, w2, d2, b2, resid=Xd, pre_elu=False, out_scale=float(S_OUT), act_scale=float(S_ACT))
    assert torch.equal(two, got), f"raw output vs two launches: {first_diff(two, got)}"
    assert torch.equal(two_act, gact), f"activated output vs two launches: {first_diff(two_act, gact)}"
    assert torch.equal(only_raw, got), f"raw-only form: {first_diff(only_raw, got)}"
    assert torch.equal(only_act, gact), f"activated-only form: {first_diff(only_act, gact)}"
    if oracle:
        X = Xd.cpu().numpy()
        u = O.sconv1d(O.sconv1d(O.elu(X * PRE), w1, None), d1, b1, groups=C)
        y = (X + S_OUT * O.sconv1d(O.sconv1d(O.elu(u), w2, None), d2, b2, groups=C)).astype(np.float32)
        close(got, y, "fused resblock vs oracle")
        close(gact, O.elu(y * S_ACT), "fused resblock (activated copy) vs oracle")


def lengths(C):
    A = WINDOW[C]
    return [4, 8, A - 4, A, A + 4, A + 12, 2 * A, 3 * A + 8]


@pytest.mark.parametrize("C,T", [(C, T) for C in WINDOW for T in lengths(C)])
def test_one_window_runs(ops, C, T):
    """(a)"""
    X = torch.from_numpy(rnd(np.random.default_rng(C * 7 + T), 3, C, T)).cuda()
    check_block(ops, X, C, C + T, oracle=True)


@pytest.mark.parametrize("C", list(WINDOW))
def test_runs_of_windows_mid_clip(ops, C):
    """(b)"""
    T = (2 * grid(C) + 3) * WINDOW[C] + 4
    assert C * T * 4 <= 70e6
    X = torch.randn(1, C, T, device="cuda", generator=torch.Generator("cuda").manual_seed(C))
    check_block(ops, X, C, C + 1, oracle=False)


@pytest.mark.parametrize("C", list(WINDOW))
def test_second_clip_resets_carries(ops, C):
    """(c)"""
    X = torch.from_numpy(rnd(np.random.default_rng(C + 5), grid(C) + 7, C, 8)).cuda()
    check_block(ops, X, C, C + 2, oracle=True)


@pytest.mark.parametrize("C", list(WINDOW))
def test_second_clip_after_a_run_of_windows(ops, C):
    """(c2)"""
    B, T = grid(C) + 7, 2 * WINDOW[C] + 4
    assert B * C * T * 4 <= 70e6
    X = torch.randn(B, C, T, device="cuda", generator=torch.Generator("cuda").manual_seed(C + 9))
    check_block(ops, X, C, C + 3, oracle=False)


@pytest.mark.parametrize("C,T", [(C, T) for C in WINDOW for T in (WINDOW[C] + 4, 2 * WINDOW[C])])
def test_training_form_saved_tensors(C, T):
    """(d)"""
    from waveverify_amd.train import TrainBlock, TrainHalf
    rng = np.random.default_rng(C * 3 + T)
    B = 3
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x = cu(rnd(rng, B, C, T))
    ps = [dict(g_pw=cu((0.5 + np.abs(rng.standard_normal((C, 1, 1)))).astype(np.float32)), v_pw=cu(rnd(rng, C, C, 1, scale=C ** -0.5)),
               g_dw=cu((0.5 + np.abs(rng.standard_normal((C, 1, 1)))).astype(np.float32)), v_dw=cu(rnd(rng, C, 1, 5, scale=0.45)),
               b_dw=cu(rnd(rng, C, scale=0.1))) for _ in range(2)]
    ident = np.zeros((C, 1, 5), np.float32)
    ident[:, 0, 4] = 1.0
    ps_id = [dict(p, g_dw=cu(np.ones((C, 1, 1), np.float32)), v_dw=cu(ident), b_dw=cu(np.zeros(C, np.float32))) for p in ps]
    pre, rs = 0.8164966, 0.5773503
    y, saved = TrainBlock(C).forward(x, ps, None, pre, rs)
    n = B * C * T * 4
    step = (n + 255) // 256 * 256                                  # the saved buffer: u, v, h0, h1, each [B, C, T] at a 256-byte boundary
    u, v, h0, h1 = (saved[i * step:i * step + n].view(torch.float32).reshape(B, C, T).clone() for i in range(4))
    half = TrainHalf(C)
    u2 = half.forward(x, ps[0], pre)
    v2 = half.forward(u2, ps[1], 1.0)
    assert torch.equal(u, u2), f"u: {first_diff(u, u2)}"
    assert torch.equal(v, v2), f"v: {first_diff(v, v2)}"
    h0_2, h1_2 = half.forward(x, ps_id[0], pre), half.forward(u2, ps_id[1], 1.0)
    assert torch.equal(h0, h0_2), f"h0: {first_diff(h0, h0_2)}"
    assert torch.equal(h1, h1_2), f"h1: {first_diff(h1, h1_2)}"
    # y = x + s v comes out of the same epilogue (one fused multiply-add per element: within an ulp of the two-step form)
    ref = x + rs * v2
    assert float((y - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
