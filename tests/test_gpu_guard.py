"""Guard bands, poisoned workspaces and misaligned placements for the library's entry points (tests/guard.py).

Every other GPU test hands the kernels fresh, 256-byte-aligned tensors and compares the valid region of the outputs.  Here each
operand sits in an arena between NaN guard bands, each output starts out holding the guard pattern, and each workspace is exactly the
size its `*_workspace_bytes` returns, filled with 0xFF (NaN as f32 and f16).  A case passes when
- the values meet the existing oracle at the existing bar (test_gpu_ops.py's for the f32 units, the whole-net bars of
  test_gpu_fuzz.py, the training bars of test_gpu_train.py);
- no guard changed, no input changed, every promised output element was written;
- a second run on a re-poisoned workspace and re-filled outputs is bit-identical to the first (the result does not depend on what
  the workspace held).
With offset=1 the same units get T % 4 == 0 operands one element past a 16-byte boundary: they must meet the same bars on the
fallback routes (confirmed by kernel name where the route has a name of its own), or refuse the call with every arena untouched.
The f16 units are compared bit for bit with the same call on fresh, aligned buffers (test_gpu_h16 holds those to the mode's
oracle); the reused tests at the end check their workspaces only."""
import os
import re

import numpy as np
import pytest
import torch

import h16_fuzz_cases as H16
from guard import GuardError, Guards, PoisonedWorkspace
from oracle import wv_oracle as O
from test_gpu_ops import close, rnd
from test_gpu_stft_basis import kernels_run

pytestmark = pytest.mark.gpu

K1_NAME = re.compile(r",(dma|dma3|reg|win)(,flat)?>$")


@pytest.fixture(scope="module")
def ops():
    from waveverify_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _ops


@pytest.fixture
def poison(monkeypatch):
    """Every workspace / saved buffer the package allocates (waveverify_amd._lib.scratch) is a poisoned, guarded arena of exactly the
    requested size; all of them are checked when the test ends."""
    from waveverify_amd import _lib
    made = []

    def scratch(nbytes, device):
        a = PoisonedWorkspace(int(nbytes), device, name=f"scratch#{len(made)} ({int(nbytes)} bytes)")
        made.append(a)
        return a.t

    monkeypatch.setattr(_lib, "scratch", scratch)
    yield made
    torch.cuda.synchronize()
    msgs = []
    for a in made:
        try:
            a.check()
        except GuardError as e:
            msgs.append(str(e))
    assert not msgs, "\n".join(msgs)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().view({torch.float32: torch.int32, torch.float16: torch.int16}[t.dtype]).clone()


def twice(g: Guards, call, outs):
    """Run `call` on the guarded buffers, check every arena, re-poison workspaces / re-fill outputs, run again: bit-identical.
    -> (the first run's outputs, the kernel names of the first run)."""
    _, names = kernels_run(call)
    g.check()
    first = [bits(o.t) for o in outs]
    g.repoison()
    call()
    g.check()
    for o, f in zip(outs, first):
        assert torch.equal(bits(o.t), f), f"{o.name}: second run on a re-poisoned workspace differs from the first"
    return [o.t.clone() for o in outs], names


def refused_cleanly(g: Guards, outs, what, e):
    """A misaligned placement the entry point does not serve: an error, every arena untouched, nothing written."""
    assert g.offset == 1, f"{what}: {e}"
    torch.cuda.synchronize()
    for a in g.arenas:
        if a in outs:
            a.check(expect_unwritten=torch.ones(a.t.shape, dtype=torch.bool))
        else:
            a.check()
    print(f"RECORD {what} misaligned: refused ({e})")


def check_route(names, offset, k1_when_aligned):
    k1 = [n for n in names if K1_NAME.search(n)]
    if offset:
        assert not k1, f"a misaligned operand must leave the LDS-DMA core: {sorted(names)}"
    elif k1_when_aligned:
        assert k1, f"expected the LDS-DMA core: {sorted(names)}"


# ================================================================== exact f32 units
# (K, M, Tin, ks, stride, dil, B, K1 route when aligned): the round-1 core, K1 per-clip tiles at tile edges, flat clip-time tiles,
# every strided stencil (r = 2 / 4 / 5 / 8, r8 flat).  Every Tin is a multiple of 4, so offset 1 alone decides the route.
PW_DW_GUARD = [
    (64, 64, 1000, 5, 1, 1, 3, False), (8, 8, 68, 5, 1, 1, 2, False), (128, 128, 124, 5, 1, 1, 2, True), (128, 256, 132, 5, 1, 1, 2, True),
    (100, 130, 252, 5, 1, 1, 2, True), (160, 288, 1000, 5, 1, 2, 2, True), (128, 128, 36, 5, 1, 1, 7, True), (192, 192, 12, 5, 1, 1, 16, True),
    (64, 128, 1000, 4, 2, 1, 2, True), (128, 256, 500 - 500 % 4, 8, 4, 1, 2, True), (256, 512, 2000, 10, 5, 1, 2, True),
    (512, 1024, 400, 16, 8, 1, 2, True), (64, 128, 1000, 16, 8, 1, 9, True), (64, 128, 8, 16, 8, 1, 2, True),
]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("mode", ["plain", "elu+resid+act", "film+act"])
@pytest.mark.parametrize("K,M,Tin,ks,stride,dil,B,k1", PW_DW_GUARD)
def test_pw_dw_guarded(ops, K, M, Tin, ks, stride, dil, B, k1, mode, offset):
    if "resid" in mode and stride != 1:
        pytest.skip("residual only on stride-1 units")
    if "film" in mode and M % 4:
        pytest.skip("FiLM needs channels divisible by the band count")
    rng = np.random.default_rng(K * 7 + M + Tin + B)
    X = rnd(rng, B, K, Tin)
    w_pw = rnd(rng, M, K, 1, scale=K ** -0.5)
    w_dw = rnd(rng, M, 1, ks, scale=ks ** -0.5)
    b_dw = rnd(rng, M, scale=0.1)
    elu = "elu" in mode
    pre = 0.8660254 if elu else 1.0
    h = O.sconv1d(O.elu(X * np.float32(pre)) if elu else X, w_pw, None)
    ref = O.sconv1d(h, w_dw, b_dw, stride=stride, dilation=dil, groups=M)
    g = Guards(offset=offset)
    x = g.input(X, "X")
    kw = {}
    if "resid" in mode:
        R = rnd(rng, *ref.shape)
        ref = ref * np.float32(0.37) + R
        kw.update(resid=g.input(R, "resid").t, out_scale=0.37)
    if "film" in mode:
        film = rnd(rng, B, 4, 2)
        bw = M // 4
        ref = ref * np.repeat(film[:, :, 0], bw, 1)[:, :, None] + np.repeat(film[:, :, 1], bw, 1)[:, :, None]
        kw.update(film=g.input(film, "film").t, bands=4)
    ref = ref.astype(np.float32)
    y = g.output(ref.shape, name="Y")
    outs = [y]
    if "act" in mode:
        ya = g.output(ref.shape, name="Yact")
        outs.append(ya)
        kw.update(act_scale=0.7071, out_act=ya.t)
    (got, *rest), names = twice(g, lambda: ops.pw_dw(x.t, w_pw, w_dw, b_dw, stride=stride, dilation=dil, pre_scale=pre, pre_elu=elu,
                                                       out=y.t, **kw), outs)
    close(got, ref, what=f"pw_dw {mode} offset {offset}")
    if rest:
        close(rest[0], O.elu(ref * np.float32(0.7071)), what=f"pw_dw {mode} activated copy, offset {offset}")
    check_route(names, offset, k1)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C,T", [(64, 244), (96, 236), (192, 116), (192, 120), (96, 8), (192, 12), (128, 244), (64, 248)])
def test_resblock_guarded(ops, C, T, offset):
    rng = np.random.default_rng(C + T)
    B = 2
    X = rnd(rng, B, C, T)
    w1, w2 = rnd(rng, C, C, 1, scale=C ** -0.5), rnd(rng, C, C, 1, scale=C ** -0.5)
    d1, d2 = rnd(rng, C, 1, 5, scale=0.45), rnd(rng, C, 1, 5, scale=0.45)
    b1, b2 = rnd(rng, C, scale=0.1), rnd(rng, C, scale=0.1)
    pre, s_out, s_act = np.float32(0.8660254), np.float32(0.41), np.float32(0.7071)
    u = O.sconv1d(O.sconv1d(O.elu(X * pre), w1, None), d1, b1, groups=C)
    ref = (X + s_out * O.sconv1d(O.sconv1d(O.elu(u), w2, None), d2, b2, groups=C)).astype(np.float32)
    g = Guards(offset=offset)
    x, y, ya = g.input(X, "X"), g.output(X.shape, name="Y"), g.output(X.shape, name="Yact")
    try:
        (got, gact), _ = twice(g, lambda: ops.resblock(x.t, w1, d1, b1, w2, d2, b2, pre_scale=float(pre), out_scale=float(s_out),
                                                       act_scale=float(s_act), out=y.t, out_act=ya.t), [y, ya])
    except RuntimeError as e:                    # the fused block serves 16-byte aligned rows only (rb_supported)
        refused_cleanly(g, [y, ya], f"resblock C={C} T={T}", e)
        return
    close(got, ref, what=f"resblock offset {offset}")
    close(gact, O.elu(ref * s_act), what=f"resblock activated copy, offset {offset}")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("K,M,Tin", [(1024, 128, 52), (64, 128, 51), (32, 16, 17)])
def test_conv_post_l2norm_guarded(ops, K, M, Tin, offset):
    rng = np.random.default_rng(K + M)
    X = rnd(rng, 2, K, Tin)
    w_dw = rnd(rng, K, 1, 5, scale=0.4)
    w_pw = rnd(rng, M, K, 1, scale=K ** -0.5)
    b = rnd(rng, M)
    hh = O.sconv1d(O.sconv1d(O.elu(X), w_dw, None, groups=K), w_pw, b)
    ref = (hh / np.maximum(np.sqrt((hh ** 2).sum(1, keepdims=True)), 1e-12) * np.float32(M ** 0.5)).astype(np.float32)
    g = Guards(offset=offset)
    x, y = g.input(X, "X"), g.output(ref.shape, name="Y")
    (got,), _ = twice(g, lambda: ops.dw_pw(x.t, w_pw, b, w_dw, mode=1, ks_or_ratio=5, pre_elu=True, l2norm=True, out=y.t), [y])
    close(got, ref, what=f"conv_post offset {offset}")


UP_GUARD = [(16, 24, Tin, r) for r in range(1, 9) for Tin in (1, 2, 3)] + [(192, 128, 1000, 2), (384, 256, 332, 4), (1536, 768, 52, 8),
                                                                           (768, 384, 400, 5)]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("K,M,Tin,r", UP_GUARD)
def test_upsample_guarded(ops, K, M, Tin, r, offset):
    rng = np.random.default_rng(K + r + Tin)
    X = rnd(rng, 2, K, Tin)
    w_ct = rnd(rng, K, 1, 2 * r, scale=(2 * r) ** -0.5)
    w_pw = rnd(rng, M, K, 1, scale=K ** -0.5)
    b = rnd(rng, M, scale=0.1)
    ref = O.sconv1d(O.sconvtr1d_depthwise(O.elu(X * np.float32(0.7071)), w_ct, r), w_pw, b).astype(np.float32)
    g = Guards(offset=offset)
    x, y, ya = g.input(X, "X"), g.output(ref.shape, name="Y"), g.output(ref.shape, name="Yact")
    (got, gact), names = twice(g, lambda: ops.dw_pw(x.t, w_pw, b, w_ct, mode=2, ks_or_ratio=r, pre_scale=0.7071, pre_elu=True,
                                                    act_scale=0.9, out=y.t, out_act=ya.t), [y, ya])
    close(got, ref, what=f"upsample offset {offset}")
    close(gact, O.elu(ref * np.float32(0.9)), what=f"upsample activated copy, offset {offset}")
    check_route(names, offset, M >= 128 and (Tin * r) % 4 == 0 and r > 1)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("F,C,T", [(65, 128, 8000), (17, 128, 4), (33, 64, 1000), (9, 8, 33)])
def test_accumulate_in_place_guarded(ops, F, C, T, offset):
    """dw_pw mode 0 adds into its output: only the surroundings are guarded; the second run starts from the same data."""
    rng = np.random.default_rng(F)
    P, Xa = rnd(rng, 2, F, T), rnd(rng, 2, C, T)
    w = rnd(rng, C, F, 1, scale=F ** -0.5)
    ref = (Xa + np.float32(0.61) * O.sconv1d(P, w, None)).astype(np.float32)
    g = Guards(offset=offset)
    p = g.input(P, "P")
    acc = g.output(Xa.shape, name="acc")
    runs = []
    for _ in range(2):
        acc.t.copy_(torch.from_numpy(Xa))
        g.repoison()
        acc.t.copy_(torch.from_numpy(Xa))
        ops.dw_pw(p.t, w, None, None, mode=0, accumulate_into=acc.t, out_scale=0.61)
        g.check()
        runs.append(bits(acc.t))
    assert torch.equal(runs[0], runs[1])
    close(acc.t, ref, what=f"accumulate offset {offset}")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n_fft,hop,T", [(64, 1, 1000), (128, 2, 1000), (128, 2, 1001), (256, 8, 4000), (1024, 320, 16000), (32, 4, 1),
                                         (16, 1, 8)])
def test_stft_logmag_guarded(ops, n_fft, hop, T, offset):
    rng = np.random.default_rng(n_fft + hop)
    wav = np.clip(rnd(rng, 2, 1, T, scale=0.1), -1, 1)
    wav[1, 0, : T // 3] = 0.0
    mag = O.causal_stft_mag(wav, n_fft, hop)
    ref = ((np.log(np.maximum(mag, np.float32(1e-5))) - np.float32(-4.3)) / np.float32(2.8)).astype(np.float32)
    g = Guards(offset=offset)
    w, P = g.input(wav, "wav"), g.output(ref.shape, name="P")
    (got,), names = twice(g, lambda: ops.stft_logmag(w.t, n_fft, hop, mean=-4.3, std=2.8, out=P.t), [P])
    got = got.cpu().numpy()
    big, mid = mag > 1e-2, (mag > 1e-3) & (mag <= 1e-2)
    assert np.abs(got - ref)[big].max(initial=0) <= 2e-5 * max(1.0, np.abs(ref).max())
    assert np.abs(got - ref)[mid].max(initial=0) <= 1e-4
    assert np.abs(got - ref)[mag <= 1e-3].max(initial=0) <= 5e-3
    # the STFT's LDS-DMA core gathers its frames and has no alignment gate: a misaligned wave / P stays on it, at the same bars
    print(f"RECORD stft_logmag n_fft={n_fft} T={T} offset={offset}: {sorted(names)}")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n_fft,hop,T", [(64, 1, 132), (64, 1, 1000), (128, 2, 264), (128, 2, 263), (128, 4, 1040)])
def test_spec_block_guarded(ops, n_fft, hop, T, offset):
    rng = np.random.default_rng(n_fft + hop + T)
    C, F, Tf = n_fft, n_fft // 2 + 1, -(-T // hop)
    wav = np.clip(rnd(rng, 3, 1, T, scale=0.1), -1, 1)
    wav[1, 0, : T // 3] = 0.0
    X = rnd(rng, 3, C, Tf)
    w = rnd(rng, C, F, 1, scale=F ** -0.5)
    s_out, s_act = np.float32(0.53), np.float32(0.7071)
    mag = O.causal_stft_mag(wav, n_fft, hop)
    P = ((np.log(np.maximum(mag, np.float32(1e-5))) - np.float32(-4.3)) / np.float32(2.8)).astype(np.float32)
    ref = (X + s_out * O.sconv1d(P, w, None)).astype(np.float32)
    g = Guards(offset=offset)
    wd, xd, y, ya = g.input(wav, "wav"), g.input(X, "x"), g.output(X.shape, name="Y"), g.output(X.shape, name="Yact")
    try:
        (got, gact), names = twice(g, lambda: ops.spec_block(wd.t, w, xd.t, n_fft, hop, mean=-4.3, std=2.8, out_scale=float(s_out),
                                                             act_scale=float(s_act), out=y.t, out_act=ya.t), [y, ya])
    except RuntimeError as e:                    # the one-launch SpecBlock may refuse a misaligned placement
        refused_cleanly(g, [y, ya], f"spec_block n_fft={n_fft} T={T}", e)
        return
    tol = 2e-5 * max(1.0, float(np.abs(ref).max())) + 5e-3 * float(s_out) * float(np.abs(w).sum(1).max()) * float((mag <= 1e-3).any())
    assert float(np.abs(got.cpu().numpy() - ref).max()) <= tol
    assert float(np.abs(gact.cpu().numpy() - O.elu(ref * s_act)).max()) <= tol
    print(f"RECORD spec_block n_fft={n_fft} T={T} offset={offset}: {sorted(names)}")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C,T,ks", [(64, 16000, 5), (32, 1000, 5), (8, 3, 7)])
def test_conv_pre_guarded(ops, C, T, ks, offset):
    rng = np.random.default_rng(C)
    x = rnd(rng, 3, 1, T, scale=0.1)
    w, b = rnd(rng, C, 1, ks), rnd(rng, C)
    ref = O.sconv1d((x * np.float32(8.912)).astype(np.float32), w, b)
    g = Guards(offset=offset)
    xd, y = g.input(x, "x"), g.output(ref.shape, name="Y")
    (got,), _ = twice(g, lambda: ops.conv_pre(xd.t, w, b, 8.912, out=y.t), [y])
    close(got, ref, what=f"conv_pre offset {offset}")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("add", [True, False])
@pytest.mark.parametrize("C,Tin,T,ks", [(96, 16320, 16001, 5), (96, 16000, 16000, 5), (8, 68, 67, 5), (8, 4, 1, 5)])
def test_tail_guarded(ops, C, Tin, T, ks, add, offset):
    rng = np.random.default_rng(C + T)
    H = rnd(rng, 2, C, Tin)
    x = rnd(rng, 2, 1, T, scale=0.1)
    w, b = rnd(rng, 1, C, ks, scale=(C * ks) ** -0.5), rnd(rng, 1)
    ref = np.tanh(O.sconv1d(O.elu(H * np.float32(0.7071)), w, b) * np.float32(0.1122))[..., :T]
    if add:
        ref = ref + x
    g = Guards(offset=offset)
    hd, out = g.input(H, "H"), g.output((2, 1, T), name="out")
    xd = g.input(x, "x").t if add else None
    (got,), _ = twice(g, lambda: ops.tail(hd.t, w, b, xd, T=T, pre_scale=0.7071, out_scale=0.1122, out=out.t), [out])
    close(got, ref.astype(np.float32), 1e-6, f"tail offset {offset}")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("want", ["both", "logits", "mean"])
@pytest.mark.parametrize("D,O_,nb,hop,Fr,T", [(128, 32, 16, 320, 51, 16001), (128, 32, 16, 320, 50, 16000), (16, 8, 16, 4, 17, 67),
                                               (64, 32, 1, 32, 500, 15999), (8, 8, 1, 4, 1, 1)])
def test_head_guarded(ops, D, O_, nb, hop, Fr, T, want, offset):
    """N * hop > T: the head computes more columns than it stores."""
    rng = np.random.default_rng(D + hop)
    Z = rnd(rng, 2, D, Fr)
    sd = {"reverse_convolution.weight": rnd(rng, D, O_, hop, scale=D ** -0.5), "reverse_convolution.bias": rnd(rng, O_, scale=0.1),
          "last_layer.weight": rnd(rng, nb, O_, 1, scale=O_ ** -0.5), "last_layer.bias": rnd(rng, nb)}
    ref = O.head_forward(O._Net(None, sd), Z, T)
    g = Guards(offset=offset)
    z = g.input(Z, "Z")
    lg = g.output((2, nb, T), name="logits") if want != "mean" else None
    mn = g.output((2, nb), name="mean") if want != "logits" else None
    outs = [a for a in (lg, mn) if a is not None]
    got, _ = twice(g, lambda: ops.head(z.t, sd["reverse_convolution.weight"], sd["reverse_convolution.bias"], sd["last_layer.weight"],
                                       sd["last_layer.bias"], T, want_logits=lg is not None, want_mean=mn is not None,
                                       out=None if lg is None else lg.t, out_mean=None if mn is None else mn.t), outs)
    if lg is not None:
        close(got[0], ref, what=f"head logits offset {offset}")
    if mn is not None:
        close(got[-1], O.mean_probabilities(ref), 2e-6, f"head mean offset {offset}")


# ================================================================== f16 units
def _f16_case(ops, name, fresh, guarded, outs, g):
    """An f16 entry point on guarded buffers against the same call on fresh buffers (which test_gpu_h16 holds to the mode's oracle):
    bit-identical, guards intact, twice.  Misaligned c8 operands may instead be refused: cleanly, every arena untouched.
    -> "ok" or "refused"."""
    ref = fresh()
    ref = [bits(r) for r in (ref if isinstance(ref, (tuple, list)) else [ref])]
    try:
        got, _ = twice(g, guarded, outs)
    except RuntimeError as e:
        refused_cleanly(g, outs, name, e)
        return "refused"
    for o, r, x in zip(outs, ref, got):
        assert torch.equal(bits(x), r), f"{name}: guarded result differs from the fresh-buffer result ({o.name})"
    print(f"RECORD {name} offset={g.offset}: computed")
    return "ok"


def _c8_input(ops, g, X, name):
    """A c8 tensor of X (f32 [B, C, T]) placed in a guarded arena."""
    x16 = ops.h16_from_f32(torch.from_numpy(X).cuda())
    return g.input(x16.cpu(), name)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("B,C,T", [(2, 33, 17), (3, 129, 300), (2, 8, 1), (2, 64, 1000)])
def test_h16_layout_guarded(ops, B, C, T, offset):
    rng = np.random.default_rng(B + C + T)
    X = rnd(rng, B, C, T)
    g = Guards(offset=offset)
    x = g.input(X, "X")
    G = (C + 15) // 16 * 2
    y16 = g.output((B, G, T, 8), torch.float16, name="c8")
    st = _f16_case(ops, f"h16_from_f32 C={C}", lambda: ops.h16_from_f32(torch.from_numpy(X).cuda(), 0.5, True),
                   lambda: ops.h16_from_f32(x.t, 0.5, True, out=y16.t), [y16], g)
    if st == "ok":                                   # channels >= C are zero-filled, the rest is the f16 rounding of elu(x / 2)
        c8 = y16.t.float().cpu().numpy().transpose(0, 1, 3, 2).reshape(B, G * 8, T)
        assert (c8[:, C:] == 0).all()
        ref16 = O.elu(X * np.float32(0.5)).astype(np.float16).astype(np.float32)
        assert (np.abs(c8[:, :C] - ref16) <= np.abs(ref16) * 2.0 ** -10 + 2.0 ** -24).all()
    g2 = Guards(offset=offset)
    src = _c8_input(ops, g2, X, "c8 in")
    y = g2.output((B, C, T), name="Y")
    _f16_case(ops, f"h16_to_f32 C={C}", lambda: ops.h16_to_f32(ops.h16_from_f32(torch.from_numpy(X).cuda()), C),
              lambda: ops.h16_to_f32(src.t, C, out=y.t), [y], g2)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C,T", [(64, 244), (64, 245), (128, 121), (64, 1)])
def test_h16_resblock_guarded(ops, C, T, offset):
    rng = np.random.default_rng(C + T)
    B = 2
    X = rnd(rng, B, C, T)
    w1, w2 = rnd(rng, C, C, 1, scale=C ** -0.5), rnd(rng, C, C, 1, scale=C ** -0.5)
    d1, d2 = rnd(rng, C, 1, 5, scale=0.45), rnd(rng, C, 1, 5, scale=0.45)
    b1, b2 = rnd(rng, C, scale=0.1), rnd(rng, C, scale=0.1)
    args = (w1, d1, b1, w2, d2, b2)
    g = Guards(offset=offset)
    x = _c8_input(ops, g, X, "X16")
    y, ya = g.output(x.t.shape, torch.float16, name="Y16"), g.output(x.t.shape, torch.float16, name="Yact16")
    fresh = ops.h16_from_f32(torch.from_numpy(X).cuda())
    _f16_case(ops, f"h16_resblock C={C} T={T}", lambda: ops.h16_resblock(fresh, *args, pre_scale=0.866, out_scale=0.41, act_scale=0.7),
              lambda: ops.h16_resblock(x.t, *args, pre_scale=0.866, out_scale=0.41, act_scale=0.7, out=y.t, out_act=ya.t), [y, ya], g)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("K,M,Tin,r", [(64, 128, 1001, 2), (128, 256, 501, 4), (32, 64, 70, 4)])
def test_h16_conv_film_guarded(ops, K, M, Tin, r, offset):
    rng = np.random.default_rng(K + M + Tin)
    B = 2
    X = rnd(rng, B, K, Tin)
    w_pw, w_dw, b = rnd(rng, M, K, 1, scale=K ** -0.5), rnd(rng, M, 1, 2 * r, scale=0.3), rnd(rng, M, scale=0.1)
    film = rnd(rng, B, 4, 2)
    Tout = -(-Tin // r)
    g = Guards(offset=offset)
    x, f = _c8_input(ops, g, X, "X16"), g.input(film, "film")
    shp = (B, (M + 15) // 16 * 2, Tout, 8)
    y, ya = g.output(shp, torch.float16, name="Y16"), g.output(shp, torch.float16, name="Yact16")
    fresh = ops.h16_from_f32(torch.from_numpy(X).cuda())
    _f16_case(ops, f"h16_conv_film r={r}",
              lambda: ops.h16_conv_film(fresh, w_pw, w_dw, b, torch.from_numpy(film).cuda(), 2 * r, r, 2 * r - r, act_scale=0.7),
              lambda: ops.h16_conv_film(x.t, w_pw, w_dw, b, f.t, 2 * r, r, 2 * r - r, act_scale=0.7, out=y.t, out_act=ya.t), [y, ya], g)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C,Tin,T,ks", [(96, 16320, 16001, 5), (96, 4, 3, 5), (48, 333, 330, 3)])
def test_h16_tail_guarded(ops, C, Tin, T, ks, offset):
    rng = np.random.default_rng(C + T)
    B = 2
    A = rnd(rng, B, C, Tin)
    x = rnd(rng, B, 1, T, scale=0.1)
    w, b = rnd(rng, 1, C, ks, scale=(C * ks) ** -0.5), rnd(rng, 1)
    g = Guards(offset=offset)
    a, xd, out = _c8_input(ops, g, A, "A16"), g.input(x, "x"), g.output((B, 1, T), name="out")
    fresh = ops.h16_from_f32(torch.from_numpy(A).cuda())
    _f16_case(ops, f"h16_tail Tin={Tin} T={T}", lambda: ops.h16_tail(fresh, w, b, T, 0.1122, x=torch.from_numpy(x).cuda()),
              lambda: ops.h16_tail(a.t, w, b, T, 0.1122, x=xd.t, out=out.t), [out], g)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("B,D,Fr", [(3, 128, 50), (2, 40, 7), (2, 128, 1)])
def test_h16_l2norm_and_head_guarded(ops, B, D, Fr, offset):
    rng = np.random.default_rng(B + D + Fr)
    lat = rnd(rng, B, D, Fr)
    g = Guards(offset=offset)
    l = g.input(lat, "lat")
    y = g.output((B, (D + 15) // 16 * 2, Fr, 8), torch.float16, name="Y16")
    _f16_case(ops, f"h16_l2norm D={D}", lambda: ops.h16_l2norm(torch.from_numpy(lat).cuda()), lambda: ops.h16_l2norm(l.t, out=y.t), [y], g)
    nb, hop, Dh = 16, 32, -(-D // 16) * 16          # head16 serves D % 16 == 0, hop % 32 == 0
    lat = rnd(rng, B, Dh, Fr)
    T = Fr * hop - 3 if Fr > 1 else hop - 3
    wc, bc = rnd(rng, Dh, nb * hop, scale=Dh ** -0.5), rnd(rng, nb)
    g2 = Guards(offset=offset)
    l2, mean = g2.input(lat, "lat"), g2.output((B, nb), name="mean")
    _f16_case(ops, f"h16_head D={Dh}", lambda: ops.h16_head(torch.from_numpy(lat).cuda(), wc, bc, T), lambda: ops.h16_head(l2.t, wc, bc, T, out=mean.t),
              [mean], g2)


# ================================================================== whole nets through the C ABI
def _small_cases():
    from test_gpu_fuzz import _net_cases
    out = []
    for idx, cfg, _, B in _net_cases(16, 99)[:4]:
        hop = int(np.prod(cfg["strides"]))
        for T in sorted({1, max(hop - 1, 1), hop, hop + 1}):
            out.append((idx, cfg, T, max(B, 2)))
    return out


def _net_guarded(net, kind, X, M, add_input, msg_rows, want, precision="f32"):
    """One forward of a HipNet's handle through the C ABI, every buffer guarded, twice -> the outputs (numpy)."""
    import ctypes as C
    from waveverify_amd import _lib
    lib = _lib.load()
    B, _, T = X.shape
    sfx = "_f16" if precision == "f16" else ""
    g = Guards()
    x = g.input(X, "x")
    ws = g.workspace(int(lib.wv_workspace_bytes(net._h, B, T)), "workspace")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = net.cfg.head_bits if kind != "generator" else 0
    if kind == "generator":
        m = g.input(M[:msg_rows], "msg")
        out = g.output((B, 1, T), name="out")
        outs = [out]
        call = lambda: _lib.check(getattr(lib, "wv_generator_forward" + sfx)(net._h, x.t.data_ptr(), m.t.data_ptr(), msg_rows, out.t.data_ptr(),
                                                                               int(add_input), B, T, ws.t.data_ptr(), ws.t.numel(), st))
    elif kind == "encoder":
        m = g.input(M[:msg_rows], "msg")
        out = g.output((B, net.cfg.dimension, -(-T // net.cfg.hop_length)), name="latent")
        outs = [out]
        call = lambda: _lib.check(lib.wv_encoder_forward(net._h, x.t.data_ptr(), m.t.data_ptr(), msg_rows, out.t.data_ptr(), B, T,
                                                         ws.t.data_ptr(), ws.t.numel(), st))
    elif kind == "detector":
        lg = g.output((B, nb, T), name="logits") if "logits" in want else None
        mn = g.output((B, nb), name="mean") if "mean" in want else None
        outs = [a for a in (lg, mn) if a is not None]
        call = lambda: _lib.check(getattr(lib, "wv_detector_forward" + sfx)(net._h, x.t.data_ptr(), None if lg is None else lg.t.data_ptr(),
                                                                              None if mn is None else mn.t.data_ptr(), B, T, ws.t.data_ptr(),
                                                                              ws.t.numel(), st))
    else:
        out = g.output((B, 1, T), name="logits")
        outs = [out]
        call = lambda: _lib.check(getattr(lib, "wv_locator_forward" + sfx)(net._h, x.t.data_ptr(), out.t.data_ptr(), B, T, ws.t.data_ptr(),
                                                                             ws.t.numel(), st))
    got, _ = twice(g, call, outs)
    return [t.cpu().numpy() for t in got]


@pytest.mark.parametrize("idx,cfgkw,T,B", _small_cases())
def test_small_nets_guarded(idx, cfgkw, T, B):
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict, synthetic_clips
    from waveverify_amd.nets import HipNet
    kw = dict(cfgkw)
    nspec = len(kw["strides"]) + 1
    kw["spec_means"] = [-4.0 + 0.1 * i for i in range(nspec)]
    kw["spec_stds"] = [2.5 + 0.05 * i for i in range(nspec)]
    x, msg = synthetic_clips(B, T, seed=1000 + idx)
    cg = default_config("generator", **kw)
    sdg = random_state_dict(cg, 31 + idx, parametrized=bool(idx & 1))
    G = HipNet(cg, sdg)
    ref = O.generator_forward(cg, sdg, x, msg)
    close(_net_guarded(G, "generator", x, msg, False, B, ())[0], ref, tol=5e-5, what=f"generator #{idx} T={T}")
    ref1 = O.generator_forward(cg, sdg, x, np.repeat(msg[:1], B, 0)) + x
    close(_net_guarded(G, "generator", x, msg, True, 1, ())[0], ref1, tol=5e-5, what=f"generator #{idx} T={T} msg_rows 1 + input")
    for kind in ("detector", "locator"):
        dk = {k: v for k, v in kw.items() if k not in ("channels_dec", "n_residual_dec", "embedding_dim", "embedding_layers")}
        cd = default_config(kind, **dk)
        sdd = random_state_dict(cd, 57 + idx)
        net = HipNet(cd, sdd)
        if kind == "detector":
            refl = O.detector_forward(cd, sdd, x)
            lg, mn = _net_guarded(net, kind, x, None, False, 0, ("logits", "mean"))
            close(lg, refl, tol=1e-4, what=f"detector #{idx} T={T}")
            close(mn, O.mean_probabilities(refl), tol=1e-4, what=f"detector mean #{idx} T={T}")
            assert np.array_equal(_net_guarded(net, kind, x, None, False, 0, ("mean",))[0], mn)
            assert np.array_equal(_net_guarded(net, kind, x, None, False, 0, ("logits",))[0], lg)
        else:
            close(_net_guarded(net, kind, x, None, False, 0, ())[0], O.locator_forward(cd, sdd, x), tol=1e-4, what=f"locator #{idx} T={T}")


@pytest.fixture(scope="module")
def default_nets():
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    out = {}
    for k in ("generator", "detector", "locator"):
        c = default_config(k)
        sd = random_state_dict(c, 0)
        out[k] = (HipNet(c, sd), c, sd)
    return out


@pytest.mark.parametrize("T", [16001, 4800])
def test_default_nets_guarded(default_nets, T):
    """The default nets at full length: every forward bit-identical to the same call on fresh buffers (which test_gpu_nets / test_gpu_h16
    hold to the reference and the oracles); at T = 4800 also the exact path against the oracle at smoke()'s bars."""
    from waveverify_amd.init import synthetic_clips
    x, msg = synthetic_clips(2, T, seed=T)
    xt, mt = torch.from_numpy(x).cuda(), torch.from_numpy(msg).cuda()
    G, cg, sdg = default_nets["generator"]
    wm = _net_guarded(G, "generator", x, msg, True, 2, ())[0]
    assert np.array_equal(wm, G.generator(xt, mt, add_input=True).cpu().numpy())
    if T == 4800:
        close(wm, O.embed(cg, sdg, x, msg), tol=1e-4, what=f"default generator T={T}")
    lat = _net_guarded(G, "encoder", x, msg, False, 2, ())[0]
    assert np.array_equal(lat, G.encoder(xt, mt).cpu().numpy())
    wm16 = _net_guarded(G, "generator", x, msg, True, 2, (), "f16")[0]
    assert np.array_equal(wm16, G.generator(xt, mt, add_input=True, precision="f16").cpu().numpy())
    D, cd, sdd = default_nets["detector"]
    wm_ref = wm
    wmt = torch.from_numpy(wm_ref).cuda()
    lg, mn = _net_guarded(D, "detector", wm_ref, None, False, 0, ("logits", "mean"))
    lg0, mn0 = D._head(wmt, True, True)
    assert np.array_equal(lg, lg0.cpu().numpy()) and np.array_equal(mn, mn0.cpu().numpy())
    if T == 4800:
        refl = O.detector_forward(cd, sdd, wm_ref)
        close(lg, refl, tol=1e-4, what=f"default detector T={T}")
        close(mn, O.mean_probabilities(refl), tol=1e-4, what=f"default detector mean T={T}")
    for want in (("logits", "mean"), ("mean",)):
        got16 = _net_guarded(D, "detector", wm_ref, None, False, 0, want, "f16")
        lg16, mn16 = D._head(wmt, "logits" in want, True, precision="f16")
        assert np.array_equal(got16[-1], mn16.cpu().numpy())
        if "logits" in want:
            assert np.array_equal(got16[0], lg16.cpu().numpy())
    L, cl, sdl = default_nets["locator"]
    lo = _net_guarded(L, "locator", wm_ref, None, False, 0, ())[0]
    assert np.array_equal(lo, L.locator(wmt).cpu().numpy())
    if T == 4800:
        close(lo, O.locator_forward(cl, sdl, wm_ref), tol=1e-3, what=f"default locator T={T}")
    assert np.array_equal(_net_guarded(L, "locator", wm_ref, None, False, 0, (), "f16")[0], L.locator(wmt, precision="f16").cpu().numpy())


def test_f16_fallback_spectrogram_route_guarded():
    """A configuration whose SpecBlocks are no spec16 geometry (test_gpu_h16's sweep configuration 4): the f16 plan runs the exact STFT
    kernel and converts to the c8 layout in the workspace, whose padded channels must be written, not inherited."""
    from test_gpu_h16 import _other_configuration
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict, synthetic_clips
    from waveverify_amd.nets import HipNet
    gkw, kw, T = _other_configuration(4)
    cg, cd = default_config("generator", **gkw), default_config("detector", **kw)
    G, D = HipNet(cg, random_state_dict(cg, 11)), HipNet(cd, random_state_dict(cd, 11))
    x, msg = synthetic_clips(2, 4000, seed=8)
    xt, mt = torch.from_numpy(x).cuda(), torch.from_numpy(msg).cuda()
    fresh, names = kernels_run(lambda: G.generator(xt, mt, add_input=True, precision="f16"))
    assert not any(n.startswith("spec16<") for n in names) and any(n.startswith("stft_logmag<") for n in names), names
    assert np.array_equal(_net_guarded(G, "generator", x, msg, True, 2, (), "f16")[0], fresh.cpu().numpy())
    lg16, mn16 = D._head(xt, True, True, precision="f16")
    got = _net_guarded(D, "detector", x, None, False, 0, ("logits", "mean"), "f16")
    assert np.array_equal(got[0], lg16.cpu().numpy()) and np.array_equal(got[1], mn16.cpu().numpy())


# ================================================================== windowed long-form
def test_window_gather_and_scatter_contracts():
    import ctypes as C
    from waveverify_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(5)
    n_src, L = 1001, 64
    src_np = rnd(rng, n_src)
    offs_np = np.array([0, 37, n_src - L, n_src - L + 1, -1, 500, n_src, -L], np.int64)
    W = len(offs_np)
    g = Guards()
    src, offs = g.input(src_np, "src"), g.input(offs_np, "offs")
    dst = g.output((W, 1, L), name="dst")
    _lib.check(lib.wv_window_gather(src.t.data_ptr(), n_src, offs.t.data_ptr(), dst.t.data_ptr(), W, L, st), "wv_window_gather")
    torch.cuda.synchronize()
    inside = (offs_np >= 0) & (offs_np + L <= n_src)
    skip = torch.from_numpy(np.repeat(~inside, L).reshape(W, 1, L))
    dst.check(expect_unwritten=skip)
    src.check(), offs.check()
    got = dst.t.cpu().numpy()
    for w in np.nonzero(inside)[0]:
        assert np.array_equal(got[w, 0], src_np[offs_np[w]: offs_np[w] + L])
    # scatter: y [W, C, L] -> out; only [lo, hi) of each window is written
    Cc, Ws, n_out = 3, 4, 3 * 400
    y_np = rnd(rng, Ws, Cc, L)
    desc_np = np.array([[0, 400, 0, 64], [64, 400, 5, 60], [124, 400, 0, 0], [336, 400, 10, 64]], np.int64)
    g2 = Guards()
    y, desc = g2.input(y_np, "y"), g2.input(desc_np, "desc")
    out = g2.output((n_out,), name="out")
    _lib.check(lib.wv_window_scatter(y.t.data_ptr(), desc.t.data_ptr(), out.t.data_ptr(), n_out, Ws, Cc, L, st), "wv_window_scatter")
    torch.cuda.synchronize()
    want = np.full(n_out, np.nan, np.float32)
    written = np.zeros(n_out, bool)
    for w, (o, rs, lo, hi) in enumerate(desc_np):
        for c in range(Cc):
            want[o + c * rs + lo: o + c * rs + hi] = y_np[w, c, lo:hi]
            written[o + c * rs + lo: o + c * rs + hi] = True
    out.check(expect_unwritten=torch.from_numpy(~written))
    y.check(), desc.check()
    assert np.array_equal(out.t.cpu().numpy()[written], want[written])


# ================================================================== whole-test reuse under poisoned workspaces
# The package allocates every workspace and saved buffer through waveverify_amd._lib.scratch; under the `poison` fixture each one is an
# exact-size 0xFF arena between guards, checked when the test ends.  These run existing tests (their oracles, their bars) that way.
def _fresh_nets(fn, *args):
    """test_gpu_window_fuzz keeps its nets from test to test; here they are built anew, so that their workspaces come from the fixture."""
    import test_gpu_window_fuzz as TF
    TF._net.cache_clear()
    try:
        fn(*args)
    finally:
        TF._net.cache_clear()


def _reuse():
    import test_gpu_train as TT
    import test_gpu_window as TW
    import test_gpu_window_fuzz as TF
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    cases = [
        ("half", lambda: TT.test_half_block_gradients_vs_oracle(5, 96, 36)),
        ("half T16000", lambda: TT.test_half_block_gradients_vs_oracle(2, 64, 16000)),
        ("block", lambda: TT.test_block_gradients_vs_oracle(3, 192, 400, True)),
        ("block paths", lambda: TT.test_block_backward_paths_agree(2, 40, 52)),
        ("convpre", lambda: TT.test_convpre_gradients_vs_reference_autograd_and_oracle(golden)),
        ("spec", lambda: TT.test_spec_add_gradients_vs_reference_autograd_and_oracle(golden)),
        ("convpost", lambda: TT.test_convpost_gradients_vs_reference_autograd_and_oracle(golden)),
        ("head N*hop>T", lambda: TT.test_head_forward_backward_vs_torch_modules(2, 128, 32, 16, 320, 51, 16001)),
        ("up", lambda: TT.test_upsample_unit_gradients_vs_reference_autograd_and_oracle(golden)),
        ("tail 16320/16001", lambda: TT.test_decoder_tail_vs_torch_autograd(2, 96, 16320, 16001, 5)),
        ("bce", lambda: TT.test_bce_at_training_size_vs_oracle_and_errors()),
        ("adamw", lambda: TT.test_flat_adamw_with_clipping_vs_torch()),
        ("window mixed lengths", lambda: TW.test_mixed_lengths_windowed_vs_whole_clip({k: TW._net(k) for k in TW.KINDS})),
        ("window detect session", lambda: TW.test_detect_session({k: TW._net(k) for k in TW.KINDS})),
        ("window f16 detect", lambda: TW.test_windowed_f16_detect_vs_the_oracle({k: TW._net(k) for k in TW.KINDS})),
    ]
    cases += [("window small net", lambda: _fresh_nets(TF.test_windowed_forwards_vs_float64, next(c for c in TF.EXACT if c[0] == "x14.detector"))),
              ("window small-net session", lambda: _fresh_nets(TF.test_sessions_vs_float64, next(c for c in TF.EXACT if c[0] == "x6.generator")))]
    for args in [(4, 64, 128, 16000, 4, 2, True), (3, 128, 256, 8000, 8, 4, True), (2, 256, 512, 2000, 10, 5, True),
                 (2, 512, 1024, 400, 16, 8, True), (3, 96, 64, 404, 5, 1, False), (2, 64, 128, 36, 7, 3, True), (3, 32, 32, 50, 5, 1, True),
                 (2, 32, 64, 1001, 16, 8, True), (2, 24, 40, 7, 5, 1, False)]:
        cases.append((f"unit {args}", lambda a=args: TT.test_unit_gradients_vs_oracle(*a)))
    return cases


REUSE = [name for name, _ in _reuse()]


@pytest.mark.parametrize("name", REUSE)
def test_existing_cases_on_poisoned_workspaces(poison, name):
    fn = dict(_reuse())[name]
    fn()
    assert poison, f"{name}: no workspace went through waveverify_amd._lib.scratch"


# ================================================================== training handles on guarded arenas
# Parameters, inputs and gradients in guarded arenas (gradient destinations through `into=`, as the trainer's flat arenas hand them
# out), workspaces and saved buffers from the poison fixture, a second backward on re-poisoned workspaces bit-identical, the oracle of
# test_gpu_train at its bars.  offset = 1 puts every operand and every gradient destination one float past a 16-byte boundary.
GKEYS = ("dx", "dg_pw", "dv_pw", "dg_dw", "dv_dw", "db_dw")


def _rel(got, ref):
    got = got.detach().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def _rerun(poison, first_ws, outs, g, call):
    """Re-poison the workspaces made from index first_ws on, re-fill the outputs, run `call` again: every output bit-identical."""
    before = [bits(o.t) for o in outs]
    for a in poison[first_ws:]:
        a.repoison()
    for o in outs:
        o.refill_pattern()
    call()
    g.check()
    for o, b in zip(outs, before):
        assert torch.equal(bits(o.t), b), f"{o.name}: second run on re-poisoned workspaces differs from the first"


def _unit_params(rng, K, M, ks):
    return dict(g_pw=(0.5 + np.abs(rng.standard_normal((M, 1, 1)))).astype(np.float32),
                v_pw=(rng.standard_normal((M, K, 1)) * K ** -0.5).astype(np.float32),
                g_dw=(0.5 + np.abs(rng.standard_normal((M, 1, 1)))).astype(np.float32),
                v_dw=(rng.standard_normal((M, 1, ks)) * ks ** -0.5).astype(np.float32),
                b_dw=(rng.standard_normal(M) * 0.1).astype(np.float32))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("B,K,M,T,ks,stride,elu", [(2, 64, 128, 1000, 4, 2, True), (2, 128, 256, 800, 8, 4, True), (2, 256, 512, 400, 10, 5, True),
                                                   (2, 64, 128, 400, 16, 8, True), (3, 96, 64, 404, 5, 1, False), (2, 64, 128, 36, 7, 3, True),
                                                   (3, 32, 32, 50, 5, 1, True), (2, 24, 40, 7, 5, 1, False)])
def test_train_unit_guarded(poison, B, K, M, T, ks, stride, elu, offset):
    """wv_train_unit_forward / _backward: every launch_dw_bwd branch the net's strides reach (r = 2 / 4 / 5 / 8, k5 stride 1, the
    generic stencil at k7 / r3), T % 4 == 0 and ragged lengths."""
    from oracle import wv_oracle_train as OT
    from waveverify_amd.train import TrainUnit
    rng = np.random.default_rng(K + M + T)
    x = rng.standard_normal((B, K, T)).astype(np.float32)
    p = _unit_params(rng, K, M, ks)
    dy = rng.standard_normal((B, M, -(-T // stride))).astype(np.float32)
    s = 0.7071068
    ref = OT.unit_backward(x, s, p["g_pw"], p["v_pw"], p["g_dw"], p["v_dw"], p["b_dw"], dy, stride=stride, elu=elu)
    g = Guards(offset=offset)
    xg, dyg = g.input(x, "x"), g.input(dy, "dy")
    pg = {k: g.input(v, k) for k, v in p.items()}
    into = {k: g.output(ref[k].shape, name=k) for k in GKEYS}
    unit = TrainUnit(K, M, ks, stride)
    pt = {k: a.t for k, a in pg.items()}
    y = unit.forward(xg.t, pt, s, pre_elu=elu)
    assert _rel(y, ref["y"]) <= 2e-5
    first = len(poison)
    call = lambda: unit.backward(xg.t, pt, s, dyg.t, pre_elu=elu, into={k: a.t for k, a in into.items()})
    _, names = kernels_run(call)
    g.check()
    for k in GKEYS:
        assert _rel(into[k].t, ref[k]) <= 1e-4, (k, _rel(into[k].t, ref[k]))
    _rerun(poison, first, list(into.values()), g, call)
    if offset:                                   # the fused ELU' epilogue needs 16-byte aligned rows: the dx GEMM falls back
        assert not any(n.startswith("pw_dw_k5_dact<") for n in names), sorted(names)
    print(f"RECORD train_unit K={K} M={M} T={T} ks={ks} r={stride} offset={offset}: {sorted(names)}")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("B,C,T,with_param", [(2, 128, 1000, True), (2, 96, 236, False), (3, 40, 36, True), (1, 128, 2000, True)])
def test_train_block_guarded(poison, B, C, T, with_param, offset):
    """wv_train_block_forward / _backward: the saved activations are bitwise unchanged by backward (twice), every gradient lands in
    its guarded destination, the oracle's bars."""
    from oracle import wv_oracle_train as OT
    from waveverify_amd.train import TrainBlock
    rng = np.random.default_rng(B * 77 + C + T)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    dy = rng.standard_normal((B, C, T)).astype(np.float32)
    ps = [_unit_params(rng, C, C, 5) for _ in range(2)]
    rsp = np.array([0.8], np.float32) if with_param else None
    pre, rs = 0.8164966, 0.5773503
    ref = OT.block_backward(x, ps, rsp, pre, rs, dy)
    g = Guards(offset=offset)
    xg, dyg = g.input(x, "x"), g.input(dy, "dy")
    pt = [{k: g.input(v, f"half{i}.{k}").t for k, v in p.items()} for i, p in enumerate(ps)]
    rt = None if rsp is None else g.input(rsp, "res_scale_param").t
    halves = [{k: g.output(ps[i][k[1:]].shape, name=f"half{i}.{k}") for k in GKEYS[1:]} for i in range(2)]
    dxg = g.output(x.shape, name="dx")
    drs = g.output((1,), name="d_res_scale_param") if with_param else None
    into = dict(halves=[{k: a.t for k, a in h.items()} for h in halves], dx=dxg.t)
    if drs is not None:
        into["d_res_scale_param"] = drs.t
    blk = TrainBlock(C)
    y, saved = blk.forward(xg.t, pt, rt, pre, rs)
    assert _rel(y, ref["y"]) <= 2e-5
    torch.cuda.synchronize()
    snap = saved.clone()
    first = len(poison)
    call = lambda: blk.backward(xg.t, pt, rt, pre, rs, dyg.t, saved, into=into)
    call()
    g.check()
    assert torch.equal(saved, snap), "the block's backward changed its saved activations"
    assert _rel(dxg.t, ref["dx"]) <= 1e-4
    for i in (0, 1):
        for k in GKEYS[1:]:
            assert _rel(halves[i][k].t, ref["halves"][i][k]) <= 1e-4, (i, k)
    if drs is not None:
        assert abs(float(drs.t.item()) - ref["d_res_scale_param"]) <= 1e-4 * max(1.0, abs(ref["d_res_scale_param"]))
    outs = [dxg] + [a for h in halves for a in h.values()] + ([drs] if drs is not None else [])
    _rerun(poison, first, outs, g, call)
    assert torch.equal(saved, snap), "the block's backward changed its saved activations"


@pytest.mark.parametrize("offset", [0, 1])
def test_adamw_and_sumsq_guarded(poison, offset):
    """wv_train_sumsq + wv_train_adamw in place on a guarded parameter arena (ragged size): surroundings untouched, gradients unchanged,
    torch's clip_grad_norm_ -> AdamW at test_gpu_train's bar; a second optimizer from the same state on a re-poisoned workspace
    is bit-identical."""
    from waveverify_amd.train import FlatAdamW
    rng = np.random.default_rng(3)
    n = 100_003
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(gs * rng.standard_normal(n)).astype(np.float32) for gs in (1.0, 2.0)]
    ref_p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([ref_p], lr=1e-2, betas=(0.8, 0.99))
    norms = []
    for gr in grads:
        ref_p.grad = torch.from_numpy(gr.copy())
        norms.append(float(torch.nn.utils.clip_grad_norm_([ref_p], 10.0)))
        opt.step()
    results = []
    for _ in range(2):
        g = Guards(offset=offset)
        pa = g.output((n,), name="params")
        pa.t.copy_(torch.from_numpy(p0))
        gg = [g.input(gr, f"grad{i}") for i, gr in enumerate(grads)]
        mine = FlatAdamW(n, lr=1e-2, betas=(0.8, 0.99), gamma=1.0)
        for gi, rn in zip(gg, norms):
            norm = mine.step(pa.t, gi.t, max_norm=10.0)
            assert abs(float(norm.item()) - rn) <= 2e-6 * rn
        g.check()
        assert float((pa.t.cpu() - ref_p.detach()).abs().max()) <= 2e-6
        results.append(bits(pa.t))
    assert torch.equal(results[0], results[1])


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 4099, 160_001])
def test_l1_guarded(poison, n, offset):
    """wv_train_l1 on guarded ragged operands: mean |a - b| and grad_scale * sign(a - b) / n (float64 reference), twice bit-identical."""
    from waveverify_amd.train import l1_loss
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    g = Guards(offset=offset)
    ag, bg = g.input(a, "a"), g.input(b, "b")
    runs = []
    for _ in range(2):
        for w in poison:
            w.repoison()
        loss, da = l1_loss(ag.t, bg.t, grad_scale=0.5)
        g.check()
        runs.append((bits(loss), bits(da)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    d = a.astype(np.float64) - b.astype(np.float64)
    assert abs(float(loss.item()) - np.abs(d).mean()) <= 1e-6 * max(1.0, np.abs(d).mean())
    assert np.allclose(da.cpu().numpy(), 0.5 * np.sign(d) / n, rtol=1e-6, atol=0)


# ================================================================== f16 units not above
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("K,M,Tin,ks,stride,pad", [(40, 64, 65, 1, 1, 0), (64, 128, 1001, 4, 2, 3), (24, 32, 17, 16, 8, 15), (100, 48, 50, 5, 1, 4)])
def test_h16_conv_guarded(ops, K, M, Tin, ks, stride, pad, offset):
    """wv_h16_conv plain and strided, c8 raw / act outputs and the f32 output, with a residual."""
    rng = np.random.default_rng(K + M + Tin + ks)
    B = 2
    X = rnd(rng, B, K, Tin)
    w_pw, w_dw = rnd(rng, M, K, 1, scale=K ** -0.5), (rnd(rng, M, 1, ks, scale=ks ** -0.5) if ks > 1 else None)
    bias = rnd(rng, M, scale=0.1)
    Tout = -(-Tin // stride)
    Gm = (M + 15) // 16 * 2
    R = rnd(rng, B, M, Tout)
    g = Guards(offset=offset)
    x, r = _c8_input(ops, g, X, "X16"), _c8_input(ops, g, R, "resid16")
    y, ya, yf = (g.output((B, Gm, Tout, 8), torch.float16, name="raw"), g.output((B, Gm, Tout, 8), torch.float16, name="act"),
                 g.output((B, M, Tout), name="f32"))
    fx, fr = ops.h16_from_f32(torch.from_numpy(X).cuda()), ops.h16_from_f32(torch.from_numpy(R).cuda())
    kw = dict(ks=ks, stride=stride, pad=pad, out_scale=0.7, act_scale=0.9, want_f32=True)

    def fresh():
        o = ops.h16_conv(fx, w_pw, w_dw, bias, resid16=fr, **kw)
        return [o["raw"], o["act"], o["f32"]]
    _f16_case(ops, f"h16_conv K={K} M={M} ks={ks} r={stride}", fresh,
              lambda: ops.h16_conv(x.t, w_pw, w_dw, bias, resid16=r.t, out=y.t, out_act=ya.t, out_f32=yf.t, **kw), [y, ya, yf], g)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C,T,ks", [(64, 1001, 7), (32, 5, 5)])
def test_h16_conv_pre_guarded(ops, C, T, ks, offset):
    rng = np.random.default_rng(C + T)
    x = rnd(rng, 3, 1, T, scale=0.1)
    w, b = rnd(rng, C, 1, ks, scale=0.4), rnd(rng, C, scale=0.1)
    g = Guards(offset=offset)
    xg, y = g.input(x, "x"), g.output((3, C // 8, T, 8), torch.float16, name="Y16")
    _f16_case(ops, f"h16_conv_pre C={C} T={T}", lambda: ops.h16_conv_pre(torch.from_numpy(x).cuda(), w, b, in_scale=8.9),
              lambda: ops.h16_conv_pre(xg.t, w, b, in_scale=8.9, out=y.t), [y], g)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("K,M,Tin,r", [(192, 96, 1, 2), (64, 32, 37, 3), (768, 384, 51, 5), (384, 192, 100, 4), (1536, 768, 50, 8)])
def test_h16_upsample_guarded(ops, K, M, Tin, r, offset):
    rng = np.random.default_rng(K + M + Tin + r)
    B = 2
    X = rnd(rng, B, K, Tin)
    w_ct, w_pw, b = rnd(rng, K, 1, 2 * r, scale=0.5), rnd(rng, M, K, 1, scale=K ** -0.5), rnd(rng, M, scale=0.1)
    g = Guards(offset=offset)
    x = _c8_input(ops, g, X, "X16")
    shp = (B, M // 8, Tin * r, 8)
    y, ya = g.output(shp, torch.float16, name="Y16"), g.output(shp, torch.float16, name="Yact16")
    fx = ops.h16_from_f32(torch.from_numpy(X).cuda())
    _f16_case(ops, f"h16_upsample K={K} r={r} Tin={Tin}", lambda: ops.h16_upsample(fx, w_ct, w_pw, b, r, act_scale=0.9),
              lambda: ops.h16_upsample(x.t, w_ct, w_pw, b, r, act_scale=0.9, out=y.t, out_act=ya.t), [y, ya], g)


# The written-out cases of the f16 fuzz (tests/h16_fuzz_cases.py: every launch_conv16 route at its smallest shape, the Tout / Tin edges, odd
# batches whose last two-clip tile holds one clip, ragged row blocks): a stray read or write there lands in padding, which no numeric
# comparison sees.  tests/test_gpu_h16_fuzz.py holds the same cases to the mode's oracle and to the restated route.
def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", H16.DENSE_EXPLICIT, ids=_ids(H16.DENSE_EXPLICIT))
def test_h16_conv_placed_cases_guarded(ops, case, offset):
    B, K, M, Tin, ks, stride, pad, epi, outs = case
    a = H16.dense_args(case)
    rng = np.random.default_rng(B + K + M + Tin + ks)
    X = rnd(rng, B, K, Tin)
    w_pw, w_dw = rnd(rng, M, K, 1, scale=K ** -0.5), (rnd(rng, M, 1, ks, scale=ks ** -0.5) if ks > 1 else None)
    bias = rnd(rng, M, scale=0.1)
    Gm = (M + 15) // 16 * 2
    g = Guards(offset=offset)
    x = _c8_input(ops, g, X, "X16")
    fx = ops.h16_from_f32(torch.from_numpy(X).cuda())
    y = g.output((B, Gm, a.Tout, 8), torch.float16, name="raw") if a.Y else None
    ya = g.output((B, Gm, a.Tout, 8), torch.float16, name="act") if a.Yact else None
    yf = g.output((B, M, a.Tout), name="f32") if a.Yf32 else None
    arenas = [o for o in (y, ya, yf) if o is not None]
    t = lambda o: None if o is None else o.t
    act = 0.9 if a.Yact else None
    if a.film:
        film = rnd(rng, B, a.bands, 2)
        f = g.input(film, "film")
        as_list = lambda r: list(r) if isinstance(r, (tuple, list)) else [r]
        fresh = lambda: as_list(ops.h16_conv_film(fx, w_pw, w_dw, bias, torch.from_numpy(film).cuda(), ks, stride, pad, act_scale=act, want_raw=a.Y))
        guarded = lambda: ops.h16_conv_film(x.t, w_pw, w_dw, bias, f.t, ks, stride, pad, act_scale=act, want_raw=a.Y, out=t(y), out_act=t(ya))
    else:
        kw = dict(ks=ks, stride=stride, pad=pad, out_scale=0.7, act_scale=act, want_raw=a.Y, want_f32=a.Yf32)
        r = fr = None
        if a.resid:
            R = rnd(rng, B, M, a.Tout)
            r, fr = _c8_input(ops, g, R, "resid16"), ops.h16_from_f32(torch.from_numpy(R).cuda())

        def fresh():
            o = ops.h16_conv(fx, w_pw, w_dw, bias, resid16=fr, **kw)
            return [o[k] for k in ("raw", "act", "f32") if k in o]
        guarded = lambda: ops.h16_conv(x.t, w_pw, w_dw, bias, resid16=t(r), out=t(y), out_act=t(ya), out_f32=t(yf), **kw)
    _f16_case(ops, f"h16_conv placed {case}", fresh, guarded, arenas, g)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", H16.UP_EXPLICIT, ids=_ids(H16.UP_EXPLICIT))
def test_h16_upsample_placed_cases_guarded(ops, case, offset):
    B, K, Mo, Tin, r, outs = case
    a = H16.up_args(case)
    rng = np.random.default_rng(B + K + Mo + Tin + r)
    X = rnd(rng, B, K, Tin)
    w_ct, w_pw, b = rnd(rng, K, 1, 2 * r, scale=0.5), rnd(rng, Mo, K, 1, scale=K ** -0.5), rnd(rng, Mo, scale=0.1)
    g = Guards(offset=offset)
    x = _c8_input(ops, g, X, "X16")
    shp = (B, Mo // 8, Tin * r, 8)
    y = g.output(shp, torch.float16, name="Y16") if a.Y else None
    ya = g.output(shp, torch.float16, name="Yact16") if a.Yact else None
    fx = ops.h16_from_f32(torch.from_numpy(X).cuda())
    act = 0.9 if a.Yact else None
    _f16_case(ops, f"h16_upsample placed {case}", lambda: ops.h16_upsample(fx, w_ct, w_pw, b, r, act_scale=act, want_raw=a.Y),
              lambda: ops.h16_upsample(x.t, w_ct, w_pw, b, r, act_scale=act, want_raw=a.Y, out=None if y is None else y.t,
                                       out_act=None if ya is None else ya.t), [o for o in (y, ya) if o is not None], g)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("basis", ["analytic", "learned"])
@pytest.mark.parametrize("n_fft,hop,T,C", [(64, 1, 257, 64), (128, 2, 255, 128), (128, 4, 1021, 64), (256, 32, 2081, 128)])
def test_h16_spec_block_guarded(ops, n_fft, hop, T, C, basis, offset):
    """wv_h16_spec_block, full and half-channel geometries, the analytic basis and a learned one with its side rows (sin_0, sin_{F-1})."""
    from test_gpu_stft_basis import make_basis
    rng = np.random.default_rng(n_fft + hop + T + C)
    F, Tf = n_fft // 2 + 1, -(-T // hop)
    wav = np.clip(rnd(rng, 3, 1, T, scale=0.1), -1, 1)
    wav[1, 0, : T // 3] = 0.0
    X = rnd(rng, 3, C, Tf)
    w = rnd(rng, C, F, 1, scale=F ** -0.5)
    bs = make_basis("learned", n_fft) if basis == "learned" else None
    g = Guards(offset=offset)
    wg, x = g.input(wav, "wav"), _c8_input(ops, g, X, "x16")
    y, ya = g.output(x.t.shape, torch.float16, name="Y16"), g.output(x.t.shape, torch.float16, name="Yact16")
    fw, fx = torch.from_numpy(wav).cuda(), ops.h16_from_f32(torch.from_numpy(X).cuda())
    kw = dict(mean=-4.3, std=2.8, out_scale=0.53, act_scale=0.7071, basis=bs)
    _f16_case(ops, f"h16_spec_block n_fft={n_fft} C={C} {basis}", lambda: ops.h16_spec_block(fw, w, fx, n_fft, hop, **kw),
              lambda: ops.h16_spec_block(wg.t, w, x.t, n_fft, hop, out=y.t, out_act=ya.t, **kw), [y, ya], g)


# ================================================================== effects on guarded inputs
@pytest.mark.parametrize("offset", [0, 1])
def test_fx_guarded_inputs(offset):
    """wv_fx_fir_bank (lowpass), wv_fx_resample and its adjoint on guarded ragged clips (B * T % 4 != 0): a read past either edge of the
    input would bring in a NaN; results bit-equal to the same calls on fresh tensors (test_gpu_effects holds those to the oracle)."""
    from waveverify_amd import effects as E
    rng = np.random.default_rng(17)
    B, T = 3, 4001
    x = (0.3 * rng.standard_normal((B, 1, T))).astype(np.float32)
    g = Guards(offset=offset)
    xg = g.input(x, "x")
    xf = torch.from_numpy(x).cuda()
    t_out = E.resampled_length(T, 16000, 11025)
    dy = (0.3 * rng.standard_normal((B, 1, t_out))).astype(np.float32)
    dyg = g.input(dy, "dy")
    for what, fresh, guarded in [
            ("lowpass", lambda: E.lowpass(xf, 0.2), lambda: E.lowpass(xg.t, 0.2)),
            ("resample", lambda: E.resample_waveform(xf, 16000, 11025), lambda: E.resample_waveform(xg.t, 16000, 11025)),
            ("resample adjoint", lambda: E.resample_waveform_adjoint(torch.from_numpy(dy).cuda(), 16000, 11025, T),
             lambda: E.resample_waveform_adjoint(dyg.t, 16000, 11025, T))]:
        ref, got = fresh(), guarded()
        g.check()
        assert torch.isfinite(got).all() and torch.equal(bits(got.contiguous()), bits(ref.contiguous())), what


# ================================================================== spectral losses through the C ABI
def _specloss_cases():
    import specloss_cases as SC
    return SC.guard_cases()


@pytest.mark.parametrize("cid", [c[0] for c in _specloss_cases()])
def test_specloss_guarded(cid):
    """wv_specloss: wm, x, terms, totals and dwm between guard bands, the workspace exactly wv_specloss_workspace_bytes long and 0xFF.
    The call adds into dwm, so dwm starts from a known pattern and must end as pattern + gradient; the float64 oracle at the bars of
    test_gpu_spectral_loss.py; a second call on a re-poisoned workspace bit-identical.  The STFT-only plan never writes the mel
    gradient region of the workspace (nothing may read it), the mel-only plan runs the bins kernel for its gradient alone."""
    import specloss_cases as SC
    from oracle import wv_oracle_specloss as OS
    from waveverify_amd import _lib
    from waveverify_amd import spectral_loss as SL
    _, scales, B, T, seed, bar = next(c for c in _specloss_cases() if c[0] == cid)
    wm, x = SC.clips(B, T, seed)
    ref = OS.spectral_oracle(wm, x, scales, stft_grad_scale=10.0, mel_grad_scale=20.0)
    plan = SL._Plan(scales)
    g = Guards()
    wm_g, x_g = g.input(wm, "wm"), g.input(x, "x")
    terms, totals, dwm = g.output((len(scales), 2), name="terms"), g.output((2,), name="totals"), g.output((B, 1, T), name="dwm")
    ws = g.workspace(int(_lib.load().wv_specloss_workspace_bytes(plan._h, B, T)), "workspace")
    base = torch.from_numpy(np.random.default_rng(seed).standard_normal((B, 1, T)).astype(np.float32)).cuda()
    runs = []
    for _ in range(2):
        g.repoison()
        dwm.t.copy_(base)
        _lib.check(SC.c_call(plan, wm_g.t, x_g.t, terms.t, totals.t, dwm.t, ws.t, 10.0, 20.0), "wv_specloss")
        g.check()
        runs.append([bits(a.t) for a in (terms, totals, dwm)])
    for a, p, q in zip((terms, totals, dwm), *runs):
        assert torch.equal(p, q), f"{a.name}: second run on a re-poisoned workspace differs from the first"
    got_terms, got_totals = terms.t.cpu().numpy().astype(np.float64), totals.t.cpu().numpy().astype(np.float64)
    grad = (dwm.t - base).cpu().numpy().astype(np.float64)
    assert np.isfinite(got_terms).all() and np.isfinite(got_totals).all() and np.isfinite(grad).all()
    for i, s in enumerate(ref["scales"]):
        for j, part in enumerate(("stft", "mel")):
            want = s[part] if s[part] is not None else 0.0
            assert abs(got_terms[i, j] - want) <= SC.TERM_BAR * abs(want), (cid, s["w"], part, got_terms[i, j], want)
    for j, part in enumerate(("stft", "mel")):
        assert abs(got_totals[j] - ref[part + "_total"]) <= SC.TERM_BAR * abs(ref[part + "_total"]), (cid, part)
    # dwm ends as pattern + gradient: the subtraction of the pattern costs one rounding of the sum, 1e-6 of the larger of the two
    fresh = torch.zeros(B, 1, T, device="cuda")
    _lib.check(SC.c_call(plan, wm_g.t, x_g.t, terms.t, totals.t, fresh, ws.t, 10.0, 20.0), "wv_specloss")
    assert float((dwm.t - base - fresh).abs().max()) <= 1e-6 * max(float(fresh.abs().max()), float(base.abs().max()))
    e = SC.rel_err(fresh.cpu().numpy(), ref["d_total"])
    print(f"RECORD specloss guarded {cid}: gradient {e:.2e} of max")
    assert e <= bar, (cid, e)
