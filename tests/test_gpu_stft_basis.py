"""Every STFT kernel route under a basis that is NOT the analytic one, against a float64 restatement of the op.

A run with spec_learnable: true (the reference's conf/base.yml) leaves trained `...spec.weight` tensors in a checkpoint, and the C ABI
takes any [2F, n_fft] basis.  Two bases:
  learned     the analytic basis plus 2 % of its peak as Gaussian noise on every row (waveverify_amd.init.learned_stft_bases' recipe);
  side        the analytic basis with sin_0 and sin_{F-1} replaced by rows of full size.  Both kernels keep those two rows out of
              their matrix part (the exact path's StftArgs::side, spec16's Spec16Args::side): a kernel that dropped or swapped them is
              off by O(1) here, while the analytic basis (sin_0 = 0, |sin_{F-1}| <= 1.4e-4) hides them.
Each case also checks, by the kernel name the profiler records, that it ran the route it is meant to cover."""
import numpy as np
import pytest
import torch

from oracle import wv_oracle as O

pytestmark = pytest.mark.gpu

MEAN, STD = -4.3, 2.8


@pytest.fixture(scope="module")
def ops():
    from waveverify_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_basis(kind: str, n_fft: int) -> np.ndarray:
    """[2F, n_fft] float32"""
    b = O.dft_basis(n_fft).astype(np.float64)
    F, peak = n_fft // 2 + 1, float(np.abs(b).max())
    rng = np.random.default_rng(1000 + n_fft)
    if kind == "learned":
        b = b + 0.02 * peak * rng.standard_normal(b.shape)
    else:
        b[F] = 0.5 * peak * rng.standard_normal(n_fft)
        b[2 * F - 1] = 0.5 * peak * rng.standard_normal(n_fft)
    return b.astype(np.float32)


def stft64(wav, basis, hop):
    """float64: frames of the causal-padded clip (n_fft - 1 zeros in front) times the basis -> (|X|, normalised 0.5 ln max(p, 1e-10))"""
    n_fft = basis.shape[1]
    F = n_fft // 2 + 1
    xp = np.pad(wav[:, 0, :].astype(np.float64), ((0, 0), (n_fft - 1, 0)))
    Tf = -(-wav.shape[-1] // hop)
    idx = np.arange(Tf)[:, None] * hop + np.arange(n_fft)[None, :]
    c = np.einsum("kn,btn->bkt", basis.astype(np.float64), xp[:, idx])
    p = c[:, :F] ** 2 + c[:, F:] ** 2
    return np.sqrt(p), (0.5 * np.log(np.maximum(p, 1e-10)) - MEAN) / STD


def clip(n_fft, hop, T, seed):
    rng = np.random.default_rng(seed)
    wav = np.clip(0.1 * rng.standard_normal((2, 1, T)), -1, 1).astype(np.float32)
    wav[1, 0, : T // 3] = 0.0                          # silence: both clamps
    return wav


def kernels_run(fn):
    from waveverify_amd import profile
    profile.enable(True)
    profile.reset()
    try:
        out = fn()
        names = {e["kernel"] for e in profile.collect()}
    finally:
        profile.enable(False)
    return out, names


def check_P(got, mag, ref, what):
    """test_stft_logmag's bars: 2e-5 relative where |X| > 1e-2, 1e-4 for 1e-3 < |X| <= 1e-2 (d log|X| = d|X| / |X| over f32 sums of
    n_fft terms: a plain f32 numpy sum of the side-row basis at n_fft 512 is 1.1e-4 off there), and the clamp allowance 5e-3 below"""
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    d = np.abs(got - ref)
    big, mid = mag > 1e-2, (mag > 1e-3) & (mag <= 1e-2)
    e_big, e_mid, e_q = float(d[big].max(initial=0)), float(d[mid].max(initial=0)), float(d[mag <= 1e-3].max(initial=0))
    print(f"MEASURE {what}: |X| > 1e-2 {e_big:.2e}, 1e-3 .. 1e-2 {e_mid:.2e}, quiet {e_q:.2e}")
    assert e_big <= 2e-5 * max(1.0, float(np.abs(ref).max())), (what, e_big)
    assert e_mid <= 1e-4, (what, e_mid)
    assert e_q <= 5e-3, (what, e_q)


def k1_bm(n_fft):
    bm, best = 128, -(-n_fft // 128) * 128
    for cand in (96, 64):
        if -(-n_fft // cand) * cand < best:
            best, bm = -(-n_fft // cand) * cand, cand
    return bm


# (n_fft, hop, T): K1 at BM 128 / 96 / 64 (more than 64 frames, a multiple of 4), the round-1 kernel (<= 64 frames or an odd count),
# the product's scales and hops (generator / detector 64/1 .. 1024/320, locator 128/4, 256/32), odd T and T = 1
STFT_CASES = [(64, 1, 16000), (64, 1, 1001), (64, 1, 60), (64, 1, 1), (96, 3, 3000), (96, 3, 301), (128, 2, 16000), (128, 2, 263),
              (128, 4, 1040), (128, 4, 1042), (256, 8, 16000), (256, 8, 1049), (256, 32, 16000), (512, 40, 16000), (512, 40, 4001),
              (1024, 320, 16000), (1024, 320, 40960), (1024, 320, 1)]


@pytest.mark.parametrize("basis_kind", ["learned", "side"])
@pytest.mark.parametrize("n_fft,hop,T", STFT_CASES)
def test_stft_logmag_with_a_basis(ops, basis_kind, n_fft, hop, T):
    basis = make_basis(basis_kind, n_fft)
    wav = clip(n_fft, hop, T, n_fft + hop + T)
    mag, ref = stft64(wav, basis, hop)
    got, names = kernels_run(lambda: ops.stft_logmag(cu(wav), n_fft, hop, mean=MEAN, std=STD, basis=basis))
    Tf = -(-T // hop)
    stft = [n for n in names if n.startswith("stft_logmag<")]
    if Tf > 64 and Tf % 4 == 0:
        assert len(stft) == 1 and stft[0].startswith(f"stft_logmag<{k1_bm(n_fft)},") and stft[0].endswith(",k1>"), names
    else:
        assert len(stft) == 1 and not stft[0].endswith(",k1>"), names
    check_P(got, mag, ref, f"stft_logmag {basis_kind} n_fft={n_fft} hop={hop} T={T} ({stft[0]})")


def _w(kind, M, F, rng):
    if kind == "selector":                             # W[m][f] = [m == f]: bin 0 and the Nyquist bin each land in a channel of their own
        w = np.zeros((M, F, 1), np.float32)
        for m in range(min(M, F)):
            w[m, m, 0] = 1.0
        return w
    return (F ** -0.5 * rng.standard_normal((M, F, 1))).astype(np.float32)


@pytest.mark.parametrize("basis_kind", ["learned", "side"])
@pytest.mark.parametrize("w_kind", ["random", "selector"])
@pytest.mark.parametrize("n_fft,hop,T", [(64, 1, 16000), (64, 1, 1000), (128, 2, 16000), (128, 2, 264), (128, 4, 1040)])
def test_spec_block_with_a_basis(ops, basis_kind, w_kind, n_fft, hop, T):
    """The fused stft_spec (the spectrum one tile, n_fft = M in {64, 128}, more than 64 frames, a multiple of 4; other shapes are refused
    by the op and run as stft_logmag + the add, covered above) against x + s W @ P with P in float64."""
    basis = make_basis(basis_kind, n_fft)
    rng = np.random.default_rng(n_fft + T)
    wav = clip(n_fft, hop, T, n_fft + T + 1)
    wav[0] *= 8.0
    C, F, Tf = n_fft, n_fft // 2 + 1, -(-T // hop)
    x = rng.standard_normal((2, C, Tf)).astype(np.float32)
    w = _w(w_kind, C, F, rng)
    s_out = 0.53
    mag, P = stft64(wav, basis, hop)
    ref = x + s_out * np.einsum("mf,bft->bmt", w[:, :, 0].astype(np.float64), P)
    got, names = kernels_run(lambda: ops.spec_block(cu(wav), w, cu(x), n_fft, hop, mean=MEAN, std=STD, out_scale=s_out, basis=basis))
    assert any(n.startswith("stft_spec<") for n in names), names
    tol = 2e-5 * max(1.0, float(np.abs(ref).max())) + 5e-3 * s_out * float(np.abs(w).sum(1).max()) * float((mag <= 1e-3).any())
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"MEASURE stft_spec {basis_kind} {w_kind} n_fft={n_fft} hop={hop} T={T}: {err:.2e} (bar {tol:.2e})")
    assert np.isfinite(got.cpu().numpy()).all() and err <= tol


# ---- spec16 (the f16 mode's whole SpecBlock) on all eight geometries: the five full-width ones, the locator's three half-channel ones
SPEC16 = [(64, 1, 16000, 64), (64, 1, 257, 64), (128, 2, 16000, 128), (128, 2, 255, 128), (256, 8, 16000, 256), (256, 8, 520, 256),
          (512, 40, 16000, 512), (512, 40, 2600, 512), (1024, 320, 16000, 1024), (1024, 320, 20481, 1024),
          (64, 1, 16000, 32), (64, 1, 257, 32), (128, 4, 16000, 64), (128, 4, 1021, 64), (256, 32, 16000, 128), (256, 32, 2081, 128)]


@pytest.mark.parametrize("basis_kind", ["learned", "side"])
@pytest.mark.parametrize("w_kind", ["random", "selector"])
@pytest.mark.parametrize("n_fft,hop,T,C", SPEC16)
def test_h16_spec_block_with_a_basis(ops, basis_kind, w_kind, n_fft, hop, T, C):
    from test_gpu_h16 import _spec_block_case
    (_, names) = kernels_run(lambda: _spec_block_case(ops, n_fft, hop, T, C, basis=make_basis(basis_kind, n_fft), w_kind=w_kind))
    assert f"spec16<{n_fft},hop{hop}" + (f",{C}ch>" if C != n_fft else ">") in names, names


# ---- whole nets with learned bases (waveverify_amd.init.learned_stft_bases in every `...spec.weight`) -----------------------------------
def _learned(kind, seed=0, **kw):
    from waveverify_amd.config import default_config
    from waveverify_amd.init import learned_stft_bases, random_state_dict
    cfg = default_config(kind, **kw)
    return cfg, {**random_state_dict(cfg, seed, parametrized=kind != "detector"), **learned_stft_bases(cfg, 0)}


@pytest.fixture(scope="module")
def learned_nets():
    from oracle import wv_oracle_torch as OT
    from waveverify_amd.nets import HipNet
    out = {}
    for k in ("generator", "detector", "locator"):
        cfg, sd = _learned(k)
        out[k] = (HipNet(cfg, sd), OT.Net(cfg, sd))
    return out


def _d(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape and np.isfinite(a).all(), (a.shape, b.shape)
    return float(np.abs(a.astype(np.float64) - b).max())


@pytest.mark.parametrize("T", [16000, 4800])
def test_exact_nets_with_learned_bases_vs_reference_golden(golden_dir, learned_nets, T):
    """The exact path against the reference run with the same learned bases (tests/golden/make_golden_learned_basis.py), with
    test_full_nets_vs_reference_golden's bars."""
    import os
    g = np.load(os.path.join(golden_dir, f"learned_basis_T{T}.npz"))
    x, msg = cu(g["x"]), cu(g["msg"])
    G, D, L = (learned_nets[k][0] for k in ("generator", "detector", "locator"))
    m = {"latent": _d(G.encoder(x, msg), g["latent"]), "delta": _d(G.generator(x, msg), g["delta"]),
         "wm": _d(G.generator(x, msg, add_input=True), g["wm"])}
    wm_ref = cu(g["wm"])
    m["det logits"] = _d(D.detector(wm_ref)[..., ::37], g["det_logits_sub"])
    mp = D.detector_mean_prob(wm_ref)
    m["mean prob"] = _d(mp, g["det_mean_prob"])
    m["loc logits"] = _d(L.locator(wm_ref)[..., ::7], g["loc_logits_sub"])
    print(f"MEASURE exact path, learned bases, T={T}: " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))
    assert m["latent"] <= 1e-4 and m["delta"] <= 2e-5 and m["wm"] <= 2e-5
    assert m["det logits"] <= 2e-4 and m["mean prob"] <= 1e-5 and m["loc logits"] <= 2e-4
    assert ((mp >= 0.5).int().cpu().numpy() == g["det_bits"]).all()


@pytest.mark.parametrize("T", [16000, 4800])
def test_f16_generator_with_learned_bases(golden_dir, learned_nets, T):
    """wm of the f16 mode within WM_BAR of the reference (same learned bases), of the mode's own oracle (wv_oracle_h16.embed, which reads
    the net's spec.weight) and of the exact path."""
    import os
    from oracle import wv_oracle_h16 as O16
    from test_gpu_h16 import WM_BAR
    g = np.load(os.path.join(golden_dir, f"learned_basis_T{T}.npz"))
    hip, net = learned_nets["generator"]
    x, msg = cu(g["x"]), cu(g["msg"])
    wm16, names = kernels_run(lambda: hip.generator(x, msg, add_input=True, precision="f16"))
    assert {f"spec16<{n},hop{h}>" for n, h in ((64, 1), (128, 2), (256, 8), (512, 40), (1024, 320))} <= names, names
    m = {"reference": _d(wm16, g["wm"]), "oracle": _d(wm16, O16.embed(net, g["x"], g["msg"])),
         "exact": _d(wm16, hip.generator(x, msg, add_input=True))}
    print(f"MEASURE f16 wm, learned bases, T={T}: " + ", ".join(f"vs {k} {v:.2e}" for k, v in m.items()))
    assert max(m.values()) <= WM_BAR, m


@pytest.mark.parametrize("B,T", [(2, 16000), (1, 12345), (3, 333)])
def test_f16_detector_and_locator_with_learned_bases(learned_nets, B, T):
    """Mean probabilities within det_mean_bar(T) of wv_oracle_h16.detect_mean_prob, logits within LOGIT_BAR of detect_logits."""
    from oracle import wv_oracle_h16 as O16
    from test_gpu_h16 import LOGIT_BAR, _vs_oracle, det_mean_bar
    from waveverify_amd.init import synthetic_clips
    x = synthetic_clips(B, T, seed=B + T + 1)[0]
    xt = cu(x)
    hip, net = learned_nets["detector"]
    _vs_oracle(f"learned bases: detector f16 mean B={B} T={T}", hip.detector_mean_prob(xt, precision="f16"), O16.detect_mean_prob(net, x), det_mean_bar(T))
    ref = O16.detect_logits(net, x).numpy()
    _vs_oracle(f"learned bases: detector f16 logits B={B} T={T}", hip.detector(xt, precision="f16"), ref, LOGIT_BAR, max(1.0, float(np.abs(ref).max())))
    hip, net = learned_nets["locator"]
    ref = O16.detect_logits(net, x).numpy()
    got, names = kernels_run(lambda: hip.locator(xt, precision="f16"))
    assert {"spec16<64,hop1,32ch>", "spec16<128,hop4,64ch>", "spec16<256,hop32,128ch>"} <= names, names
    _vs_oracle(f"learned bases: locator f16 logits B={B} T={T}", got, ref, LOGIT_BAR, max(1.0, float(np.abs(ref).max())))


def test_f16_fallback_scales_with_learned_bases():
    """Configuration 4 of test_gpu_h16's sweep (base width 96 at n_fft 64: no SpecBlock is a spec16 geometry) runs the f16 plan's fallback, the exact
    STFT kernel and the 1x1 on the f16 pipe, under learned bases: against the exact path and the mode's oracle."""
    from oracle import wv_oracle_h16 as O16
    from oracle import wv_oracle_torch as OT
    from test_gpu_h16 import LOGIT_BAR, WM_BAR, _other_configuration, _vs_oracle
    from waveverify_amd.init import synthetic_clips
    from waveverify_amd.nets import HipNet
    gkw, kw, T = _other_configuration(4)
    cg, sg = _learned("generator", 11, **gkw)
    cd, sd = _learned("detector", 11, **kw)
    G, D = HipNet(cg, sg), HipNet(cd, sd)
    x_np, msg_np = synthetic_clips(2, T, seed=8)
    x, msg = cu(x_np), cu(msg_np)
    wm16, names = kernels_run(lambda: G.generator(x, msg, add_input=True, precision="f16"))
    assert not any(n.startswith("spec16<") for n in names) and any(n.startswith("stft_logmag<") for n in names), names
    m = {"exact": _d(wm16, G.generator(x, msg, add_input=True)), "oracle": _d(wm16, O16.embed(OT.Net(cg, sg), x_np, msg_np))}
    print("MEASURE fallback f16 wm, learned bases: " + ", ".join(f"vs {k} {v:.2e}" for k, v in m.items()))
    assert max(m.values()) <= WM_BAR, m
    ref = O16.detect_logits(OT.Net(cd, sd), x_np).numpy()
    _vs_oracle("learned bases: fallback detector f16 logits", D.detector(x, precision="f16"), ref, LOGIT_BAR, max(1.0, float(np.abs(ref).max())))
