"""The multi-scale STFT and mel reconstruction losses on the GPU (waveverify_amd.spectral_loss, csrc/wv_specloss.hip): every scale's
term, both totals and the gradient towards wm against the reference's own loss classes (tests/golden/spectral_loss.npz,
make_golden_specloss.py); grad_scale / accumulation, determinism, batch means; the primitives against their written restatement;
WatermarkTrainer(spectral_losses=True) against a float64 torch restatement of the five non-adversarial terms; and, against the float64
oracle (oracle/wv_oracle_specloss.py, pinned to the fixture by test_oracle_specloss.py) on the cases of tests/specloss_cases.py: every
scale's and every part's own gradient at B = 3, exact and analytic properties, geometry corners, one plan of three kinds of scale, the
C ABI's refusals and a side stream."""
import math
import os

import numpy as np
import pytest
import scipy.signal
import torch

import specloss_cases as SC
from oracle import wv_oracle_specloss as OS
from oracle.wv_oracle_specloss import slaney_filters, spectral_restatement   # noqa: F401  (the trainer test's restatement lives there)
from waveverify_amd import spectral_loss as SL

MEL_N, MEL_W, STFT_W = [5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048], [2048, 512]


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_window_and_mel_filters_equal_the_restatement():
    for w in MEL_W:
        assert np.abs(SL.hann_window(w) - scipy.signal.get_window("hann", w)).max() <= 1e-15
        assert scipy.signal.get_window("hann", w)[0] == 0.0 and abs(scipy.signal.get_window("hann", w)[w // 2] - 1.0) < 1e-15   # periodic
    for n, w in zip(MEL_N, MEL_W):
        got, ref = SL.mel_filters(16000, w, n), slaney_filters(16000, w, n)
        assert got.dtype == np.float32 and got.shape == (n, w // 2 + 1)
        assert np.abs(got - ref).max() <= 2e-7 * np.abs(ref).max(), (n, w)
        assert (got.max(axis=1) > 0).all()


def test_clip_too_short_for_reflect_padding_raises():
    for f, w in ((SL.MultiScaleSTFTLoss(), 2048), (SL.MelSpectrogramLoss(n_mels=[5], window_lengths=[64]), 64)):
        a = torch.zeros(1, 1, w // 2)
        with pytest.raises(ValueError):
            f(a, a)


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "spectral_loss.npz"))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [16000, 4800, 1100])
def test_terms_totals_and_gradient_vs_reference(golden_dir, T):
    g = _golden(golden_dir)
    wm, x = _cu(g[f"wm_{T}"]), _cu(g[f"x_{T}"])
    stft, mel = SL.MultiScaleSTFTLoss(), SL.MelSpectrogramLoss()
    for name, f in (("stft", stft), ("mel", mel)):
        loss, d = f(wm, x)
        terms = f.last_terms.cpu().numpy().astype(np.float64)
        ref_terms = g[f"{name}_terms_{T}"]
        assert np.all(np.abs(terms - ref_terms) <= 1e-5 * np.abs(ref_terms)), (name, terms, ref_terms)
        ref = float(g[f"{name}_total_{T}"])
        assert abs(float(loss.item()) - ref) <= 1e-5 * ref, (name, float(loss.item()), ref)
        dref = g[f"d_{name}_{T}"]
        e = float(np.abs(d.cpu().numpy() - dref).max())
        # 2e-3, not 2e-4: the gradient of a log term scales with 1 / |X|, and the smallest live |X| (the clamp is 1e-5) carry the
        # f32 transform's absolute error as a large relative one
        assert e <= 2e-3 * float(np.abs(dref).max()), (name, e, float(np.abs(dref).max()))
    # both through one plan (the 2048 and 512 spectra shared): the same terms and the sum of the two gradients
    both = SL.SpectralLosses(stft, mel)
    ls, lm, d = both(wm, x, stft_grad_scale=10.0, mel_grad_scale=20.0)
    assert abs(float(ls.item()) - float(g[f"stft_total_{T}"])) <= 1e-5 * float(g[f"stft_total_{T}"])
    assert abs(float(lm.item()) - float(g[f"mel_total_{T}"])) <= 1e-5 * float(g[f"mel_total_{T}"])
    dref = 10.0 * g[f"d_stft_{T}"].astype(np.float64) + 20.0 * g[f"d_mel_{T}"]
    assert float(np.abs(d.cpu().numpy() - dref).max()) <= 2e-3 * float(np.abs(dref).max())


@pytest.mark.gpu
def test_grad_scale_accumulation_and_determinism():
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal((4, 1, 9000))).astype(np.float32)
    wm = x + (0.02 * rng.standard_normal(x.shape)).astype(np.float32)
    wm_t, x_t = _cu(wm), _cu(x)
    f = SL.SpectralLosses()
    ls, lm, d1 = f(wm_t, x_t, stft_grad_scale=1.0, mel_grad_scale=0.0)
    ls2, lm2, none = f(wm_t, x_t, want_grad=False)
    assert none is None and torch.equal(ls, ls2) and torch.equal(lm, lm2)
    _, _, d2 = f(wm_t, x_t, stft_grad_scale=0.0, mel_grad_scale=1.0)
    _, _, d = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0)
    scale = float(d.abs().max())
    assert float((d - (10.0 * d1 + 20.0 * d2)).abs().max()) <= 1e-5 * scale
    base = torch.from_numpy(rng.standard_normal(x.shape).astype(np.float32)).cuda()
    acc = base.clone()
    r_ls, r_lm, r = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0, out=acc)
    assert r is acc and torch.equal(r_ls, ls) and torch.equal(r_lm, lm)
    assert float((acc - base - d).abs().max()) <= 1e-6 * max(scale, float(base.abs().max()))
    # the single-loss objects: grad_scale multiplies the gradient, the loss stays
    s = SL.MultiScaleSTFTLoss()
    l1, g1 = s(wm_t, x_t)
    l3, g3 = s(wm_t, x_t, grad_scale=3.0)
    assert torch.equal(l1, l3) and float((g3 - 3.0 * g1).abs().max()) <= 1e-5 * float(g3.abs().max())
    # two identical calls: bit for bit
    a = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0)
    b = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and torch.equal(f.last_terms["mel"], f.last_terms["mel"])


@pytest.mark.gpu
def test_batch_of_64_is_the_mean_of_its_halves():
    rng = np.random.default_rng(6)
    x = (0.1 * rng.standard_normal((64, 1, 16000))).astype(np.float32)
    wm = x + (0.03 * rng.standard_normal(x.shape)).astype(np.float32)
    f = SL.SpectralLosses()
    full = f(_cu(wm), _cu(x), stft_grad_scale=1.0, mel_grad_scale=1.0)
    h0 = f(_cu(wm[:32]), _cu(x[:32]), stft_grad_scale=1.0, mel_grad_scale=1.0)
    h1 = f(_cu(wm[32:]), _cu(x[32:]), stft_grad_scale=1.0, mel_grad_scale=1.0)
    for i in range(2):
        want = 0.5 * (float(h0[i].item()) + float(h1[i].item()))
        assert abs(float(full[i].item()) - want) <= 1e-5 * want
    halves = 0.5 * torch.cat([h0[2], h1[2]])
    assert float((full[2] - halves).abs().max()) <= 1e-5 * float(halves.abs().max())


# ----------------------------------------------------------------------------------------------------------- trainer (GPU)
def check_grads(tr, ref_grads, tol, loose=None):
    scalar_scale = max([float(np.abs(r).max()) for r in ref_grads.values() if r.size <= 4] + [1e-30])
    worst = ("", 0.0)
    for k, r in ref_grads.items():
        got = tr.gviews[k].detach().cpu().numpy().astype(np.float64)
        scale = max(float(np.abs(r).max()), scalar_scale if r.size <= 4 else 0.0, 1e-30)
        e = float(np.abs(got - r.reshape(got.shape)).max() / scale)
        if loose and any(t in k for t in loose[0]):
            assert e <= loose[1], (k, e)
        elif e > worst[1]:
            worst = (k, e)
    assert worst[1] <= tol, worst


def _step_reference(cfgs, sds, x, msg, plan, seg_len, seq, lambdas):
    """The five non-adversarial terms of the reference's generator objective in float64 torch: G, the augmentation as a differentiable
    select with the trainer's plan, D and L (oracle/wv_oracle_train_torch.py's pieces), waveform L1, and the spectral restatement."""
    import torch.nn.functional as F
    from oracle import wv_oracle_train_torch as OTT
    G, D, L = (OTT.LiveNet(c, s) for c, s in zip(cfgs, sds))
    xt, mt = torch.tensor(x, dtype=torch.float64), torch.tensor(msg, dtype=torch.float64)
    B, _, T = xt.shape
    wm = OTT.OTc.decoder_forward(G, OTT.OTc.encoder_forward(G, xt, mt))[..., :T] + xt
    mode, a, b, c, perm, t_out = seq
    t = np.arange(t_out)
    src = {1: lambda: T - 1 - t, 2: lambda: (t - a) % T, 3: lambda: np.asarray(perm)[t // a] * a + t % a,
           4: lambda: np.where((t >= a) & (t < a + c), b + (t - a), np.where((t >= b) & (t < b + c), a + (t - b), t))}.get(mode, lambda: t)()
    src_t = torch.from_numpy(src.astype(np.int64))
    code = torch.from_numpy(np.asarray(plan)[:, src // seg_len].astype(np.int64))[:, None, :]
    x_other = torch.stack([xt[torch.clamp(code - 3, min=0)[i, 0], 0, src_t] for i in range(B)])[:, None, :]
    wm_s, x_s = wm[:, :, src_t], xt[:, :, src_t]
    wm_aug = torch.where(code == 0, wm_s, torch.where(code == 1, x_s, torch.where(code == 2, torch.zeros_like(x_s), x_other)))
    mask = (code == 0).to(torch.float64)
    dec = F.binary_cross_entropy_with_logits(OTT.logits_of(D, wm_aug), mt.unsqueeze(2) * mask)
    loc = F.binary_cross_entropy_with_logits(OTT.logits_of(L, wm_aug), mask)
    wav = (wm - xt).abs().mean()
    stft, mel = spectral_restatement(wm, xt)
    terms = {"dec/loss": dec, "loc/loss": loc, "waveform/loss": wav, "stft/loss": stft, "mel/loss": mel}
    loss = sum(lambdas[k] * v for k, v in terms.items())
    loss.backward()
    grads = [{k: p.grad.numpy() for k, p in n.leaf.items() if p.grad is not None} for n in (G, D, L)]
    return dict({k: float(v.detach()) for k, v in terms.items()}, loss=float(loss.detach())), grads


@pytest.mark.gpu
def test_watermark_step_with_spectral_losses_vs_restatement():
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import WatermarkTrainer
    # the configuration of test_watermark_step_vs_oracle (half-width generator / detector, default locator): at the default widths one
    # weight-norm magnitude of the generator lands at 2.5e-2 of the 2e-2 bar
    cfgs = [default_config("generator", channels_enc=32, channels_dec=48), default_config("detector", channels_enc=32), default_config("locator")]
    sds = [random_state_dict(c, 0, parametrized=True) for c in cfgs]
    rng = np.random.default_rng(8)
    x = (0.1 * rng.standard_normal((2, 1, 8000))).astype(np.float32)
    msg = rng.integers(0, 2, (2, 16)).astype(np.float32)
    tr = WatermarkTrainer(cfgs[0], sds[0], cfgs[1], sds[1], cfgs[2], sds[2], lr=1e-4, spectral_losses=True)
    assert tr.lambdas["stft/loss"] == 10.0 and tr.lambdas["mel/loss"] == 20.0
    np.random.seed(4); torch.manual_seed(4)
    out = tr.step(_cu(x), _cu(msg))
    plan, seg_len, sm, _ = tr.aug.last
    ref, (gG, gD, gL) = _step_reference(cfgs, sds, x, msg, plan, seg_len, (sm.mode, sm.a, sm.b, sm.c, sm.perm, sm.t_out), tr.lambdas)
    for k in ("dec/loss", "loc/loss", "waveform/loss", "stft/loss", "mel/loss", "loss"):
        assert abs(float(out[k].item()) - ref[k]) <= 5e-5 * abs(ref[k]), (k, float(out[k].item()), ref[k])
    check_grads(tr.D, gD, tol=1e-3)
    check_grads(tr.L, gL, tol=1e-3)
    check_grads(tr.G, gG, tol=2e-2, loose=(("film_layers", "msg_embedding"), 2e-1))
    norm_ref = math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in gG.values()))
    assert abs(float(out["grad_norm"].item()) - norm_ref) <= 2e-2 * norm_ref, (float(out["grad_norm"].item()), norm_ref)
    for net, sd in zip((tr.G, tr.D, tr.L), sds):
        for k in list(net.params)[:20]:
            d = float((net.params[k].cpu() - torch.from_numpy(np.asarray(sd[k], np.float32))).abs().max())
            assert 0.0 < d <= 1.2e-4 + 1e-6 * float(np.abs(sd[k]).max()), (k, d)


@pytest.mark.gpu
def test_watermark_step_without_spectral_losses_is_unchanged():
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import WatermarkTrainer
    cfgs = [default_config(k) for k in ("generator", "detector", "locator")]
    sds = [random_state_dict(c, 0, parametrized=True) for c in cfgs]
    rng = np.random.default_rng(9)
    x = (0.1 * rng.standard_normal((2, 1, 8000))).astype(np.float32)
    msg = rng.integers(0, 2, (2, 16)).astype(np.float32)
    runs = []
    for kw in ({}, {"spectral_losses": False}):
        tr = WatermarkTrainer(cfgs[0], sds[0], cfgs[1], sds[1], cfgs[2], sds[2], lr=1e-4, **kw)
        np.random.seed(1); torch.manual_seed(1)
        out = tr.step(_cu(x), _cu(msg))
        runs.append((tr, out))
    (a, oa), (b, ob) = runs
    assert a.lambdas == b.lambdas == WatermarkTrainer.LAMBDAS and "stft/loss" not in ob and "mel/loss" not in ob
    assert sorted(oa) == sorted(ob)
    for k in ("loss", "dec/loss", "loc/loss", "waveform/loss", "grad_norm"):
        assert torch.equal(oa[k], ob[k]), k
    for n, m in ((a.G, b.G), (a.D, b.D), (a.L, b.L)):
        assert torch.equal(n.arena, m.arena) and torch.equal(n.grads, m.grads)


# ------------------------------------------------------------------------------- per-scale, per-part gradients vs the oracle (GPU)
def _loss_of(scale):
    """The public loss object of one single-term scale dict."""
    if scale["stft"]:
        lw, mw, p, eps = scale["stft"]
        return SL.MultiScaleSTFTLoss(window_lengths=[scale["w"]], clamp_eps=eps, mag_weight=mw, log_weight=lw, pow=p)
    lw, mw, p, eps = scale["mel"]
    return SL.MelSpectrogramLoss(n_mels=[scale["n_mels"]], window_lengths=[scale["w"]], sample_rate=scale["sr"], clamp_eps=eps, mag_weight=mw,
                                 log_weight=lw, pow=p, mel_fmin=[scale["fmin"]], mel_fmax=[scale["fmax"]])


def _both_losses(w, n, mel_term):
    """SpectralLosses holding one scale: the magnitude-only STFT term and one mel term on the same window."""
    lw, mw, p, eps = mel_term
    return SL.SpectralLosses(SL.MultiScaleSTFTLoss(window_lengths=[w], log_weight=0.0, mag_weight=1.0),
                             SL.MelSpectrogramLoss(n_mels=[n], window_lengths=[w], sample_rate=SC.SR, clamp_eps=eps, mag_weight=mw, log_weight=lw, pow=p))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _term_close(got, ref, what):
    assert math.isfinite(got) and abs(got - ref) <= SC.TERM_BAR * abs(ref), (what, got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SC.PART_CASES, ids=SC.PART_IDS)
def test_each_part_of_each_scale_vs_oracle(case):
    """One term of one scale at B = 3: its value at 1e-5 and its own gradient at 1e-4 of max against the float64 oracle (2e-3 for the
    STFT log part at the reference's clamp of 1e-5).  The floor printed next to it is the float32 oracle's error."""
    cid, part, scale, T, seed, bar = case
    wm, x = SC.clips(SC.PART_B, T, seed)
    r64 = OS.spectral_oracle(wm, x, [scale])["scales"][0]
    r32 = OS.spectral_oracle(wm, x, [scale], dtype=torch.float32)["scales"][0]
    f = _loss_of(scale)
    loss, d = f(_cu(wm), _cu(x))
    e, floor = SC.rel_err(_np(d), r64["d_" + part]), SC.rel_err(r32["d_" + part], r64["d_" + part])
    print(f"RECORD specloss {cid}: floor {floor:.2e} gpu {e:.2e} of max |grad| {np.abs(r64['d_' + part]).max():.3e}; "
          f"term gpu {float(loss.item()):.8e} oracle {r64[part]:.8e}")
    _term_close(float(loss.item()), r64[part], cid)
    _term_close(float(f.last_terms[0].item()), r64[part], cid)
    assert np.isfinite(_np(d)).all() and e <= bar, (cid, e, floor)


# ----------------------------------------------------------------------------------------- exact and analytic properties (GPU)
@pytest.mark.gpu
def test_identical_signals_give_exactly_zero():
    """wm and x with the same contents in two allocations: both go through the same GEMM on the same basis, so every |X| pair is
    bit-identical, every difference and every sign() is 0: both losses and the whole gradient are exactly 0."""
    x = (0.1 * np.random.default_rng(12).standard_normal((3, 1, 4801))).astype(np.float32)
    a, b = _cu(x), _cu(x.copy())
    assert a.data_ptr() != b.data_ptr()
    f = SL.SpectralLosses()
    ls, lm, d = f(a, b, stft_grad_scale=10.0, mel_grad_scale=20.0)
    assert float(ls.item()) == 0.0 and float(lm.item()) == 0.0
    assert not f.last_terms["stft"].any() and not f.last_terms["mel"].any()
    assert int((d != 0).sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("w,gain,seed", SC.GAIN_CASES)
def test_gain_of_a_power_of_two(w, gain, seed):
    """wm = 2 x or x / 2, exact in float32 and through the GEMM: every live bin has |log difference| = pow * log10(2), no kinks."""
    wm, x = SC.gain_clips(gain, seed)
    n = SC.MEL_N[SC.MEL_W.index(w)]
    for what, scale, with_grad in (("mag", SC.stft_scale(w, SC.STFT_MAG), True), ("log raised", SC.stft_scale(w, SC.stft_log(w)), True),
                                   ("log ref", SC.stft_scale(w, SC.STFT_LOG_REF), False), ("mel", SC.mel_scale(w, n), False)):
        part = "stft" if scale["stft"] else "mel"
        r = OS.spectral_oracle(wm, x, [scale])["scales"][0]
        loss, d = _loss_of(scale)(_cu(wm), _cu(x))
        _term_close(float(loss.item()), r[part], (what, w, gain))
        e = SC.rel_err(_np(d), r["d_" + part])
        print(f"RECORD specloss gain {gain} w {w} {what}: gpu {e:.2e} of max")
        assert np.isfinite(_np(d)).all()
        if with_grad:
            assert e <= SC.GRAD_BAR, (what, w, gain, e)
    # the analytic values: the mel term of a pure gain is log10(2) wherever no band clamps; the magnitude term is |gain - 1| mean|X_x|
    lm, _ = _loss_of(SC.mel_scale(w, n))(_cu(wm), _cu(x), want_grad=False)
    r = OS.spectral_oracle(wm, x, [SC.mel_scale(w, n)], want_bins=True)["scales"][0]
    fb = OS.slaney_filters_f32(SC.SR, w, n).astype(np.float64)
    if (np.einsum("mf,bft->bmt", fb, np.minimum(r["mag_wm"], r["mag_x"])) >= 1e-5).all():
        assert abs(float(lm.item()) - math.log10(2.0)) <= SC.TERM_BAR * math.log10(2.0)


@pytest.mark.gpu
def test_clips_of_a_batch_are_independent():
    """Five clips of different content in one call, one of them silent: rows 0, 2 and 4 of the gradient are 1/5 of the gradient of a
    B = 1 call on that clip alone (1e-6 of max: the 1 / (B F Tf) factor rounds differently and a short call may take another GEMM
    tile), and every B = 1 loss enters the B = 5 loss with weight 1/5."""
    m = SC.BATCH
    wm, x = SC.batch_clips()
    f = SL.SpectralLosses(SL.MultiScaleSTFTLoss(window_lengths=m["stft_windows"], log_weight=0.0, mag_weight=1.0),
                          SL.MelSpectrogramLoss(n_mels=m["n_mels"], window_lengths=m["mel_windows"]))
    assert [(s["w"], bool(s["stft"]), bool(s["mel"])) for s in f.scales] == [(s["w"], bool(s["stft"]), bool(s["mel"])) for s in SC.batch_scales()]
    ls, lm, d = f(_cu(wm), _cu(x), stft_grad_scale=10.0, mel_grad_scale=20.0)
    assert torch.isfinite(d).all() and math.isfinite(float(ls.item())) and math.isfinite(float(lm.item()))
    assert int((d[m["silent"]] != 0).sum()) == 0                  # |X| = 0: no direction, no gradient
    singles = [f(_cu(wm[b: b + 1]), _cu(x[b: b + 1]), stft_grad_scale=10.0, mel_grad_scale=20.0) for b in range(m["B"])]
    for i, total in enumerate((ls, lm)):
        want = sum(float(s[i].item()) for s in singles) / m["B"]
        assert abs(float(total.item()) - want) <= SC.TERM_BAR * want, (i, float(total.item()), want)
    ref = OS.spectral_oracle(wm, x, SC.batch_scales(), stft_grad_scale=10.0, mel_grad_scale=20.0)
    assert SC.rel_err(_np(d), ref["d_total"]) <= SC.GRAD_BAR
    for b in (0, 2, 4):
        one = _np(singles[b][2])[0] / m["B"]
        e = float(np.abs(_np(d)[b] - one).max() / np.abs(one).max())
        print(f"RECORD specloss batch clip {b}: row vs B=1 call {e:.2e} of max")
        assert e <= 1e-6, (b, e)


# ----------------------------------------------------------------------------------------------------- geometry corners (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("case", SC.GEOMETRY_CASES, ids=SC.GEOMETRY_IDS)
def test_geometry_corners_vs_oracle(case):
    """Windows that are no multiple of the GEMM's K step, the shortest legal clips, T < w, T around a hop multiple, padding columns,
    a 256-column workgroup edge: a magnitude-only STFT term and one mel term on one scale, each term at 1e-5 and each term's own
    gradient at 1e-4 of max."""
    cid, w, n, mel_term, B, T, seed = case
    wm, x = SC.clips(B, T, seed)
    r = OS.spectral_oracle(wm, x, [SC.geometry_scale(w, n, mel_term)])["scales"][0]
    f = _both_losses(w, n, mel_term)
    assert len(f.scales) == 1
    wm_t, x_t = _cu(wm), _cu(x)
    for part, scales in (("stft", (1.0, 0.0)), ("mel", (0.0, 1.0))):
        ls, lm, d = f(wm_t, x_t, stft_grad_scale=scales[0], mel_grad_scale=scales[1])
        _term_close(float(ls.item()), r["stft"], (cid, "stft"))
        _term_close(float(lm.item()), r["mel"], (cid, "mel"))
        e = SC.rel_err(_np(d), r["d_" + part])
        print(f"RECORD specloss corner {cid} {part}: gpu {e:.2e} of max |grad| {np.abs(r['d_' + part]).max():.3e}")
        assert np.isfinite(_np(d)).all() and e <= SC.GRAD_BAR, (cid, part, e)
    if (w, n) == SC.ONE_EMPTY_BAND:
        # band 0 holds no bin: it adds |log10(eps) - log10(eps)| = 0 to the sum, stays in the count, and has no gradient.
        # test_oracle_specloss.py shows exactly that of the oracle's term and gradient, which the mel term and the mel-only gradient
        # above have just met; here, that the filters the plan was given have the same empty row
        assert OS.empty_bands(SC.SR, w, n) == [0]
        got = SL.mel_filters(SC.SR, w, n)
        assert not got[0].any() and got[1:].any(axis=1).all()


# --------------------------------------------------------------------------------------- one plan of three kinds of scale (GPU)
@pytest.mark.gpu
def test_mixed_plan_with_and_without_gradient():
    """A mel-only, a shared and an STFT-only scale in one plan: the same terms bitwise with want_grad=True, want_grad=False and out=,
    every term against the oracle, and out - base equal to the fresh gradient."""
    m = SC.MIXED
    wm, x = SC.clips(m["B"], m["T"], m["seed"])
    f = SL.SpectralLosses(SL.MultiScaleSTFTLoss(window_lengths=m["stft_windows"], log_weight=0.0, mag_weight=1.0),
                          SL.MelSpectrogramLoss(n_mels=m["n_mels"], window_lengths=m["mel_windows"]))
    scales = SC.mixed_scales()
    assert [(s["w"], bool(s["stft"]), bool(s["mel"])) for s in f.scales] == [(s["w"], bool(s["stft"]), bool(s["mel"])) for s in scales]
    ref = OS.spectral_oracle(wm, x, scales, stft_grad_scale=10.0, mel_grad_scale=20.0)
    wm_t, x_t = _cu(wm), _cu(x)
    ls, lm, d = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0)
    t_stft, t_mel = f.last_terms["stft"].clone(), f.last_terms["mel"].clone()
    ls0, lm0, none = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0, want_grad=False)
    assert none is None and torch.equal(ls, ls0) and torch.equal(lm, lm0)
    assert torch.equal(t_stft, f.last_terms["stft"]) and torch.equal(t_mel, f.last_terms["mel"])
    base = torch.from_numpy(np.random.default_rng(1).standard_normal(wm.shape).astype(np.float32)).cuda()
    acc = base.clone()
    ls1, lm1, r = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0, out=acc)
    assert r is acc and torch.equal(ls, ls1) and torch.equal(lm, lm1)
    assert torch.equal(t_stft, f.last_terms["stft"]) and torch.equal(t_mel, f.last_terms["mel"])
    assert float((acc - base - d).abs().max()) <= 1e-6 * max(float(d.abs().max()), float(base.abs().max()))
    _term_close(float(ls.item()), ref["stft_total"], "stft total")
    _term_close(float(lm.item()), ref["mel_total"], "mel total")
    for got, s in zip(t_mel.tolist(), scales[:2]):
        _term_close(got, ref["scales"][scales.index(s)]["mel"], ("mel", s["w"]))
    for got, w in zip(t_stft.tolist(), m["stft_windows"]):
        _term_close(got, next(q for q in ref["scales"] if q["w"] == w)["stft"], ("stft", w))
    assert SC.rel_err(_np(d), ref["d_total"]) <= SC.GRAD_BAR


# ------------------------------------------------------------------------------------------------- the C ABI's refusals (GPU)
@pytest.mark.gpu
def test_c_abi_refuses_bad_calls_and_writes_nothing():
    """T == w / 2, a workspace one byte short, B = 65536 and a null `terms`: an error code before anything is launched, with terms,
    totals and dwm still holding the guard pattern."""
    from guard import Guards
    from waveverify_amd import _lib
    WV_EINVAL, WV_ENOMEM = -1, -5
    plan = SL._Plan(SC.refusal_scales())
    B, T, Ts = SC.REFUSAL["B"], SC.REFUSAL["T"], SC.REFUSAL["T_short"]
    wm, x, wm_s, x_s = SC.refusal_clips()
    g = Guards()
    wm_g, x_g = g.input(wm, "wm"), g.input(x, "x")
    terms, totals, dwm = g.output((2, 2), name="terms"), g.output((2,), name="totals"), g.output((B, 1, T), name="dwm")
    need = int(_lib.load().wv_specloss_workspace_bytes(plan._h, B, T))
    assert need > 0 and int(_lib.load().wv_specloss_workspace_bytes(plan._h, 0, T)) == 0
    ws = g.workspace(need, "workspace")

    def untouched():
        torch.cuda.synchronize()
        for a in (terms, totals, dwm):
            a.check(expect_unwritten=torch.ones(a.t.shape, dtype=torch.bool))
        wm_g.check(), x_g.check(), ws.check()
        assert int((ws.t != 0xFF).sum()) == 0

    assert SC.c_call(plan, wm_g.t, x_g.t, terms.t, totals.t, dwm.t, ws.t, ws_bytes=need - 1) == WV_ENOMEM
    untouched()
    assert SC.c_call(plan, wm_g.t, x_g.t, terms.t, totals.t, dwm.t, None, ws_bytes=need) == WV_ENOMEM
    untouched()
    assert SC.c_call(plan, wm_g.t, x_g.t, terms.t, totals.t, dwm.t, ws.t, T=32) == WV_EINVAL       # T == w / 2 of the 64 window
    assert SC.c_call(plan, wm_g.t, x_g.t, terms.t, totals.t, dwm.t, ws.t, T=16) == WV_EINVAL
    assert SC.c_call(plan, wm_g.t, x_g.t, terms.t, totals.t, dwm.t, ws.t, B=65536) == WV_EINVAL
    assert SC.c_call(plan, wm_g.t, x_g.t, None, totals.t, dwm.t, ws.t) == WV_EINVAL
    assert SC.c_call(plan, wm_g.t, x_g.t, terms.t, None, dwm.t, ws.t) == WV_EINVAL
    assert SC.c_call(plan, None, x_g.t, terms.t, totals.t, dwm.t, ws.t, B=B, T=T) == WV_EINVAL
    untouched()
    # and the same buffers serve a good call: T = w / 2 + 1 of the larger window
    dwm.t.zero_()
    assert Ts == 64 // 2 + 1 and SC.c_call(plan, wm_g.t, x_g.t, terms.t, totals.t, dwm.t, ws.t, B=B, T=Ts) == 0
    g.check()
    r = OS.spectral_oracle(wm_s, x_s, plan.scales)
    _term_close(float(totals.t[0].item()), r["stft_total"], "stft total at the shortest T")
    _term_close(float(totals.t[1].item()), r["mel_total"], "mel total at the shortest T")
    got = _np(dwm.t).reshape(-1)
    assert SC.rel_err(got[: B * Ts], (r["d_stft"] + r["d_mel"]).reshape(-1)) <= SC.GRAD_BAR
    assert not got[B * Ts:].any()                                 # a [B, 1, Ts] call writes B * Ts floats of dwm


# ---------------------------------------------------------------------------------------------------------- side stream (GPU)
@pytest.mark.gpu
def test_side_stream_equals_default_stream():
    wm, x = SC.clips(3, 4800, 41)
    wm_t, x_t = _cu(wm), _cu(x)
    f = SL.SpectralLosses()
    a = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0)
        t_side = {k: v.clone() for k, v in f.last_terms.items()}
    side.synchronize()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    c = f(wm_t, x_t, stft_grad_scale=10.0, mel_grad_scale=20.0)
    assert all(torch.equal(t_side[k], f.last_terms[k]) for k in t_side) and all(torch.equal(p, q) for p, q in zip(a, c))
