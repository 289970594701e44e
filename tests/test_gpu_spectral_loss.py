"""The multi-scale STFT and mel reconstruction losses on the GPU (waveverify_amd.spectral_loss, csrc/wv_specloss.hip): every scale's
term, both totals and the gradient towards wm against the reference's own loss classes (tests/golden/spectral_loss.npz,
make_golden_specloss.py); grad_scale / accumulation, determinism, batch means; the primitives against their written restatement; and
WatermarkTrainer(spectral_losses=True) against a float64 torch restatement of the five non-adversarial terms."""
import math
import os

import numpy as np
import pytest
import scipy.signal
import torch

from waveverify_amd import spectral_loss as SL

MEL_N, MEL_W, STFT_W = [5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048], [2048, 512]


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def slaney_filters(sr, n_fft, n_mels):
    """librosa.filters.mel defaults written out: Slaney mel scale (linear to 1 kHz at 200/3 Hz per mel, then log-spaced with step
    ln(6.4)/27), n_mels + 2 equally spaced mel points from 0 to sr/2, triangles over the bin frequencies k sr / n_fft, each scaled by
    2 / (upper edge - lower edge) in Hz; float32."""
    step = math.log(6.4) / 27.0
    hz2mel = lambda f: 15.0 + math.log(f / 1000.0) / step if f >= 1000.0 else 3.0 * f / 200.0      # noqa: E731
    mel2hz = lambda m: 1000.0 * math.exp(step * (m - 15.0)) if m >= 15.0 else 200.0 * m / 3.0      # noqa: E731
    top = hz2mel(sr / 2.0)
    edges = [mel2hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)]
    W = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        lo, mid, hi = edges[m], edges[m + 1], edges[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * sr / n_fft
            W[m, k] = max(0.0, min((f - lo) / (mid - lo), (hi - f) / (hi - mid))) * 2.0 / (hi - lo)
    return W


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
def spectral_restatement(wm, x, sr=16000):
    """float64 torch: the STFT and mel losses of the module docstring (torch.stft centred, reflect padding, periodic Hann; Slaney
    filters as written above)."""
    T = wm.shape[-1]

    def mag(s, w):
        win = torch.from_numpy(scipy.signal.get_window("hann", w))
        return torch.stft(s.reshape(-1, T), n_fft=w, hop_length=w // 4, window=win, center=True, pad_mode="reflect", return_complex=True).abs()

    def l1log(a, b, p):
        return (torch.log10(a.clamp(1e-5) ** p) - torch.log10(b.clamp(1e-5) ** p)).abs().mean()
    stft = sum(l1log(mag(wm, w), mag(x, w), 2.0) + (mag(wm, w) - mag(x, w)).abs().mean() for w in STFT_W)
    mel = 0.0
    for n, w in zip(MEL_N, MEL_W):
        fb = torch.from_numpy(slaney_filters(sr, w, n).astype(np.float32).astype(np.float64))
        mel = mel + l1log(fb @ mag(wm, w), fb @ mag(x, w), 1.0)
    return stft, mel


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
