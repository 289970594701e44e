"""WatermarkTrainer.validate on the GPU (small nets, 1600-sample clips): its keys, that it leaves the trainer, the scheduler and the
random streams as it found them, that its numbers are the existing pieces composed (the units' forwards, bce_logits, l1_loss, the
spectral losses, the BER / MIOU classes on host copies), the shipped seven-effect list, and the refusal of an effect the GPU path lacks."""
import random

import numpy as np
import pytest
import torch

from waveverify_amd import effects as E
from waveverify_amd.config import default_config
from waveverify_amd.init import random_state_dict

pytestmark = pytest.mark.gpu

B, T = 3, 1600
LOSS_KEYS = ("dec/loss", "loc/loss", "waveform/loss", "stft/loss", "mel/loss")


def _trainer(**kw):
    from waveverify_amd.train import WatermarkTrainer
    small = dict(channels_enc=8, dimension=16, strides=[2, 2], n_fft_base=16)
    cg = default_config("generator", channels_dec=8, n_residual_dec=1, **small)
    cd, cl = default_config("detector", output_dim=8, **small), default_config("locator", output_dim=8, **small)
    return WatermarkTrainer(cg, random_state_dict(cg, 1, parametrized=True), cd, random_state_dict(cd, 1, parametrized=True), cl,
                            random_state_dict(cl, 1, parametrized=True), **kw)


def _batch(seed=0):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy((0.1 * rng.standard_normal((B, 1, T))).astype(np.float32)).cuda()
    msg = torch.from_numpy(rng.integers(0, 2, (B, 16)).astype(np.float32)).cuda()
    return x, msg


def _seed(s):
    np.random.seed(s); random.seed(s); torch.manual_seed(s)


def test_validate_exists_and_returns_the_listed_keys():
    tr = _trainer(spectral_losses=True)
    x, msg = _batch()
    out = tr.validate(x, msg)
    names = [n for n, _ in E.EVAL_EFFECTS]
    want = set(LOSS_KEYS) | {"loss", "SISNR", "per_clip"} | {f"{n}/ber" for n in names} | {f"{n}/miou" for n in names}
    assert set(out) == want and "STOI" not in out and "PESQ" not in out
    for k in LOSS_KEYS + ("loss",):
        assert out[k].is_cuda and tuple(out[k].shape) == (1,) and np.isfinite(float(out[k]))
    lam = tr.lambdas
    total = lam["dec/loss"] * out["dec/loss"] + lam["loc/loss"] * out["loc/loss"] + lam["waveform/loss"] * out["waveform/loss"]
    assert torch.equal(out["loss"], total + lam["stft/loss"] * out["stft/loss"] + lam["mel/loss"] * out["mel/loss"])
    pc = out["per_clip"]
    assert pc["effects"] == names and pc["sisnr"].shape == (B,) and out["SISNR"] == float(pc["sisnr"].mean())
    for k in ("errors", "valid", "ber", "miou"):
        assert pc[k].shape == (len(names), B), k
    for i, n in enumerate(names):
        assert 0.0 <= out[f"{n}/ber"] <= 1.0 and 0.0 <= out[f"{n}/miou"] <= 1.0
        assert out[f"{n}/ber"] == pc["errors"][i].sum() / max(pc["valid"][i].sum(), 1)
    plain = _trainer().validate(x, msg, eval_effects=[("identity", {})])
    assert "stft/loss" not in plain and "mel/loss" not in plain and set(plain) == {"dec/loss", "loc/loss", "waveform/loss", "loss", "SISNR",
                                                                                    "per_clip", "identity/ber", "identity/miou"}


def test_validate_between_two_steps_changes_nothing():
    """step(); step() against step(); validate(); step(): bit-equal losses, parameter arenas, AdamW moments and step counts, with an
    attached EffectScheduler whose state validate neither reads nor writes, and the global random streams where they were."""
    from waveverify_amd.effect_scheduler import EffectScheduler
    grid = {"identity": {}, "lowpass_filter": {"cutoff_freq": {"choices": [3000, 2000]}}, "random_noise": {"noise_std": {"choices": [0.001, 0.002]}}}
    x, msg = _batch(1)

    def run(with_validate):
        sched = EffectScheduler(grid)
        tr = _trainer(effect_scheduler=sched, apply_effect=E.apply_effect, spectral_losses=True)
        _seed(5)
        outs = [tr.step(x, msg)]
        if with_validate:
            calls = []
            sel, upd = sched.select_effects, sched.update_effect_metrics
            sched.select_effects = lambda *a, **k: (calls.append("select"), sel(*a, **k))[1]
            sched.update_effect_metrics = lambda *a, **k: (calls.append("update"), upd(*a, **k))[1]
            before = (sched.get_effect_statistics(), sched.get_effect_probabilities(), tr.effect_update_count)
            rng = (np.random.get_state(), random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state())
            arenas = [t.clone() for net in (tr.G, tr.D, tr.L) for t in (net.arena, net.grads, net.opt.m, net.opt.v)]
            val = tr.validate(x, msg)
            assert np.isfinite(float(val["loss"]))
            assert calls == [] and before == (sched.get_effect_statistics(), sched.get_effect_probabilities(), tr.effect_update_count)
            now = (np.random.get_state(), random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state())
            assert rng[1] == now[1] and torch.equal(rng[2], now[2]) and torch.equal(rng[3], now[3])
            assert rng[0][0] == now[0][0] and np.array_equal(rng[0][1], now[0][1]) and rng[0][2:] == now[0][2:]
            assert all(torch.equal(a, b) for a, b in zip(arenas, [t for net in (tr.G, tr.D, tr.L) for t in (net.arena, net.grads, net.opt.m, net.opt.v)]))
            sched.select_effects, sched.update_effect_metrics = sel, upd
        outs.append(tr.step(x, msg))
        return tr, sched, outs
    a, sa, oa = run(False)
    b, sb, ob = run(True)
    for p, q in zip(oa, ob):
        for k in LOSS_KEYS + ("loss", "grad_norm"):
            assert torch.equal(p[k], q[k]), k
        assert p["stats"] == q["stats"]
    for na, nb in ((a.G, b.G), (a.D, b.D), (a.L, b.L)):
        assert torch.equal(na.arena, nb.arena) and torch.equal(na.opt.m, nb.opt.m) and torch.equal(na.opt.v, nb.opt.v) and na.opt.t == nb.opt.t == 2
    assert sa.get_effect_statistics() == sb.get_effect_statistics() and a.effect_update_count == b.effect_update_count


def test_identity_validation_is_the_existing_pieces_composed():
    from waveverify_amd.metrics import BER, MIOU
    from waveverify_amd.train import bce_logits, l1_loss
    tr = _trainer(spectral_losses=True)
    x, msg = _batch(2)
    out = tr.validate(x, msg, eval_effects=[("identity", {})], augment=False)
    wm = tr.G.forward(x, msg)
    mask = torch.ones_like(wm)
    logits_d, logits_l = tr.D.forward(wm), tr.L.forward(wm)
    dec, _ = bce_logits(logits_d, mask, msg, want_grad=False)
    loc, _ = bce_logits(logits_l, mask, None, want_grad=False)
    wav, _ = l1_loss(wm, x, want_grad=False)
    stft, mel, _ = tr.spectral(wm, x, want_grad=False)
    lam = tr.lambdas
    total = lam["dec/loss"] * dec + lam["loc/loss"] * loc + lam["waveform/loss"] * wav
    total = total + lam["stft/loss"] * stft + lam["mel/loss"] * mel
    for k, v in (("dec/loss", dec), ("loc/loss", loc), ("waveform/loss", wav), ("stft/loss", stft), ("mel/loss", mel), ("loss", total)):
        assert torch.equal(out[k], v), (k, float(out[k]), float(v))
    ld, ll, m, g = logits_d.cpu(), logits_l.cpu(), mask.cpu(), msg.cpu()
    assert np.float32(out["identity/ber"]) == np.float32(float(BER()(ld, g, m)))             # the class returns a float32 ratio
    assert out["identity/miou"] == MIOU()((ll > 0.5).float(), m)
    for b in range(B):
        assert np.float32(out["per_clip"]["ber"][0, b]) == np.float32(float(BER()(ld[b:b + 1], g[b:b + 1], m[b:b + 1])))
        assert out["per_clip"]["miou"][0, b] == MIOU()((ll[b:b + 1] > 0.5).float(), m[b:b + 1])


def test_the_shipped_seven_effects_run_on_the_whole_batch():
    """Every <effect>/ber and /miou equals the BER / MIOU classes on that effect's logits, recomputed here under the seed validate uses:
    the augmentation drawn by an augmenter of the test's own, then effects.apply_effect in the list's order (random_noise draws from
    torch's device generator)."""
    from waveverify_amd.augment import TemporalAugmenter
    from waveverify_amd.metrics import BER, MIOU
    tr = _trainer()
    x, msg = _batch(3)
    out = tr.validate(x, msg, seed=7)
    assert out["per_clip"]["effects"] == [n for n, _ in E.EVAL_EFFECTS] and len(E.EVAL_EFFECTS) == 7
    _seed(7)
    wm = tr.G.forward(x, msg)
    sig, mask, _, _ = TemporalAugmenter(16000, 0.1).forward(x, wm)
    seen = []
    for name, params in E.EVAL_EFFECTS:
        a_e, m_e = E.apply_effect(name, dict(params), sig.audio_data, mask)
        assert a_e.shape == wm.shape
        seen.append(a_e)
        ld, ll = tr.D.forward(a_e).cpu(), tr.L.forward(a_e).cpu()
        assert np.float32(out[f"{name}/ber"]) == np.float32(float(BER()(ld, msg.cpu(), m_e.cpu()))), name
        assert out[f"{name}/miou"] == MIOU()((ll > 0.5).float(), m_e.cpu()), name
    assert all(not torch.equal(seen[0], s) for s in seen[1:])                     # six effects that do something
    again = tr.validate(x, msg, seed=7)                                           # the same seed evaluates the same pass
    assert all(out[k] == again[k] for k in out if k.endswith(("/ber", "/miou"))) and torch.equal(out["loss"], again["loss"])


def test_a_refused_effect_raises_by_name_before_any_launch():
    tr = _trainer()
    x, msg = _batch()

    def boom(*a, **k):
        raise AssertionError("the generator ran")
    tr.G.forward = boom
    for name in E.REFUSED:
        with pytest.raises(NotImplementedError, match=name):
            tr.validate(x.cpu(), msg.cpu(), eval_effects=[("identity", {}), (name, {})])
    with pytest.raises(NotImplementedError, match="no_such_effect"):
        tr.validate(x.cpu(), msg.cpu(), eval_effects=[("no_such_effect", {})])
