"""The validation metrics without a GPU: the fixture itself (the reference's SI-SNR against a float64 restatement of its statements),
the torch route of metrics.ber_per_clip / miou_per_clip / SISNR against the reference's records in tests/golden/validation_metrics.npz
and tests/golden/metrics.npz, the shipped evaluation-effect list, and the C ABI's declarations."""
import json
import os
import re

import numpy as np
import pytest
import torch

from validation_cases import (MET_BER, MIOU_CASES, SI_BATCH, SI_BATCH_MEAN, SI_CASES, VAL_BER, check_decode, iou_counts_np, sisnr_bound,
                              sisnr_f64)
from waveverify_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("wv_metrics_decode", "wv_metrics_decode_workspace_bytes", "wv_metrics_iou", "wv_metrics_iou_workspace_bytes", "wv_metrics_sisnr",
               "wv_metrics_sisnr_workspace_bytes")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def test_fixture_sisnr_is_the_float64_restatement_within_float32():
    """d_i = |reference (float32) - float64 restatement| per case, printed: the only tolerance source of the GPU test.  What float32 can
    hold: the noise power is a float32 difference of signals, so its relative error is about 2^-23 times the signal-to-noise ratio (times
    the DC power over the signal power where a clip rides on an offset) -- 0.05 dB at 30 dB, a few dB at 60 dB.  The eps-driven values
    (silent reference, one-sample clips) are exact."""
    assert {c["T"] for c in SI_CASES} == {1, 63, 64, 65, 400, 4097, 16000}
    assert {c["kind"] for c in SI_CASES} == {"noise", "identical", "silent", "dc"}
    for c in SI_CASES:
        print(f"si{c['i']:02d} {c['kind']:9s} T={c['T']:5d} ref_f32={c['ref_f32']:+.6f} f64={c['f64']:+.6f} d={c['d']:.3e}")
        assert np.isfinite(c["ref_f32"]) and np.isfinite(c["f64"])
        if c["kind"] == "silent" or c["T"] == 1:
            assert abs(c["f64"] - 10 * np.log10(1e-8)) < 1e-9 and c["d"] < 1e-4
        elif c["kind"] == "noise":
            snr = 10.0 ** (c["f64"] / 10.0)
            assert c["d"] <= 10 / np.log(10) * 64 * 2.0 ** -23 * snr + 1e-4, c
    levels = sorted(round(c["f64"], -1) for c in SI_CASES if c["kind"] == "noise" and c["T"] == 400)
    assert levels == [10.0, 30.0, 60.0], levels


@pytest.mark.parametrize("c", SI_CASES, ids=lambda c: f"si{c['i']}-{c['kind']}-T{c['T']}")
def test_sisnr_cpu_route(c):
    m = metrics.SISNR()
    got = m(_t(c["est"])[None, None], _t(c["ref"])[None, None])
    assert got.dtype == torch.float64 and tuple(got.shape) == (1,)
    assert abs(float(got) - c["f64"]) <= (1e-9 if c["kind"] in ("silent", "identical") else sisnr_bound(c["f64"])), (float(got), c["f64"])
    assert abs(float(got) - c["ref_f32"]) <= c["d"] + sisnr_bound(c["f64"])
    x, y = c["est"].astype(np.float64), c["ref"].astype(np.float64)
    want = np.array([x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()])
    assert np.allclose(m.last_moments.numpy()[0], want, rtol=1e-13, atol=0)


def test_sisnr_mean_is_the_reference_scalar():
    cs = [SI_CASES[i] for i in SI_BATCH]
    est, ref = (_t(np.stack([c[k] for c in cs]))[:, None] for k in ("est", "ref"))
    m = metrics.SISNR()
    per_clip = m(est, ref)
    assert [float(v) for v in per_clip] == [float(m(est[i:i + 1], ref[i:i + 1])) for i in range(len(cs))]
    tol = float(np.mean([c["d"] for c in cs])) + 1e-6
    assert abs(float(m.mean(est, ref)) - SI_BATCH_MEAN) <= tol
    assert abs(float(m.mean(est, ref)) - float(np.mean(sisnr_f64(est.numpy()[:, 0], ref.numpy()[:, 0])))) <= 1e-6
    with pytest.raises(ValueError):
        m(est, ref[:, :, :-1])


@pytest.mark.parametrize("case", VAL_BER + MET_BER, ids=lambda c: c["name"])
def test_ber_per_clip_cpu_route(case):
    errors, valid, avg = metrics.ber_per_clip(_t(case["logits"]), _t(case["bits"]), _t(case["mask"]), threshold=case["thr"])
    assert errors.dtype == torch.int32 and valid.dtype == torch.int32 and avg.dtype == torch.float32
    check_decode(case, errors.numpy(), valid.numpy(), avg.numpy())
    ref = metrics.BER(threshold=case["thr"])(_t(case["logits"]), _t(case["bits"]), _t(case["mask"]))      # the class is untouched and agrees
    total = int(valid.sum())
    assert abs(float(ref) - (float(errors.sum()) / total if total else 0.0)) < 1e-7


def test_ber_per_clip_counts_cases_and_shapes():
    assert len(MET_BER) == 17
    assert {c["logits"].shape[1] for c in VAL_BER} == {1, 8, 16} and max(c["logits"].shape[0] for c in VAL_BER) <= 4
    assert any(c["mask"] is not None and (c["mask"].sum(axis=2) == 0).any() for c in VAL_BER)
    z = torch.zeros(2, 4, 8)
    with pytest.raises(ValueError):
        metrics.ber_per_clip(z, torch.zeros(2, 3))
    with pytest.raises(ValueError):
        metrics.ber_per_clip(z, torch.zeros(2, 4), torch.ones(2, 1, 9))


@pytest.mark.parametrize("case", MIOU_CASES, ids=lambda c: c["name"])
def test_miou_cpu_route(case):
    p, g = _t(case["p"]), _t(case["g"])
    counts = metrics.iou_counts(p, g)
    assert counts.dtype == torch.int32 and np.array_equal(counts.numpy(), iou_counts_np(case["p"], case["g"]))
    per_clip = metrics.miou_per_clip(p, g)
    assert per_clip.dtype == np.float64 and per_clip.shape == (p.shape[0],)
    assert float(metrics.miou_from_counts(counts.numpy().astype(np.int64).sum(axis=0))) == case["out"]     # the whole tensor, as MIOU takes it
    for b in range(p.shape[0]):
        assert per_clip[b] == metrics.MIOU()(p[b:b + 1], g[b:b + 1])


def test_miou_binarises_the_raw_locator_output():
    raw = torch.tensor([[[0.2, 0.5, 0.500001, 3.0, -1.0, float("nan")]]])
    g = torch.tensor([[[0.0, 1.0, 1.0, 1.0, 0.0, 0.0]]])
    assert metrics.iou_counts(raw, g).tolist() == [[2, 3, 3, 4]]
    assert metrics.miou_per_clip(raw, g)[0] == (2 / 3 + 3 / 4) / 2
    assert metrics.miou_per_clip(torch.zeros(1, 1, 4), torch.zeros(1, 1, 4))[0] == 1.0          # empty foreground union counts as 1


def test_eval_effects_constant_is_the_shipped_list():
    from waveverify_amd import effects
    with open(os.path.join(ROOT, "tests", "golden", "eval_effects.json")) as f:
        shipped = [(e["name"], e["params"]) for e in json.load(f)["eval_effects"]]
    assert [(n, dict(q)) for n, q in effects.EVAL_EFFECTS] == shipped
    assert [n for n, _ in shipped] == ["identity", "resample", "speed", "random_noise", "lowpass_filter", "highpass_filter", "bandpass_filter"]
    assert all(hasattr(effects.AudioEffects, n) and n not in effects.REFUSED for n, _ in shipped)


def test_the_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    declared = set(re.findall(r"\b(wv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert lib.wv_metrics_decode_workspace_bytes(3, 16, 4097) >= 3 * 16 * 2 * 2 * 8
    assert lib.wv_metrics_decode_workspace_bytes(0, 16, 10) == 0 and lib.wv_metrics_iou_workspace_bytes(70000, 10) == 0
    assert lib.wv_metrics_sisnr_workspace_bytes(2, 4096) >= 2 * 5 * 8


def test_validate_is_part_of_the_trainer():
    from waveverify_amd.train import WatermarkTrainer
    assert callable(getattr(WatermarkTrainer, "validate", None))
    assert "STOI" in WatermarkTrainer.validate.__doc__ and "PESQ" in WatermarkTrainer.validate.__doc__
