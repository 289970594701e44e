"""The float64 spectral-loss oracle (oracle/wv_oracle_specloss.py) against the reference's own loss classes
(tests/golden/spectral_loss.npz, make_golden_specloss.py), the exactness properties of the formula that the GPU tests rely on, and the
conditioning of every case the GPU tests run (tests/specloss_cases.py): the float32 evaluation of the oracle within 1e-5 of max of the
float64 one and no element at a jump of the gradient.  CPU only."""
import math
import os

import numpy as np
import pytest
import torch

import specloss_cases as SC
from oracle import wv_oracle_specloss as OS


@pytest.mark.parametrize("T", [16000, 4800, 1100])
def test_float64_oracle_reproduces_the_reference_fixture(golden_dir, T):
    g = np.load(os.path.join(golden_dir, "spectral_loss.npz"))
    assert list(g["stft_windows"]) == OS.STFT_W and list(g["mel_windows"]) == OS.MEL_W and list(g["mel_n"]) == OS.MEL_N
    stft, mel = OS.default_scales()
    for name, scales in (("stft", stft), ("mel", mel)):
        r = OS.spectral_oracle(g[f"wm_{T}"], g[f"x_{T}"], scales)
        terms, ref_terms = np.array([s[name] for s in r["scales"]]), g[f"{name}_terms_{T}"]
        assert np.all(np.abs(terms - ref_terms) <= 1e-9 * np.abs(ref_terms)), (name, terms, ref_terms)
        ref = float(g[f"{name}_total_{T}"])
        assert abs(r[f"{name}_total"] - ref) <= 1e-9 * ref, (name, r[f"{name}_total"], ref)
        dref = g[f"d_{name}_{T}"]
        e = SC.rel_err(r[f"d_{name}"], dref)
        assert e <= 1e-6, (name, e)
        # the per-scale gradients add up to the total's (autograd of the summed loss, the way the fixture was made)
        per_scale = sum(s[f"d_{name}"] for s in r["scales"])
        assert SC.rel_err(per_scale, r[f"d_{name}"]) <= 1e-12
        other = "mel" if name == "stft" else "stft"
        assert r[f"{other}_total"] == 0.0 and not r[f"d_{other}"].any()
    # both losses in one call and the combination of the two gradients
    both = OS.spectral_oracle(g[f"wm_{T}"], g[f"x_{T}"], SC.default_scales(), stft_grad_scale=10.0, mel_grad_scale=20.0)
    assert abs(both["stft_total"] - float(g[f"stft_total_{T}"])) <= 1e-9 * float(g[f"stft_total_{T}"])
    assert abs(both["mel_total"] - float(g[f"mel_total_{T}"])) <= 1e-9 * float(g[f"mel_total_{T}"])
    dref = 10.0 * g[f"d_stft_{T}"].astype(np.float64) + 20.0 * g[f"d_mel_{T}"]
    assert SC.rel_err(both["d_total"], dref) <= 1e-6


def test_restated_filters_with_fmin_fmax_and_empty_bands():
    # the float32 filters are the float64 ones to float32 rounding; fmin / fmax move the edges: nothing outside [fmin, fmax]
    for n, w in zip(OS.MEL_N, OS.MEL_W):
        a, b = OS.slaney_filters(16000, w, n), OS.slaney_filters_f32(16000, w, n)
        assert b.dtype == np.float32 and np.abs(a - b).max() <= 2e-7 * np.abs(a).max()
        assert OS.empty_bands(16000, w, n) == []
    W = OS.slaney_filters(16000, 512, 10, fmin=300.0, fmax=4000.0)
    f = np.arange(257) * 16000 / 512
    assert not W[:, (f <= 300.0) | (f >= 4000.0)].any() and (W.max(axis=1) > 0).all()
    w, n = SC.ONE_EMPTY_BAND
    assert OS.empty_bands(SC.SR, w, n) == [0]
    assert OS.empty_bands(SC.SR, 8, 5) == [0, 1]
    # the rule "skip mel where the restated filter has only empty bands" removes no case of the table
    for _, w, n, _, _, _, _ in SC.GEOMETRY_CASES:
        assert len(OS.empty_bands(SC.SR, w, n)) < n, (w, n)


def test_empty_band_contributes_nothing():
    """An empty band's energy is 0 on both sides: |log10(eps) - log10(eps)| = 0 in the mean (which still counts the band), and no
    gradient: the term is the non-empty bands' sum over all n_mels * frames elements, and a filter bank without the empty row gives
    the same gradient scaled by (n_mels - 1) / n_mels."""
    w, n = SC.ONE_EMPTY_BAND
    wm, x = SC.clips(3, 1001, 5)
    r = OS.spectral_oracle(wm, x, [SC.mel_scale(w, n)], want_bins=True)
    fb = torch.from_numpy(OS.slaney_filters_f32(SC.SR, w, n)).double()
    a, b = fb @ torch.from_numpy(r["scales"][0]["mag_wm"]), fb @ torch.from_numpy(r["scales"][0]["mag_x"])
    per_band = (torch.log10(a.clamp(1e-5)) - torch.log10(b.clamp(1e-5))).abs().mean(dim=(0, 2))
    assert float(per_band[0]) == 0.0 and (per_band[1:] > 0).all()
    assert abs(float(per_band[1:].sum()) / n - r["scales"][0]["mel"]) <= 1e-12 * r["scales"][0]["mel"]
    a4 = a[:, 1:].detach().requires_grad_(True)
    (torch.log10(a4.clamp(1e-5)) - torch.log10(b[:, 1:].clamp(1e-5))).abs().mean().backward()
    dmag = torch.einsum("mf,bmt->bft", fb[1:], a4.grad) * (n - 1) / n
    assert SC.rel_err(dmag.numpy(), r["scales"][0]["dmag_mel"]) <= 1e-12


def test_identical_signals_and_a_gain_of_two():
    rng = np.random.default_rng(3)
    x = (0.1 * rng.standard_normal((3, 1, 1201))).astype(np.float32)
    scales = SC.default_scales()[:5] + [SC.stft_scale(64, (1.0, 1.0, 2.0, 1e-5))]
    r = OS.spectral_oracle(x.copy(), x, scales)
    assert r["stft_total"] == 0.0 and r["mel_total"] == 0.0 and not r["d_total"].any()
    # wm = 2 x: every bin with both sides >= eps has |log difference| = pow * log10(2); the magnitude part is mean |X_x|
    for w in (32, 512):
        for p in (1.0, 2.0):
            eps = SC.raised_clamp(w)
            for gain in (2.0, 0.5):
                r = OS.spectral_oracle(gain * x, x, [SC.stft_scale(w, (1.0, 0.0, p, eps)), SC.stft_scale(w, SC.STFT_MAG)], want_bins=True)
                a, b = r["scales"][0]["mag_wm"], r["scales"][0]["mag_x"]
                both = (a >= eps) & (b >= eps)
                neither = (a < eps) & (b < eps)
                rest = ~both & ~neither                 # one side clamped: |p log10(larger / eps)| < p log10(2)
                big = np.maximum(a, b)
                want = (p * math.log10(2.0) * both.sum() + (p * np.log10(big[rest] / eps)).sum()) / both.size
                assert abs(r["scales"][0]["stft"] - want) <= 1e-12 * want
                assert abs(r["scales"][0]["stft"] - p * math.log10(2.0) * both.mean()) <= p * math.log10(2.0) * rest.mean()
                assert abs(r["scales"][1]["stft"] - abs(gain - 1.0) * b.mean()) <= 1e-12 * b.mean()


def _floor(wm, x, scales):
    """-> (float64 result, float32 result)."""
    return OS.spectral_oracle(wm, x, scales), OS.spectral_oracle(wm, x, scales, dtype=torch.float32)


@pytest.mark.parametrize("case", SC.PART_CASES, ids=SC.PART_IDS)
def test_part_cases_are_conditioned(case):
    cid, part, scale, T, seed, bar = case
    wm, x = SC.clips(SC.PART_B, T, seed)
    r64, r32 = _floor(wm, x, [scale])
    e = SC.rel_err(r32["scales"][0]["d_" + part], r64["scales"][0]["d_" + part])
    print(f"RECORD floor {cid}: float32 oracle vs float64 {e:.2e} of max, unsafe elements {r64['scales'][0]['unsafe']}")
    if bar == SC.GRAD_BAR:                              # the reference's clamp is not conditionable and keeps its old bar
        assert e <= SC.FLOOR_BAR, (cid, e)
        assert r64["scales"][0]["unsafe"] == 0, cid
    assert abs(r32["scales"][0][part] - r64["scales"][0][part]) <= 1e-6 * r64["scales"][0][part]


@pytest.mark.parametrize("case", SC.GEOMETRY_CASES, ids=SC.GEOMETRY_IDS)
def test_geometry_cases_are_conditioned(case):
    cid, w, n, mel_term, B, T, seed = case
    wm, x = SC.clips(B, T, seed)
    r64, r32 = _floor(wm, x, [SC.geometry_scale(w, n, mel_term)])
    s64, s32 = r64["scales"][0], r32["scales"][0]
    for part in ("stft", "mel"):
        e = SC.rel_err(s32["d_" + part], s64["d_" + part])
        assert e <= SC.FLOOR_BAR, (cid, part, e)
    assert s64["unsafe"] == 0, cid


def test_geometry_table_holds_the_corners_it_promises():
    cols = {SC.n_columns(w, B, T) for _, w, _, _, B, T, _ in SC.GEOMETRY_CASES}
    assert {1, 2, 3} <= {c % 4 for c in cols} and {255, 256, 257} <= cols
    for w in (8, 12, 40, 100, 32, 512):
        Ts = {T for _, ww, _, _, _, T, _ in SC.GEOMETRY_CASES if ww == w}
        hop = w // 4
        assert {w // 2 + 1, w // 2 + 2, w - 1, w, w + 1, 5 * hop - 1, 5 * hop, 5 * hop + 1} <= Ts and any(T > 900 and T % 2 for T in Ts)
    assert {B for _, _, _, _, B, _, _ in SC.GEOMETRY_CASES} == {1, 2, 3, 7}
    assert any((w, n) == SC.ONE_EMPTY_BAND for _, w, n, _, _, _, _ in SC.GEOMETRY_CASES)


def _conditioned(wm, x, scales, what):
    r64, r32 = _floor(wm, x, scales)
    for s64, s32 in zip(r64["scales"], r32["scales"]):
        for part in ("stft", "mel"):
            if s64[part] is not None:
                assert SC.rel_err(s32["d_" + part], s64["d_" + part]) <= SC.FLOOR_BAR, (what, s64["w"], part)
        assert s64["unsafe"] == 0, (what, s64["w"])


def test_mixed_batch_gain_and_guard_plans_are_conditioned():
    m = SC.MIXED
    _conditioned(*SC.clips(m["B"], m["T"], m["seed"]), SC.mixed_scales(), "mixed")
    _conditioned(*SC.batch_clips(), SC.batch_scales(), "batch")
    wm, x = SC.batch_clips()
    for b in (0, 2, 4):
        _conditioned(wm[b: b + 1], x[b: b + 1], SC.batch_scales(), f"batch clip {b}")
    for w, gain, seed in SC.GAIN_CASES:
        _conditioned(*SC.gain_clips(gain, seed), [SC.stft_scale(w, SC.STFT_MAG), SC.stft_scale(w, SC.stft_log(w))], f"gain {gain} w {w}")
    _conditioned(*SC.refusal_clips()[2:], SC.refusal_scales(), "refusal")
    for cid, scales, B, T, seed, bar in SC.guard_cases():
        if bar == SC.GRAD_BAR:
            _conditioned(*SC.clips(B, T, seed), scales, cid)
