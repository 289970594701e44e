"""STOI on the GPU (csrc/wv_stoi.hip) against the float64 oracle of tests/stoi_cases.py, stage by stage: which frames are kept (equal),
the third-octave magnitudes (to the f32-MFMA error model), d (to a bar under 1e-5, a tenth of the last digit the reference prints), the
1e-5 of a clip with 29 frames; and, called through the C ABI with guard bands round every output, a poisoned workspace and every input
one float past an aligned boundary, its contract: nothing else written, two runs bit-equal, a clip's numbers independent of its batch.

Bars = the measured maximum over the case list x 4, rounded up to one significant digit (the kernels are deterministic: the margin is for
compilers, not noise).  Measured on an MI355X:
    |d - d64|                                      max 5.17e-8 -> D_BAR   = 3e-7   (cap: 1e-5)
    |tob - tob64| / (1e-7 sqrt(sum_bins S^2))      max 3.802   -> K_TOB   = 20     (S = sum_n |basis frame| of a bin's re / im sum)
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import stoi_cases as sc
from guard import Guards
from waveverify_amd import _lib, metrics, stoi as S

pytestmark = pytest.mark.gpu

D_BAR = 3e-7
K_TOB = 20.0
assert D_BAR <= 1e-5


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(x, y, fs):
    """One wv_metrics_stoi call on [B, T] float32 arrays (x = the clean clips) with everything guarded -> dict of host arrays."""
    lib = _lib.load()
    B, T = x.shape
    k, up, down, L, width = S.resample_kernels(fs)
    if fs == S.FS:
        up = down = 1
        L = width = 0
    g = Guards(offset=1)
    xi, yi = g.input(x, "reference"), g.input(y, "estimate")
    ki = g.input(k.astype(np.float32), "kernels") if fs != S.FS else None
    bi = g.input(S.dft_basis().astype(np.float32), "basis")
    total = S.n_frames(S.resampled_length(T, fs))
    d = g.output((B,), torch.int64, "stoi")                                     # float64, guarded as 8-byte words
    fr = g.output((B, 2), torch.int32, "frames")
    ki_out = g.output((B, total), torch.int32, "kept_idx")
    tob = g.output((B, 2, 15, max(total - 1, 0)), torch.float32, "tob")
    ws = g.workspace(int(lib.wv_metrics_stoi_workspace_bytes(B, T, up, down, L, width)))
    rc = lib.wv_metrics_stoi(xi.t.data_ptr(), yi.t.data_ptr(), B, T, None if ki is None else ki.t.data_ptr(), up, down, L, width, bi.t.data_ptr(),
                             d.t.data_ptr(), fr.t.data_ptr(), ki_out.t.data_ptr(), tob.t.data_ptr(), ws.t.data_ptr(), ws.n, _stream())
    assert rc == 0, lib.wv_last_error()
    g.check()
    return {"d": d.t.clone().view(torch.float64).cpu().numpy(), "frames": fr.t.cpu().numpy(), "kept_idx": ki_out.t.cpu().numpy(),
            "tob": tob.t.cpu().numpy()}


@lru_cache(maxsize=None)
def _batch(name):
    c = next(k for k in sc.cases() if k.name == name)
    return _call(c.x, c.y, c.fs)


NAMES = [c.name for c in sc.cases()]


def test_kept_frames_equal_the_oracles():
    for name in NAMES:
        got, want = _batch(name), sc.oracle(name)
        for b, o in enumerate(want):
            assert got["frames"][b].tolist() == [o["kept"], o["total"]], (name, b)
            assert np.array_equal(got["kept_idx"][b, : o["kept"]], o["kept_idx"]) and (got["kept_idx"][b, o["kept"]:] == -1).all(), (name, b)


def test_band_magnitudes_within_the_f32_mfma_error_model():
    """|tob - tob64| <= K_TOB 1e-7 sqrt(sum over the band's bins of S_re^2 + S_im^2), S = sum_n |basis[n] frame[n]| of that bin's real /
    imaginary sum: the error of an f32 fmaf chain per bin sum (about 1e-7 sum |a b|), carried through sqrt(sum re^2 + im^2)."""
    n = np.arange(256)
    bins = np.arange(S.BIN_LO, S.BIN_HI)
    ang = 2 * np.pi * ((n[:, None] * bins[None, :]) % 512) / 512
    c_abs, s_abs = np.abs(np.cos(ang)), np.abs(np.sin(ang))
    worst = 0.0
    for name in NAMES:
        got, want = _batch(name), sc.oracle(name)
        for b, o in enumerate(want):
            J = o["J"]
            if J < 1:
                continue
            for s, key in enumerate(("x", "y")):
                fr = np.abs(o[f"frames_{key}"])                                 # [J, 256], windowed
                s2 = (fr @ c_abs) ** 2 + (fr @ s_abs) ** 2                      # [J, 212]
                scale = np.stack([np.sqrt(s2[:, lo - S.BIN_LO: hi - S.BIN_LO].sum(axis=1)) for lo, hi in S.band_edges()])     # [15, J]
                err = np.abs(got["tob"][b, s, :, :J].astype(np.float64) - o[f"{key}_tob"])
                worst = max(worst, float((err / (1e-7 * scale)).max()))
                assert not got["tob"][b, s, :, J:].any(), (name, b)             # zeros behind the clip's own frames
    print(f"MEASURE tob: max |gpu - f64| / (1e-7 sqrt(sum S^2)) over the case list = {worst:.3f} (bar {K_TOB})")
    assert worst <= K_TOB


def test_d_against_the_oracle():
    worst = 0.0
    for name in NAMES:
        got, want = _batch(name), sc.oracle(name)
        for b, o in enumerate(want):
            worst = max(worst, abs(got["d"][b] - o["d"]))
    print(f"MEASURE d: max |gpu - f64| over the case list = {worst:.2e} (bar {D_BAR:.0e}, cap 1e-5)")
    assert worst <= D_BAR


def test_29_frames_give_exactly_1e_minus_5():
    assert _batch("T6553")["d"].tolist() == [1e-5] * 3 and _batch("T6553")["frames"].tolist() == [[30, 30]] * 3
    assert all(0.5 < v < 1 for v in _batch("T6554")["d"]) and _batch("T6554")["frames"].tolist() == [[31, 31]] * 3
    c = next(k for k in sc.cases() if k.name == "T6553")
    tiny = _call(c.x[:, :300], c.y[:, :300], 16000)                             # 188 samples at 10 kHz: no frame at all
    assert tiny["d"].tolist() == [1e-5] * 3 and tiny["frames"].tolist() == [[0, 0]] * 3


@pytest.mark.parametrize("name", ["T16001", "quiet", "fs10000"])
def test_two_runs_and_any_batch_give_the_same_bits(name):
    c = next(k for k in sc.cases() if k.name == name)
    first, again = _batch(name), _call(c.x, c.y, c.fs)
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    for b in range(3):
        one = _call(c.x[b:b + 1], c.y[b:b + 1], c.fs)
        for k in first:
            assert np.array_equal(first[k][b:b + 1], one[k]), (k, b)


def test_the_module_is_the_same_call_in_the_references_argument_order():
    c = next(k for k in sc.cases() if k.name == "T16000")
    x, y = torch.from_numpy(c.x)[:, None].cuda(), torch.from_numpy(c.y)[:, None].cuda()
    m = metrics.STOI()
    d = m(y, x, sample_rate=c.fs)                                               # (estimates, references)
    assert d.is_cuda and d.dtype == torch.float64 and tuple(d.shape) == (3,)
    assert np.array_equal(d.cpu().numpy(), _batch("T16000")["d"]) and np.array_equal(m.last_frames.cpu().numpy(), _batch("T16000")["frames"])
    assert float(metrics.STOI().mean(y, x, c.fs)) == pytest.approx(float(d.cpu().numpy().mean()), abs=1e-15)
    swapped = metrics.STOI()(x, y).cpu().numpy()                                # the noisy clip as the reference: another number
    want = sc.stoi(c.y[2], c.x[2], c.fs)
    assert abs(swapped[2] - want) <= D_BAR and abs(swapped[2] - float(d[2])) > 1e-3
    with pytest.raises(ValueError):
        m(y[:, 0], x[:, 0])


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    z = torch.zeros(2, 4000, device="cuda")
    basis = torch.zeros(256 * 513, device="cuda")
    d = torch.empty(2, dtype=torch.float64, device="cuda")
    fr = torch.empty(2, 2, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    ok = (z.data_ptr(), z.data_ptr(), 2, 4000, None, 1, 1, 0, 0, basis.data_ptr(), d.data_ptr(), fr.data_ptr(), None, None)
    assert lib.wv_metrics_stoi(*ok, ws.data_ptr(), 8, _stream()) == -5                                   # WV_ENOMEM
    assert lib.wv_metrics_stoi(*ok[:4], basis.data_ptr(), *ok[5:], ws.data_ptr(), ws.numel(), _stream()) == -1      # kernels without a ratio
    assert lib.wv_metrics_stoi(*ok[:4], None, 5, 8, 124, 58, *ok[9:], ws.data_ptr(), ws.numel(), _stream()) == -1   # a ratio without kernels
    assert lib.wv_metrics_stoi(*ok[:10], d.data_ptr() + 4, *ok[11:], ws.data_ptr(), ws.numel(), _stream()) == -1    # stoi off its 8 bytes
    assert lib.wv_metrics_stoi(*ok[:2], 0, *ok[3:], ws.data_ptr(), ws.numel(), _stream()) == -1
    torch.cuda.synchronize()


def test_validate_with_stoi_adds_two_keys_and_is_the_module_on_the_watermarked_clips():
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import WatermarkTrainer
    small = dict(channels_enc=8, dimension=16, strides=[2, 2], n_fft_base=16)
    cg = default_config("generator", channels_dec=8, n_residual_dec=1, **small)
    cd, cl = default_config("detector", output_dim=8, **small), default_config("locator", output_dim=8, **small)
    tr = WatermarkTrainer(cg, random_state_dict(cg, 1, parametrized=True), cd, random_state_dict(cd, 1, parametrized=True), cl,
                          random_state_dict(cl, 1, parametrized=True))
    c = next(k for k in sc.cases() if k.name == "T8000")
    x = torch.from_numpy(c.x)[:, None].cuda()
    msg = torch.from_numpy(np.random.default_rng(0).integers(0, 2, (3, 16)).astype(np.float32)).cuda()
    plain = tr.validate(x, msg, eval_effects=[("identity", {})])
    out = tr.validate(x, msg, eval_effects=[("identity", {})], stoi=True)
    assert set(out) - set(plain) == {"STOI"} and set(out["per_clip"]) - set(plain["per_clip"]) == {"stoi"} and set(plain) <= set(out)
    assert "STOI" not in plain and "stoi" not in plain["per_clip"]
    for k in plain:
        if k != "per_clip":
            assert (torch.equal(out[k], plain[k]) if torch.is_tensor(plain[k]) else out[k] == plain[k]), k
    wm = tr.G.forward(x, msg)
    d = metrics.STOI()(wm, x, sample_rate=tr.aug.sample_rate)
    assert np.array_equal(out["per_clip"]["stoi"], d.cpu().numpy()) and out["per_clip"]["stoi"].dtype == np.float64
    assert out["STOI"] == float(out["per_clip"]["stoi"].mean())
    assert out["STOI"] == pytest.approx(float(metrics.STOI().mean(wm, x, tr.aug.sample_rate)), abs=1e-15)
    assert 0 < out["STOI"] <= 1 and (metrics.STOI().last_frames is None)
    want = [sc.stoi(c.x[b], wm[b, 0].cpu().numpy(), 16000) for b in range(3)]
    assert np.abs(out["per_clip"]["stoi"] - np.array(want)).max() <= D_BAR
