"""STOI without a GPU: the float64 oracle of tests/stoi_cases.py against what third parties are available (scipy's polyphase resampler),
against the published tables, and against itself broken on purpose; the host tables the kernels read (wv_fx_resample's kernel table, the
DFT basis, the gather that replaces overlap-add); the case list's conditions; metrics.STOI on CPU tensors; the two exports."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import stoi_cases as sc
from waveverify_amd import _lib, stoi as S
from waveverify_amd.metrics import STOI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("wv_metrics_stoi", "wv_metrics_stoi_workspace_bytes")


def _clip(name="T16000", b=0):
    c = next(k for k in sc.cases() if k.name == name)
    return c.x[b].astype(np.float64), c.y[b].astype(np.float64), c.fs


# ---- the resampler ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs, taps", [(16000, 581), (8000, 365)])
def test_oracle_resampler_is_scipys_resample_poly(fs, taps):
    sig = pytest.importorskip("scipy.signal")
    p, q = S.ratio(fs)
    h, half = sc.resample_window(p, q)
    assert len(h) == taps == 2 * half + 1 and abs(h.sum() - 1) < 1e-15
    for T in (16000, 16001, 6553, 700):
        x = _clip()[0][:T] if T <= 16000 else np.concatenate([_clip()[0], [0.25]])
        want = sig.resample_poly(x, p, q, window=h)
        got = sc.resample(x, fs)
        assert got.shape == want.shape == (-(-T * p // q),)
        err = np.abs(got - want).max()
        print(f"MEASURE oracle resampler vs scipy fs={fs} T={T}: {err:.2e}")
        assert err < 1e-12


@pytest.mark.parametrize("fs, geom", [(16000, (5, 8, 124, 58)), (8000, (5, 4, 78, 37))])
def test_kernel_table_reproduces_the_resampler_by_wv_fx_resamples_formula(fs, geom):
    """y[m] = sum_j kernels[m % nw][j] xz[(m / nw) orig + j - width], nw = up, orig = down, as include/waveverify_hip.h documents it,
    evaluated index by index; and the package's vectorised route through the same table."""
    k, up, down, L, width = S.resample_kernels(fs)
    assert (up, down, L, width) == geom and k.shape == (up, L) and L == 2 * width + down
    h, half = sc.resample_window(up, down)
    assert abs(k.sum() - up) < 1e-12 and np.count_nonzero(k) == np.count_nonzero(h)          # every tap of h exactly once
    for T in (700, 6553):
        x = _clip()[0][:T]
        want = sc.resample(x, fs)
        t_out = S.resampled_length(T, fs)
        assert t_out == len(want) and t_out <= (-(-T // down) + 1) * up                       # within what wv_fx_resample serves
        m = np.arange(t_out)
        src = (m // up)[:, None] * down + np.arange(L)[None, :] - width
        xz = np.where((src >= 0) & (src < T), x[np.clip(src, 0, T - 1)], 0.0)
        got = (k[m % up] * xz).sum(axis=1)
        assert np.abs(got - want).max() < 1e-12
        assert np.abs(S.resample(x, fs) - want).max() < 1e-12
    assert S.resample(_clip()[0], S.FS) is not None and np.array_equal(S.resample(_clip()[0][:50], S.FS), _clip()[0][:50])


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def test_band_bins_are_the_published_ranges():
    obm = sc.thirdoct()
    for i, (lo, hi) in enumerate(sc.BAND_BINS):
        assert np.array_equal(np.nonzero(obm[i])[0], np.arange(lo, hi + 1)), i
    assert [tuple(e) for e in S.band_edges()] == [(lo, hi + 1) for lo, hi in sc.BAND_BINS]
    assert (S.BIN_LO, S.BIN_HI) == (sc.BAND_BINS[0][0], sc.BAND_BINS[-1][1] + 1)
    src = open(os.path.join(ROOT, "waveverify_amd", "csrc", "wv_stoi.hip")).read()
    table = re.search(r"st_band_lo\[ST_BANDS \+ 1\] = \{([^}]*)\}", src).group(1)
    assert [int(v) for v in table.split(",")] == [lo for lo, _ in sc.BAND_BINS] + [sc.BAND_BINS[-1][1] + 1]


def test_the_frame_range_convention_has_one_switch_per_route_and_they_agree():
    src = open(os.path.join(ROOT, "waveverify_amd", "csrc", "wv_stoi.hip")).read()
    c_side = re.search(r"constexpr bool ST_FRAME_END_EXCLUSIVE = (true|false);", src).group(1) == "true"
    assert sc.FRAME_END_EXCLUSIVE is True and S.FRAME_END_EXCLUSIVE is True and c_side
    for n in (0, 256, 257, 384, 385, 4096, 4097, 10000):
        assert S.n_frames(n) == len(sc.frame_starts(n))
    assert S.n_frames(4096) == 30 and S.n_frames(4097) == 31                                   # 256 + 128 k samples: k frames


def test_dft_basis_is_the_windowed_rfft_of_the_bins_the_bands_read():
    flat = S.dft_basis()
    assert flat.shape == (256 * 512 + 256,)
    basis, w = flat[: 256 * 512].reshape(256, 512), flat[256 * 512:]
    assert np.array_equal(w, sc.W) and not basis[:, 424:].any()
    fr = np.random.default_rng(0).standard_normal((5, 256))
    spec = np.fft.rfft(fr * sc.W, 512, axis=1)[:, 7:219]
    got = fr @ basis
    assert np.abs(got[:, 0:424:2] - spec.real).max() < 1e-12 and np.abs(got[:, 1:424:2] - spec.imag).max() < 1e-12


def test_the_gather_is_overlap_add_then_framing_exactly():
    """Leading, interior and trailing frames dropped, and none: the frames the kernel builds from the kept frames and their two
    neighbours are bit for bit the oracle's (remove silent frames by overlap-add, frame again)."""
    seen = 0
    for name in ("quiet", "T16000", "T8000"):
        c = next(k for k in sc.cases() if k.name == name)
        for b, o in enumerate(sc.oracle(name)):
            for sig, key in ((c.x[b], "frames_x"), (c.y[b], "frames_y")):
                x10 = sc.resample(sig.astype(np.float64), c.fs)
                kept, total = S.kept_frames(sc.resample(c.x[b].astype(np.float64), c.fs))
                assert np.array_equal(kept, o["kept_idx"]) and total == o["total"]
                assert np.array_equal(S.gathered_frames(x10, kept) * sc.W, o[key])
                seen += 1
    assert seen == 18


# ---- the oracle on its own -------------------------------------------------------------------------------------------------------
def test_identical_clips_give_one():
    for name in ("T16000", "fs10000", "fs8000"):
        for b in range(3):
            x, _, fs = _clip(name, b)
            assert abs(sc.stoi(x, x, fs) - 1) < 1e-12


def test_29_frames_give_1e_minus_5_and_the_warning():
    x, y, fs = _clip("T6553", 2)
    with pytest.warns(RuntimeWarning, match="Not enough STFT frames"):
        r = sc.stoi_stages(x, y, fs)
    assert r["J"] == 29 and r["kept"] == r["total"] == 30 and r["d"] == 1e-5
    x, y, fs = _clip("T6554", 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = sc.stoi_stages(x, y, fs)
    assert r["J"] == 30 and 0 < r["d"] < 1
    with pytest.warns(RuntimeWarning):
        assert sc.stoi_stages(x[:300], y[:300], fs)["d"] == 1e-5                               # no frame at all


def test_a_broken_oracle_moves_d_by_more_than_the_bars_can_miss():
    x, y, fs = _clip("T16000", 2)
    d = sc.stoi(x, y, fs)
    moved = []
    for band in range(sc.NUMBAND):
        obm = sc.thirdoct()
        obm[band] = np.roll(obm[band], 1)
        moved.append(abs(sc.stoi(x, y, fs, bands=obm) - d))
    n29 = abs(sc.stoi(x, y, fs, n_seg=29) - d)
    print(f"MEASURE one band rolled by one bin moves d by at most {max(moved):.2e}; N = 29 by {n29:.2e}")
    assert max(moved) > 1e-3 and n29 > 1e-3


def test_float32_stages_stay_far_inside_the_cap():
    worst = 0.0
    for c in sc.cases():
        for b, o in enumerate(sc.oracle(c.name)):
            worst = max(worst, abs(sc.stoi(c.x[b], c.y[b], c.fs, dtype=np.float32) - o["d"]))
    print(f"MEASURE float32 emulation of every stage but the DFT: max |d - d64| = {worst:.2e}")
    assert worst < 1e-6


# ---- the case list ---------------------------------------------------------------------------------------------------------------
def test_case_list_conditions():
    names = [c.name for c in sc.cases()]
    assert names == ["T16000", "T16001", "T8000", "T6553", "T6554", "fs10000", "fs8000", "quiet"]
    assert {c.x.shape[1] for c in sc.cases() if c.fs == 16000} == {6553, 6554, 8000, 16000, 16001}
    kinds = {k for c in sc.cases() for k in c.kinds}
    assert kinds == {"wm", "n20", "n5", "n0"}
    none = lead = inner = trail = clipped = False
    margin = np.inf
    for c in sc.cases():
        assert c.x.shape == c.y.shape and c.x.shape[0] == 3 and c.x.dtype == c.y.dtype == np.float32
        for o in sc.oracle(c.name):
            margin = min(margin, np.abs(o["margins"]).min())
            gone = np.nonzero(o["margins"] >= 0)[0]
            assert o["kept"] + len(gone) == o["total"]
            none |= len(gone) == 0
            lead |= len(gone) > 1 and gone[0] == 0 and gone[1] == 1
            trail |= len(gone) > 1 and gone[-1] == o["total"] - 1 and gone[-2] == o["total"] - 2
            inner |= any(0 < a and a + 1 == b_ and b_ < o["total"] - 1 and (a - 1) not in gone and o["kept_idx"][0] < a < o["kept_idx"][-1]
                         for a, b_ in zip(gone, gone[1:]))
            clipped |= o.get("clipped", 0.0) > 0
    print(f"MEASURE nearest frame to the keep threshold over the case list: {margin:.4f} dB")
    assert margin > 1e-3
    assert none and lead and inner and trail and clipped
    assert [o["J"] for o in sc.oracle("T6553")] == [29, 29, 29] and [o["J"] for o in sc.oracle("T6554")] == [30, 30, 30]
    x, y, fs = _clip("T16000", 2)
    assert abs(sc.stoi(x, y, fs) - sc.stoi(y, x, fs)) > 1e-3                                    # not symmetric


# ---- metrics.STOI on the CPU -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T16000", "T6554", "fs10000", "fs8000", "quiet"])
def test_cpu_tensors_take_the_float64_route_and_equal_the_oracle(name):
    c = next(k for k in sc.cases() if k.name == name)
    m = STOI()
    d = m(torch.from_numpy(c.y)[:, None], torch.from_numpy(c.x)[:, None], sample_rate=c.fs)
    assert d.dtype == torch.float64 and tuple(d.shape) == (3,) and not d.is_cuda
    o = sc.oracle(name)
    assert np.abs(d.numpy() - np.array([r["d"] for r in o])).max() < 1e-12
    assert m.last_frames.dtype == torch.int32 and m.last_frames.tolist() == [[r["kept"], r["total"]] for r in o]
    assert float(STOI().mean(torch.from_numpy(c.y)[:, None], torch.from_numpy(c.x)[:, None], c.fs)) == float(d.mean())


def test_cpu_route_argument_order_short_clips_and_refusals():
    c = next(k for k in sc.cases() if k.name == "T16000")
    x, y = torch.from_numpy(c.x[2:3])[:, None], torch.from_numpy(c.y[2:3])[:, None]
    o = sc.oracle("T16000")[2]
    assert abs(float(STOI()(y, x)[0]) - o["d"]) < 1e-12                                        # (estimates, references): x is the reference
    assert abs(float(STOI()(x, y)[0]) - sc.stoi(c.y[2], c.x[2], 16000)) < 1e-12 and abs(float(STOI()(x, y)[0]) - o["d"]) > 1e-3
    s = next(k for k in sc.cases() if k.name == "T6553")
    with pytest.warns(RuntimeWarning, match="Not enough STFT frames"):
        d = STOI()(torch.from_numpy(s.y)[:, None], torch.from_numpy(s.x)[:, None])
    assert d.tolist() == [1e-5] * 3
    with pytest.raises(NotImplementedError):
        STOI(extended=True)
    for bad in (x[0], x[:, 0], torch.zeros(2, 2, 100)):
        with pytest.raises(ValueError):
            STOI()(bad, bad)
    with pytest.raises(ValueError):
        STOI()(x, y[..., :-1])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    lib = _lib.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES and getattr(lib, name) is not None
    k, up, down, L, width = S.resample_kernels(16000)
    n = lib.wv_metrics_stoi_workspace_bytes(3, 16000, up, down, L, width)
    t10, f = 10000, 77
    assert n >= 2 * 3 * t10 * 4 + 3 * f * (8 + 4) + 3 * 2 * 15 * (f - 1) * 4 and n % 256 == 0
    assert 0 < lib.wv_metrics_stoi_workspace_bytes(3, 16000, 1, 1, 0, 0) < n                    # no resampled copies at 10 kHz
    assert lib.wv_metrics_stoi_workspace_bytes(1, 100, 1, 1, 0, 0) > 0                          # too short for a frame is still served
    for bad in ((0, 16000, up, down, L, width), (65536, 16000, up, down, L, width), (3, 0, up, down, L, width), (3, 16000, 0, down, L, width),
                (3, 16000, up, down, 0, width), (3, 16000, up, down, L, -1)):
        assert lib.wv_metrics_stoi_workspace_bytes(*bad) == 0, bad
    zero = {_lib.C.c_int: 0, _lib.C.c_size_t: 0}
    assert lib.wv_metrics_stoi(*[zero.get(t) for t in _lib.SIGNATURES["wv_metrics_stoi"][1]]) == -1
    assert b"null pointer" in lib.wv_last_error()


def test_validate_documents_the_option():
    from waveverify_amd.train import WatermarkTrainer
    doc = WatermarkTrainer.validate.__doc__
    assert "stoi=True" in doc and "pystoi" in doc and "unpinned" in doc and "PESQ" in doc
