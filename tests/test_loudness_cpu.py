"""BS.1770-4 loudness and the clip pool's host logic without a GPU: the K-weighting table against the standard's printed digits, the
float64 oracle of tests/loudness_cases.py against the standard's calibration tone, the condition the shared case list has to meet, the
float64 oracle's own rounding where only the filter rings, the draw order and the accept rule of
ClipPool.sample, metrics.Loudness on CPU tensors, and the exports."""
import os
import re

import numpy as np
import pytest
import torch

import loudness_cases as lc
from waveverify_amd import _lib, loudness as L
from waveverify_amd.metrics import Loudness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("wv_loudness", "wv_loudness_workspace_bytes", "wv_loudness_chunk", "wv_pool_sample")
BS1770_48K = ((1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585),
              (1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621))


def test_the_48_khz_table_is_the_standards():
    for table in (L.k_weighting(48000), lc.sos(48000)):
        assert table.shape == (2, 6) and np.abs(table - np.array(BS1770_48K)).max() < 1e-12
    for fs in (16000, 44100, 48000):
        assert np.array_equal(L.k_weighting(fs), lc.sos(fs))
    poles = [np.abs(np.roots(row[3:])).max() for row in L.k_weighting(16000)]
    assert abs(poles[0] - 0.628) < 1e-3 and abs(poles[1] - 0.985) < 1e-3


def test_the_oracle_reads_the_calibration_tone():
    """A full-scale 997 Hz sine reads -3.01 LUFS (BS.1770: 0 dB FS 997 Hz in one channel); at 16 kHz the bilinear warp of the shelf
    moves it, within EBU Tech 3341's meter tolerance of 0.1 LU."""
    at48 = lc.loudness(np.sin(2 * np.pi * 997.0 * np.arange(5 * 48000) / 48000), 48000)
    at16 = lc.loudness(np.sin(2 * np.pi * 997.0 * np.arange(5 * 16000) / 16000), 16000)
    print(f"MEASURE 997 Hz full scale: {at48:.4f} LUFS at 48 kHz, {at16:.4f} LUFS at 16 kHz")
    assert abs(at48 - (-3.01)) <= 0.01
    assert abs(at16 - at48) <= 0.1


def test_no_gate_decision_of_the_case_list_can_turn_on_rounding():
    """Every block of every case is at least 1e-6 LU away from the absolute gate and from its window's relative gate."""
    assert [(k.fs, k.T) for k in lc.cases()] == list(lc.SHAPES)
    nearest = np.inf
    for k in lc.cases():
        assert {"noise", "quiet_half_1e-3", "quiet_half_1e-2", "sine997", "zeros", "half_valid", "impulse@0", f"impulse@{k.T - 1}",
                f"impulse@{lc.chunk() - 1}", f"impulse@{lc.chunk()}", f"impulse@{lc.chunk() + 1}"} <= set(k.labels)
        for label, o in zip(k.labels, lc.reference(k.name)):
            d = np.abs(o["l"] - (-70.0)).min()
            if o["relative_gate"] is not None:
                d = min(d, np.abs(o["l"] - o["relative_gate"]).min())
            assert d >= 1e-6, (k.name, label, d)
            nearest = min(nearest, d)
    print(f"MEASURE nearest block to a gate over the case list: {nearest:.3e} LU")


def test_the_cases_exercise_both_gates_and_the_floor():
    k = next(k for k in lc.cases() if k.name == "fs16000_T16000")
    ref = dict(zip(k.labels, lc.reference(k.name)))
    assert ref["zeros"]["lufs"] == -70.0 == L.MIN_LOUDNESS
    l, gate = ref["quiet_half_1e-3"]["l"], ref["quiet_half_1e-3"]["relative_gate"]
    assert (l < -70.0).any() and (l > gate).any()                                # the absolute gate removes blocks
    l, gate = ref["quiet_half_1e-2"]["l"], ref["quiet_half_1e-2"]["relative_gate"]
    assert ((l > -70.0) & (l < gate)).any()                                      # the relative gate removes blocks the absolute one kept
    # white noise at rms 0.1 is -20.691 unweighted; the shelf lifts what lies above 1.7 kHz by up to 4 dB
    assert -20.8 < ref["noise"]["lufs"] < -16.6 and ref["half_valid"]["lufs"] != ref["noise"]["lufs"]
    short = next(k for k in lc.cases() if k.name == "fs16000_T6401")
    assert dict(zip(short.labels, lc.reference(short.name)))["impulse@6400"]["lufs"] == -70.0    # behind the last whole sub-block


def test_the_oracles_own_rounding_where_only_the_filter_rings():
    """How far the float64 oracle is from the same recurrence in extended precision: an impulse's ringing at 16 kHz, sub-block by
    sub-block.  Driven sub-blocks agree to 1e-15; in the ringing ones float64 itself is 1e-11 .. 3e-10 off, more than the GPU test's relative 1e-11 on
    `sub`: that bar holds there only for a kernel that keeps the oracle's own order of operations, which is why wv_loudness does."""
    if np.finfo(np.longdouble).eps > 1e-18:
        return                                                                   # no extended precision on this platform: nothing to measure
    fs, T, h = 16000, 16000, 1600
    c = [[np.longdouble(v) for v in row] for row in lc.sos(fs)]
    y, s = np.zeros(T, np.longdouble), [[np.longdouble(0)] * 2, [np.longdouble(0)] * 2]
    for t in range(T):
        v = np.longdouble(1.0 if t == 0 else 0.0)
        for k in range(2):
            b0, b1, b2, _, a1, a2 = c[k]
            o = b0 * v + s[k][0]
            s[k] = [b1 * v - a1 * o + s[k][1], b2 * v - a2 * o]
            v = o
        y[t] = v
    x = np.zeros(T)
    x[0] = 1.0
    true = (y.reshape(T // h, h) ** 2).sum(axis=1)
    rel = np.array(np.abs(lc.oracle(x, fs)["sub"] - true) / true, np.float64)
    print("MEASURE float64 oracle against 80-bit, impulse at 0, per sub-block:", " ".join(f"{v:.1e}" for v in rel))
    assert rel[0] < 1e-14 and rel.max() < 1e-8


# ---- the host route's own recurrence ------------------------------------------------------------------------------------------------
def test_the_numpy_recurrence_is_scipys_bit_for_bit():
    pytest.importorskip("scipy.signal")
    from scipy.signal import sosfilt
    x = 0.1 * np.random.default_rng(5).standard_normal((3, 700))
    assert np.array_equal(L._sosfilt_rows(L.k_weighting(16000), x), sosfilt(L.k_weighting(16000), x, axis=-1))


# ---- ClipPool.sample's host side ---------------------------------------------------------------------------------------------------
def _draw_restated(seed, lengths, B, T, tries):
    rng = np.random.default_rng(seed)
    c = rng.integers(len(lengths), size=B)
    u = rng.random((B, tries))
    offset = np.array([[int(np.floor(u[b, k] * (max(lengths[c[b]] - T, 0) + 1))) for k in range(tries)] for b in range(B)])
    return c, offset, np.array([min(lengths[i], T) for i in c])


def test_the_draw_order_is_the_documented_one():
    lengths = [48000, 16000, 9000, 100000]
    for seed in (0, 1, 7):
        c, off, lens = L.draw(np.random.default_rng(seed), np.array(lengths), 6, 16000, 8)
        wc, woff, wlens = _draw_restated(seed, lengths, 6, 16000, 8)
        assert np.array_equal(c, wc) and np.array_equal(off, woff) and np.array_equal(lens, wlens)
        assert off.shape == (6, 8) and (off >= 0).all() and (off + lens[:, None] <= np.array(lengths)[c][:, None]).all()
        assert (off[np.array(lengths)[c] <= 16000] == 0).all()                   # a clip no longer than T has one place to start
    # numpy's PCG64 stream for seed 0, pinned: clip first, then the offsets
    c, off, _ = L.draw(np.random.default_rng(0), np.array(lengths), 6, 16000, 8)
    rng = np.random.default_rng(0)
    assert c.tolist() == rng.integers(4, size=6).tolist()
    assert off[0].tolist() == np.floor(rng.random((6, 8))[0] * (lengths[c[0]] - 16000 + 1 if lengths[c[0]] > 16000 else 1)).astype(int).tolist()
    assert "rng.integers(len(pool), size=B)" in __import__("waveverify_amd.data", fromlist=["ClipPool"]).ClipPool.sample.__doc__


def test_the_accept_rule_first_strictly_above_else_last():
    lufs = np.array([[-50.0, -30.0, -20.0, -60.0],         # second try
                     [-39.0, -10.0, -10.0, -10.0],         # first try
                     [-50.0, -41.0, -70.0, -45.0],         # none above: the last
                     [-40.0, -40.0, -40.0, -39.999],       # equality is not above
                     [-40.0, -40.0, -40.0, -40.0]])        # equality everywhere: the last
    assert L.choose(lufs, -40.0).tolist() == [1, 0, 3, 3, 3]
    assert L.choose(lufs[:, :1], -40.0).tolist() == [0] * 5
    doc = __import__("waveverify_amd.data", fromlist=["ClipPool"]).ClipPool.sample.__doc__
    assert "strictly above" in doc and "LAST try" in doc and "unpinned" in doc


# ---- metrics.Loudness on the CPU ---------------------------------------------------------------------------------------------------
def test_loudness_on_cpu_tensors_equals_the_oracle():
    k = next(k for k in lc.cases() if k.name == "fs16000_T16001")
    full = [n for n in range(len(k.x)) if k.lens[n] == k.T]
    m = Loudness()
    got = m(torch.from_numpy(k.x[full])[:, None], k.fs)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(full),) and not got.is_cuda
    want = np.array([lc.reference(k.name)[n]["lufs"] for n in full])
    assert np.abs(got.numpy() - want).max() <= 1e-9
    assert np.abs(m.last_sub.numpy() - np.stack([lc.reference(k.name)[n]["sub"] for n in full])).max() <= 1e-9
    assert float(Loudness().mean(torch.from_numpy(k.x[full])[:, None], k.fs)) == pytest.approx(want.mean(), abs=1e-9)
    half = next(n for n in range(len(k.x)) if k.labels[n] == "half_valid")
    assert abs(L.loudness_numpy(k.x[half], k.fs, length=int(k.lens[half])) - lc.reference(k.name)[half]["lufs"]) <= 1e-9
    at48 = next(k for k in lc.cases() if k.fs == 48000)
    assert abs(float(Loudness()(torch.from_numpy(at48.x[3:4])[:, None], 48000)[0]) - lc.reference(at48.name)[3]["lufs"]) <= 1e-9


def test_too_short_and_a_rate_without_100_ms_sub_blocks_raise():
    x = torch.zeros(2, 1, 6399)
    with pytest.raises(ValueError):
        Loudness()(x, 16000)                                                     # T < 4 h
    assert float(Loudness()(torch.zeros(1, 1, 6400), 16000)[0]) == -70.0
    with pytest.raises(ValueError):
        Loudness()(torch.zeros(1, 1, 22055), 22055)                              # fs % 10
    with pytest.raises(ValueError):
        Loudness()(torch.zeros(2, 6400), 16000)
    for fn in (L.sub_block, L.k_weighting):
        with pytest.raises(ValueError):
            fn(22055)
    with pytest.raises(ValueError):
        lc.oracle(np.zeros(6399), 16000)
    with pytest.raises(ValueError):
        lc.oracle(np.zeros(22055), 22055)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    lib = _lib.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES and getattr(lib, name) is not None
    c = lib.wv_loudness_chunk()
    assert 1 <= c <= 1600                                                        # a chunk is no longer than a sub-block at 16 kHz
    n = lib.wv_loudness_workspace_bytes(512, 16000, 16000)
    assert n > 0 and n % 256 == 0
    for bad in ((0, 16000, 16000), (4, 6399, 16000), (4, 22055, 22055), (4, 16000, 0), (4, 16000, -10)):
        assert lib.wv_loudness_workspace_bytes(*bad) == 0, bad
    zero = {_lib.C.c_int: 0, _lib.C.c_size_t: 0, _lib.C.c_double: 0.0}
    for name in ("wv_loudness", "wv_pool_sample"):
        assert getattr(lib, name)(*[zero.get(t) for t in _lib.SIGNATURES[name][1]]) == -1
        assert name.encode() in lib.wv_last_error() and b"null pointer" in lib.wv_last_error()


def test_the_docs_state_the_rules():
    from waveverify_amd.train import WatermarkTrainer
    assert "loudness=True" in WatermarkTrainer.validate.__doc__ and "unpinned" in WatermarkTrainer.validate.__doc__
    assert "pool.sample" in WatermarkTrainer.fit.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 7i."):]
    for word in ("unpinned", "rng.integers", "strictly above", "MIN_LOUDNESS"):
        assert word in section, word
