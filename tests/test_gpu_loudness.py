"""BS.1770-4 loudness on the GPU (csrc/wv_loudness.hip) against the float64 oracle of tests/loudness_cases.py, through the C ABI with
guard bands round every output, the input arena checked unchanged and a poisoned workspace: the K-weighted signal, the sub-block
energies and the loudness of every case, then the contract -- bit-equal runs, a window's bits independent of N and of its row,
overlapping windows, nothing read past a window's own length, bad arguments refused with nothing written.

Bars (none taken from what the kernel gives):
    filtered  1 f32 ulp of the oracle's value + 1e-12: the state is f64, the only f32 rounding is the final store
    sub       relative 1e-11: both sides are f64 sums of the same squares in another order (the kernel keeps sosfilt's own order of
              operations in the recurrence: see csrc/wv_loudness.hip for what any other order costs)
    lufs      1e-9 LU: both sides are f64 on identical f32 inputs and differ in summation order and in the state propagation, a relative
              error of order 1e-12; d(10 log10 z) = 4.34 dz / z, so about 4e-12 LU, with two orders of margin"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import loudness_cases as lc
from guard import Guards
from waveverify_amd import _lib, loudness as L

pytestmark = pytest.mark.gpu

LUFS_BAR = 1e-9
SUB_RTOL = 1e-11
NAMES = [f"fs{fs}_T{T}" for fs, T in lc.SHAPES]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(fs):
    return L.k_weighting(fs).reshape(-1).copy()


def _call(arena, starts, lens, T, fs, filtered=True, offset=1):
    """One wv_loudness call on a flat float32 arena with everything guarded -> dict of host arrays (f64 outputs wrapped as int64 words)."""
    lib = _lib.load()
    N = len(starts)
    g = Guards(offset=offset)
    pool = g.input(np.asarray(arena, np.float32), "pool")
    st = g.input(np.asarray(starts, np.int64), "starts", offset=0)
    ln = g.input(np.asarray(lens, np.int32), "lens")
    tab = g.input(_table(fs).view(np.int64), "table", offset=0)
    lufs = g.output((N,), torch.int64, "lufs")
    sub = g.output((N, T // (fs // 10)), torch.int64, "sub")
    filt = g.output((N, T), torch.float32, "filtered") if filtered else None
    ws = g.workspace(int(lib.wv_loudness_workspace_bytes(N, T, fs)))
    rc = lib.wv_loudness(pool.t.data_ptr(), st.t.data_ptr(), ln.t.data_ptr(), N, T, fs, tab.t.data_ptr(), lufs.t.data_ptr(), sub.t.data_ptr(),
                         None if filt is None else filt.t.data_ptr(), ws.t.data_ptr(), ws.n, _stream())
    assert rc == 0, lib.wv_last_error()
    g.check()
    out = {"lufs": lufs.t.clone().view(torch.float64).cpu().numpy(), "sub": sub.t.clone().view(torch.float64).cpu().numpy()}
    if filtered:
        out["filtered"] = filt.t.cpu().numpy()
    return out


def _case(name):
    return next(k for k in lc.cases() if k.name == name)


@lru_cache(maxsize=None)
def _batch(name):
    k = _case(name)
    return _call(k.x.reshape(-1), np.arange(len(k.x)) * k.T, k.lens, k.T, k.fs)


@pytest.mark.parametrize("name", NAMES)
def test_filtered_and_lufs_against_the_oracle(name):
    k, got, want = _case(name), _batch(name), lc.reference(name)
    worst_f = worst_l = 0.0
    for n, o in enumerate(want):
        ref = o["filtered"]
        bar = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-12
        err = np.abs(got["filtered"][n].astype(np.float64) - ref)
        worst_f = max(worst_f, float((err / bar).max()))
        worst_l = max(worst_l, abs(got["lufs"][n] - o["lufs"]))
        assert (err <= bar).all(), (name, k.labels[n], int(np.argmax(err / bar)), float((err / bar).max()))
        assert abs(got["lufs"][n] - o["lufs"]) <= LUFS_BAR, (name, k.labels[n], got["lufs"][n], o["lufs"])
    print(f"MEASURE {name}: filtered max err / (1 ulp + 1e-12) = {worst_f:.3f}, lufs max |gpu - f64| = {worst_l:.2e} LU (bar {LUFS_BAR:.0e})")
    zeros = k.labels.index("zeros")
    assert got["lufs"][zeros] == -70.0 and not got["sub"][zeros].any() and not got["filtered"][zeros].any()


def _ringing(label):
    """Windows whose input falls silent before their end: the sub-blocks behind it hold the filter's ringing alone."""
    return label == "half_valid" or label.startswith("impulse@")


@pytest.mark.parametrize("ringing", [False, True], ids=["driven", "ringing"])
@pytest.mark.parametrize("name", NAMES)
def test_sub_block_energies_against_the_oracle(name, ringing):
    """Relative 1e-11 on every sub-block the oracle holds a non-zero energy for; exact zero where it holds zero.  `ringing` are the
    windows whose input stops (half_valid, impulses): their later sub-blocks hold the filter's ringing alone, where the float64 oracle is
    itself 1e-11 .. 3e-10 from 80-bit arithmetic (test_loudness_cpu.py measures it) and only its own order of operations reproduces it."""
    k, got, want = _case(name), _batch(name), lc.reference(name)
    worst, where = 0.0, None
    for n, o in enumerate(want):
        if _ringing(k.labels[n]) != ringing:
            continue
        live = o["sub"] > 0
        assert not got["sub"][n][~live].any(), (name, k.labels[n])
        rel = np.abs(got["sub"][n] - o["sub"])[live] / o["sub"][live]
        if rel.size and rel.max() > worst:
            worst, where = float(rel.max()), (k.labels[n], int(np.nonzero(live)[0][int(np.argmax(rel))]))
    print(f"MEASURE {name} {'ringing' if ringing else 'driven'}: sub max |gpu - f64| / f64 = {worst:.2e} at {where} (bar {SUB_RTOL:.0e})")
    assert worst <= SUB_RTOL, (name, where, worst)


@pytest.mark.parametrize("name", ["fs16000_T16001", "fs44100_T22050"])
def test_runs_are_bit_equal_with_and_without_filtered_alone_and_as_row_2_of_3(name):
    k, first = _case(name), _batch(name)
    N = len(k.x)
    again = _call(k.x.reshape(-1), np.arange(N) * k.T, k.lens, k.T, k.fs)
    for key in first:
        assert np.array_equal(first[key], again[key]), key
    bare = _call(k.x.reshape(-1), np.arange(N) * k.T, k.lens, k.T, k.fs, filtered=False, offset=0)      # NULL: never written, same numbers
    assert set(bare) == {"lufs", "sub"} and np.array_equal(bare["lufs"], first["lufs"]) and np.array_equal(bare["sub"], first["sub"])
    for n in (0, 1, 5, N - 1):
        alone = _call(k.x[n], [0], k.lens[n:n + 1], k.T, k.fs)
        rows = [(n + 3) % N, (n + 7) % N, n]                                     # the same window as row 2 of 3
        three = _call(k.x[rows].reshape(-1), np.arange(3) * k.T, k.lens[rows], k.T, k.fs)
        for key in first:
            assert np.array_equal(alone[key][0], first[key][n]) and np.array_equal(three[key][2], first[key][n]), (key, n)


def test_overlapping_windows_of_one_arena_give_what_disjoint_copies_give():
    fs, T = 16000, 8000
    arena = (0.1 * np.random.default_rng(3).standard_normal(2 * T)).astype(np.float32)
    starts = np.array([0, 1, 100, T // 2, T - 1, T], np.int64)
    lens = np.array([T, T, T - 7, T, T // 3, T], np.int32)
    over = _call(arena, starts, lens, T, fs)
    copies = np.stack([arena[s: s + T] for s in starts])
    apart = _call(copies.reshape(-1), np.arange(len(starts)) * T, lens, T, fs)
    for key in over:
        assert np.array_equal(over[key], apart[key]), key
    for n, s in enumerate(starts):
        assert abs(over["lufs"][n] - lc.loudness(arena[s: s + T], fs, int(lens[n]))) <= LUFS_BAR


def test_nothing_is_read_past_a_windows_own_length():
    """The arena's last clip ends where the guard band (NaN) begins and its window reaches T // 2 samples into it; lens past T and
    under 0 are clamped."""
    fs, T = 16000, 16000
    clip = (0.1 * np.random.default_rng(4).standard_normal(T // 2)).astype(np.float32)
    got = _call(clip, [0, 0, T // 4], [T // 2, -5, T // 4], T, fs)
    assert np.isfinite(got["filtered"]).all() and np.isfinite(got["sub"]).all()
    padded = np.concatenate([clip, np.zeros(T // 2, np.float32)])
    assert abs(got["lufs"][0] - lc.loudness(padded, fs)) <= LUFS_BAR
    assert got["lufs"][1] == -70.0 and not got["filtered"][1].any()
    assert abs(got["lufs"][2] - lc.loudness(np.concatenate([clip[T // 4:], np.zeros(3 * T // 4, np.float32)]), fs)) <= LUFS_BAR
    k = _case("fs16000_T16000")
    half = k.labels.index("half_valid")                                          # live noise behind lens inside the arena: not read either
    assert _batch(k.name)["lufs"][half] != _batch(k.name)["lufs"][k.labels.index("noise")]


def test_bad_arguments_return_minus_1_name_the_call_and_write_nothing():
    lib = _lib.load()
    fs, T, N = 16000, 6400, 2
    g = Guards()
    pool = g.input(np.zeros(N * T, np.float32), "pool")
    st = g.input(np.arange(N, dtype=np.int64) * T, "starts")
    ln = g.input(np.full(N, T, np.int32), "lens")
    tab = g.input(_table(fs).view(np.int64), "table")
    lufs, sub = g.output((N,), torch.int64, "lufs"), g.output((N, 4), torch.int64, "sub")
    filt = g.output((N, T), torch.float32, "filtered")
    ws = g.workspace(int(lib.wv_loudness_workspace_bytes(N, T, fs)))
    ok = [pool.t.data_ptr(), st.t.data_ptr(), ln.t.data_ptr(), N, T, fs, tab.t.data_ptr(), lufs.t.data_ptr(), sub.t.data_ptr(), filt.t.data_ptr(),
          ws.t.data_ptr(), ws.n, _stream()]

    def refused(**change):
        args = list(ok)
        for i, v in change.items():
            args[int(i[1:])] = v
        assert lib.wv_loudness(*args) == -1, change
        assert b"wv_loudness" in lib.wv_last_error(), lib.wv_last_error()

    for i in (0, 1, 2, 6, 7, 8):                                                 # NULL pool, starts, lens, table, lufs, sub
        refused(**{f"a{i}": None})
    refused(a3=0)                                                                # N = 0
    refused(a4=T - 1)                                                            # T < 4 h
    refused(a4=22055, a5=22055)                                                  # fs % 10
    refused(a5=0)
    refused(a10=None)                                                            # no workspace
    refused(a11=ws.n - 1)                                                        # a short workspace
    refused(a7=lufs.t.data_ptr() + 4)                                            # lufs off its 8 bytes
    torch.cuda.synchronize()
    for out in (lufs, sub, filt):
        out.check(expect_unwritten=torch.ones(out.shape, dtype=torch.bool))      # nothing written, guards intact
    for a in (pool, st, ln, tab, ws):
        a.check()
    assert (ws.t == 0xFF).all()
    assert lib.wv_loudness(*ok) == 0
    g.check()


def test_the_module_is_the_same_call_on_a_plain_batch():
    from waveverify_amd import metrics
    k = _case("fs16000_T16000")
    full = [n for n in range(len(k.x)) if k.lens[n] == k.T]
    m = metrics.Loudness()
    x = torch.from_numpy(k.x[full])[:, None].cuda()
    got = m(x, k.fs)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(full),)
    assert np.array_equal(got.cpu().numpy(), _batch(k.name)["lufs"][full]) and np.array_equal(m.last_sub.cpu().numpy(), _batch(k.name)["sub"][full])
    cpu = metrics.Loudness()(x.cpu(), k.fs).numpy()
    assert np.abs(cpu - got.cpu().numpy()).max() <= LUFS_BAR
    with pytest.raises(ValueError):
        m(x[..., :6399], k.fs)
    with pytest.raises(ValueError):
        m(x[:, 0], k.fs)
