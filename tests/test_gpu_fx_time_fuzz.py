"""Every entry point of csrc/wv_fx_time.hip against the oracle of its operation (oracle/wv_oracle_fx_time.py), on the case lists of
tests/fx_time_cases.py (whose edges and discriminating power tests/test_fx_time_cases_cpu.py checks without a GPU).  Every case goes
through the wrappers of waveverify_amd/effects.py, or through the C ABI where an operand has to be misaligned.

EQUAL: the pointwise pass and shush bit for bit (NaN where the oracle has NaN), the median and scatter-zero by value, smooth's mask, and
smooth's audio where w is a power of two (the data are multiples of 2^-10 below 1 there, so every order of summation is exact).
BARS, each the float32 roundings a sample passes on the device, eps = 2^-24:
    echo forward      8 eps of max|x|          (volume * x, the add, the same two inside max|c|, the divide, the multiply: six)
    echo gradient     2e-5 of the gradient's peak (DESIGN section 7c's bar for this kernel)
    smooth            (w + 2) eps of max|x|    (1 / w, w products and a sequential sum of w terms)
    smooth transpose  3 (w + 2) eps of max|g|  (up to three such sums per sample: the interior and the two folded pads)
    stretch           4 eps of max|x|          (three roundings in the blend; the coordinate is the oracle's bit for bit)
Every test prints its worst measured error."""
import ctypes as C

import numpy as np
import pytest
import torch

import fx_time_cases as K
from oracle import wv_oracle_fx_time as O
from waveverify_amd import _lib
from waveverify_amd import effects as E

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
GRAD_BAR = 2e-5
WV_EINVAL = -1


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits_equal(got, want):
    """Bit for bit, except that any NaN matches a NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max())


def by(cases, key):
    return sorted({c[key] for c in cases})


def off_by_one_float(a):
    """`a` on the device, its first element one float past a 16-byte boundary."""
    n = int(np.prod(a.shape))
    buf = torch.empty(n + 8, dtype=torch.float32, device="cuda")
    v = buf[1: 1 + n].view(a.shape)
    if isinstance(a, np.ndarray):
        v.copy_(cu(a))
    assert v.data_ptr() % 16 == 4
    return v


# ---- pointwise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", by(K.POINTWISE, "op"))
def test_pointwise_is_the_oracle_bit_for_bit(op):
    lib, bad = _lib.load(), []
    for c in (c for c in K.POINTWISE if c["op"] == op):
        x, noise = K.pointwise_inputs(c)
        want = O.pointwise(x, op, c["a"], noise)
        if c["offset"]:
            xd, zd, yd = off_by_one_float(x), off_by_one_float(noise), off_by_one_float(np.empty_like(x))
            yd.fill_(float("nan"))
            _lib.check(lib.wv_fx_pointwise(xd.data_ptr(), zd.data_ptr(), yd.data_ptr(), c["rows"], c["T"], op, float(c["a"]), _lib.stream()), "wv_fx_pointwise")
            got = host(yd)
        else:
            got = host(E.pointwise(cu(x), op, c["a"], cu(noise)))
        if not bits_equal(got, want):
            bad.append((c["id"], int((got.view(np.uint32) != want.view(np.uint32)).sum())))
    print(f"pointwise op {op}: {sum(c['op'] == op for c in K.POINTWISE)} cases, differing (case, samples): {bad}")
    assert not bad, bad


# ---- median --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", by(K.MEDIAN, "k"))
def test_median_is_the_oracle(k):
    bad, worst = [], 0.0
    for c in (c for c in K.MEDIAN if c["k"] == k):
        x = K.median_inputs(c)
        got, want = host(E.median(cu(x), k)), O.median(x, k)
        worst = max(worst, err(got, want.astype(np.float64)))
        if not np.array_equal(got, want):
            bad.append(c["id"])
    print(f"median k={k}: worst |d| {worst:.3g}, differing: {bad}")
    assert not bad, bad


# ---- shush ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.SHUSH_KINDS)
def test_shush_is_the_oracle_bit_for_bit(kind):
    bad = []
    for c in (c for c in K.SHUSH if c["kind"] == kind):
        x, mask = K.shush_inputs(c)
        y, keep, mo = E.shush_forward(cu(x), c["k"], cu(mask))
        wy, wkeep, wmo = O.shush(x, c["k"], mask)
        ok = bits_equal(host(y), wy) and bits_equal(host(keep), wkeep) and ((mo is None and wmo is None) or bits_equal(host(mo), wmo))
        if not ok:
            bad.append((c["id"], int((host(keep) != wkeep).sum())))
    print(f"shush {kind}: {sum(c['kind'] == kind for c in K.SHUSH)} cases, differing (case, keep entries): {bad}")
    assert not bad, bad


# ---- echo ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.ECHO, ids=[c["id"] for c in K.ECHO])
def test_echo_forward_is_within_six_roundings_of_the_oracle(c):
    x, _ = K.echo_inputs(c)
    got = host(E.echo_forward(cu(x), c["n"], c["volume"])[0])
    e, peak = err(got, O.echo(x, c["n"], c["volume"])), float(np.abs(x).max())
    print(f"echo forward {c['id']}: |d| {e:.3g} = {e / max(peak, 1e-300) / EPS:.3g} eps of max|x|")
    assert not got[:, c["T"] - c["n"] + 1:].any(), "the tail is 0"
    assert e <= 8 * EPS * peak, (e, peak)


@pytest.mark.parametrize("c", K.ECHO, ids=[c["id"] for c in K.ECHO])
def test_echo_gradient_is_the_reference_autograd(c):
    x, g = K.echo_inputs(c)
    xd = cu(x)
    _, rec = E.echo_forward(xd, c["n"], c["volume"])
    got = host(E.echo_backward(xd, cu(g), rec, c["n"], c["volume"]))
    want = O.echo_gradient(x, g, c["n"], c["volume"])
    e, peak = err(got, want), float(np.abs(want).max())
    print(f"echo gradient {c['id']}: |d| {e:.3g} = {e / max(peak, 1e-300):.3g} of the gradient's peak")
    assert e <= GRAD_BAR * peak, (e, peak)


# ---- smooth and its transpose --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", by(K.SMOOTH, "w"))
def test_smooth_is_the_oracle(w):
    bad, worst = [], 0.0
    for c in (c for c in K.SMOOTH if c["w"] == w):
        x, _, mask = K.smooth_inputs(c)
        y, mo = E.smooth_forward(cu(x), w, cu(mask), c["thr"])
        wy, wmo = O.smooth(x, w, mask, c["thr"])
        e, peak = err(host(y), wy), float(np.abs(x).max())
        worst = max(worst, e / peak / EPS)
        if not (e == 0.0 if c["dyadic"] else e <= (w + 2) * EPS * peak):
            bad.append((c["id"], "audio", e))
        if (mo is None) != (wmo is None) or (mo is not None and not np.array_equal(host(mo), wmo)):
            bad.append((c["id"], "mask", int((host(mo) != wmo).sum())))
    print(f"smooth w={w}: worst {worst:.3g} eps of max|x| (bar {0 if (w & (w - 1)) == 0 else w + 2}), failing: {bad}")
    assert not bad, bad


@pytest.mark.parametrize("w", by(K.SMOOTH, "w"))
def test_smooth_backward_is_the_transposed_oracle(w):
    bad, worst = [], 0.0
    for c in (c for c in K.SMOOTH if c["w"] == w and c["mask"] == "none"):
        _, g, _ = K.smooth_inputs(c)
        e, peak = err(host(E.smooth_backward(cu(g), w)), O.smooth_transpose(g, w)), float(np.abs(g).max())
        worst = max(worst, e / peak / EPS)
        if e > 3 * (w + 2) * EPS * peak:
            bad.append((c["id"], e))
    print(f"smooth transpose w={w}: worst {worst:.3g} eps of max|g| (bar {3 * (w + 2)}), failing: {bad}")
    assert not bad, bad


# ---- scatter-zero --------------------------------------------------------------------------------------------------------------------
def test_scatter_zero_is_the_oracle_and_skips_indices_outside_the_row():
    bad = []
    for c in K.SCATTER:
        y, mask, idx = K.scatter_inputs(c)
        yd, md = cu(y), cu(mask)
        E.scatter_zero(yd, cu(idx), md)
        wy, wm = O.scatter_zero(y, mask, idx)
        if not (bits_equal(host(yd), wy) and (md is None or bits_equal(host(md), wm))):
            bad.append(c["id"])
    print(f"scatter-zero: {len(K.SCATTER)} cases, differing: {bad}")
    assert not bad, bad


# ---- stretch -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.STRETCH, ids=[c["id"] for c in K.STRETCH])
def test_stretch_is_within_three_roundings_of_the_oracle(c):
    x = K.stretch_inputs(c)
    e, peak = err(host(E.stretch_linear(cu(x), c["t_out"])), O.stretch(x, c["t_out"])), float(np.abs(x).max())
    print(f"stretch {c['id']}: |d| {e:.3g} = {e / peak / EPS:.3g} eps of max|x|")
    assert e <= 4 * EPS * peak, (e, peak)


# ---- the row limit -------------------------------------------------------------------------------------------------------------------
def test_the_largest_row_count_runs_every_grid_row():
    """rows = 65535, the most the ABI accepts, for the entry points whose launch grid carries the rows."""
    x, mask, idx = K.row_limit_inputs()
    xd, md, T = cu(x), cu(mask), K.ROW_LIMIT_T
    ok = {"median": np.array_equal(host(E.median(xd, 3)), O.median(x, 3))}
    y, keep, mo = E.shush_forward(xd, 1, md)
    wy, wkeep, wmo = O.shush(x, 1, mask)
    ok["shush"] = bits_equal(host(y), wy) and bits_equal(host(keep), wkeep) and bits_equal(host(mo), wmo)
    y, mo = E.smooth_forward(xd, 2, md, 0.5)
    wy, wmo = O.smooth(x, 2, mask, 0.5)
    ok["smooth"] = err(host(y), wy) == 0.0 and np.array_equal(host(mo), wmo)                                 # quarters: the sums are exact
    ok["smooth_backward"] = err(host(E.smooth_backward(xd, 2)), O.smooth_transpose(x, 2)) == 0.0
    yd, sd = xd.clone(), md.clone()
    E.scatter_zero(yd, cu(idx), sd)
    wy, wm = O.scatter_zero(x, mask, idx)
    ok["scatter_zero"] = bits_equal(host(yd), wy) and bits_equal(host(sd), wm)
    e = err(host(E.stretch_linear(xd, 4)), O.stretch(x, 4))
    ok["stretch"] = e <= 4 * EPS * float(np.abs(x).max())
    print(f"rows = {K.MAX_ROWS}, T = {T}: {ok}, stretch |d| {e:.3g}")
    assert tuple(ok) == K.GRID_ROW_ENTRY_POINTS and all(ok.values()), ok


def test_one_row_more_is_refused_by_every_entry_point():
    """rows = 65536 returns WV_EINVAL.  The buffers are large enough for that many rows, so a call that was not refused stays in bounds."""
    lib, R, T, s = _lib.load(), K.MAX_ROWS + 1, K.ROW_LIMIT_T, None
    a, b, c, d, e = (torch.zeros(R, T + 1, device="cuda") for _ in range(5))
    idx = torch.zeros(R, 2, dtype=torch.int32, device="cuda")
    rec = torch.zeros(2, dtype=torch.int64, device="cuda")
    nbytes = int(lib.wv_fx_echo_backward_workspace_bytes())
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    calls = {
        "pointwise": lambda r: lib.wv_fx_pointwise(p(a), p(b), p(c), r, T, E.OP_ADD_NOISE, 0.5, s),
        "median": lambda r: lib.wv_fx_median(p(a), p(c), r, T, 3, s),
        "shush": lambda r: lib.wv_fx_shush(p(a), p(b), p(c), p(d), p(e), r, T, 1, s),
        "echo_peaks": lambda r: lib.wv_fx_echo_peaks(p(a), p(rec), r, T, 2, 0.5, s),
        "echo_apply": lambda r: lib.wv_fx_echo_apply(p(a), p(rec), p(c), r, T, 2, 0.5, s),
        "echo_backward": lambda r: lib.wv_fx_echo_backward(p(a), p(b), p(rec), p(c), r, T, 2, 0.5, p(ws), nbytes, s),
        "smooth": lambda r: lib.wv_fx_smooth(p(a), p(b), p(c), p(d), r, T, 2, 0.5, s),
        "smooth_backward": lambda r: lib.wv_fx_smooth_backward(p(a), p(c), r, T, 2, s),
        "scatter_zero": lambda r: lib.wv_fx_scatter_zero(p(c), p(d), p(idx), r, T, 2, s),
        "stretch": lambda r: lib.wv_fx_stretch_linear(p(a), p(c), r, T, T + 1, s),
    }
    got = {name: (call(R), call(R - 1)) for name, call in calls.items()}
    torch.cuda.synchronize()
    print("rows = 65536 / 65535 ->", got)
    assert all(v == (WV_EINVAL, 0) for v in got.values()), got
