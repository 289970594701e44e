"""The time-domain effects' oracle (oracle/wv_oracle_fx_time.py) and case lists (tests/fx_time_cases.py) on the CPU, no GPU:

a. the oracle reproduces what the REFERENCE recorded in tests/golden/effects_time.npz: bit for bit where the GPU test asks that of the
   kernels, within the fixture's 2e-5 of the peak for echo, smooth, the stretch pairs and their gradients;
b. median equals scipy.signal.medfilt and stretch is within 4 * 2^-24 of the peak of torch's CPU interpolate on every listed pair;
c. the lists hold every edge they are meant to hold;
d. the inputs discriminate: each plausible wrong variant restated below differs from the oracle, on at least one listed case, by more
   than the bar tests/test_gpu_fx_time_fuzz.py holds that kernel to."""
import json
import os

import numpy as np
import pytest
import torch

import fx_time_cases as K
from oracle import wv_oracle_fx_time as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "effects_time.npz"))
CASES = json.loads(str(GOLD["cases"]))
BAR = 2e-5                              # the fixture's bar (tests/test_gpu_effects_time.py)
EPS = 2.0 ** -24


def of(*names):
    got = [c for c in CASES if c["name"] in names]
    assert got, names
    return got


def rows2(a):
    return np.ascontiguousarray(a).reshape(-1, a.shape[-1])


def gold_inputs(c):
    T = c["T"]
    return rows2(GOLD[f"x_{T}"]), rows2(GOLD[f"mask_{T}"]), rows2(GOLD[f"r_{T}"])


def gold_grad(c, r):
    return r if f"{c['key']}_grad_is_r" in GOLD.files else rows2(GOLD[c["key"] + "_grad"])


def rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max() / max(1e-300, np.abs(ref).max()))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- a. the oracle against the reference's recorded outputs --------------------------------------------------------------------------
def test_oracle_reproduces_the_bit_exact_effects_of_the_fixture():
    for c in of("median_filter", "quantization", "amplitude_scaling", "shush", "sample_suppression", "pink_noise", "random_noise", "white_noise"):
        x, mask, r = gold_inputs(c)
        p, name, want_m, grad = c["params"], c["name"], mask, r
        if name == "median_filter":
            y = O.median(x, p["kernel_size"] + (p["kernel_size"] % 2 == 0))
        elif name == "quantization":
            y = O.pointwise(x, O.OP_QUANTIZE, 2 ** (p["bit_depth"] - 1) - 1)
        elif name == "amplitude_scaling":
            y, grad = O.pointwise(x, O.OP_SCALE, p["scale"]), O.pointwise(r, O.OP_SCALE, p["scale"])
        elif name == "shush":
            y, keep, want_m = O.shush(x, min(int(c["T"] * p["fraction"]), c["T"] - 1), mask)
            grad = O.pointwise(r, O.OP_MUL, 0.0, keep)
        elif name == "sample_suppression":
            idx = GOLD[c["key"] + "_idx"]
            (y, want_m), grad = O.scatter_zero(x, mask, idx), O.scatter_zero(r, None, idx)[0]
        else:
            y = O.pointwise(x, O.OP_ADD_NOISE, p["noise_std"], rows2(GOLD[c["key"] + "_noise"]))
        assert same(y, rows2(GOLD[c["key"] + "_y"])), (c, "audio")
        assert same(want_m, rows2(GOLD[c["key"] + "_m"])), (c, "mask")
        assert same(grad, gold_grad(c, r)), (c, "gradient")


def test_oracle_reproduces_echo_smooth_and_stretch_of_the_fixture():
    worst = {}
    for c in of("echo", "smooth"):
        x, mask, r = gold_inputs(c)
        if c["name"] == "echo":
            n, v = int(GOLD[c["key"] + "_n"]), float(GOLD[c["key"] + "_volume"])
            y, m, g = O.echo(x, n, v), mask, O.echo_gradient(x, r, n, v)
        else:
            w = int(GOLD[c["key"] + "_w"])
            (y, m), g = O.smooth(x, w, mask, c["params"].get("valid_threshold", 0.5)), O.smooth_transpose(r, w)
        ey, eg = rel(y, rows2(GOLD[c["key"] + "_y"])), rel(g, rows2(GOLD[c["key"] + "_grad"]))
        worst[c["name"]] = max(worst.get(c["name"], 0.0), ey, eg)
        assert same(m, rows2(GOLD[c["key"] + "_m"])), (c, "mask")
        assert ey <= BAR and eg <= BAR, (c, ey, eg)
    for tin, tout in GOLD["stretch"]:
        e = rel(O.stretch(rows2(GOLD[f"stretch_{tin}_{tout}_x"]), int(tout)), rows2(GOLD[f"stretch_{tin}_{tout}_y"]))
        worst["stretch"] = max(worst.get("stretch", 0.0), e)
        assert e <= BAR, (tin, tout, e)
    print("oracle vs fixture, worst of the peak:", {k: f"{v:.3g}" for k, v in worst.items()})


# ---- b. against scipy and torch ----------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:kernel_size exceeds volume extent")
def test_median_oracle_is_scipy_medfilt():
    from scipy.signal import medfilt
    for c in K.MEDIAN:
        x = K.median_inputs(c)
        want = np.stack([medfilt(row.astype(np.float64), c["k"]) for row in x])
        assert np.array_equal(O.median(x, c["k"]), want), c["id"]


def test_stretch_oracle_is_torch_interpolate():
    matched = {}
    for c in K.STRETCH:
        x = K.stretch_inputs(c)
        want = torch.nn.functional.interpolate(torch.from_numpy(x)[:, None], size=c["t_out"], mode="linear", align_corners=False)[:, 0].numpy()
        errs = {form: rel(O.stretch(x, c["t_out"], fused=(form == "fused")), want) for form in ("fused", "two roundings")}
        form = "fused" if errs["fused"] <= 4 * EPS else "two roundings"
        matched[c["id"]] = (form, f"{errs[form]:.3g}")
        assert errs[form] <= 4 * EPS, (c["id"], errs)           # a host whose torch does not fuse matches the two-roundings form instead
    print("torch CPU interpolate matches:", matched)


# ---- c. the lists hold the edges ---------------------------------------------------------------------------------------------------
def test_pointwise_cases_hold_the_edges():
    counts = {c["rows"] * c["T"] for c in K.POINTWISE}
    for op in (K.OP_SCALE, K.OP_ADD_NOISE, K.OP_QUANTIZE, K.OP_MUL):
        assert {1, 3, 4, 5, 1023, 1025} <= {c["rows"] * c["T"] for c in K.POINTWISE if c["op"] == op}, op
        assert any(c["op"] == op and c["offset"] == 0 and c["rows"] * c["T"] // 4 > 2048 * 256 and c["rows"] * c["T"] % 4 for c in K.POINTWISE)
        assert any(c["op"] == op and c["offset"] == 1 and c["rows"] * c["T"] > 2048 * 256 for c in K.POINTWISE)
    assert max(counts) * 4 <= 9.5e6
    q = [c for c in K.POINTWISE if c["op"] == K.OP_QUANTIZE]
    assert {0.0, 1.0, 127.0} <= {c["a"] for c in q}
    halves = [c for c in q if c["data"] == "halves"]
    assert halves and set(np.abs(K.pointwise_inputs(halves[0])[0]).ravel()) == {0.5, 1.5, 2.5}
    assert np.array_equal(O.pointwise(K.pointwise_inputs(halves[0])[0], O.OP_QUANTIZE, 1.0), [[0.0, -0.0, 2.0, -2.0, 2.0, -2.0]])
    zero = [c for c in q if c["a"] == 0.0]
    assert zero and np.isnan(O.pointwise(K.pointwise_inputs(zero[0])[0], O.OP_QUANTIZE, 0.0)).all()


def test_median_cases_hold_the_edges():
    assert {c["k"] for c in K.MEDIAN} == set(range(1, 32, 2)) | {33, 63, 255}
    for k in {c["k"] for c in K.MEDIAN}:
        assert {c["T"] for c in K.MEDIAN if c["k"] == k} == {1, 2, k // 2, k - 1, k, 255, 256, 257, 513} - {0}
    assert {c["rows"] for c in K.MEDIAN} == set(K.ROWS)
    for c in K.MEDIAN:
        x = K.median_inputs(c)
        assert np.array_equal(x, np.round(x * 4) / 4)
        if c["T"] >= 2:
            z = x[x == 0]
            assert np.signbit(z).any() and not np.signbit(z).all(), c["id"]
        if c["T"] >= 255:
            assert len(np.unique(x)) < 40                   # windows full of duplicates


def test_shush_cases_hold_the_edges():
    for kind in K.SHUSH_KINDS:
        mine = [c for c in K.SHUSH if c["kind"] == kind]
        assert {c["T"] for c in mine} == {t for t in K.SHUSH_TS if kind != "seam" or t >= 1025}
        for T in {c["T"] for c in mine}:
            assert {c["k"] for c in mine if c["T"] == T} == {0, 1, T // 2, T - 1} & set(range(T))
        assert {c["mask"] for c in mine} == {False, True} and {c["rows"] for c in mine} == set(K.ROWS)
    seen = set()
    for c in K.SHUSH:
        x, mask = K.shush_inputs(c)
        a = np.abs(x)
        assert x.dtype == np.float32 and x.shape == (c["rows"], c["T"]) and (mask is None) == (not c["mask"])
        if c["kind"] == "one_magnitude":
            assert len(np.unique(a)) == 1 and (c["T"] < 8 or len(np.unique(x)) == 2)
        elif c["kind"] == "zeros":
            assert not a.any() and (c["T"] < 8 or (np.signbit(x).any() and not np.signbit(x).all()))
        elif c["kind"] == "few_values":
            assert len(np.unique(a)) <= 12
        elif c["kind"] == "low_byte":
            b = a.view(np.uint32)
            assert len(np.unique(b >> 8)) == 1 and (c["T"] < 64 or len(np.unique(b)) > 16)
        elif c["kind"] == "subnormal":
            assert c["T"] < 8 or ((a > 0) & (a < np.finfo(np.float32).tiny)).any()
        else:
            tied, below, go = K.seam_plan(c["T"], c["k"])
            assert tied[0] == 1022 and tied[-1] >= 1024 and (a[:, tied] == 0.25).all() and (a == 0.25).sum() == c["rows"] * len(tied)
            assert ((a < 0.25).sum(1) == below).all() and 0 <= go < len(tied)
            if c["k"] >= 2:
                assert go == len(tied) - 1                 # the ordered count runs: some of the tied go, the one past the seam stays
                keep = O.shush(x, c["k"])[1]
                assert not keep[:, tied[:-1]].any() and keep[:, tied[-1]].all()
                seen.add(c["T"])
    assert seen == {1025, 2049}


def test_echo_cases_hold_the_edges():
    for T in K.ECHO_TS:
        for place in K.ECHO_PLACES:
            assert {c["n"] for c in K.ECHO if c["T"] == T and c["kind"] == place} == {2, 3, T // 2, T - 1, T} & set(range(2, T + 1)), (T, place)
    assert {c["volume"] for c in K.ECHO if not c["tied"]} >= {0.5, 0.25, 0.37, -0.4}
    assert {c["kind"] for c in K.ECHO} == set(K.ECHO_PLACES) | set(K.ECHO_TIES) | {"zero", "c_zero"}
    assert any(c["rows"] * c["T"] > 1024 * 1024 for c in K.ECHO) and max(c["rows"] * c["T"] for c in K.ECHO) * 4 <= 9.5e6
    tie_counts = {}
    for c in K.ECHO:
        x, g = K.echo_inputs(c)
        rows, T, n, kind = c["rows"], c["T"], c["n"], c["kind"]
        v, L = np.float32(c["volume"]), T - n + 1
        a = np.abs(x)
        cc = x[:, :L].astype(np.float64) + float(v) * x[:, n - 1:].astype(np.float64)
        ip = np.flatnonzero(a.ravel() == a.max())
        jp = np.argwhere(np.abs(cc) == np.abs(cc).max())
        if kind == "first":
            assert list(ip) == [0]
        elif kind == "last_tail":
            assert list(ip) == [rows * T - 1] and T - 1 >= L
        elif kind == "middle_row":
            assert len(ip) == 1 and 0 < ip[0] // T < rows - 1
        elif kind == "c_at_T_minus_n":
            assert len(jp) == 1 and jp[0][1] == T - n and len(ip) == 1
        elif kind == "zero":
            assert not x.any()
        elif kind == "c_zero":
            assert n == T and a.max() > 0 and not cc.any() and x[:, -1].all()
        if c["tied"]:
            assert np.array_equal(x * 256, np.round(x * 256)) and c["volume"] in (0.5, 0.25)
            assert np.array_equal(cc, (x[:, :L] + v * x[:, n - 1:]).astype(np.float64))        # c is exact in float32: a tie is a tie in both
            tie_counts.setdefault(kind, []).append((len(ip), len(jp)))
            if kind in ("x2", "x3"):
                assert len(ip) == int(kind[1]) and len(set(np.sign(x.ravel()[ip]))) == 2
            elif kind == "c2":
                assert len(jp) == 2 and len(set(np.sign(cc[tuple(jp.T)]))) == 2
            else:
                assert a.max() == 0.5 and len(ip) >= 3
    assert any(nx >= 9 for nx, _ in tie_counts["clipped"]) and any(nc >= 2 for _, nc in tie_counts["clipped"])


def test_smooth_cases_hold_the_edges():
    assert {c["w"] for c in K.SMOOTH} == {1, 2, 3, 7, 10, 255, 256, 257, 2048}
    for w in K.SMOOTH_WS:
        lo = w - 1 - (w - 1) // 2 + 1
        assert {c["T"] for c in K.SMOOTH if c["w"] == w} == {t for t in (lo, 255, 256, 257, 600) if t >= lo}
        assert {"none", "random"} <= {c["mask"] for c in K.SMOOTH if c["w"] == w}
        if w % 2 == 0:
            assert any(c["mask"] == "exact" and c["thr"] == 0.5 for c in K.SMOOTH if c["w"] == w)
    assert any(c["mask"] == "exact7" and c["thr"] == 0.7 and c["w"] == 10 for c in K.SMOOTH)
    for c in K.SMOOTH:
        x, g, mask = K.smooth_inputs(c)
        w = c["w"]
        if c["dyadic"]:
            assert w in (1, 2, 256, 2048) and np.abs(x).max() < 1 and np.array_equal(x * 1024, np.round(x * 1024)) and np.array_equal(g * 1024, np.round(g * 1024))
        if c["mask"] in ("exact", "exact7") and c["T"] >= 2 * w:
            full = np.lib.stride_tricks.sliding_window_view(mask, w, axis=1).sum(-1)
            assert (full == (7 if c["mask"] == "exact7" else w // 2)).all()                 # every full window sits on the threshold
            assert O.smooth(x, w, mask, c["thr"])[1][:, w: c["T"] - w].all()


def test_scatter_stretch_and_row_limit_cases_hold_the_edges():
    assert {(c["T"], c["num"]) for c in K.SCATTER} == {(1, 0), (1, 1), (300, 0), (300, 1), (300, 257), (300, 300)}
    assert {c["mask"] for c in K.SCATTER} == {False, True}
    out_of_range, dups, hit_t1 = set(), False, False
    for c in K.SCATTER:
        y, mask, idx = K.scatter_inputs(c)
        assert idx.dtype == np.int32 and idx.shape == (c["rows"], c["num"]) and y.all()
        out_of_range |= set(idx[(idx < 0) | (idx >= c["T"])].tolist())
        dups |= any(len(np.unique(r)) < len(r) for r in idx)
        hit_t1 |= c["T"] == 1 and bool((O.scatter_zero(y, mask, idx)[0] == 0).any())
    assert {-1, 1, 300, 2 ** 31 - 1} <= out_of_range and dups and hit_t1
    assert [(c["t_in"], c["t_out"]) for c in K.STRETCH] == [(1, 1), (1, 7), (7, 1), (2, 3), (256, 257), (257, 256), (1000, 1000), (20000, 16000), (12800, 16000),
                                                            (16000, 20000), (12345, 54321), (3, 100000)]
    assert {c["rows"] for c in K.STRETCH} == set(K.ROWS)
    assert K.MAX_ROWS == 65535 and K.ROW_LIMIT_T == 3 and row_limit_shapes() == [(65535, 3)] * 2 + [(65535, 2)]


def row_limit_shapes():
    return [a.shape for a in K.row_limit_inputs()]


# ---- d. the inputs discriminate ----------------------------------------------------------------------------------------------------
def separates(cases, inputs, oracle, variant, bar):
    """The largest amount by which `variant` exceeds `bar` over the cases, as (margin, case id); > 0 means some case tells them apart."""
    best = (-np.inf, None)
    for c in cases:
        args = inputs(c)
        want, got = oracle(c, args), variant(c, args)
        if got is None:
            continue
        d = float(np.abs(np.nan_to_num(np.asarray(got, np.float64)) - np.nan_to_num(np.asarray(want, np.float64))).max())
        best = max(best, (d - bar(c, args, want), c["id"]))
    return best


def test_median_inputs_discriminate():
    def reflect(c, x):
        h = c["k"] // 2
        return None if c["T"] <= h else np.sort(np.lib.stride_tricks.sliding_window_view(np.pad(x, ((0, 0), (h, h)), mode="reflect"), c["k"], axis=1), axis=-1)[..., h]

    def lower(c, x):
        h = c["k"] // 2
        return None if c["k"] < 3 else np.sort(np.lib.stride_tricks.sliding_window_view(np.pad(x, ((0, 0), (h, h))), c["k"], axis=1), axis=-1)[..., h - 1]

    for variant in (reflect, lower):
        m, cid = separates(K.MEDIAN, K.median_inputs, lambda c, x: O.median(x, c["k"]), variant, lambda *_: 0.0)
        assert m > 0, variant.__name__


def test_shush_inputs_discriminate():
    def latest_first(c, a):
        y, keep, mo = O.shush(a[0][:, ::-1], c["k"], None if a[1] is None else a[1][:, ::-1])
        return keep[:, ::-1]

    def threshold_kept(c, a):
        return None if c["k"] < 1 else O.shush(a[0], c["k"] - 1)[1]

    for variant in (latest_first, threshold_kept):
        m, cid = separates(K.SHUSH, K.shush_inputs, lambda c, a: O.shush(a[0], c["k"])[1], variant, lambda *_: 0.0)
        assert m > 0, variant.__name__
    seam = [c for c in K.SHUSH if c["kind"] == "seam"]
    assert separates(seam, K.shush_inputs, lambda c, a: O.shush(a[0], c["k"])[1], latest_first, lambda *_: 0.0)[0] > 0


def echo_earliest_tie_gradient(x, g, n, volume):
    """float64 restatement of a backward that sends each peak's gradient to the EARLIEST of its tied positions (not the reference's
    autograd, which shares it)."""
    x, g = x.astype(np.float64), g.astype(np.float64)
    v, L = float(np.float32(volume)), x.shape[1] - n + 1
    c = x[:, :L] + v * x[:, n - 1:]
    mo, mr = np.abs(x).max(), np.abs(c).max()
    dc = g[:, :L].copy()
    dx = np.zeros_like(x)
    if mo > 0 and mr > 0:
        s, S = mo / mr, (g[:, :L] * c).sum() / mr
        dc *= s
        jp = np.unravel_index(np.argmax(np.abs(c)), c.shape)
        dc[jp] -= S * s * np.sign(c[jp])
        ip = np.unravel_index(np.argmax(np.abs(x)), x.shape)
        dx[ip] += S * np.sign(x[ip])
    dx[:, :L] += dc
    dx[:, n - 1:] += v * dc
    return dx


def test_echo_inputs_discriminate():
    small = [c for c in K.ECHO if c["T"] <= 1025]

    def after(c, a):
        x, n, v = a[0].astype(np.float64), c["n"], float(np.float32(c["volume"]))
        L = c["T"] - n + 1
        cc = x[:, n - 1:] + v * x[:, :L]
        mo, mr = np.abs(x).max(), np.abs(cc).max()
        y = np.zeros_like(x)
        y[:, :L] = cc / mr * mo if mo > 0 and mr > 0 else cc
        return y

    def per_row(c, a):
        return np.concatenate([O.echo(row[None], c["n"], c["volume"]) for row in a[0]])

    fwd_bar = lambda c, a, want: 8 * EPS * float(np.abs(a[0]).max())
    for variant in (after, per_row):
        m, cid = separates(small, K.echo_inputs, lambda c, a: O.echo(a[0], c["n"], c["volume"]), variant, fwd_bar)
        assert m > 0, variant.__name__
    grad = lambda c, a: O.echo_gradient(a[0], a[1], c["n"], c["volume"])
    earliest = lambda c, a: echo_earliest_tie_gradient(a[0], a[1], c["n"], c["volume"])
    grad_bar = lambda c, a, want: BAR * float(np.abs(want).max())
    for kind in K.ECHO_TIES:                                  # every kind of tie tells the two rules apart
        m, cid = separates([c for c in small if c["kind"] == kind], K.echo_inputs, grad, earliest, grad_bar)
        assert m > 0, kind
    m, cid = separates([c for c in small if not c["tied"]], K.echo_inputs, grad, earliest, lambda c, a, want: 1e-12 * max(1.0, float(np.abs(want).max())))
    assert m <= 0, (m, cid)                                   # and without ties the two rules are one


def test_smooth_inputs_discriminate():
    small = [c for c in K.SMOOTH if c["w"] <= 257]

    def box(xp, w):
        return np.lib.stride_tricks.sliding_window_view(xp, w, axis=1).sum(-1) / w

    def pad_half(c, a):
        w, pl = c["w"], c["w"] // 2
        return None if (pl >= c["T"] or w - 1 - pl >= c["T"] or w - 1 - pl < 0) else box(np.pad(a[0].astype(np.float64), ((0, 0), (pl, w - 1 - pl)), mode="reflect"), w)

    def zero_pad(c, a):
        w, pl = c["w"], (c["w"] - 1) // 2
        return box(np.pad(a[0].astype(np.float64), ((0, 0), (pl, w - 1 - pl))), w)

    bar = lambda c, a, want: (c["w"] + 2) * EPS * float(np.abs(a[0]).max())
    for variant in (pad_half, zero_pad):
        m, cid = separates(small, K.smooth_inputs, lambda c, a: O.smooth(a[0], c["w"])[0], variant, bar)
        assert m > 0, variant.__name__

    def reflected_mask(c, a):
        w, pl = c["w"], (c["w"] - 1) // 2
        cnt = np.lib.stride_tricks.sliding_window_view(np.pad(a[2], ((0, 0), (pl, w - 1 - pl)), mode="reflect"), w, axis=1).sum(-1)
        return (cnt.astype(np.float32) / np.float32(w) >= np.float32(c["thr"])).astype(np.float32)

    def double_threshold(c, a):
        w, pl = c["w"], (c["w"] - 1) // 2
        cnt = np.lib.stride_tricks.sliding_window_view(np.pad(a[2], ((0, 0), (pl, w - 1 - pl))), w, axis=1).sum(-1)
        return ((cnt.astype(np.float32) / np.float32(w)).astype(np.float64) >= c["thr"]).astype(np.float32)      # the float32 ratio against the double 0.7

    masked = [c for c in small if c["mask"] != "none"]
    for variant in (reflected_mask, double_threshold):
        m, cid = separates(masked, K.smooth_inputs, lambda c, a: O.smooth(a[0], c["w"], a[2], c["thr"])[1], variant, lambda *_: 0.0)
        assert m > 0, variant.__name__


def test_stretch_inputs_discriminate():
    def blend(x, src, t_in):
        i0 = np.minimum(np.maximum(src, 0).astype(np.int64), t_in - 1)
        i1 = i0 + (i0 < t_in - 1)
        l1 = (src - i0.astype(np.float32)).astype(np.float64)
        return (1 - l1) * x[:, i0] + l1 * x[:, i1]

    def corners(c, x):
        scale = np.float32((c["t_in"] - 1) / (c["t_out"] - 1)) if c["t_out"] > 1 else np.float32(0)
        return blend(x.astype(np.float64), scale * np.arange(c["t_out"], dtype=np.float32), c["t_in"])

    def two_roundings(c, x):
        return O.stretch(x, c["t_out"], fused=False)

    def no_clamp(c, x):
        scale = np.float32(c["t_in"]) / np.float32(c["t_out"])
        src = (np.float64(scale) * (np.arange(c["t_out"]) + 0.5) - 0.5).astype(np.float32)
        return blend(x.astype(np.float64), src, c["t_in"])

    bar = lambda c, x, want: 4 * EPS * float(np.abs(x).max())
    for variant in (corners, two_roundings, no_clamp):
        m, cid = separates(K.STRETCH, K.stretch_inputs, lambda c, x: O.stretch(x, c["t_out"]), variant, bar)
        assert m > 0, variant.__name__
    exact = [c for c in K.STRETCH if c["id"].endswith("12800-to-16000")]
    assert separates(exact, K.stretch_inputs, lambda c, x: O.stretch(x, c["t_out"]), two_roundings, bar)[0] > 0


def test_quantise_inputs_discriminate():
    def away(c, a):
        if c["op"] != K.OP_QUANTIZE or c["a"] == 0:
            return None
        t = a[0] * np.float32(c["a"])
        return (np.sign(t) * np.floor(np.abs(t) + np.float32(0.5))).astype(np.float32) / np.float32(c["a"])

    small = [c for c in K.POINTWISE if c["rows"] * c["T"] <= 2048]
    m, cid = separates(small, K.pointwise_inputs, lambda c, a: O.pointwise(a[0], c["op"], c["a"], a[1]), away, lambda *_: 0.0)
    assert m > 0
