"""The case lists of the time-domain effects fuzz (a plain module, pure numpy, importable without a GPU: `import fx_time_cases`).

tests/test_fx_time_cases_cpu.py checks on the CPU that the lists hold every edge they are meant to hold and that their inputs tell
the oracle (oracle/wv_oracle_fx_time.py) from plausible wrong variants; tests/test_gpu_fx_time_fuzz.py runs them through
csrc/wv_fx_time.hip.  A case is a dict of parameters; `<kernel>_inputs(case)` builds its arrays from the case's own seed, so a
case is the same wherever and in whatever order it is built.  Shapes are the smallest at which each kernel can go wrong: both sides of
the 256-sample tile, of the 1024-thread chunk of shush, of every threshold between two code paths, and one input per grid-stride loop
that is long enough to make the loop iterate (the largest is 9 MB)."""
from __future__ import annotations

import numpy as np

ROWS = (1, 3, 7)
OP_SCALE, OP_ADD_NOISE, OP_QUANTIZE, OP_MUL = 0, 1, 2, 3
BIG_T = 262147                      # 2^18 + 3: rows * BIG_T is no multiple of 4 for the row counts used with it (3, 5, 9)


def _rng(*key):
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


def _cycle(seq, i):
    return seq[i % len(seq)]


# ---- pointwise ---------------------------------------------------------------------------------------------------------------------
def _pointwise_cases():
    out = []
    shapes = [(1, 1), (3, 1), (1, 3), (1, 4), (1, 5), (3, 341), (1, 1025), (7, 37)]          # rows * T = 1, 3, 3, 4, 5, 1023, 1025, 259
    for op, a in ((OP_SCALE, 0.7), (OP_SCALE, -1.3), (OP_ADD_NOISE, 0.01), (OP_QUANTIZE, 127.0), (OP_QUANTIZE, 32767.0), (OP_MUL, 0.0)):
        for rows, T in shapes:
            out.append(dict(rows=rows, T=T, op=op, a=a, offset=0, data="noise"))
        out.append(dict(rows=9, T=BIG_T, op=op, a=a, offset=0, data="noise"))                # the 2048-workgroup loop on the 16-byte path
        out.append(dict(rows=3, T=BIG_T, op=op, a=a, offset=1, data="noise"))                # and on the scalar path
    out.append(dict(rows=1, T=6, op=OP_QUANTIZE, a=1.0, offset=0, data="halves"))
    out.append(dict(rows=3, T=37, op=OP_QUANTIZE, a=0.0, offset=0, data="noise"))
    for i, c in enumerate(out):
        c["seed"] = 100 + i
        c["id"] = f"op{c['op']}-a{c['a']:g}-{c['rows']}x{c['T']}-{c['data']}-off{c['offset']}"
    return out


def pointwise_inputs(c):
    """-> (x, noise)"""
    r = _rng(1, c["seed"])
    if c["data"] == "halves":
        return np.array([[0.5, -0.5, 1.5, -1.5, 2.5, -2.5]], dtype=np.float32), np.zeros((1, 6), dtype=np.float32)
    x = (0.3 * r.standard_normal((c["rows"], c["T"]))).astype(np.float32)
    if c["op"] == OP_QUANTIZE and c["a"] > 0:                 # exact ties of x * a at .5 wherever a row is long enough
        h = (np.arange(c["T"]) % 5 == 0)
        x[:, h] = ((np.arange(c["T"])[h] % 13 - 6 + 0.5) / np.float32(c["a"])).astype(np.float32)
    noise = r.standard_normal((c["rows"], c["T"])).astype(np.float32)
    if c["op"] == OP_MUL:
        noise = (noise > 0).astype(np.float32)
    return x, noise


# ---- median ------------------------------------------------------------------------------------------------------------------------
MEDIAN_NET_KS = tuple(range(1, 32, 2))
MEDIAN_RANK_KS = (33, 63, 255)


def _median_cases():
    out, i = [], 0
    for k in MEDIAN_NET_KS + MEDIAN_RANK_KS:
        for T in sorted({1, 2, k // 2, k - 1, k, 255, 256, 257, 513} - {0}):
            out.append(dict(k=k, T=T, rows=_cycle(ROWS, i), seed=200 + i, id=f"k{k}-{_cycle(ROWS, i)}x{T}"))
            i += 1
    return out


def median_inputs(c):
    """Quarters, so that every window is full of duplicates; +0 and -0 in every row that has room for both."""
    r = _rng(2, c["seed"])
    x = (np.round(r.standard_normal((c["rows"], c["T"])) * 4) / 4).astype(np.float32)
    if c["T"] >= 2:
        x[:, r.integers(0, c["T"] // 2)] = 0.0
        x[:, c["T"] // 2 + r.integers(0, c["T"] - c["T"] // 2)] = -0.0
    return x


# ---- shush -------------------------------------------------------------------------------------------------------------------------
SHUSH_TS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
SHUSH_KINDS = ("one_magnitude", "zeros", "few_values", "seam", "low_byte", "subnormal")
SEAM = (1022, 1023, 1024, 1025, 1026)               # the tied samples of the `seam` rows: both sides of the 1024-sample chunk


def _shush_cases():
    out, i = [], 0
    for kind in SHUSH_KINDS:
        for T in SHUSH_TS:
            if kind == "seam" and T < 1025:
                continue
            for k in sorted({0, 1, T // 2, T - 1} & set(range(T))):
                for with_mask in (False, True):
                    rows = _cycle(ROWS, i)
                    out.append(dict(kind=kind, T=T, k=k, rows=rows, mask=with_mask, seed=300 + i, id=f"{kind}-{rows}x{T}-k{k}-mask{int(with_mask)}"))
                    i += 1
    return out


def seam_plan(T, k):
    """-> (tied positions, how many samples lie below them, how many of the tied ones go): all but the last tied sample go where k
    allows it, so the ordered count has to carry its base across the chunk seam."""
    tied = [t for t in SEAM if t < T]
    below = min(max(k - (len(tied) - 1), 0), T - len(tied))
    return tied, below, k - below


def shush_inputs(c):
    """-> (x, mask or None)"""
    r = _rng(3, c["seed"])
    rows, T, k = c["rows"], c["T"], c["k"]
    sign = np.where(r.random((rows, T)) < 0.5, -1.0, 1.0).astype(np.float32)
    if c["kind"] == "one_magnitude":
        x = np.float32(0.375) * sign
    elif c["kind"] == "zeros":
        x = np.float32(0.0) * sign
    elif c["kind"] == "few_values":
        x = (np.round(r.standard_normal((rows, T)) * 2) / 2).astype(np.float32) * np.float32(0.25)
    elif c["kind"] == "seam":
        tied, below, _ = seam_plan(T, k)
        x = np.empty((rows, T), dtype=np.float32)
        for row in x:
            rest = np.setdiff1d(np.arange(T), tied)
            r.shuffle(rest)
            row[rest[:below]] = (0.01 + 0.2 * r.random(below)).astype(np.float32)
            row[rest[below:]] = (0.5 + 0.4 * r.random(len(rest) - below)).astype(np.float32)
            row[tied] = 0.25
        x *= sign
    elif c["kind"] == "low_byte":
        bits = np.uint32(0x3E800000) + r.integers(0, 256, (rows, T)).astype(np.uint32)       # 0.25 plus 0 .. 255 ulps: the last radix pass decides
        x = bits.view(np.float32) * sign
    elif c["kind"] == "subnormal":
        bits = r.integers(0, 1 << 23, (rows, T)).astype(np.uint32)                           # subnormals and +-0
        bits[:, ::3] = r.integers(0x00800000, 0x3F800000, bits[:, ::3].shape).astype(np.uint32)
        x = bits.view(np.float32) * sign
    else:
        raise ValueError(c["kind"])
    mask = (r.random((rows, T)) > 0.3).astype(np.float32) if c["mask"] else None
    return np.ascontiguousarray(x, dtype=np.float32), mask


# ---- echo --------------------------------------------------------------------------------------------------------------------------
ECHO_TS = (2, 3, 37, 256, 1025)
ECHO_VOLUMES = (0.5, 0.25, 0.37, -0.4)
ECHO_PLACES = ("first", "last_tail", "middle_row", "c_at_T_minus_n", "random")
ECHO_TIES = ("x2", "x3", "c2", "clipped")


def _echo_ns(T):
    return sorted({2, 3, T // 2, T - 1, T} & set(range(2, T + 1)))


def _echo_cases():
    out, i = [], 0
    for T in ECHO_TS:
        for n in _echo_ns(T):
            for place in ECHO_PLACES:
                rows = _cycle((3, 7), i) if place == "middle_row" else _cycle(ROWS, i)
                out.append(dict(kind=place, T=T, n=n, rows=rows, volume=_cycle(ECHO_VOLUMES, i)))
                i += 1
    for T in (2, 37, 1025):
        out.append(dict(kind="zero", T=T, n=2, rows=_cycle(ROWS, i), volume=0.5))
        out.append(dict(kind="c_zero", T=T, n=T, rows=_cycle(ROWS, i + 1), volume=0.5))
        i += 1
    for kind in ECHO_TIES:
        for T in (37, 256, 1025):
            for n in (2, 5, T // 2):
                out.append(dict(kind=kind, T=T, n=n, rows=_cycle(ROWS, i), volume=_cycle((0.5, 0.25), i // 3)))
                i += 1
    out.append(dict(kind="random", T=BIG_T, n=4001, rows=5, volume=0.37))                   # the 1024-workgroup loops iterate
    for j, c in enumerate(out):
        c["seed"] = 400 + j
        c["tied"] = c["kind"] in ECHO_TIES
        c["id"] = f"{c['kind']}-{c['rows']}x{c['T']}-n{c['n']}-v{c['volume']:g}"
    return out


def echo_inputs(c):
    """-> (x, g): the clip and the gradient towards the output."""
    r = _rng(4, c["seed"])
    rows, T, n, v, kind = c["rows"], c["T"], c["n"], c["volume"], c["kind"]
    g = r.standard_normal((rows, T)).astype(np.float32)
    if kind in ECHO_TIES:                                     # dyadic: multiples of 2^-8, v a power of two, so c is exact in float32
        x = np.clip(np.round(r.standard_normal((rows, T)) * 0.125 * 256) / 256, -0.25, 0.25).astype(np.float32)
        L = T - n + 1
        if kind in ("x2", "x3"):
            flat = r.choice(rows * T, 3, replace=False)
            for j, s in zip(flat[: int(kind[1])], (1.0, -1.0, -1.0)):
                x.reshape(-1)[j] = 0.75 * s
        elif kind == "c2":                                    # two isolated spikes in the valid part, nothing under their echo taps
            ra, rb = 0, rows - 1
            ta, tb = (0, L - 1) if rows == 1 else (int(r.integers(0, L)), int(r.integers(0, L)))
            for rr, tt, s in ((ra, ta, 1.0), (rb, tb, -1.0)):
                x[rr, tt + n - 1] = 0.0
            for rr, tt, s in ((ra, ta, 1.0), (rb, tb, -1.0)):
                x[rr, tt] = 0.75 * s
        else:                                                 # a clipped clip: many samples at exactly +-0.5
            x = np.clip(np.round(r.standard_normal((rows, T)) * 0.5 * 256) / 256, -0.5, 0.5).astype(np.float32)
        return x, g
    if kind == "zero":
        return np.zeros((rows, T), dtype=np.float32), g
    if kind == "c_zero":                                      # n = T, v = 0.5: the one valid sample of every row cancels, max|x| > 0
        x = np.zeros((rows, T), dtype=np.float32)
        x[:, T - 1] = (np.round(r.uniform(0.25, 0.75, rows) * 256) / 256).astype(np.float32)
        x[:, 0] = np.float32(-0.5) * x[:, T - 1]
        return x, g
    x = (0.3 * r.standard_normal((rows, T))).astype(np.float32)
    x[np.abs(x) > 0.8] *= np.float32(0.25)                    # below the placed peaks, and not by clipping: these cases have no ties
    s = np.float32(1.0 if r.random() < 0.5 else -1.0)
    if kind == "first":
        x[0, 0] = 0.95 * s
    elif kind == "last_tail":
        x[rows - 1, T - 1] = 0.95 * s
    elif kind == "middle_row":
        x[rows // 2, T // 2] = 0.95 * s
    elif kind == "c_at_T_minus_n":
        row = rows // 2
        x[row, T - n], x[row, T - 1] = 0.9 * s, 0.85 * s * np.sign(np.float32(v))
    return x, g


# ---- smooth and its transpose ------------------------------------------------------------------------------------------------------
SMOOTH_WS = (1, 2, 3, 7, 10, 255, 256, 257, 2048)
SMOOTH_MASKS = ("none", "random", "exact", "exact7")


def smooth_min_t(w):
    return w - 1 - (w - 1) // 2 + 1


def _smooth_cases():
    out, i = [], 0
    for w in SMOOTH_WS:
        for T in sorted(t for t in {smooth_min_t(w), 255, 256, 257, 600} if t >= smooth_min_t(w)):
            for mk in SMOOTH_MASKS:
                if (mk == "exact" and w % 2) or (mk == "exact7" and w != 10):
                    continue
                thr = 0.7 if mk == "exact7" else 0.5
                rows = _cycle(ROWS, i)
                out.append(dict(w=w, T=T, rows=rows, mask=mk, thr=thr, dyadic=(w & (w - 1)) == 0, seed=500 + i, id=f"w{w}-{rows}x{T}-{mk}-thr{thr:g}"))
                i += 1
    return out


def smooth_inputs(c):
    """-> (x, g, mask or None).  For w a power of two x and g are multiples of 2^-10 below 1: every order of summation is exact.
    The `exact` masks put exactly w / 2 ones (7 of 10 for w = 10) into every full window, so the ratio sits on the threshold."""
    r = _rng(5, c["seed"])
    rows, T, w = c["rows"], c["T"], c["w"]
    if c["dyadic"]:
        x = (r.integers(-1023, 1024, (rows, T)) / 1024.0).astype(np.float32)
        g = (r.integers(-1023, 1024, (rows, T)) / 1024.0).astype(np.float32)
    else:
        x = (0.3 * r.standard_normal((rows, T))).astype(np.float32)
        g = r.standard_normal((rows, T)).astype(np.float32)
    mask = None
    if c["mask"] == "random":
        mask = (r.random((rows, T)) > 0.45).astype(np.float32)
        mask[:, T // 3: T // 3 + w // 2 + 2] = 0.0
    elif c["mask"] in ("exact", "exact7"):
        period = np.array([1, 1, 1, 0, 1, 1, 0, 1, 1, 0] if c["mask"] == "exact7" else [1, 0], dtype=np.float32)
        mask = np.stack([period[(np.arange(T) + int(s)) % len(period)] for s in r.integers(0, len(period), rows)])
    return x, g, mask


# ---- scatter-zero ------------------------------------------------------------------------------------------------------------------
def _scatter_cases():
    out, i = [], 0
    for T in (1, 300):
        for num in sorted({0, 1, 257, T} & set(range(T + 1))):
            for with_mask in (False, True):
                rows = _cycle(ROWS, i)
                out.append(dict(T=T, num=num, rows=rows, mask=with_mask, seed=600 + i, id=f"{rows}x{T}-num{num}-mask{int(with_mask)}"))
                i += 1
    return out


def scatter_inputs(c):
    """-> (y, mask or None, idx int32 [rows, num]): drawn WITH replacement (duplicates within a row), every seventh entry one of
    -1, T, 2^31 - 1 (no-ops: the kernel skips an index outside [0, T))."""
    r = _rng(6, c["seed"])
    rows, T, num = c["rows"], c["T"], c["num"]
    y = (0.3 * r.standard_normal((rows, T)) + 1.0).astype(np.float32)
    mask = np.ones((rows, T), dtype=np.float32) if c["mask"] else None
    idx = r.integers(0, T, (rows, num)).astype(np.int64)
    if num >= 3:
        idx[:, 2] = idx[:, 1]
    outside = np.array([-1, T, 2 ** 31 - 1], dtype=np.int64)
    for j in range(0, num, 7):                                # in every other row, so that a row of one index is zeroed somewhere too
        sel = (np.arange(rows) + j // 7) % 2 == (0 if num > 1 else 1)
        idx[sel, j] = outside[(j // 7 + T) % 3]
    return y, mask, idx.astype(np.int32)


# ---- stretch -----------------------------------------------------------------------------------------------------------------------
STRETCH_PAIRS = ((1, 1), (1, 7), (7, 1), (2, 3), (256, 257), (257, 256), (1000, 1000), (20000, 16000), (12800, 16000), (16000, 20000),
                 (12345, 54321), (3, 100000))


def _stretch_cases():
    return [dict(t_in=a, t_out=b, rows=_cycle(ROWS, i), seed=700 + i, id=f"{_cycle(ROWS, i)}x{a}-to-{b}") for i, (a, b) in enumerate(STRETCH_PAIRS)]


def stretch_inputs(c):
    return _rng(7, c["seed"]).standard_normal((c["rows"], c["t_in"])).astype(np.float32)


# ---- row limit ---------------------------------------------------------------------------------------------------------------------
MAX_ROWS = 65535
ROW_LIMIT_T = 3
GRID_ROW_ENTRY_POINTS = ("median", "shush", "smooth", "smooth_backward", "scatter_zero", "stretch")      # their launch grids carry the rows


def row_limit_inputs():
    r = _rng(8, 800)
    x = (np.round(r.standard_normal((MAX_ROWS, ROW_LIMIT_T)) * 4) / 4).astype(np.float32)
    return x, (r.random((MAX_ROWS, ROW_LIMIT_T)) > 0.3).astype(np.float32), r.integers(0, ROW_LIMIT_T, (MAX_ROWS, 2)).astype(np.int32)


POINTWISE = _pointwise_cases()
MEDIAN = _median_cases()
SHUSH = _shush_cases()
ECHO = _echo_cases()
SMOOTH = _smooth_cases()
SCATTER = _scatter_cases()
STRETCH = _stretch_cases()
