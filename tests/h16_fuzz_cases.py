"""Case lists of the f16 mode's route-by-route fuzz (tests/test_gpu_h16_fuzz.py), and next to them a short Python restatement of the
dispatch of csrc/wv_h16.hip: launch_conv16 (its refusals, flat / staged / ups, SHORT, wgm x wgn, the grid and the name wv::prof records),
up16_block and the packers' Kp / Mp / nchunks (wv_kernels.h), and -- through infer_fuzz_cases, which already restates rh_launch -- the
RH<...> row, per_cu and grid of the persistent ResnetBlock kernel at all nine widths.  The GPU test holds the restated name to the
library's; tests/test_h16_fuzz_cases_cpu.py asserts that every route and edge keeps its cases, and the boundaries of the restatement.
A changed launcher is restated here.  Operands are taken as 16-byte aligned (fresh torch allocations).  Pure Python: no GPU, no library."""
from types import SimpleNamespace

import numpy as np

from infer_fuzz_cases import persistent_grid, persistent_walk_case, rh16_width, rh_geometry  # noqa: F401  (one restatement of rh_launch)

H_OOB = 0x7f000000                                                # byte offset beyond any num_records (wv_h16.hip)
RING = 8                                                          # conv16_kernel's register ring D, in (16 channels, tap) chunks
BOUND = 6e6                                                       # B * max(K, M) * T: keeps a case's float64 oracle in the low seconds


def _ru(a, b):
    return -(-a // b) * b


def _cdiv(a, b):
    return -(-a // b)


# ---- the packers (wv_kernels.h) --------------------------------------------------------------------------------------------------------
def pack_h16(M, K, ks):
    """H16Weight of pack_h16: Kp = roundup(K, 16), Mp = roundup(M, 32), chunks (16 channels, tap) padded to a multiple of 8."""
    Kp = _ru(K, 16)
    return SimpleNamespace(K=K, M=M, Kp=Kp, Mp=_ru(M, 32), nchunks=_ru(ks * (Kp // 16), 8))


def up16_block(Mo, r):
    """Channels per row block of the upsample form: the largest multiple of 8 with r * mb <= 256 that divides Mo, else 0."""
    for mb in range((256 // r) // 8 * 8, 7, -8):
        if Mo % mb == 0:
            return mb
    return 0


def pack_up16(Mo, K, r):
    """H16Weight of pack_up16: M = Mo * r rows (block, phase, channel in block), two taps."""
    Kp = _ru(K, 16)
    return SimpleNamespace(K=K, M=Mo * r, Kp=Kp, Mp=_ru(Mo * r, 32), nchunks=_ru(2 * (Kp // 16), 8))


# ---- Conv16Args as the entry points fill them (wv_ops.hip) -------------------------------------------------------------------------------
def conv16(B, K, M, Tin, ks=1, stride=1, pad=0, resid=False, film=False, bands=1, Y=True, Yact=False, Yf32=False):
    """wv_h16_conv (resid, the f32 output) / wv_h16_conv_film (film: film_stride = 2 * bands)."""
    return SimpleNamespace(B=B, M=M, Tin=Tin, Tout=_cdiv(Tin, stride), ks=ks, stride=stride, pad=pad, w=pack_h16(M, K, ks), resid=bool(resid),
                           film=bool(film), bands=bands, film_stride=2 * bands, Y=bool(Y), Yact=bool(Yact), Yf32=bool(Yf32), up=0, up_mb=0)


def up16(B, K, Mo, Tin, r, Y=True, Yact=False):
    """wv_h16_upsample: a two-tap stride-1 conv over the input frames with r * Mo rows; up_mb = up16_block(Mo, r), or Mo where it finds none."""
    return SimpleNamespace(B=B, M=Mo * r, Tin=Tin, Tout=Tin, ks=2, stride=1, pad=1, w=pack_up16(Mo, K, r), resid=False, film=False, bands=1,
                           film_stride=0, Y=bool(Y), Yact=bool(Yact), Yf32=False, up=r, up_mb=up16_block(Mo, r) or Mo)


def launch_conv16(a):
    """-> (kernel name as wv::prof records it, info), or None where the launcher refuses the arguments (hipErrorInvalidValue).
    info: kernel ("conv16u" / "conv16s" / "conv16"), route (the template instance), short, flat, wgm, wgn, grid (x, y)."""
    w = a.w
    if not (a.Y or a.Yact or a.Yf32) or a.B < 1 or a.M < 1 or a.Tin < 1 or a.Tout < 1 or a.ks < 1 or a.stride < 1:
        return None
    if w.Kp % 16 or w.Mp % 32 or w.nchunks % 8 or w.nchunks < a.ks * (w.Kp // 16) or w.M != a.M:
        return None
    if w.Kp * a.Tin * 2 >= H_OOB or _ru(a.M, 16) * a.Tout * 2 >= H_OOB or w.nchunks * w.Mp * 32 >= H_OOB:
        return None
    if a.up < 0 or (a.up > 0 and (a.M % a.up or a.resid or a.Yf32 or a.stride != 1 or (a.M // a.up) % 16 or a.up_mb < 4 or (a.up_mb & 3) or
                                  (a.M // a.up) % a.up_mb)):
        return None
    Mo, upr = (a.M // a.up, a.up) if a.up > 0 else (a.M, 1)
    if (a.Y or a.Yact or a.resid) and Mo % 16:
        return None
    if a.film and (a.bands < 1 or Mo % a.bands or (Mo // a.bands) % 4 or a.film_stride < 2 * a.bands):
        return None
    if _ru(Mo, 16) * a.Tout * upr * 2 >= H_OOB:
        return None
    xbytes, ybytes = w.Kp * a.Tin * 2 * a.B, _ru(Mo, 16) * a.Tout * upr * 2 * a.B
    flat = a.Tout < 512 and xbytes < H_OOB and ybytes < H_OOB
    staged = (a.ks == 2 * a.stride and a.pad == a.stride and a.ks in (8, 10, 16) and not a.resid and not a.up and a.M >= 256 and ybytes < H_OOB and
              (a.Tout > 64 or xbytes < H_OOB))
    ups = (a.up > 0 and a.ks == 2 and a.pad == 1 and w.Kp % 32 == 0 and not a.film and a.up_mb % 8 == 0 and 128 <= a.up * a.up_mb <= 256 and
           ybytes < H_OOB and (a.Tin > 64 or xbytes < H_OOB))
    name = (f"conv16<k{a.ks},s{a.stride},{a.M}x{w.K}" + (f",up{a.up}" if a.up else "") +
            (",lds>" if staged or ups else ",flat>" if flat else ">"))
    if ups:
        short = a.Tin <= 64
        cps, nsub = (64, 2) if short else (128, 1)
        ts = cps * a.up
        smem = max(2 * 4 * nsub * (cps + 1) * 16, (a.up_mb // 8) * nsub * (ts + ts // 16 + 1) * 16)
        if smem > 80 * 1024:
            return None
        gx = (a.B + 1) // 2 if short else _cdiv(a.Tin, 128) * a.B
        return name, dict(kernel="conv16u", route=f"conv16u<{'short' if short else 'long'}>", short=short, flat=False, wgm=4, wgn=1,
                          grid=(gx, a.M // (a.up * a.up_mb)))
    if staged:
        short = a.Tout <= 64
        gx = (a.B + 1) // 2 if short else _cdiv(a.Tout, 128) * a.B
        return name, dict(kernel="conv16s", route=f"conv16s<{a.ks},{'short' if short else 'long'}>", short=short, flat=False, wgm=4, wgn=1,
                          grid=(gx, _cdiv(a.M, 256)))
    if flat:
        wgm = 1 if a.M >= 512 else 2 if a.M >= 128 else 1
        wgn = 4 // wgm
        return name, dict(kernel="conv16", route=f"conv16<{wgm},{wgn},flat>", short=False, flat=True, wgm=wgm, wgn=wgn,
                          grid=(_cdiv(a.B * a.Tout, 64 * wgn) * _cdiv(a.M, 64 * wgm), 1))
    wgm = 4 if a.M >= 256 else 2 if a.M >= 128 else 1
    wgn = 4 // wgm
    return name, dict(kernel="conv16", route=f"conv16<{wgm},{wgn}>", short=False, flat=False, wgm=wgm, wgn=wgn,
                      grid=(_cdiv(a.Tout, 64 * wgn) * a.B, _cdiv(a.M, 64 * wgm)))


def spans_clips(info):
    """Do the kernel's column tiles hold columns of several clips?  (The flat run and both two-clip SHORT forms.)"""
    return info["flat"] or info["short"]


def conv16_edges(a, info):
    """The edges of a case, as the labels tests/test_h16_fuzz_cases_cpu.py counts."""
    e = [("route", info["route"])]
    Mo = a.M // a.up if a.up else a.M
    if info["kernel"] == "conv16s":
        e.append(("staged steps", min(a.w.Kp // 16, 3)))                       # 16-channel steps against the window double buffer: 1, 2, 3 and more
        if a.M % 256:
            e.append(("staged", "ragged last row block"))
            if a.film and (a.M // a.bands) % 256:
                e.append(("staged", "ragged last row block, FiLM band edge inside a block"))
        if a.film:
            e.append(("staged FiLM", info["route"]))
        if info["short"] and a.B % 2:
            e.append(("staged", "short: the last tile holds one clip"))
        if a.Tout in (64, 65):
            e.append(("staged Tout", (a.ks, a.Tout)))
        if a.Tout in (128, 129):
            e.append(("staged Tout", a.Tout))
    elif info["kernel"] == "conv16u":
        e.append(("ups steps", min(a.w.Kp // 32, 4)))                          # 32-channel steps against the three-step A ring: 1, 2, 3, 4 and more
        e.append(("ups row block", a.up * a.up_mb))
        if info["short"] and a.B % 2:
            e.append(("ups", "short: the last tile holds one clip"))
        if info["short"] and a.B % 2 == 0:
            e.append(("ups", "short: every tile holds two clips"))
        if a.Tin in (1, 64, 65, 128, 129):
            e.append(("ups Tin", a.Tin))
    else:
        steps = a.ks * (a.w.Kp // 16)
        e.append(("generic chunks", "below the ring" if steps < RING else "the ring" if steps == RING else "above the ring"))
        if steps % RING:
            e.append(("generic chunks", "zero-padded"))
        if a.film:
            e.append(("generic FiLM", info["route"]))
        if a.resid:
            e.append(("generic residual", info["route"]))
        if a.up:
            e.append(("generic up", info["route"]))
            e.append(("generic up", "Kp % 32 != 0" if a.w.Kp % 32 else f"{a.up * a.up_mb}-row block"))
        if a.ks > 1 and a.stride > 1:
            e.append(("generic taps and stride", info["route"]))
        if info["flat"] and a.B > 1 and (a.B * a.Tout) % (64 * info["wgn"]) and a.Tout % (64 * info["wgn"]):
            e.append(("flat tile spans a clip boundary", info["route"] + (" FiLM" if a.film else "")))
        if a.Tout in (511, 512):
            e.append(("generic Tout", a.Tout))
        if Mo % 16:
            e.append(("generic", "rows outside c8 (f32 output only)"))
    if a.Yf32:
        e.append(("f32 output", info["kernel"]))
    e.append(("outputs", ("raw" if a.Y else "") + ("+act" if a.Yact else "")))
    return e


# ---- case lists --------------------------------------------------------------------------------------------------------------------------
# Dense conv: (B, K, M, Tin, ks, stride, pad, epi, outs); epi in "none", "resid" (out_scale 0.7 and a c8 residual), "film3", "film4";
# outs in "raw", "act", "both", "all" (both c8 outputs and the f32 one), "f32" (the f32 output alone: M need not fill c8 groups).
def dense_args(case):
    B, K, M, Tin, ks, stride, pad, epi, outs = case
    return conv16(B, K, M, Tin, ks, stride, pad, resid=epi == "resid", film=epi.startswith("film"), bands=int(epi[4]) if epi.startswith("film") else 1,
                  Y=outs in ("raw", "both", "all"), Yact=outs in ("act", "both", "all"), Yf32=outs in ("all", "f32"))


def dense_cases(n=60, seed=4117):
    """n seeded draws: B 1..7, K with 16-channel step counts below, at and above the ring depths, the suite's taps / strides / pads and the
    downsample form, M with and without c8 outputs, residual, FiLM with 3 and 4 bands, every output set; half the draws ask for at least 512
    outputs per clip or the staged form's shape, so that the routes other than flat keep at least a third of the list."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        B = int(rng.integers(1, 8))
        K = int(rng.choice([8, 16, 24, 32, 48, 64, 100, 144]))
        if rng.random() < 0.45:                                   # the downsample unit's composed conv
            stride = int(rng.choice([2, 4, 5, 8]))
            ks, pad = 2 * stride, stride
        else:
            ks, stride = int(rng.choice([1, 2, 3, 5, 7, 8, 10, 16])), int(rng.choice([1, 1, 2, 3, 4, 5, 8]))
            pad = int(rng.integers(0, ks))
        c8 = rng.random() < 0.7
        M = int(rng.choice([16, 32, 48, 64, 96, 128, 192, 256, 320, 384, 512])) if c8 else int(rng.choice([1, 7, 16, 33, 64, 130, 256, 320]))
        Tout = int(rng.choice([512, 513, 600, 1000])) if rng.random() < 0.5 else int(rng.choice([1, 2, 17, 50, 63, 64, 65, 128, 129, 200, 511]))
        Tin = max(1, Tout * stride - int(rng.integers(0, stride)))
        epi = str(rng.choice(["none", "resid", "film3", "film4"])) if c8 else "none"
        outs = str(rng.choice(["raw", "act", "both", "all", "f32"])) if c8 else "f32"
        if epi.startswith("film"):
            if M % int(epi[4]) or (M // int(epi[4])) % 4:
                epi = "none"
            elif outs in ("all", "f32"):
                outs = "both"
        if B * max(K, M) * Tin > BOUND:
            continue
        out.append((B, K, M, Tin, ks, stride, pad, epi, outs))
    return out


# The written-out list: the smallest shape that has each route or edge.  K = 16 or 32 unless the route needs otherwise.
DENSE_EXPLICIT = [
    # ---- staged (x through LDS): ks = 2 * stride in {8, 10, 16}, M >= 256, no residual
    (2, 32, 256, 1032, 16, 8, 8, "none", "both"),                 # k16 long, Tout = 129: a second column tile of one column
    (3, 32, 256, 201, 8, 4, 4, "none", "both"),                   # k8 short, Tout = 51, B = 3: the last two-clip tile holds one clip
    (2, 32, 256, 201, 8, 4, 4, "none", "raw"),                    # ... and B = 2: both sub-windows of the one tile in use
    # M = 320: a ragged second row block of 64 rows (one wave computes, three only copy); with 4 bands of 80 rows a band edge inside each block.
    # Tout = 64 | 65 on each of k8 / k10 / k16: the two-clip tile against the one-clip tile
    (2, 16, 320, 256, 8, 4, 4, "none", "both"),                   # k8, Tout = 64 (short)
    (2, 16, 320, 260, 8, 4, 4, "film4", "both"),                  # k8, Tout = 65 (long)
    (2, 16, 320, 325, 10, 5, 5, "none", "both"),                  # k10, Tout = 65
    (3, 16, 320, 320, 10, 5, 5, "film4", "both"),                 # k10, Tout = 64, odd B
    (3, 16, 320, 512, 16, 8, 8, "none", "act"),                   # k16, Tout = 64, odd B
    (2, 16, 320, 520, 16, 8, 8, "film4", "raw"),                  # k16, Tout = 65
    (3, 32, 256, 260, 8, 4, 4, "none", "all"),                    # k8, Tout = 65, the f32 output
    (3, 32, 256, 253, 8, 4, 4, "film4", "both"),                  # k8, Tout = 64 from a ragged Tin
    (3, 32, 256, 316, 10, 5, 5, "film4", "both"),                 # k10, Tout = 64
    (1, 32, 256, 321, 10, 5, 5, "none", "all"),                   # k10, Tout = 65, one clip
    (1, 32, 256, 505, 16, 8, 8, "film4", "act"),                  # k16, Tout = 64, one clip: a two-clip tile with its second clip absent
    (3, 32, 512, 513, 16, 8, 8, "none", "both"),                  # k16, Tout = 65, two row blocks
    (2, 16, 256, 512, 8, 4, 4, "none", "both"),                   # Tout = 128: one full column tile
    (2, 16, 256, 513, 8, 4, 4, "film4", "both"),                  # Tout = 129
    (2, 16, 256, 640, 10, 5, 5, "film4", "both"),                 # k10, Tout = 128
    (1, 16, 320, 641, 10, 5, 5, "none", "both"),                  # k10, Tout = 129, ragged row block
    (2, 16, 256, 1024, 16, 8, 8, "none", "all"),                  # k16, Tout = 128
    (2, 32, 256, 645, 10, 5, 5, "film4", "both"),                 # FiLM on the forms not yet above: k10 long, Tout = 129
    (2, 32, 512, 1029, 16, 8, 8, "film4", "both"),                # k16 long, Tout = 129, two row blocks of two bands each
    (2, 16, 256, 509, 16, 8, 8, "film4", "both"),                 # k16 short, Tout = 64, both clips of the tile present
    (4, 16, 256, 255, 8, 4, 4, "film4", "act"),                   # k8 short, two full tiles
    # ---- per clip (Tout >= 512): <4,1> from 256 rows, <2,2> from 128, <1,4> below; 33 rows: the f32 output alone
    (2, 16, 320, 513, 5, 1, 4, "resid", "both"),
    (2, 16, 128, 513, 5, 1, 4, "resid", "both"),
    (2, 16, 64, 513, 5, 1, 4, "resid", "all"),
    (2, 16, 33, 513, 5, 1, 4, "none", "f32"),
    (2, 16, 320, 1026, 4, 2, 2, "none", "both"),
    (2, 16, 128, 1026, 4, 2, 2, "none", "all"),
    (2, 16, 64, 1026, 4, 2, 2, "none", "both"),
    (2, 16, 33, 1025, 4, 2, 2, "none", "f32"),
    (2, 16, 320, 1026, 4, 2, 2, "film4", "both"),                 # FiLM on <4,1>: band edges at rows 80 / 160 / 240 inside the 256-row tile
    (3, 32, 256, 1025, 4, 2, 2, "film4", "act"),
    (2, 16, 128, 1026, 4, 2, 2, "film4", "both"),
    # ---- the 511 | 512 edge on the same weights (weights are seeded by (K, M, taps) alone): flat against per clip
    (2, 16, 320, 511, 5, 1, 4, "resid", "both"),
    (2, 16, 320, 512, 5, 1, 4, "resid", "both"),
    (2, 16, 128, 511, 5, 1, 4, "resid", "both"),
    (2, 16, 128, 512, 5, 1, 4, "resid", "both"),
    (2, 16, 64, 1022, 4, 2, 2, "none", "both"),
    (2, 16, 64, 1024, 4, 2, 2, "none", "both"),
    # ---- flat with FiLM, B * Tout no multiple of the tile's columns (128 at <2,2>, 256 at <1,4>): a tile spans a clip boundary
    (3, 16, 128, 200, 8, 4, 4, "film4", "both"),                  # <2,2,flat>, 3 x 50 columns
    (5, 32, 192, 99, 4, 2, 2, "film3", "both"),                   # <2,2,flat>, 5 x 50 columns, 64-row bands in 128-row tiles
    (3, 16, 512, 100, 4, 2, 2, "film4", "both"),                  # <1,4,flat> at M = 512, 3 x 50 columns in one 256-column tile
    (5, 16, 512, 130, 4, 2, 2, "film4", "act"),                   # <1,4,flat>, 5 x 65 columns: a tile of two and a half clips
    (3, 16, 64, 50, 5, 1, 4, "film4", "both"),                    # <1,4,flat> below 128 rows
    (7, 16, 96, 17, 3, 1, 2, "film3", "raw"),                     # <1,4,flat>, seven clips in one tile
    (3, 16, 64, 50, 5, 1, 4, "resid", "all"),                     # the residual on <1,4,flat>, every output
]


# Upsample form: (B, K, Mo, Tin, r, outs); outs in "raw", "act", "both"
def up_args(case):
    B, K, Mo, Tin, r, outs = case
    return up16(B, K, Mo, Tin, r, Y=outs in ("raw", "both"), Yact=outs in ("act", "both"))


def up_cases(n=24, seed=4118):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        r = (2, 3, 4, 5, 8)[len(out) % 5]
        case = (int(rng.integers(1, 7)), int(rng.choice([16, 32, 48, 64, 96, 128])), int(rng.choice([16, 32, 48, 64, 96, 128])),
                int(rng.choice([1, 37, 50, 64, 65, 128, 129, 200, 513, 600])), r, str(rng.choice(["raw", "act", "both"])))
        if case[0] * max(case[1], case[2] * r) * case[3] <= BOUND:
            out.append(case)
    return out


UP_EXPLICIT = [
    # ---- conv16u SHORT (Tin <= 64: two clips per tile) at B = 1 and 3, Tin = 64 and 1; Tin = 65 takes the long form; long at 128 | 129
    (1, 32, 32, 64, 8, "both"),                                   # 256-row blocks (Mo = 32, r = 8); one clip: the tile's second clip is absent
    (3, 32, 32, 64, 8, "both"),
    (1, 32, 32, 1, 8, "both"),
    (3, 32, 32, 1, 8, "raw"),
    (2, 32, 32, 65, 8, "both"),
    (3, 32, 32, 65, 8, "act"),
    (2, 32, 32, 128, 8, "both"),
    (1, 32, 32, 129, 8, "both"),
    # ---- the other row blocks: 240 (Mo = 48, r = 5), 128 (Mo = 16, r = 8; Mo = 64, r = 2), 192 (Mo = 96, r = 2)
    (3, 32, 48, 64, 5, "both"),
    (2, 32, 48, 129, 5, "both"),
    (1, 32, 16, 64, 8, "both"),
    (2, 32, 16, 128, 8, "both"),
    (3, 32, 64, 50, 2, "both"),
    (2, 32, 64, 129, 2, "both"),
    (3, 32, 96, 64, 2, "both"),
    (2, 32, 96, 65, 2, "both"),
    (4, 64, 32, 50, 8, "both"),                                   # SHORT with every tile full, two 32-channel steps
    (2, 96, 64, 64, 4, "act"),                                    # three steps: the A ring's depth
    # ---- the fall-throughs to the generic kernel, flat (Tin = 37) and per clip (Tin = 513)
    (2, 48, 32, 37, 8, "both"),                                   # Kp % 32 != 0
    (2, 48, 32, 513, 8, "both"),
    (3, 32, 32, 37, 3, "both"),                                   # a 96-row block
    (2, 32, 32, 513, 3, "both"),
    (1, 48, 64, 512, 4, "both"),                                  # 256 rows per clip: <4,1> in the up form
    (2, 48, 32, 513, 4, "act"),                                   # 128 rows: <2,2>
]

# the widths of launch_resblock16's switch whose older cases never give a workgroup a second tile (64 / 96 / 128 / 192: test_gpu_infer_fuzz.py)
WALK_WIDTHS = (32, 256, 384, 512, 768)
