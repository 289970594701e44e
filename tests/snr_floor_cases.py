"""Cases of the SNR-floor tests (tests/test_snr_floor_cpu.py, tests/test_gpu_snr_floor.py): a plain module, fixed seeds, importable without a
GPU.

kernel_case(L)    ONE raw geometry of wv_snr_floor per frame length: the arenas, the descriptor table with every kind of row the issue names
                  beside every kind of bad row, the state array and the gains array
FLOORS            the floors the route tests run under
The nets, clip lists and bank schedules are span_cases' and bank_cases' own (x1 / x6 / x13 exact, h.sweep4 for f16)."""
from __future__ import annotations

import numpy as np

import span_cases as SC
import window_cases as W
from waveverify_amd import snr_floor as SF

FRAMES = (12, 16, 32, 320)                                        # the hops of x13, x6, x1 / h.sweep4 and the full-size generator
TILE_FRAMES = 32                                                  # SF_TF of csrc/wv_snr_floor.hip
MIN_SNR_DB = 20.0
# The route tests' floor.  The small nets' residual does not follow the programme's level (about 0.013 .. 0.027 rms whatever goes in), so on
# span_cases' clips (rms 0.1) it lies 9 .. 20 dB under a full-level block and above a quiet one: at 10 dB full-level blocks keep the whole
# residual, quiet blocks are turned down, silent ones get none
ROUTE_DB = 10.0
LEVELS = (1.0, 1.0, 0.3, 0.03, 0.003)
FLOORS = (10.0, 20.0, 40.0)
STRENGTHS = (1.0, 0.75)
BOUND_DB = 1e-5                                                   # the issue's: the derived bound is 1.1e-6 dB
EXACT_IDS, F16_ID = SC.EXACT_IDS, SC.F16_ID
N_STATE = 7
POISON = np.float32(np.nan)                                       # what a state holds that the fresh flag must keep from being read


def envelope(rng, F, lo=1e-4, hi=1.0):
    """One level per frame, log-uniform over [lo, hi]: from frame to frame it rises and falls by orders of magnitude."""
    return np.exp(rng.uniform(np.log(lo), np.log(hi), F))


def signal(rng, n, L, special=True):
    """-> (x, r) float32 [n]: noise under independent per-frame envelopes spanning 1e-4 .. 1, so that frames where the floor caps the gain and
    frames where the strength does both occur, gains rise and fall; with `special` (and enough frames) a frame of x = 0, a frame of r = 0, a
    frame of both, and -0.0 samples in x and r."""
    F = -(-n // L)
    f = np.arange(n) // L
    x = (rng.standard_normal(n) * envelope(rng, F)[f]).astype(np.float32)
    r = (rng.standard_normal(n) * envelope(rng, F)[f] * 0.3).astype(np.float32)
    if special and F >= 8:
        x[2 * L:3 * L] = 0.0                                      # silence under a residual: the gain is 0, silence stays silent
        r[4 * L:5 * L] = 0.0                                      # nothing to add: the gain is s
        x[6 * L:7 * L] = 0.0
        r[6 * L:7 * L] = 0.0
        x[2 * L + 1] = -0.0
        x[4 * L + 2] = -0.0
        r[5 * L + 1] = -0.0
        x[5 * L + 1] = -0.0
    return x, r


# (x, r, out) offsets mod 4 of the good rows: all three on a 16-byte boundary when the arenas start on one (0, 0, 0) or one element past
# it (3, 3, 3), so both guard offsets run the 16-byte moves; the rest mix residues and run the scalar ones
RESIDUES = ((0, 0, 0), (1, 2, 3), (3, 3, 3), (0, 0, 0), (0, 0, 0), (3, 3, 3), (2, 1, 1), (3, 3, 3), (1, 1, 2))


def shape_level(x, block, tag):
    """x (the last axis is time) times a block envelope: every block at one of LEVELS, the first at full level, one inner block silent:
    loud and quiet passages and digital silence."""
    n = x.shape[-1]
    if n == 0:
        return x.astype(np.float32)
    nb = -(-n // block)
    rng = np.random.default_rng(W.seed_of("snr floor level", tag, n))
    env = rng.choice(LEVELS, nb)
    env[0] = 1.0
    if nb > 3:
        env[int(rng.integers(1, nb - 1))] = 0.0
    return (x * env[np.arange(n) // block].astype(np.float32)).astype(np.float32)


def batch_clips(cid):
    """[2, T] float32: the equal-length batch of the embed_batch test, 40 frames and a ragged end, under a block envelope of five hops."""
    cfg = W.net_config(SC.net_case(cid))[0]
    hop = cfg.hop_length
    T = 40 * hop + 5
    raw = [W.clip_data(SC.net_case(cid), T, 70 + b)[0][0, 0] for b in range(2)]
    return np.stack([shape_level(x, 5 * hop, (cid, "batch", b)) for b, x in enumerate(raw)])


def kernel_case(L, seed_tag="kernel"):
    """-> dict(x, r, n_out, rows [A, 8] int64, bad (row indices), gstate [N_STATE] float32, n_gains, n_max, kinds {row index: name}).
    Good rows: n = 0, n < L, n = L, n = 9L + 1, one row longer than a tile plus a frame, rows at every residue mod 4 of the three offsets;
    state fresh (over a poisoned entry), carried, and -1; strengths 1 and 0.75; gains wanted or not.  Bad rows of every kind aim at a gap of
    `out` that must stay untouched."""
    rng = np.random.default_rng(W.seed_of("snr floor", seed_tag, L))
    long_n = (TILE_FRAMES + 1) * L + L // 2 + 1                   # more than one tile plus a frame, ragged
    two_tiles = 2 * TILE_FRAMES * L                               # exactly two tiles
    specs = [  # (name, n, strength, state, fresh, want gains)
        ("n=0", 0, 1.0, 0, 0, True), ("n<L", max(L - 3, 1), 0.75, -1, 0, True), ("n=L", L, 1.0, 1, 0, True),
        ("n=9L+1", 9 * L + 1, 1.0, 2, 1, True), ("long", long_n, 0.75, 3, 0, True), ("two-tiles", two_tiles, 1.0, -1, 1, False),
        ("carried", 9 * L, 0.75, 4, 0, True), ("fresh-poisoned", 10 * L + 5, 1.0, 5, 1, True), ("s=0", 3 * L, 0.0, -1, 0, True),
    ]
    xs, rs, rows = [], [], []
    xo = ro = oo = go = 0
    for i, (name, n, s, si, fresh, wants) in enumerate(specs):
        x, r = signal(rng, n, L)
        want = RESIDUES[i]                                         # gaps of 1 .. 4 that put the three offsets at these residues mod 4
        gx, gr, gout = ((want[0] - xo - 1) % 4 + 1, (want[1] - ro - 1) % 4 + 1, (want[2] - oo - 1) % 4 + 1)
        xs += [rng.standard_normal(gx).astype(np.float32), x]
        rs += [rng.standard_normal(gr).astype(np.float32), r]
        xo, ro, oo = xo + gx, ro + gr, oo + gout
        F = -(-n // L)
        rows.append([xo, ro, oo, n, SF.strength_bits(s), si, fresh, go if wants else -1])
        xo, ro, oo = xo + n, ro + n, oo + n
        go += F + 1 if wants else 0
    gap, room = oo + 5, 4 * L                                     # the bad rows aim here
    n_out = gap + room + 3
    xs.append(rng.standard_normal(room).astype(np.float32))
    rs.append(rng.standard_normal(room).astype(np.float32))
    x, r = np.concatenate(xs), np.concatenate(rs)
    n_x, n_r, n_gains, n_max = len(x), len(r), go + 2, two_tiles
    one = SF.strength_bits(1.0)
    bad = [
        ("n<0", [0, 0, gap, -1, one, -1, 0, -1]), ("n>n_max", [0, 0, 0, n_max + 1, one, -1, 0, -1]),
        ("x before 0", [-1, 0, gap, L, one, -1, 0, -1]), ("x past its end", [n_x - L + 1, 0, gap, L, one, -1, 0, -1]),
        ("r before 0", [0, -1, gap, L, one, -1, 0, -1]), ("r past its end", [0, n_r - L + 1, gap, L, one, -1, 0, -1]),
        ("out before 0", [0, 0, -1, L, one, -1, 0, -1]), ("out past its end", [0, 0, n_out - L + 1, L, one, -1, 0, -1]),
        ("s<0", [0, 0, gap, L, SF.strength_bits(-0.5), -1, 0, -1]), ("s=nan", [0, 0, gap, L, SF.strength_bits(np.nan), -1, 0, -1]),
        ("s=inf", [0, 0, gap, L, SF.strength_bits(np.inf), -1, 0, -1]), ("s bits beyond 32", [0, 0, gap, L, 1 << 32, -1, 0, -1]),
        ("s bits negative", [0, 0, gap, L, -1, -1, 0, -1]),
        ("state<-1", [0, 0, gap, L, one, -2, 0, -1]), ("state>=n_state", [0, 0, gap, L, one, N_STATE, 0, -1]),
        ("gains<-1", [0, 0, gap, L, one, -1, 0, -2]), ("gains past their end", [0, 0, gap, 2 * L, one, -1, 0, n_gains - 1]),
        ("bad beside a state", [0, 0, gap, -1, one, 6, 1, 0]),       # names state 6 and gains 0: neither may change
    ]
    table, bad_idx = [], []
    k = 0
    for i, row in enumerate(rows):                                # a bad row after every other good one
        table.append(row)
        if i % 2 == 0:
            for _ in range(3):
                if k < len(bad):
                    bad_idx.append(len(table))
                    table.append(bad[k][1])
                    k += 1
    while k < len(bad):
        bad_idx.append(len(table))
        table.append(bad[k][1])
        k += 1
    names = {}
    gi = iter(n for n, *_ in specs)
    bi = iter(n for n, _ in bad)
    for i in range(len(table)):
        names[i] = next(bi) if i in bad_idx else next(gi)
    gstate = rng.uniform(0.05, 1.0, N_STATE).astype(np.float32)
    gstate[2] = gstate[5] = POISON                                # read only if the fresh flag fails
    return dict(x=x, r=r, n_out=n_out, rows=np.array(table, np.int64), bad=bad_idx, gstate=gstate, n_gains=n_gains, n_max=n_max, kinds=names,
                gap=(gap, gap + room))


def twin(case, L, rho, add):
    """The twin on a kernel case -> (out, gstate, gains, written mask of out, written mask of gains); out and gains start as NaN."""
    ramp = SF.floor_ramp(L)
    out = np.full(case["n_out"], np.nan, np.float32)
    gains = np.full(case["n_gains"], np.nan, np.float32)
    gstate = case["gstate"].copy()
    SF.numpy_snr_floor(case["x"], case["r"], out, case["rows"], case["n_max"], gstate, gains, ramp, rho, add)
    kept, gkept = np.zeros(case["n_out"], bool), np.zeros(case["n_gains"], bool)
    for i, row in enumerate(case["rows"]):
        if i in case["bad"]:
            continue
        _, _, oo, n, _, _, _, go = (int(v) for v in row)
        kept[oo:oo + n] = True
        if go >= 0:
            gkept[go:go + -(-n // L)] = True
    return out, gstate, gains, kept, gkept


def random_rows(L, count=25, seed_tag="bound"):
    """[(x, r)] of random lengths up to 40 frames for the bound test."""
    rng = np.random.default_rng(W.seed_of("snr floor", seed_tag, L))
    return [signal(rng, int(rng.integers(1, 40 * L)), L, special=bool(i % 2)) for i in range(count)]


def reference64(x, delta, rho, L, s=1.0, g_prev=None, add=True):
    """The twin's formula in float64 on a float64 residual: plain sums, no f32 rounding anywhere -> (out, g)."""
    n = len(x)
    F = -(-n // L)
    x64, d = x.astype(np.float64), np.asarray(delta, np.float64)
    pad = F * L - n
    Ex = (np.pad(x64, (0, pad)) ** 2).reshape(F, L).sum(1)
    Er = (np.pad(d, (0, pad)) ** 2).reshape(F, L).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(Er == 0, s, np.minimum(s, np.sqrt(rho * Ex / Er)))
    gp = np.concatenate([[g[0] if g_prev is None else g_prev], g[:-1]])
    f = np.arange(n) // L
    k = np.arange(n) - f * L
    ramp = (k + 1.0) / L
    w = np.where(gp[f] < g[f], np.minimum(g[f], gp[f] + (g[f] - gp[f]) * ramp), g[f])
    v = w * d
    return (x64 + v if add else v), g
