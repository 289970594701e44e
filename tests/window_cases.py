"""Cases of the windowed / live-session fuzz (tests/test_window_cases_cpu.py, tests/test_gpu_window_fuzz.py): a plain module, fixed seeds,
plain tuples, importable without a GPU.

net_cases()       the nets: a subset of infer_fuzz_cases.net_cases() for the exact path (each as generator, detector and locator) and the
                  configurations of h16_plan_cases.net_configs() that the f16 mode is run on
clip_cases(cfg)   per net: windows and, per window, a list of clip lengths on the planner's edges
push_cases(cfg)   per net: schedules of push sizes for live sessions
advance_cases()   raw geometries of wv_session_advance inside its documented contract
and the tables of the data-movement tests (reduce_mean_cases, GATHER_L, scatter_cases)."""
from __future__ import annotations

import zlib

import numpy as np

import infer_fuzz_cases as IC

KINDS = ("generator", "detector", "locator")
MAX_WINDOWS = (1, 2, 64)

# ---- nets --------------------------------------------------------------------------------------------------------------------------------
# indices into infer_fuzz_cases.net_cases(): hop 20 / 32 / 16 / 20 / 16 / 32 / 24 / 12 / 8; dilation_base 2 in #0, #1, #4, #9; residual kernel
# 3 in #6, #7; no encoder blocks in #0, #6, #9 and three in #3, #4, #13; no decoder blocks in #4, #13 and three in #0, #1, #6, #7, #9; four
# strides in #6 and #9
EXACT = (0, 1, 3, 4, 6, 7, 9, 13, 14)
_DEC_ONLY = ("channels_dec", "n_residual_dec", "embedding_dim", "embedding_layers")

# ids of h16_plan_cases.net_configs(): the defaults, two sweep triples (hop 64 and 32), a 36-bit detector (f32 tail behind the f16 encoder)
# and the 16-channel nets, which have no f16 plan: the windowed f16 routes must refuse them as the whole-clip ones do
F16 = ("generator", "detector", "locator", "sweep1.generator", "sweep1.detector", "sweep1.locator", "sweep4.generator", "sweep4.detector",
       "sweep4.locator", "nbits36.detector", "narrow16.detector", "narrow16.generator")
F16_REFUSED = ("narrow16.detector", "narrow16.generator")


def net_cases():
    """-> [(case id, precision, kind, source)]: source is ("fuzz", idx, cfg kwargs) or ("h16", id of h16_plan_cases.net_configs())."""
    nets = {i: kw for i, kw, _, _ in IC.net_cases()}
    out = []
    for idx in EXACT:
        for kind in KINDS:
            out.append((f"x{idx}.{kind}", "f32", kind, ("fuzz", idx, nets[idx])))
    for nid in F16:
        kind = nid.split(".")[-1]
        out.append((f"h.{nid}", "f16", kind, ("h16", nid)))
    return out


def fuzz_kwargs(cfgkw, kind):
    """The kwargs test_gpu_infer_fuzz.test_whole_nets_fuzz gives default_config for a drawn configuration."""
    kw = dict(cfgkw)
    nspec = len(kw["strides"]) + 1
    kw["spec_means"] = [-4.0 + 0.1 * i for i in range(nspec)]
    kw["spec_stds"] = [2.5 + 0.05 * i for i in range(nspec)]
    if kind != "generator":
        kw = {k: v for k, v in kw.items() if k not in _DEC_ONLY}
    return kw


_H16 = None


def net_config(case):
    """-> (NetConfig, seed of random_state_dict)."""
    from waveverify_amd.config import default_config
    global _H16
    _, _, kind, src = case
    if src[0] == "fuzz":
        return default_config(kind, **fuzz_kwargs(src[2], kind)), {"generator": 131, "detector": 157, "locator": 157}[kind] + src[1]
    if _H16 is None:
        import h16_plan_cases
        _H16 = h16_plan_cases.net_configs()
    return _H16[src[1]], 7


def seed_of(*what):
    return zlib.crc32(repr(what).encode())


# ---- clips -------------------------------------------------------------------------------------------------------------------------------
# one-window and several-window kinds in turn, so that each half of the list (and of any rotation of it) mixes them
LENGTH_KINDS = ("one", "L+1", "hop-1", "edge-1", "hop", "edge", "L-1", "edge+1", "L", "four-ragged")
WINDOW_KINDS = ("min", "min+hop", "drawn", "unrounded")


def lengths_of(L, H, hop, k4):
    """{length kind: T} for the hop-rounded window L.  edge = L + (L - H): plan's `while k + (L - H) < T` is false there (two windows, the last
    full) and true one sample later (three, the last keeping one sample).  four-ragged: k4 >= 2 full windows after the first and a ragged end."""
    step = L - H
    return {"one": 1, "hop-1": hop - 1, "hop": hop, "L-1": L - 1, "L": L, "L+1": L + 1, "edge-1": L + step - 1, "edge": L + step,
            "edge+1": L + step + 1, "four-ragged": L + k4 * step + hop // 2 + 1}


def clip_cases(cfg, windows=WINDOW_KINDS, salt=0, full=True):
    """-> [(window kind, window, length kinds, lengths)]: lists of five clips.  full: two lists per window, together all ten length kinds at
    that window; else one list per window, the two halves in turn.  salt rotates the kinds, so the halves differ from net to net.  Every
    list holds clips of one and of several windows, and no clip is longer than 4 L."""
    from waveverify_amd.window import halo
    hop, H = cfg.hop_length, halo(cfg)
    rng = np.random.default_rng(seed_of("clips", H, hop, salt))
    k = int(rng.integers(3, 9))
    win = {"min": H + hop, "min+hop": H + 2 * hop, "drawn": H + k * hop, "unrounded": H + 2 * hop + max(1, hop // 3)}
    order = [LENGTH_KINDS[(salt + j) % len(LENGTH_KINDS)] for j in range(len(LENGTH_KINDS))]
    out = []
    for i, wk in enumerate(windows):
        L = -(-win[wk] // hop) * hop
        by_kind = lengths_of(L, H, hop, 2)                            # four windows; L + 2 (L - H) + hop / 2 + 1 <= 4 L
        for half in ((0, 1) if full else (i % 2,)):
            kinds = order[5 * half: 5 * half + 5]
            out.append((wk, win[wk], tuple(kinds), tuple(by_kind[n] for n in kinds)))
    return out


# ---- pushes ------------------------------------------------------------------------------------------------------------------------------
def push_cases(cfg, long=True):
    """-> [(name, S, sizes)]: flush() follows every schedule.  long=False leaves out the pushes beyond the history capacity."""
    from waveverify_amd.window import halo
    hop, H = cfg.hop_length, halo(cfg)
    cap = H + hop
    dribble = [1] * 3 + [max(1, hop // 4)] if hop > 7 else [1] * 3                # after a hop multiple: none of them completes a frame
    assert 1 + sum(dribble) < hop
    a = [0, 1, hop - 1, hop, hop + 1] + dribble                                    # total so far: 3 hop + 1 + sum(dribble)
    a.append(hop - (1 + sum(dribble)) % hop if (1 + sum(dribble)) % hop else 0)     # up to a hop multiple
    if long:
        a += [cap + 1 + hop // 2, 0]
        a.append(hop - sum(a) % hop)                                               # a hop multiple again: flush() has nothing to emit
    b = [0, hop + 1, 1, hop - 1, hop, 2 * hop + 3] + ([cap + hop + 2] if long else [])
    if sum(b) % hop == 0:
        b.append(1)
    return [("aligned", 1, tuple(a)), ("ragged", 3, tuple(b)), ("flush-only", 3, ()), ("one-short-push", 1, (hop - 1,))]


# ---- wv_session_advance ------------------------------------------------------------------------------------------------------------------
def advance_cases():
    """-> [(S, hcap, hv, n, wlen, drop, hv2)] inside the contract: 0 <= hv <= hcap, 0 <= wlen <= hv + n, 0 <= hv2 <= hcap, drop + hv2 == hv + n."""
    return [
        (1, 7, 0, 5, 5, 0, 5),                    # hv = 0: everything from x
        (3, 37, 11, 0, 0, 0, 11),                 # n = 0, wlen = 0: the history carried over
        (2, 37, 11, 0, 11, 4, 7),                 # n = 0 with a window (what flush() runs)
        (2, 37, 20, 9, 29, 29, 0),                # hv2 = 0: flush, nothing kept
        (1, 37, 0, 0, 0, 0, 0),                   # nothing at all: no launch
        (3, 301, 43, 257, 255, 0, 300),           # wlen < 256 < hv2
        (3, 301, 43, 257, 257, 45, 255),          # hv2 < 256 < wlen
        (2, 600, 300, 213, 513, 1, 512),          # both beyond 256, wlen > hv2
        (2, 600, 300, 213, 258, 0, 513),          # both beyond 256, hv2 > wlen
        (1, 257, 256, 1, 256, 1, 256),            # wlen == hv2 == 256: one full block
        (5, 39, 13, 50, 63, 30, 33),              # drop > hv: the next history from x only; hcap, n, wlen odd
        (2, 39, 39, 3, 42, 39, 3),                # drop == hv: a full history dropped whole
        (65, 6, 3, 2, 5, 1, 4),                   # more streams than a wave
    ]


# ---- wv_window_reduce_mean ---------------------------------------------------------------------------------------------------------------
def reduce_mean_cases():
    """-> [(n_rows, nb, ptr, rows, lengths)]: rows in permuted order, an empty row range, a clip of length 0, row indices -1 and n_rows (skipped);
    nb in {1, 16, 36}; B * nb = 5, 6 / 96, 272 / 216, 288."""
    out = []
    for nb, B in ((1, 5), (1, 6), (16, 6), (16, 17), (36, 6), (36, 8)):
        rng = np.random.default_rng(seed_of("reduce", nb, B))
        n_rows = 3 * B + 1
        perm = [int(v) for v in rng.permutation(n_rows)]
        ptr, rows, lengths = [0], [], []
        for b in range(B):
            take = 0 if b == 1 else int(rng.integers(1, 5))        # clip 1: an empty row range
            mine = perm[:take]
            perm = perm[take:]
            if b == 2:
                mine = [-1] + mine + [n_rows]                          # skipped indices around real ones
            rows += mine
            ptr.append(len(rows))
            lengths.append(0 if b == 3 else int(rng.integers(1, 100000)))   # clip 3: len == 0 -> 0
        out.append((n_rows, nb, tuple(ptr), tuple(rows), tuple(lengths)))
    return out


# ---- wv_window_gather / wv_window_scatter --------------------------------------------------------------------------------------------------
GATHER_L = (1, 3, 1023, 1024, 1025, 2051)            # WIN_TILE = 1024: below, on and past one tile, past two; L % 4 in {0, 1, 3}
SCATTER_C = (1, 3, 17)


GATHER_INSIDE = 16
SCATTER_HOP = 8


def gather_offsets(n_src, L):
    """Sixteen in-range offsets, then the out-of-range ones of the contract test.  Row w of dst starts w * L floats in, so its 16-byte
    alignment depends on w % 4 alone; the offsets give every row class every residue mod 4 of the source, so whatever L % 4 and the
    buffers' own alignment, aligned and misaligned sources meet aligned and misaligned rows (where L % 4 leaves both)."""
    inside = [(w // 4 + w) % 4 + 4 * (w % 3) for w in range(GATHER_INSIDE)]
    assert max(inside) + L <= n_src
    return inside + [n_src - L, n_src - L + 1, -1, n_src, -L]


def gather_paths(L, e, n_src):
    """{(source 16-byte aligned, dst row 16-byte aligned)} over the in-range rows, both buffers e floats past a 256-byte boundary."""
    return {((e + o) % 4 == 0, (e + w * L) % 4 == 0) for w, o in enumerate(gather_offsets(n_src, L)) if 0 <= o <= n_src - L}


def scatter_cases():
    """-> [(C, L, unit, [(lo, hi)])]: keep ranges at every residue mod 4 of lo and hi, with lo == hi, hi == L and lo == 0; unit "sample" (the
    descriptor of window.scatter) or "frame" (that of window.frame_scatter_desc)."""
    out = []
    for i, L in enumerate(GATHER_L):
        C = SCATTER_C[i % 3]
        keeps = [(0, L), (0, 0), (L, L), (L - 1, L), (0, 1)]
        if L > 8:
            keeps += [(a, L - b) for a, b in ((1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (6, 6), (7, 5), (0, 7))] + [(5, 5), (L // 2, L // 2 + 1)]
            keeps += [(0, L), (0, L), (0, L)]                        # whole windows at other destination alignments
        out.append((C, L, "sample" if i % 2 == 0 else "frame", tuple(keeps)))
        out.append((SCATTER_C[(i + 1) % 3], L, "frame" if i % 2 == 0 else "sample", tuple(keeps)))
    return out


def scatter_layout(case):
    """One window per keep range, each the last L columns of a clip of its own that has `start` earlier ones, so the destinations take every
    residue mod 4 -> (clip lengths Ts, descriptors [[offset, row stride, lo, hi]], n_out).  Sample units: window.scatter's descriptor.
    Frame units: window.frame_scatter_desc's on windows of L frames of SCATTER_HOP samples, the clip's last kept frame partial."""
    from waveverify_amd.window import Window, frame_scatter_desc
    Cc, L, unit, keeps = case
    hop = SCATTER_HOP
    starts = [(3 * w) % 7 for w in range(len(keeps))]
    Ts = [s_ + L for s_ in starts]
    bases = [sum(Ts[:w]) for w in range(len(Ts))]
    if unit == "sample":
        desc = [[Cc * bases[w] + starts[w], Ts[w], lo, hi] for w, (lo, hi) in enumerate(keeps)]
    else:
        wins = [Window(w, starts[w] * hop, L * hop, (starts[w] + lo) * hop, (starts[w] + hi) * hop - (3 if hi == L and hi > lo else 0))
                for w, (lo, hi) in enumerate(keeps)]
        desc = frame_scatter_desc(wins, bases, Ts, hop, Cc)
    return Ts, desc, Cc * sum(Ts)


def scatter_paths(case, e):
    """{True, False}: whether some thread of a (window, row) takes the 16-byte path (both rows 16-byte aligned and four columns inside the keep
    range at a multiple of four) or every thread the scalar one, y and out e floats past a 256-byte boundary."""
    Cc, L, _, _ = case
    _, desc, _ = scatter_layout(case)
    out = set()
    for w, (o, rs, lo, hi) in enumerate(desc):
        for c in range(Cc):
            rows16 = (e + (w * Cc + c) * L) % 4 == 0 and (e + o + c * rs) % 4 == 0
            out.add(bool(rows16 and -(-lo // 4) * 4 + 4 <= hi))
    return out


# ---- the float64 oracle ------------------------------------------------------------------------------------------------------------------
def oracle_net(case):
    """-> (cfg, state dict, oracle/wv_oracle._Net in float64) of a net case."""
    from oracle import wv_oracle as O
    from waveverify_amd.init import random_state_dict
    cfg, seed = net_config(case)
    parametrized = case[3][0] == "fuzz" and case[2] == "generator" and bool(case[3][1] & 1)
    sd = random_state_dict(cfg, seed, parametrized=True) if parametrized else random_state_dict(cfg, seed)
    return cfg, sd, O._Net(cfg, sd, np.float64)


def oracle_forward(cfg, onet, x, msg=None, add_input=True):
    """The float64 oracle on whole clips x [B,1,T] (float32 samples): G(x, msg) (+ x) for a generator, logits for a detector or a locator."""
    from oracle import wv_oracle as O
    if cfg.kind == "generator":
        y = O.generator_forward(cfg, onet, x, msg, dtype=np.float64)
        return y + x.astype(np.float64) if add_input else y
    return (O.detector_forward if cfg.kind == "detector" else O.locator_forward)(cfg, onet, x, dtype=np.float64)


def clip_data(case, T, slot):
    """Clip `slot` of length T of a net case -> (x [1,1,T] float32, msg [1,16] float32)."""
    from waveverify_amd.init import synthetic_clips
    return synthetic_clips(1, T, seed=seed_of(case[0], T, slot) % (2 ** 31))
