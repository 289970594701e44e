"""Cases of the span-embedding tests (tests/test_span_cases_cpu.py, tests/test_gpu_span.py): a plain module, fixed seeds, plain tuples,
importable without a GPU.

NETS              the nets: three exact small nets of window_cases (dilation_base 2 / four strides / no decoder blocks) and one h16 sweep
                  generator for the f16 mode
clip_list(cfg)    ONE list of five clips of mixed lengths with their spans, which between them hit every edge of SPAN_KINDS by name
messages(cid)     the message rows the spans' third element points into
reference(...)    x + w * delta of the whole clip, sample by sample in float64: what every route is held to
kernel tables     gather_case / scatter_case: raw geometries of wv_span_gather / wv_span_scatter_add with every kind of bad row
switch_plan(...)  when each stream of a bank schedule changes its id or switches it off"""
from __future__ import annotations

import numpy as np

import window_cases as W

# x1: dilation_base 2, hop 32; x6: four strides, residual kernel 3, hop 16; x13: no decoder blocks, hop 12
EXACT_IDS = ("x1.generator", "x6.generator", "x13.generator")
F16_ID = "h.sweep4.generator"                                     # hop 32
PAD_LIMITS = (1.0, 1.5, float("inf"))
FADES = (0, 7)
N_MSG = 3
SPAN_KINDS = ("at-0", "ragged-end", "one-sample", "sub-hop", "off-grid", "abutting", "three-pieces", "inside-halo", "span-less")
GAIN = 0.75                                                       # exactly representable, not 1: the gain multiply is a real rounding


def net_case(cid):
    return next(c for c in W.net_cases() if c[0] == cid)


def messages(cid):
    """[N_MSG, 16] float32 rows of 0 / 1, pairwise different."""
    rng = np.random.default_rng(W.seed_of("span messages", cid))
    while True:
        m = rng.integers(0, 2, (N_MSG, 16)).astype(np.float32)
        if len({tuple(r) for r in m}) == N_MSG:
            return m


# where, in its two-hop slot, the one-sample span sits: a sample at which that net's residual is not small by chance (seeds chosen so that
# tests/test_span_cases_cpu.py's input condition holds: one sample has no neighbours to make up for it)
ONE_SAMPLE_AT = {"x1.generator": 45, "x6.generator": 8, "x13.generator": 14, "h.sweep4.generator": 58}


def clip_list(cfg, one_at=1):
    """-> (window, lengths, spans, kinds): spans[b] = [(start, end, message row)], kinds[b] = the SPAN_KINDS its spans are, in order.
    L = 2 H is the window: a piece after the first keeps H samples, so a span of a little over 2 H is longer than the window and runs as
    three pieces."""
    from waveverify_amd.window import halo
    hop, H = cfg.hop_length, halo(cfg)
    L = 2 * H
    T0 = 3 * L + hop // 2 + 1                                     # ragged
    c0 = [(0, hop + 3, 0), (T0 - hop - 5, T0, 1)]
    a = H + 5 * hop
    c1 = [(a + one_at, a + one_at + 1, 2), (a + 2 * hop + 3, a + 3 * hop + 1, 0), (a + 5 * hop + 3, a + 7 * hop + 5, 1)]
    T1 = a + 9 * hop
    p = H + hop
    c2 = [(p + 3, p + hop + 7, 0), (p + hop + 7, p + 2 * hop + 1, 1), (3 * H, 5 * H + hop + 3, 2)]
    T2 = 6 * H
    assert 1 <= one_at <= 2 * hop + 1
    c4 = [(3, H - 2, 1)]
    lengths = (T0, T1, T2, hop + 3, H + 7)
    spans = (tuple(c0), tuple(c1), tuple(c2), (), tuple(c4))
    kinds = (("at-0", "ragged-end"), ("one-sample", "sub-hop", "off-grid"), ("abutting", "abutting", "three-pieces"), ("span-less",),
             ("inside-halo",))
    return L, lengths, spans, kinds


def cases(cid):
    return clip_list(W.net_config(net_case(cid))[0], ONE_SAMPLE_AT[cid])


def clip_data(cid, lengths):
    case = net_case(cid)
    return [W.clip_data(case, T, 40 + b)[0][0, 0] for b, T in enumerate(lengths)]      # float32 [T]


def weights(s, e, ramp, gain, dtype=np.float64):
    """w(t) for t in [s, e): gain * ramp[min(t - s, e - 1 - t)] inside the ramp, gain beyond it, the product taken in `dtype`."""
    j = np.arange(s, e)
    m = np.minimum(j - s, e - 1 - j)
    w = np.full(e - s, dtype(gain), dtype)
    if ramp is not None:
        F = len(ramp)
        w[m < F] = dtype(gain) * ramp[m[m < F]].astype(dtype)
    return w


def reference(x, deltas, spans, ramp=None, gain=1.0, add_input=True):
    """x [T] float32, deltas {message row: whole-clip residual [T] float64} -> x + w * delta over the spans, x elsewhere, float64."""
    out = x.astype(np.float64) if add_input else np.zeros(x.shape, np.float64)
    for s, e, m in spans:
        out[s:e] = out[s:e] + weights(s, e, ramp, gain) * deltas[m][s:e]
    return out


def outside(T, spans):
    mask = np.ones(T, bool)
    for s, e, _ in spans:
        mask[s:e] = False
    return mask


# ---- wv_span_gather / wv_span_scatter_add ------------------------------------------------------------------------------------------------
KERNEL_L = W.GATHER_L                                             # 1, 3, 1023, 1024, 1025, 2051: below, on and past one tile, past two
KERNEL_F = (0, 1, 5, "long")                                      # "long": a ramp longer than every keep range


def gather_case(Lmax):
    """-> (n_src, rows [(off, wlen)], bad): wlen in {0, 1, Lmax - 1, Lmax} at every residue mod 4 of the offset, then the rows the kernel must
    skip (bad = their indices): off < 0, off + wlen > n_src, wlen > Lmax, wlen < 0."""
    n_src = 2 * Lmax + 19
    good = [(o, wl) for o in (0, 1, 2, 3, 8) for wl in sorted({0, 1, max(Lmax - 1, 0), Lmax})]
    good += [(n_src - Lmax, Lmax), (n_src, 0)]
    bad = [(-1, 1), (n_src - Lmax + 1, Lmax), (0, Lmax + 1), (4, -1), (n_src + 1, 0)]
    rows = good[:3] + [bad[0]] + good[3:7] + bad[1:3] + good[7:] + bad[3:]
    return n_src, rows, [i for i, r in enumerate(rows) if r in bad]


def scatter_case(Lmax, F):
    """-> (n_out, rows [(o, lo, hi, span start, span end)], bad): disjoint destinations o + [lo, hi) laid one after another with gaps, keep
    ranges at every residue mod 4, a negative span start, a span end beyond Lmax, a span exactly the keep range (both ramps meet), and every
    kind of bad row (bad = their indices) aimed at a gap that must stay untouched."""
    keeps = [(0, Lmax), (0, 1), (Lmax - 1, Lmax)]
    if Lmax > 8:
        keeps += [(1, Lmax), (2, Lmax - 1), (3, Lmax - 2), (4, Lmax - 3), (5, 9), (0, Lmax - 4), (Lmax // 2, Lmax // 2 + 1)]
    far = Lmax + 3 * (F if isinstance(F, int) else Lmax)
    rows, base = [], 5
    for i, (lo, hi) in enumerate(keeps):
        ss, se = ((lo, hi), (lo - 2, hi + 1), (-far, hi), (lo, far), (-far, far))[i % 5]
        o = base - lo + (i % 4)                                    # destinations at every residue mod 4
        rows.append((o, lo, hi, ss, se))
        base = o + hi + 6
    gap = base                                                     # the bad rows aim here
    n_out = gap + Lmax + 9
    lo, hi = (0, Lmax)
    bad = [(gap, -1, hi, -1, hi), (gap, lo, Lmax + 1, lo, Lmax + 1), (gap, hi, hi, lo, hi), (gap, lo, hi, lo + 1, hi + 1), (gap, lo, hi, lo, hi - 1),
           (-1, lo, hi, lo, hi), (n_out - hi + 1, lo, hi, lo, hi)]
    if Lmax > 1:
        bad.append((gap, 1, 0, 0, Lmax))
    out = rows[:2] + bad[:3] + rows[2:] + bad[3:]
    return n_out, out, [i for i, r in enumerate(out) if r in bad]


# ---- live: a bank schedule with id switches ----------------------------------------------------------------------------------------------
def switch_plan(steps):
    """steps: a bank_cases schedule -> {stream: [state per global push step]} and the state each stream opens in; a state is a message row or
    None (pass-through).  Stream i (in opening order) at push step k is in state (0, None, 1)[((k + i) // 2) % 3]: every stream goes id ->
    None -> another id, two steps each, and every third stream opens in pass-through."""
    names = [arg for kind, arg in steps if kind == "open"]
    n_push = sum(1 for kind, _ in steps if kind == "push")
    return {n: [(0, None, 1)[((k + i) // 2) % 3] for k in range(n_push + 1)] for i, n in enumerate(names)}


def run_switching(bank, steps, xs, plan, open_stream, set_state, take=lambda x: x):
    """Plays a schedule with its switch plan -> ({stream: [result per push / close]}, {stream: [(from sample, state)]}, launches per push step,
    which push steps had only pass-through slots).  open_stream(state) -> slot; set_state(slot, state) -> the sample it holds from."""
    slot, pos, out, marks, state = {}, {}, {}, {}, {}
    k, launches, only_through = 0, [], []
    for kind, arg in steps:
        if kind == "open":
            state[arg] = plan[arg][k]
            slot[arg] = open_stream(state[arg])
            pos[arg], out[arg], marks[arg] = 0, [], [(0, state[arg])]
        elif kind == "close":
            out[arg].append(bank.close(slot[arg]))
            del state[arg]
        else:
            for n in list(state):
                if plan[n][k] != state[n]:
                    state[n] = plan[n][k]
                    marks[n].append((set_state(slot[n], state[n]), state[n]))
            before = bank.stats["launches"]
            res = bank.push({slot[n]: take(xs[n][pos[n]:pos[n] + c]) for n, c in arg.items()})
            launches.append(bank.stats["launches"] - before)
            only_through.append(all(state[n] is None for n in arg))
            for n, c in arg.items():
                pos[n] += c
                out[n].append(res[slot[n]])
            k += 1
    return out, marks, launches, only_through


def spans_of(marks, T):
    """[(from sample, state)] in call order -> the stream's spans [(start, end, message row)]: a later mark at the same sample wins."""
    pts = {}
    for t, st in marks:
        pts[t] = st
    edges = sorted(pts) + [T]
    return [(a, b, pts[a]) for a, b in zip(edges, edges[1:]) if b > a and pts[a] is not None]
