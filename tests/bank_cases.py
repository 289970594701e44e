"""Cases of the session-bank tests (tests/test_bank_cases_cpu.py, tests/test_gpu_session_bank.py): a plain module, fixed seeds, plain tuples,
importable without a GPU.

net_cases()        the session nets of the window fuzz (#0, #6, #9, #13, #14: hops 20, 16, 24, 12 and 8) as generator, detector and locator,
                   and the h16 configurations that fuzz runs its f16 sessions on
schedules(cfg)     per net: [(name, steps)], a step ("open", stream) | ("push", {stream: n}) | ("close", stream); streams are named by
                   letters, run() maps them to slots
advance_cases()    raw geometries of wv_bank_advance inside its documented contract, bad_rows(case) the rows it must skip
detect_cases()     tables of wv_bank_detect_update"""
from __future__ import annotations

import numpy as np

import window_cases as W

SESSION_NETS = (0, 6, 9, 13, 14)
PAD_LIMITS = (1.0, 1.5, float("inf"))
F16_BANKS = ("h.generator", "h.locator", "h.detector", "h.nbits36.detector")
CAPACITY = 6                                                      # the mixed schedule fills every slot at its tick 3


def net_cases():
    """-> (exact cases, f16 cases, f16 cases that must refuse) out of window_cases.net_cases()."""
    nets = W.net_cases()
    exact = [c for c in nets if c[1] == "f32" and c[3][1] in SESSION_NETS]
    f16 = [c for c in nets if c[0] in F16_BANKS]
    refused = [c for c in nets if c[1] == "f16" and c[3][1] in W.F16_REFUSED]
    return exact, f16, refused


# ---- schedules ---------------------------------------------------------------------------------------------------------------------------
def mixed_schedule(hop, H):
    """Six slots.  Tick 3 mixes pushes of 0, 1, hop - 1, hop, hop + 1 and 2 hop + 3 over all six; B dribbles for four ticks without completing
    a frame and closes with a partial one; C pushes more than the history holds, is absent at tick 2 and closes on a hop multiple; D, E and
    F open at tick 3; G takes B's slot over, Z opens and closes without a push (in C's slot); A, D, E, F are each absent somewhere."""
    cap = H + hop
    long_c = cap + hop // 2 + 1
    fill_c = -(hop + long_c + hop - 1) % hop or hop               # brings C to a hop multiple
    return [
        ("open", "A"), ("open", "B"), ("open", "C"),
        ("push", {"A": hop + 1, "B": 1, "C": hop}),
        ("push", {"A": 0, "B": 1, "C": long_c}),
        ("push", {"A": hop - 1, "B": 1}),
        ("open", "D"), ("open", "E"), ("open", "F"),
        ("push", {"A": 0, "B": 1, "C": hop - 1, "D": hop, "E": hop + 1, "F": 2 * hop + 3}),
        ("push", {"A": 1, "B": hop + 1, "C": fill_c, "D": 1, "E": 0}),
        ("close", "B"), ("close", "C"),
        ("open", "G"), ("open", "Z"), ("close", "Z"),
        ("push", {"A": 2 * hop + 3, "D": hop - 1, "F": 1, "G": hop + 1}),
        ("push", {"D": hop, "E": hop - 1, "G": H + 2 * hop + 5}),
        ("push", {"A": 1, "F": hop, "G": 1}),
        ("close", "A"), ("close", "D"), ("close", "E"), ("close", "F"), ("close", "G"),
    ]


def equal_schedule(cfg, S=4):
    """S streams that open together, push the sizes of window_cases' "aligned" schedule (a push beyond the history capacity among them)
    together, then half a hop more so that the close has a partial frame to run, and close together: what a lockstep session of S streams
    does.  -> (steps, sizes)"""
    names = "ABCDEF"[:S]
    sizes = tuple(next(s for n, _, s in W.push_cases(cfg) if n == "aligned")) + (cfg.hop_length // 2 + 1,)
    return ([("open", n) for n in names] + [("push", {n: k for n in names}) for k in sizes] + [("close", n) for n in names]), sizes


def schedules(cfg):
    from waveverify_amd.window import halo
    return [("mixed", mixed_schedule(cfg.hop_length, halo(cfg))), ("equal", equal_schedule(cfg)[0])]


def stream_lengths(steps):
    """-> {stream: samples it pushes in all}, in the order the streams open."""
    out = {}
    for kind, arg in steps:
        if kind == "open":
            out[arg] = 0
        elif kind == "push":
            for name, n in arg.items():
                out[name] += n
    return out


def stream_data(case, steps):
    """-> {stream: (x [T] float32, msg [16] float32)}; a stream of no samples gets an empty x."""
    out = {}
    for i, (name, T) in enumerate(stream_lengths(steps).items()):
        x, msg = W.clip_data(case, max(T, 1), 100 + i)
        out[name] = (x[0, 0, :T], msg[0])
    return out


def run(bank, steps, xs, open_args=lambda name: (), take=lambda x: x):
    """Plays a schedule on a bank -> ({stream: [(step kind, samples pushed so far, result)]}, {stream: slot}).  xs {stream: 1-D samples}."""
    slot, pos, out = {}, {}, {}
    for kind, arg in steps:
        if kind == "open":
            slot[arg], pos[arg], out[arg] = bank.open(*open_args(arg)), 0, []
        elif kind == "close":
            out[arg].append(("close", pos[arg], bank.close(slot[arg])))
        else:
            res = bank.push({slot[name]: take(xs[name][pos[name]: pos[name] + n]) for name, n in arg.items()})
            assert set(res) == {slot[name] for name in arg}
            for name, n in arg.items():
                pos[name] += n
                out[name].append(("push", pos[name], res[slot[name]]))
    return out, slot


# ---- wv_bank_advance ---------------------------------------------------------------------------------------------------------------------
HCAPS = (7, 255, 256, 257, 1025, 2051)
ADVANCE_CAPACITY = 9
ROW_KINDS = ("still", "overlap", "from-x", "hv0", "no-window", "hop")


def advance_case(hcap):
    """-> (capacity, hcap, A, Lmax, n_x, rows, kinds): six of nine slots named, scattered; five window rows of which row 4 is named by nobody.
    Row kinds: still (drop = 0, n = 0: nothing moves), overlap (0 < drop < hv: the shift reads what it overwrites), from-x (drop >= hv, hv2 =
    hcap, wlen = Lmax), hv0 (no history yet), no-window (wlen = 0 among windowed rows), hop (a short window, wlen = 8, beside the longest)."""
    h = hcap
    d = max(1, h // 3)
    n1 = max(1, d - 1)
    geo = {                                                       # slot, hv, n, row, wlen, drop, hv2
        "still": (7, h // 2, 0, 0, 0, 0, h // 2),
        "overlap": (2, h, n1, 2, min(8, h + n1), d, h + n1 - d),
        "from-x": (5, 3, h + 5, 0, h + 8, 8, h),
        "hv0": (0, 0, min(h, 13), 3, min(h, 13), 0, min(h, 13)),
        "no-window": (8, h // 2, 2, 0, 0, 1, h // 2 + 1),
        "hop": (3, min(h, 20), 9, 1, 8, 9, min(h, 20)),
    }
    rows, x_off = [], 3                                           # x starts with three samples nobody reads
    for kind in ROW_KINDS:
        slot, hv, n, row, wlen, drop, hv2 = geo[kind]
        rows.append((slot, hv, x_off, n, row, wlen, drop, hv2))
        x_off += n + (1 if kind == "hv0" else 0)                  # and has a gap
    return ADVANCE_CAPACITY, h, 5, h + 8, x_off + 2, tuple(rows), ROW_KINDS


def advance_cases():
    return [advance_case(h) for h in HCAPS]


def second_tick(case):
    """The tick after advance_case's on the same bank: every named slot's hv is the first tick's hv2 (so what the first tick left beyond hv2
    must not be read), each pushes n = 5 and takes everything as its window."""
    capacity, hcap, _, _, _, rows, _ = case
    out, x_off, Lmax = [], 0, 0
    for r, (slot, _, _, _, _, _, _, hv2) in enumerate(rows):
        hv, n = hv2, 5
        keep = min(hcap, hv + n)
        out.append((slot, hv, x_off, n, r, hv + n, hv + n - keep, keep))
        x_off += n
        Lmax = max(Lmax, hv + n)
    return capacity, hcap, len(rows), Lmax, x_off, tuple(out)


def bad_rows(case):
    """-> [(why, row)]: the `overlap` row of a case changed so that one condition of the contract alone fails."""
    capacity, hcap, A, Lmax, n_x, rows, kinds = case
    slot, hv, x_off, n, row, wlen, drop, hv2 = rows[kinds.index("overlap")]
    return [
        ("slot == capacity", (capacity, hv, x_off, n, row, wlen, drop, hv2)),
        ("slot < 0", (-1, hv, x_off, n, row, wlen, drop, hv2)),
        ("hv > hcap", (slot, hcap + 1, x_off, n, row, wlen, drop + 1, hv2)),
        ("hv < 0", (slot, -1, x_off, n + 1, row, min(wlen, n), drop, hv2)),
        ("hv2 > hcap", (slot, hv, x_off, n, row, wlen, hv + n - hcap - 1, hcap + 1)),
        ("hv2 < 0", (slot, hv, x_off, n, row, wlen, hv + n + 1, -1)),
        ("drop + hv2 != hv + n", (slot, hv, x_off, n, row, wlen, drop, hv2 - 1)),
        ("wlen > hv + n", (slot, 1, x_off, 2, row, 4, 0, 3)),
        ("wlen > Lmax", (slot, hv, x_off, n, row, Lmax + 1, drop, hv2)),
        ("x_off + n > n_x", (slot, hv, n_x - n + 1, n, row, wlen, drop, hv2)),
        ("x_off < 0", (slot, hv, -1, n, row, wlen, drop, hv2)),
        ("row == A", (slot, hv, x_off, n, A, wlen, drop, hv2)),
        ("row < 0", (slot, hv, x_off, n, -1, wlen, drop, hv2)),
    ]


def advance_data(case, seed):
    """-> (hist [capacity, hcap] float32 with the guard's NaN pattern beyond each named slot's hv, x [n_x] float32)."""
    capacity, hcap, _, _, n_x, rows = case[:6]
    rng = np.random.default_rng(W.seed_of("bank advance", hcap, seed))
    hist = rng.standard_normal((capacity, hcap)).astype(np.float32)
    for slot, hv in ((r[0], r[1]) for r in rows):
        hist[slot, hv:].view(np.int32)[:] = 0x7FA5A5A5
    return hist, rng.standard_normal(n_x).astype(np.float32)


# ---- wv_bank_detect_update ---------------------------------------------------------------------------------------------------------------
def detect_cases():
    """-> [(capacity, nb, desc rows (slot, samples))]: scattered slots, a slot that has seen nothing and adds nothing (max(seen, 1)), one row
    whose slot is outside the bank (skipped)."""
    return [(9, nb, ((7, 40), (0, 0), (4, 8), (9, 8), (2, 1000003))) for nb in (1, 16, 36)]
