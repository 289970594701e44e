"""Cases of the native-rate bank tests (tests/test_native_bank_cpu.py, tests/test_gpu_native_bank.py): a plain module, fixed seeds, plain
tuples, importable without a GPU.

STREAMS            the five (rate, channels) of the issue; NAMED gives the mixed schedule's eight stream names a rate and channel count each
schedules(hop, H)  [(name, steps, {stream: (rate, channels)})], a step ("open", stream) | ("push", {stream: n}) | ("close", stream):
                   `mixed` is bank_cases.mixed_schedule with every size scaled by orig / nw of the stream's rate, so frames complete on
                   different ticks per slot; `edges` pushes per rate 0, 1, fewer than width in total, exactly orig, a push that crosses a
                   256-output tile and one longer than ten histories, each stream absent on one tick
equal(sr, hop)     one rate, three streams, the same sizes together: what a lockstep session does
stage_ticks(...)   the plans' ticks of a set of streams, tick by tick, for the two kernels alone
bad_down_rows / bad_up_rows   a served row changed so that one clause of the row rule fails, one per clause"""
from __future__ import annotations

import numpy as np

import bank_cases as BC
from waveverify_amd import native
from waveverify_amd import native_session as NS

M = 16000
STREAMS = ((48000, 2), (44100, 1), (8000, 3), (16000, 1), (22050, 2))
RATES = tuple(sr for sr, _ in STREAMS)
MAX_CHANNELS = 3
NAMED = {"A": (48000, 2), "B": (44100, 1), "C": (8000, 3), "D": (16000, 1), "E": (22050, 2), "F": (44100, 2), "G": (8000, 1), "Z": (48000, 1)}
PEAK = 0.5
HOP, HALO = 16, 40                                   # the toy inner bank of the CPU tests


def scaled(n: int, sr: int) -> int:
    """n 16 kHz samples' worth of samples at sr (rounded up, so 1 stays 1 sample and 0 stays 0)."""
    orig, nw, _, _ = native.table_geometry(sr, M)
    return -(-n * orig // nw)


def mixed(hop: int, H: int):
    steps = []
    for kind, arg in BC.mixed_schedule(hop, H):
        steps.append((kind, {s: scaled(n, NAMED[s][0]) for s, n in arg.items()}) if kind == "push" else (kind, arg))
    return steps, dict(NAMED)


def edge_sizes(sr: int, hop: int, H: int = 0):
    orig, nw, L, width = native.table_geometry(sr, M)
    lat = NS.EmbedPlan(sr, hop, H).latency_samples
    return (0, 1, width // 2, max(0, width - 2 - width // 2), orig, -(-257 * orig // nw), 10 * max(L, lat) + 7, 2)


def edges(hop: int, H: int):
    """Five streams, one per rate; on tick j stream i pushes its j-th edge size, but stream i sits tick i out (its sizes move one tick on)."""
    names = "ABCDE"
    who = {n: STREAMS[i] for i, n in enumerate(names)}
    sizes = {n: list(edge_sizes(who[n][0], hop, H)) for n in names}
    steps = [("open", n) for n in names]
    for j in range(len(sizes["A"]) + 1):
        push = {}
        for i, n in enumerate(names):
            if j != i and sizes[n]:
                push[n] = sizes[n].pop(0)
        steps.append(("push", push))
    return steps + [("close", n) for n in names], who


def schedules(hop: int, H: int):
    return [("mixed",) + mixed(hop, H), ("edges",) + edges(hop, H)]


def equal(sr: int, hop: int, H: int = 0, S: int = 3):
    """-> (steps, {stream: (sr, 2)}, sizes): S streams of one rate that open, push the same sizes and close together."""
    orig, nw, L, _ = native.table_geometry(sr, M)
    sizes = (scaled(hop, sr), 0, 1, scaled(hop - 1, sr), 10 * L + 7, scaled(2 * hop + 3, sr), scaled(hop // 2 + 1, sr))
    names = "ABC"[:S]
    return ([("open", n) for n in names] + [("push", {n: k for n in names}) for k in sizes] + [("close", n) for n in names],
            {n: (sr, 2) for n in names}, sizes)


def stream_data(steps, who, seed: int = 0, dtype=np.float32):
    """-> {stream: x [C, T]} uniform in [-PEAK, PEAK), seeded by the stream."""
    out = {}
    for i, (name, T) in enumerate(BC.stream_lengths(steps).items()):
        sr, C = who[name]
        out[name] = np.random.default_rng([seed, i, sr, C, T]).uniform(-PEAK, PEAK, (C, T)).astype(dtype)
    return out


def run(bank, steps, xs, who, open_args=lambda name: (), take=lambda x: x, after=None):
    """Plays a schedule on a native bank -> ({stream: [(step kind, samples pushed so far, result)]}, {stream: slot}).  after(kind, slots): a hook
    run after every push and close with the slots the step named."""
    slot, pos, out = {}, {}, {}
    for kind, arg in steps:
        if kind == "open":
            slot[arg], pos[arg], out[arg] = bank.open(*open_args(arg), sample_rate=who[arg][0], channels=who[arg][1]), 0, []
        elif kind == "close":
            out[arg].append(("close", pos[arg], bank.close(slot[arg])))
            if after:
                after(kind, [slot[arg]])
        else:
            res = bank.push({slot[name]: take(xs[name][:, pos[name]: pos[name] + n]) for name, n in arg.items()})
            if res is not None:
                assert set(res) == {slot[name] for name in arg}
            for name, n in arg.items():
                pos[name] += n
                out[name].append(("push", pos[name], None if res is None else res[slot[name]]))
            if after:
                after(kind, [slot[name] for name in arg])
    return out, slot


# ---- the two kernels alone ---------------------------------------------------------------------------------------------------------------
STAGE_CAPACITY = 7
STAGE_SLOTS = (5, 0, 3, 6, 1)                        # stream i lives in slot STAGE_SLOTS[i]; slots 2 and 4 are named by nobody
STAGE_GAINS = (1.0, 0.37, 1.0, 0.37, 0.37)


def stage_ticks(hop: int = HOP):
    """-> ([per tick {stream index: EmbedTick}], [per stream its total samples]): the edge sizes of every rate, stream i absent on tick i, a
    stream's flush on the tick after its last push."""
    plans = [NS.EmbedPlan(sr, hop) for sr, _ in STREAMS]
    sizes = [list(edge_sizes(sr, hop)) for sr, _ in STREAMS]
    totals = [sum(s) for s in sizes]
    done = [False] * len(STREAMS)
    ticks, j = [], 0
    while not all(done):
        tick = {}
        for i, plan in enumerate(plans):
            if done[i] or j == i:
                continue
            if sizes[i]:
                tick[i] = plan.push(sizes[i].pop(0))
            else:
                tick[i], done[i] = plan.flush(), True
        ticks.append(tick)
        j += 1
    return ticks, totals


def state_caps(hop: int = HOP):
    """-> (hcap, rcap, pcap) of a bank over RATES: the largest front L, back L and EmbedPlan.pcap."""
    return (max(native.table_geometry(sr, M)[2] for sr in RATES), max(native.table_geometry(M, sr)[2] for sr in RATES),
            max(NS.EmbedPlan(sr, hop).pcap for sr in RATES))


def pack_tick(tick, half):
    """One tick's descriptor tables for the two kernels, every arena with three floats nobody reads in front and a gap of one float between
    rows.  tick {stream index: EmbedTick}, half {slot: 0 / 1} -> dict(front [P, 12], back [P, 15], gain [P], n_x, n_y, n_r, n_out, order)."""
    from waveverify_amd import native_bank as NB
    front, back, gain, at = [], [], [], dict(x=3, y=3, r=3, out=3)
    for i in sorted(tick):
        t, slot, C = tick[i], STAGE_SLOTS[i], STREAMS[i][1]
        front.append(NB.down_row(slot, i, C, t.front, at["x"], at["y"], half[slot]))
        back.append(NB.up_row(slot, i, C, t, at["r"], at["x"], t.front.n, at["out"], half[slot]))
        gain.append(STAGE_GAINS[i])
        at["x"] += C * t.front.n + 1
        at["y"] += t.front.n_out + 1
        at["r"] += t.n_res + 1
        at["out"] += C * t.back.n_out + 1
    return dict(front=np.array(front, np.int64).reshape(-1, 12), back=np.array(back, np.int64).reshape(-1, 15), gain=np.array(gain, np.float32),
                n_x=at["x"] + 2, n_y=at["y"] + 2, n_r=at["r"] + 2, n_out=at["out"] + 2, order=sorted(tick))


def bad_down_rows(row, capacity, hcap, n_x, n_y, geo):
    """-> [(clause, row)] from a served row of wv_native_bank_down; geo [(orig, nw, L, width)] of the call's rate table."""
    slot, rate, C, hv, x_off, n, y_off, n_out, pad, drop, hv2, half = (int(v) for v in row)
    orig, nw, _, width = geo[rate]
    r = dict(slot=slot, rate=rate, C=C, hv=hv, x_off=x_off, n=n, y_off=y_off, n_out=n_out, pad=pad, drop=drop, hv2=hv2, half=half)

    def w(**k):
        d = dict(r, **k)
        return tuple(d[f] for f in ("slot", "rate", "C", "hv", "x_off", "n", "y_off", "n_out", "pad", "drop", "hv2", "half"))
    return [("slot < 0", w(slot=-1)), ("slot == capacity", w(slot=capacity)), ("rate < 0", w(rate=-1)), ("rate == n_rates", w(rate=len(geo))),
            ("C == 0", w(C=0)), ("C == 65", w(C=65)), ("half == 2", w(half=2)), ("half < 0", w(half=-1)),
            ("hv > hcap", w(hv=hcap + 1, drop=drop + hcap + 1 - hv)), ("hv < 0", w(hv=-1, hv2=hv2 - hv - 1)),
            ("hv2 > hcap", w(hv2=hcap + 1, n=n + hcap + 1 - hv2)), ("hv2 < 0", w(hv2=-1, drop=drop + hv2 + 1)),
            ("n < 0", w(n=-1, hv2=0, drop=hv - 1)), ("drop < 0", w(drop=-1, hv2=hv + n + 1)), ("drop + hv2 != hv + n", w(drop=drop + 1)),
            ("pad < 0", w(pad=-1)), ("pad > width", w(pad=width + 1)), ("n_out < 0", w(n_out=-1)),
            ("n_out beyond the inputs", w(n_out=(-(-(hv + n + pad) // orig) + 1) * nw + 1)),
            ("x_off < 0", w(x_off=-1)), ("x_off + C * n > n_x", w(x_off=n_x - C * n + 1)), ("y_off < 0", w(y_off=-1)),
            ("y_off + n_out > n_y", w(y_off=n_y - n_out + 1))]


def bad_up_rows(row, capacity, rcap, pcap, Cmax, n_r, n_x, n_out, geo):
    """-> [(clause, row)] from a served row of wv_native_bank_up_add."""
    slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half = (int(v) for v in row)
    orig, nw, _, width = geo[rate]
    r = dict(slot=slot, rate=rate, C=C, rv=rv, r_off=r_off, nr=nr, x_off=x_off, n=n, out_off=out_off, k=k, pad=pad, rdrop=rdrop, rv2=rv2, pv=pv,
             half=half)

    def w(**kw):
        d = dict(r, **kw)
        return tuple(d[f] for f in ("slot", "rate", "C", "rv", "r_off", "nr", "x_off", "n", "out_off", "k", "pad", "rdrop", "rv2", "pv", "half"))
    return [("slot < 0", w(slot=-1)), ("slot == capacity", w(slot=capacity)), ("rate < 0", w(rate=-1)), ("rate == n_rates", w(rate=len(geo))),
            ("C == 0", w(C=0)), ("C > Cmax", w(C=Cmax + 1)), ("half == 2", w(half=2)), ("half < 0", w(half=-1)),
            ("rv > rcap", w(rv=rcap + 1, rdrop=rdrop + rcap + 1 - rv)), ("rv < 0", w(rv=-1, rv2=rv2 - rv - 1)),
            ("rv2 > rcap", w(rv2=rcap + 1, nr=nr + rcap + 1 - rv2)), ("rv2 < 0", w(rv2=-1, rdrop=rdrop + rv2 + 1)),
            ("nr < 0", w(nr=-1, rv2=0, rdrop=rv - 1)), ("rdrop < 0", w(rdrop=-1, rv2=rv + nr + 1)), ("rdrop + rv2 != rv + nr", w(rdrop=rdrop + 1)),
            ("pv < 0", w(pv=-1)), ("pv > pcap", w(pv=pcap + 1)), ("n < 0", w(n=-1)), ("k < 0", w(k=-1)), ("pv2 < 0", w(k=pv + n + 1)),
            ("pv2 > pcap", w(pv=pcap, k=0, n=1)),
            ("pad < 0", w(pad=-1)), ("pad > width", w(pad=width + 1)), ("k beyond the residual", w(k=(-(-(rv + nr + pad) // orig) + 1) * nw + 1)),
            ("r_off < 0", w(r_off=-1)), ("r_off + nr > n_r", w(r_off=n_r - nr + 1)), ("x_off < 0", w(x_off=-1)),
            ("x_off + C * n > n_x", w(x_off=n_x - C * n + 1)), ("out_off < 0", w(out_off=-1)), ("out_off + C * k > n_out", w(out_off=n_out - C * k + 1))]
