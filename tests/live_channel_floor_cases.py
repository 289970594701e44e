"""Cases of the live per-channel SNR floor tests (tests/test_live_channel_floor_cpu.py, tests/test_gpu_live_channel_floor.py; DESIGN.md section
7d-13): a plain module, fixed seeds, importable without a GPU.

GEOMETRIES         (sample rate, hop): 48000 / 16 a whole ratio, frames of 48; 44100 / 16 frames of 44 and 45, not phase-group aligned; 11025 / 320
                   frames of 220 and 221 and 11025 / 16 of 11 and 12; 8000 / 1 every second frame EMPTY (its gain is the cap); 16000 / 16 the
                   one-tap table
schedules(sr, hop) [(name, push sizes)] of ONE stream, closed after its last push: close only, one sample, pushes of 0, pushes shorter than a
                   frame (some ticks emit nothing), a push ending one sample before, on and after a frame's start, one push longer than two
                   workgroups' frames plus the delay line, totals under one frame, on a frame's edge and inside a frame
mixed(hop, H)      native_bank_cases' scaled 10 / 20 / 60-style mix (bank_cases.mixed_schedule), over these rates, C in {1, 2, 3}
stream_x(...)      a stream's samples: per-frame envelopes over 1e-3 .. 0.5, so that gains rise, fall, reach the cap and stay under it; a
                   silent channel holds +0 and -0
floor_ticks / pack_floor_tick / bad_floor_rows     the plans' ticks of five streams for the entry point alone, one tick's tables, and a served row
                   changed so that one clause of the row rule fails, one per clause"""
from __future__ import annotations

import numpy as np

import bank_cases as BC
import native_bank_cases as NBC
from waveverify_amd import channel_floor as CF
from waveverify_amd import native
from waveverify_amd import native_bank as NB
from waveverify_amd import native_session as NS
from waveverify_amd import snr_floor

M = 16000
HALO = 40
MIN_SNR_DB = 20.0
RHO = snr_floor.rho_of(MIN_SNR_DB)
GEOMETRIES = ((48000, 16), (44100, 16), (11025, 320), (11025, 16), (8000, 1), (16000, 16))
GEO_IDS = [f"{sr}.hop{hop}" for sr, hop in GEOMETRIES]
MAX_CHANNELS = 3
MIX_RATES = (48000, 44100, 8000, 16000, 11025)
MIX_NAMED = {"A": (48000, 2), "B": (44100, 1), "C": (8000, 3), "D": (16000, 1), "E": (11025, 2), "F": (44100, 2), "G": (8000, 1), "Z": (48000, 1)}
MIX_HOP = 16


def back(sr: int):
    """(orig, nw, L, width) of the back table, 16 kHz -> sr."""
    return native.table_geometry(M, sr)


def start(f: int, sr: int, hop: int) -> int:
    orig, nw, _, _ = back(sr)
    return -(-f * nw * hop // orig)


def schedules(sr: int, hop: int):
    orig, nw, L, _ = back(sr)
    Lf = -(-nw * hop // orig)
    NF = NB.floor_tile_frames(orig, nw, L, hop)
    lat = NS.EmbedPlan(sr, hop, HALO, True).latency_samples
    s = lambda f: start(f, sr, hop)                                            # noqa: E731
    step, forig = max(1, Lf // 3), native.table_geometry(sr, M)[0]
    return [("close only", ()), ("one sample", (1,)), ("zeros", (0, 0, 5, 0)),
            ("dribble", (lat,) + (step,) * -(-(2 * forig + 3 * Lf) // step)),   # the stages filled, then two front phase groups and three frames in pushes shorter than a frame
            ("edges", (s(7) - 1, 1, 1, 2 * lat, s(3) + 1)),                     # the stream's length passes start(7) - 1, start(7), start(7) + 1
            ("long", (3, s(2 * NF + 3) + lat, 2)),                              # a row of more than two workgroups' frames
            ("under a frame", (max(1, Lf - 1),)), ("on an edge", (s(5 + (s(5) == s(4))),)), ("inside a frame", (s(6) + max(1, Lf // 2),))]


def mixed(hop: int = MIX_HOP, H: int = HALO):
    steps = []
    for kind, arg in BC.mixed_schedule(hop, H):
        steps.append((kind, {n: NBC.scaled(k, MIX_NAMED[n][0]) for n, k in arg.items()}) if kind == "push" else (kind, arg))
    return steps, dict(MIX_NAMED)


def stream_x(sr: int, hop: int, C: int, T: int, seed, silent=None) -> np.ndarray:
    """[C, T] float32; channel `silent` is zeros of both signs."""
    rng = np.random.default_rng([int(v) for v in np.atleast_1d(seed)] + [sr, hop, C, T])
    x = np.zeros((C, T), np.float32)
    if T == 0:
        return x
    orig, nw, _, _ = back(sr)
    f = CF.frame_of(np.arange(T), orig, nw, hop)
    for c in range(C):
        env = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), int(f[-1]) + 1))
        x[c] = (rng.standard_normal(T) * env[f]).clip(-1, 1)
    if silent is not None:
        x[silent] = np.where(rng.integers(0, 2, T) == 1, np.float32(-0.0), np.float32(0.0))
    return x


def whole_u(residual: np.ndarray, sr: int, Tn: int) -> np.ndarray:
    """u [Tn] of the twin: the whole 16 kHz residual through the back stage's chain on numpy (native_session.numpy_resample), cut to Tn."""
    _, _, _, width = back(sr)
    r = np.asarray(residual).reshape(1, -1)
    return NS.numpy_resample(r, width, Tn, native.transposed_table(M, sr))[0].astype(np.float32)


def twin(x: np.ndarray, u: np.ndarray, sr: int, hop: int, s, rho: float = RHO):
    """channel_floor.numpy_channel_floor on the whole stream -> (out [C, Tn], g [C, F]); an empty stream gives two empty arrays."""
    if x.shape[1] == 0:
        return np.zeros((x.shape[0], 0), np.float32), np.zeros((x.shape[0], 0), np.float32)
    orig, nw, _, _ = back(sr)
    return CF.numpy_channel_floor(x, u, orig, nw, hop, s, rho)


# ---- the entry point alone ---------------------------------------------------------------------------------------------------------------
STAGE_STREAMS = ((48000, 2), (44100, 1), (8000, 3), (16000, 1), (11025, 2))     # five rates in one call
STAGE_RATES = tuple(sr for sr, _ in STAGE_STREAMS)
STAGE_CAPACITY = 7
STAGE_SLOTS = (5, 0, 3, 6, 1)                        # slots 2 and 4 are named by nobody
STAGE_CAPS = (1.0, 0.37, 1.0, 0.75, 0.5)
STAGE_HOP = 16


def stage_sizes(sr: int, hop: int = STAGE_HOP):
    orig, nw, L, _ = back(sr)
    Lf = -(-nw * hop // orig)
    NF = NB.floor_tile_frames(orig, nw, L, hop)
    lat = NS.EmbedPlan(sr, hop, 0, True).latency_samples
    return (0, 1, max(1, Lf // 3), max(1, Lf // 3), start(4, sr, hop), lat, start(NF + 2, sr, hop) + lat, 2)


def floor_ticks(hop: int = STAGE_HOP):
    """-> ([per tick {stream index: EmbedTick}], [per stream its total samples]): stream i sits tick i out; a stream's flush on the tick after
    its last push."""
    plans = [NS.EmbedPlan(sr, hop, 0, True) for sr, _ in STAGE_STREAMS]
    sizes = [list(stage_sizes(sr, hop)) for sr, _ in STAGE_STREAMS]
    totals = [sum(s) for s in sizes]
    done = [False] * len(plans)
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


def state_caps(hop: int = STAGE_HOP):
    """-> (rcap, pcap, ucap) of a bank over STAGE_RATES under the floor."""
    plans = [NS.EmbedPlan(sr, hop, 0, True) for sr in STAGE_RATES]
    return max(back(sr)[2] for sr in STAGE_RATES), max(p.pcap for p in plans), max(p.ucap for p in plans)


def pack_floor_tick(tick, half):
    """One tick's table for wv_native_bank_floor_up_add, every arena with three floats nobody reads in front and a gap of one float between rows.
    -> dict(back [P, 21], cap [P], n_x, n_r, n_out, n_gains, order)."""
    rows, caps, at = [], [], dict(x=3, r=3, out=3, g=3)
    for i in sorted(tick):
        t, slot, C = tick[i], STAGE_SLOTS[i], STAGE_STREAMS[i][1]
        rows.append(NB.floor_up_row(slot, i, C, t, at["r"], at["x"], t.front.n, at["out"], half[slot], at["g"]))
        caps.append(STAGE_CAPS[i])
        at["x"] += C * t.front.n + 1
        at["r"] += t.n_res + 1
        at["out"] += C * t.floor.k + 1
        at["g"] += C * t.floor.nf + 1
    return dict(back=np.array(rows, np.int64).reshape(-1, NB.FLOOR_DESC), cap=np.array(caps, np.float32), n_x=at["x"] + 2, n_r=at["r"] + 2,
                n_out=at["out"] + 2, n_gains=at["g"] + 2, order=sorted(tick))


FIELDS = ("slot", "rate", "C", "rv", "r_off", "nr", "x_off", "n", "out_off", "k", "pad", "rdrop", "rv2", "pv", "half", "f0", "nf", "uv", "uv2",
          "g_off", "final")


def bad_floor_rows(row, capacity, rcap, pcap, ucap, Cmax, n_r, n_x, n_out, n_gains, geo, hop):
    """-> [(clause, row)] from a served row of wv_native_bank_floor_up_add; geo [(orig, nw, L, width)] of the call's rate table.  Every bad row
    breaks the named clause (some break a neighbour too: a row has to fail, not to fail for one reason only)."""
    r = dict(zip(FIELDS, (int(v) for v in row)))
    orig, nw, _, width = geo[r["rate"]]
    Mh = nw * hop
    nu = r["k"] + r["uv2"] - r["uv"]

    def w(**kw):
        d = dict(r, **kw)
        return tuple(d[f] for f in FIELDS)
    whole = -(-(r["f0"] + r["nf"]) * Mh // orig) - -(-r["f0"] * Mh // orig)
    over = whole + 1 - r["k"] if r["final"] else 1                              # a cut last frame may hold any part of its nominal length
    bad = [("slot < 0", w(slot=-1)), ("slot == capacity", w(slot=capacity)), ("rate < 0", w(rate=-1)), ("rate == n_rates", w(rate=len(geo))),
           ("C == 0", w(C=0)), ("C > Cmax", w(C=Cmax + 1)), ("half == 2", w(half=2)), ("half < 0", w(half=-1)),
           ("rv > rcap", w(rv=rcap + 1, rdrop=r["rdrop"] + rcap + 1 - r["rv"])), ("rv < 0", w(rv=-1, rv2=r["rv2"] - r["rv"] - 1)),
           ("rv2 > rcap", w(rv2=rcap + 1, nr=r["nr"] + rcap + 1 - r["rv2"])), ("rv2 < 0", w(rv2=-1, rdrop=r["rdrop"] + r["rv2"] + 1)),
           ("nr < 0", w(nr=-1, rv2=0, rdrop=r["rv"] - 1)), ("rdrop < 0", w(rdrop=-1, rv2=r["rv"] + r["nr"] + 1)),
           ("rdrop + rv2 != rv + nr", w(rdrop=r["rdrop"] + 1)),
           ("pv < 0", w(pv=-1)), ("pv > pcap", w(pv=pcap + 1)), ("n < 0", w(n=-1)), ("k < 0", w(k=-1)), ("pv2 < 0", w(n=r["k"] - r["pv"] - 1)),
           ("pv2 > pcap", w(n=r["k"] - r["pv"] + pcap + 1)),
           ("pad < 0", w(pad=-1)), ("pad > width", w(pad=width + 1)),
           ("new u beyond the residual", w(uv2=r["uv2"] + (-(-(r["rv"] + r["nr"] + r["pad"]) // orig) + 1) * nw + 1 - nu)),
           ("new u < 0", w(uv=r["uv"] + nu + 1)), ("uv < 0", w(uv=-1)), ("uv > ucap", w(uv=ucap + 1)), ("uv2 < 0", w(uv2=-1)),
           ("uv2 > ucap", w(uv2=ucap + 1)), ("final == 2", w(final=2)), ("final < 0", w(final=-1)),
           ("f0 < 0", w(f0=-1)), ("nf < 0", w(nf=-1)), ("f0 beyond int64's frames", w(f0=2 ** 62 // Mh + 1)),
           ("k is not the frames'", w(k=r["k"] + over, n=r["n"] + over)), ("one frame more", w(nf=r["nf"] + 2)),
           ("r_off < 0", w(r_off=-1)), ("r_off + nr > n_r", w(r_off=n_r - r["nr"] + 1)), ("x_off < 0", w(x_off=-1)),
           ("x_off + C * n > n_x", w(x_off=n_x - r["C"] * r["n"] + 1)), ("out_off < 0", w(out_off=-1)),
           ("out_off + C * k > n_out", w(out_off=n_out - r["C"] * r["k"] + 1)), ("g_off < -1", w(g_off=-2)),
           ("g_off + C * nf > n_gains", w(g_off=n_gains - r["C"] * r["nf"] + 1))]
    if r["final"]:
        bad.append(("final with u held", w(uv2=1, k=r["k"] - 1)))
        if r["nf"]:
            bad.append(("final cut before its last frame", w(k=0, uv=0, n=0, pv=0)))
    else:
        bad.append(("final with u held", w(final=1)) if r["uv2"] else ("a whole frame short", w(nf=r["nf"] + 1)))
    return bad
