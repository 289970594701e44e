"""Cost of the live per-channel SNR floor -> profiles/live_channel_floor_bench.json.

    python tools/livechannelfloorbench.py [--reps 15] [--out profiles/live_channel_floor_bench.json]

The default full-size generator with seeded random weights, exact and f16.  The scenario is section 7d-8's: 48 streams over one second of stream
time, a third each at 48 kHz stereo, 44.1 kHz stereo and 8 kHz mono, and within every rate a third each on 10, 20 and 60 ms packets, all in phase.
Every time is the host clock around one push that ends in a device synchronise; each repetition opens its banks afresh, repetition 0 warms up, and
the figures are medians over the repetitions with their min and max (the spread).  The yardstick is the SAME bank with the floor off in the same
run, tick by tick in turn (interleaved).  0.4 s of stream time fills the histories, then the pushes of one second are timed and summed:
milliseconds of device time per second of audio.
    scenario   NativeEmbedBank with set_channel_snr_floor(20) against without; `beyond_spread` says whether the difference of the medians is larger
               than the floor-less bank's own max - min
    kernels    wv_native_bank_floor_up_add alone against wv_native_bank_up_add alone, each on the 48 rows of that scenario's tick on which every
               packet is due (the floor's rows emit whole frames, so the two write different sample counts: both are recorded)
    added_lag_ms   one nominal native frame per rate, from the plan; not measured
No bar is set on any of these: they are recorded."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import _lib, native, snr_floor  # noqa: E402
from waveverify_amd import native_bank as NB  # noqa: E402
from waveverify_amd import native_session as NS  # noqa: E402
from waveverify_amd.core import WaveVerify  # noqa: E402

DB = 20.0
STREAMS = ((48000, 2), (44100, 2), (8000, 1))
RATES = tuple(sr for sr, _ in STREAMS)
PACKETS_MS = (10, 20, 60)
S, PREROLL, TICKS = 48, 40, 100                                      # 10 ms ticks: 0.4 s un-timed, then one second


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def rate_of(s):
    return STREAMS[s // 16]


def packet_of(s):
    return PACKETS_MS[s % 3]


def due(tick, ms):
    return (tick + 1) * 10 % ms == 0


def audio(seed):
    out = []
    for s in range(S):
        sr, C = rate_of(s)
        rng = np.random.default_rng([sr, s, seed])
        out.append(torch.from_numpy(np.clip(0.1 * rng.standard_normal((C, sr * (PREROLL + TICKS) // 100), dtype=np.float32), -1, 1)).cuda())
    return out


def opened(wv, db):
    bank = wv.open_native_embed_bank(RATES, S, channel_snr_floor_db=db)
    assert [bank.open(s + 1, sample_rate=rate_of(s)[0], channels=rate_of(s)[1]) for s in range(S)] == list(range(S))
    return bank


def scenario(wv, reps):
    x = audio(1)
    names = ("no_floor", "floor")
    totals, counts, down = {n: [] for n in names}, {}, []
    for rep in range(reps + 1):
        banks = {"no_floor": opened(wv, None), "floor": opened(wv, DB)}
        spent = {n: 0.0 for n in names}
        for tick in range(PREROLL + TICKS):
            if tick == PREROLL:
                before = {n: dict(b.stats) for n, b in banks.items()}
            items = {}
            for s in range(S):
                ms = packet_of(s)
                if due(tick, ms):
                    end, n = rate_of(s)[0] * (tick + 1) // 100, rate_of(s)[0] * ms // 1000
                    items[s] = x[s][:, end - n:end]
            for n in names:
                t = timed(lambda: banks[n].push(items))
                spent[n] += t if tick >= PREROLL else 0.0
            if rep == 1 and tick == PREROLL + 7:                       # every packet is due: how many frames the floor turns down
                g = torch.cat([banks["floor"].gains(s).reshape(-1) for s in items])
                down.append(float((g < 1).float().mean()))
        if rep:
            for n in names:
                totals[n].append(spent[n])
            counts = {n: {k: banks[n].stats[k] - before[n][k] for k in banks[n].stats} for n in names}
    off, on = stat(totals["no_floor"]), stat(totals["floor"])
    return {"no_floor_ms_per_second_of_audio": off, "floor_ms_per_second_of_audio": on, "over": on["median"] / off["median"],
            "added_us_per_tick": (on["median"] - off["median"]) * 1e3 / TICKS,
            "beyond_spread": bool(on["median"] - off["median"] > off["max"] - off["min"]), "gains_under_the_cap": down[0] if down else None,
            "stage_counters_per_second": counts}


def kernels(wv, reps):
    """The two back launches alone, each on the rows of its own plan's tick on which all 48 packets are due (0.48 s into the streams)."""
    lib, dev = _lib.load(), wv.device
    cfg = wv.configs["generator"]
    from waveverify_amd.window import halo
    hop, H = cfg.hop_length, halo(cfg)
    out = {"rows": S}
    pairs = [native.tables(sr, dev) for sr in RATES]
    btab = (_lib.WvNativeRate * len(pairs))(*[_lib.WvNativeRate(p[1][0].data_ptr(), *p[1][1:]) for p in pairs])
    geo = [tuple(p[1][1:]) for p in pairs]
    z = lambda *shape: torch.zeros(shape, device=dev)                 # noqa: E731
    calls = {}
    for floor in (False, True):
        plans = [NS.EmbedPlan(rate_of(s)[0], hop, H, floor) for s in range(S)]
        for t in range(PREROLL + 8):                                  # tick 47 ends at 480 ms: every packet size is due on it
            tick = {s: plans[s].push(rate_of(s)[0] * packet_of(s) // 1000) for s in range(S) if due(t, packet_of(s))}
        assert len(tick) == S
        rows, at = [], dict(x=0, r=0, out=0, g=0)
        for s, t in tick.items():
            C = rate_of(s)[1]
            k = t.floor.k if floor else t.back.n_out
            rows.append(NB.floor_up_row(s, s // 16, C, t, at["r"], at["x"], t.front.n, at["out"], 0, at["g"]) if floor else
                        NB.up_row(s, s // 16, C, t, at["r"], at["x"], t.front.n, at["out"], 0))
            at["x"] += C * t.front.n
            at["r"] += t.n_res
            at["out"] += C * k
            at["g"] += C * t.floor.nf if floor else 0
        rcap, pcap = max(g[2] for g in geo), max(p.pcap for p in plans)
        rhist, pend = z(S, 2, rcap), z(S, 2, 2, pcap)
        x, r, o = 0.1 * torch.randn(max(1, at["x"]), device=dev), 0.01 * torch.randn(max(1, at["r"]), device=dev), z(max(1, at["out"]))
        d = torch.tensor(rows, dtype=torch.int64, device=dev)
        gain = torch.ones(S, device=dev)
        if floor:
            ucap = max(p.ucap for p in plans)
            uhold, gprev, gains = z(S, 2, ucap), z(S, 2, 2), z(max(1, at["g"]))
            blocks = NB.floor_up_blocks(rows, geo, hop)
            calls["floor"] = (lambda a=dict(at), rhist=rhist, pend=pend, x=x, r=r, o=o, d=d, gain=gain, rcap=rcap, pcap=pcap: _lib.check(
                lib.wv_native_bank_floor_up_add(rhist.data_ptr(), rcap, pend.data_ptr(), pcap, uhold.data_ptr(), ucap, gprev.data_ptr(), 2, S, r.data_ptr(),
                                                a["r"], x.data_ptr(), a["x"], btab, len(RATES), d.data_ptr(), gain.data_ptr(), S, blocks, hop,
                                                snr_floor.rho_of(DB), o.data_ptr(), a["out"], gains.data_ptr(), a["g"], _lib.stream())))
            out["floor_up_add"] = {"samples_in": at["x"], "samples_out": at["out"], "frames": at["g"], "blocks": blocks}
        else:
            bb = NB.up_blocks(rows)
            calls["plain"] = (lambda a=dict(at), rhist=rhist, pend=pend, x=x, r=r, o=o, d=d, gain=gain, rcap=rcap, pcap=pcap, bb=bb: _lib.check(
                lib.wv_native_bank_up_add(rhist.data_ptr(), rcap, pend.data_ptr(), pcap, 2, S, r.data_ptr(), a["r"], x.data_ptr(), a["x"], btab, len(RATES),
                                          d.data_ptr(), gain.data_ptr(), S, bb, o.data_ptr(), a["out"], _lib.stream())))
            out["up_add"] = {"samples_in": at["x"], "samples_out": at["out"], "blocks": bb}
    tp, tf = [], []
    for rep in range(reps + 1):
        a, b = [], []
        for _ in range(50):
            a.append(timed(calls["plain"]))
            b.append(timed(calls["floor"]))
        if rep:
            tp.append(statistics.median(a))
            tf.append(statistics.median(b))
    out["up_add"]["ms"], out["floor_up_add"]["ms"] = stat(tp), stat(tf)
    out["over"] = out["floor_up_add"]["ms"]["median"] / out["up_add"]["ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "live_channel_floor_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("livechannelfloorbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    cfg = wv.configs["generator"]
    from waveverify_amd.window import halo
    lag = {sr: 1e3 * NS.EmbedPlan(sr, cfg.hop_length, halo(cfg), True).ucap / sr for sr in RATES}
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "streams": S, "min_snr_db": DB, "hop": cfg.hop_length, "added_lag_ms": lag,
           "kernels": kernels(wv, a.reps), "scenario": {}}
    print(json.dumps(res["kernels"]), flush=True)
    for precision in ("f32", "f16"):
        wv.set_precision(precision)
        res["scenario"][precision] = scenario(wv, a.reps)
        print(json.dumps(res["scenario"]), flush=True)
    wv.set_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
