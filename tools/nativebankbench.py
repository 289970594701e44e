"""Cost of a native-rate session bank's tick against the routes that exist without it -> profiles/native_bank_bench.json.

    python tools/nativebankbench.py [--reps 15] [--out profiles/native_bank_bench.json]

The default full-size nets with seeded random weights, exact and f16, embed and detect.  48 streams over one second of stream time, a third each
at 48 kHz stereo, 44.1 kHz stereo and 8 kHz mono, and within every rate a third each on 10, 20 and 60 ms packets, all in phase.  Every time is
the host clock around one push that ends in a device synchronise; each repetition opens its banks and sessions afresh, repetition 0 warms up, and
the figures are medians over the repetitions with their min and max (the spread).  Within a repetition the contenders take turns tick by tick
(interleaved).  0.4 s of stream time fills the histories, then the pushes of one second are timed and summed: milliseconds of device time per
second of audio.
    native_bank              ONE native bank ticked every 10 ms (a slot is named on the ticks its packet is due)
    nine_lockstep_sessions   (a) one lockstep Native*Session per (rate, packet size) group: the only route without the bank
    bank_16k_preresampled    (b) the 16 kHz bank given every stream's 16 kHz copy (made beforehand, untimed) in packets of the same duration:
                             the difference to native_bank is what the two stage launches and their table add per tick
    kernels                  wv_native_bank_down and wv_native_bank_up_add alone on the 48 rows of a tick on which every packet is due
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
from waveverify_amd import _lib, native  # noqa: E402
from waveverify_amd import native_bank as NB  # noqa: E402
from waveverify_amd import native_session as NS  # noqa: E402
from waveverify_amd.core import WaveVerify  # noqa: E402

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


def groups():
    """-> [(rate, channels, packet ms, [streams])]: the nine lockstep groups."""
    out = []
    for g, (sr, C) in enumerate(STREAMS):
        for ms in PACKETS_MS:
            out.append((sr, C, ms, [s for s in range(16 * g, 16 * g + 16) if packet_of(s) == ms]))
    return out


def opened(wv, kind):
    """-> (native bank with S open slots, the nine lockstep native sessions, the 16 kHz bank with S open slots)."""
    if kind == "embed":
        nb, b16 = wv.open_embed_bank(S, rates=RATES), wv.open_embed_bank(S)
        slots = [nb.open(s + 1, sample_rate=rate_of(s)[0], channels=rate_of(s)[1]) for s in range(S)]
        slots16 = [b16.open(s + 1) for s in range(S)]
        sessions = [wv.open_embed_session([s + 1 for s in members], sample_rate=sr, channels=C) for sr, C, _, members in groups()]
    else:
        nb, b16 = wv.open_detect_bank(S, rates=RATES), wv.open_detect_bank(S)
        slots = [nb.open(sample_rate=rate_of(s)[0], channels=rate_of(s)[1]) for s in range(S)]
        slots16 = [b16.open() for _ in range(S)]
        sessions = [wv.open_detect_session(len(members), sample_rate=sr, channels=C) for sr, C, _, members in groups()]
    assert slots == slots16 == list(range(S))
    return nb, sessions, b16


def scenario(wv, kind, reps):
    x = audio(1)
    x16 = [native.downmix_resample(x[s][None], rate_of(s)[0])[0, 0] for s in range(S)]
    stacked = [torch.stack([x[s] for s in members]) for _, _, _, members in groups()]
    names = ("native_bank", "nine_lockstep_sessions", "bank_16k_preresampled")
    totals, counts = {n: [] for n in names}, {}
    for rep in range(reps + 1):
        nb, sessions, b16 = opened(wv, kind)
        spent = {n: 0.0 for n in names}
        for tick in range(PREROLL + TICKS):
            on = tick >= PREROLL
            if tick == PREROLL:
                before = dict(nb.stats)
            items, items16 = {}, {}
            for s in range(S):
                ms = packet_of(s)
                if due(tick, ms):
                    end, n = rate_of(s)[0] * (tick + 1) // 100, rate_of(s)[0] * ms // 1000
                    items[s] = x[s][:, end - n:end]
                    items16[s] = x16[s][160 * (tick + 1) - 16 * ms:160 * (tick + 1)]
            t = timed(lambda: nb.push(items))
            spent["native_bank"] += t if on else 0.0
            for (sr, C, ms, members), sess, xs in zip(groups(), sessions, stacked):
                if due(tick, ms):
                    end, n = sr * (tick + 1) // 100, sr * ms // 1000
                    t = timed(lambda: sess.push(xs[:, :, end - n:end]))
                    spent["nine_lockstep_sessions"] += t if on else 0.0
            t = timed(lambda: b16.push(items16))
            spent["bank_16k_preresampled"] += t if on else 0.0
        if rep:
            for n in names:
                totals[n].append(spent[n])
            counts = {k: nb.stats[k] - before[k] for k in nb.stats}
    out = {n: {"device_ms_per_second_of_audio": stat(v)} for n, v in totals.items()}
    med = {n: statistics.median(v) for n, v in totals.items()}
    out["native_bank"].update(over_nine_lockstep_sessions=med["native_bank"] / med["nine_lockstep_sessions"],
                              minus_bank_16k_ms=med["native_bank"] - med["bank_16k_preresampled"],
                              minus_bank_16k_us_per_tick=(med["native_bank"] - med["bank_16k_preresampled"]) * 1e3 / TICKS,
                              stage_counters_per_second=counts)
    for n in names[1:]:
        out[n]["spread_ms"] = max(totals[n]) - min(totals[n])
    return out


def kernels(wv, reps):
    """The two stage launches alone, on the descriptors of a tick on which all 48 packets are due (0.48 s into the streams)."""
    lib, dev = _lib.load(), wv.device
    cfg = wv.configs["generator"]
    from waveverify_amd.window import halo
    plans = [NS.EmbedPlan(rate_of(s)[0], cfg.hop_length, halo(cfg)) for s in range(S)]
    for t in range(PREROLL + 8):                                      # tick 47 ends at 480 ms: every packet size is due on it
        tick = {s: plans[s].push(rate_of(s)[0] * packet_of(s) // 1000) for s in range(S) if due(t, packet_of(s))}
    assert len(tick) == S
    front, back, at = [], [], dict(x=0, y=0, r=0, out=0)
    for s, t in tick.items():
        C = rate_of(s)[1]
        front.append(NB.down_row(s, s // 16, C, t.front, at["x"], at["y"], 0))
        back.append(NB.up_row(s, s // 16, C, t, at["r"], at["x"], t.front.n, at["out"], 0))
        at["x"] += C * t.front.n
        at["y"] += t.front.n_out
        at["r"] += t.n_res
        at["out"] += C * t.back.n_out
    pairs = [native.tables(sr, dev) for sr in RATES]
    mk = lambda ts: (_lib.WvNativeRate * len(ts))(*[_lib.WvNativeRate(t[0].data_ptr(), *t[1:]) for t in ts])      # noqa: E731
    ftab, btab = mk([p[0] for p in pairs]), mk([p[1] for p in pairs])
    hcap, rcap, pcap = max(p[0][3] for p in pairs), max(p[1][3] for p in pairs), max(p.pcap for p in plans)
    z = lambda *shape: torch.zeros(shape, device=dev)                 # noqa: E731
    hist, rhist, pend = z(S, 2, hcap), z(S, 2, rcap), z(S, 2, 2, pcap)
    x, r, y, out = torch.rand(max(1, at["x"]), device=dev), torch.rand(max(1, at["r"]), device=dev), z(max(1, at["y"])), z(max(1, at["out"]))
    fd, bd = torch.tensor(front, dtype=torch.int64, device=dev), torch.tensor(back, dtype=torch.int64, device=dev)
    gain = torch.ones(S, device=dev)
    fb, bb = NB.down_blocks(front), NB.up_blocks(back)
    down = lambda: _lib.check(lib.wv_native_bank_down(hist.data_ptr(), S, hcap, x.data_ptr(), at["x"], ftab, len(RATES), fd.data_ptr(), S, fb,
                                                      y.data_ptr(), at["y"], _lib.stream()))
    up = lambda: _lib.check(lib.wv_native_bank_up_add(rhist.data_ptr(), rcap, pend.data_ptr(), pcap, 2, S, r.data_ptr(), at["r"], x.data_ptr(), at["x"],
                                                      btab, len(RATES), bd.data_ptr(), gain.data_ptr(), S, bb, out.data_ptr(), at["out"], _lib.stream()))
    td, tu = [], []
    for rep in range(reps + 1):
        pd, pu = [], []
        for _ in range(50):
            pd.append(timed(down))
            pu.append(timed(up))
        if rep:
            td.append(statistics.median(pd))
            tu.append(statistics.median(pu))
    return {"rows": S, "samples_in": at["x"], "samples_out": at["out"], "native_bank_down_ms": stat(td), "native_bank_up_add_ms": stat(tu)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "native_bank_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nativebankbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "streams": S, "scenario": {}, "kernels": kernels(wv, a.reps)}
    for precision in ("f32", "f16"):
        wv.set_precision(precision)
        for kind in ("embed", "detect"):
            res["scenario"][f"{kind}_{precision}"] = scenario(wv, kind, a.reps)
            print(json.dumps(res["scenario"]), flush=True)
    wv.set_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
