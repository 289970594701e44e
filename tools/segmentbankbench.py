"""Cost of a segment bank's tick against the lockstep segment sessions -> profiles/segment_bank_bench.json.

    python tools/segmentbankbench.py [--reps 15] [--out profiles/segment_bank_bench.json]

The default full-size nets with seeded random weights, exact and f16, locator-driven (the form a monitoring server runs).  Every time is the
host clock around one push that ends in a device synchronise; each repetition opens its banks and sessions afresh, repetition 0 warms up,
and the figures are medians over the repetitions with their min and max (the spread).  Within a repetition the contenders take turns push by
push (interleaved).
    (a) equal   S = 1, 16, 64 streams that all push 20 ms (320 samples): SegmentBank.push of S slots against SegmentSession.push of [S, 320],
                50 pushes, the first 20 (the halo still filling) left out; the difference stands next to the lockstep push's own spread.
    (b) mixed   48 streams, 16 each on 10, 20 and 60 ms packets, all in phase: ONE segment bank ticked every 10 ms at pad_limit 1.0, 1.5 and
                none, against the three lockstep SegmentSessions of 16 streams.  0.4 s of stream time fills the halos, then the pushes of one
                second are timed and summed: milliseconds of device time per second of audio.  padded_share: samples run only as right
                padding / samples run; net_launches_per_second: window batches (each is one locator and one detector forward).
    (c) kernel  wv_bank_segment_track alone: 64 rows of one new frame each, 16 bits.
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
from waveverify_amd import ops  # noqa: E402
from waveverify_amd.core import WaveVerify  # noqa: E402

PUSH, PUSHES, SKIP = 320, 50, 20
TICK, PREROLL, TICKS = 160, 40, 100                                  # 10 ms ticks: 0.4 s un-timed, then one second
PACKETS = (160, 320, 960)
PAD_LIMITS = (("1.0", 1.0), ("1.5", 1.5), ("none", float("inf")))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def audio(S, n, seed):
    rng = np.random.default_rng([16000, S, seed])
    return torch.from_numpy(np.clip(0.1 * rng.standard_normal((S, n), dtype=np.float32), -1, 1)).cuda()


def opened(wv, S, pad=1.5):
    """-> (segment bank with S open slots, lockstep segment session of S streams)."""
    bank, sess = wv.open_segment_bank(S, pad), wv.open_segment_session(S)
    assert [bank.open() for _ in range(S)] == list(range(S))
    return bank, sess


def equal(wv, S, reps):
    x = audio(S, PUSH * PUSHES, 0)
    tb, tl = [], []
    for rep in range(reps + 1):
        bank, sess = opened(wv, S)
        pb, pl = [], []
        for i in range(PUSHES):
            xi = x[:, i * PUSH:(i + 1) * PUSH]
            pb.append(timed(lambda: bank.push({s: xi[s] for s in range(S)})))
            pl.append(timed(lambda: sess.push(xi)))
        if rep:
            tb.append(statistics.median(pb[SKIP:]))
            tl.append(statistics.median(pl[SKIP:]))
    b, l = statistics.median(tb), statistics.median(tl)
    return {"bank_push_ms": stat(tb), "lockstep_push_ms": stat(tl), "bank_minus_lockstep_ms": b - l, "bank_over_lockstep": b / l,
            "lockstep_spread_ms": max(tl) - min(tl)}


def mixed(wv, reps):
    S, n = 48, TICK * (PREROLL + TICKS)
    x = audio(S, n, 1)
    packet = [PACKETS[s // 16] for s in range(S)]
    due = lambda tick, p: (tick + 1) * TICK % p == 0                 # a packet is pushed on the tick that completes it
    totals = {name: [] for name, _ in PAD_LIMITS}
    totals["three_lockstep_sessions"] = []
    shares = {}
    for rep in range(reps + 1):
        banks = {name: opened(wv, S, pad)[0] for name, pad in PAD_LIMITS}
        sessions = [wv.open_segment_session(16) for _ in PACKETS]
        spent = {name: 0.0 for name in totals}
        for tick in range(PREROLL + TICKS):
            end = (tick + 1) * TICK
            items = {s: x[s, end - packet[s]: end] for s in range(S) if due(tick, packet[s])}
            if tick == PREROLL:
                before = {name: dict(b.stats) for name, b in banks.items()}
            for name, bank in banks.items():                          # interleaved: every contender runs this tick before the next tick
                t = timed(lambda: bank.push(items))
                spent[name] += t if tick >= PREROLL else 0.0
            for g, p in enumerate(PACKETS):
                if due(tick, p):
                    t = timed(lambda: sessions[g].push(x[16 * g: 16 * g + 16, end - p: end]))
                    spent["three_lockstep_sessions"] += t if tick >= PREROLL else 0.0
        if rep:
            for name in totals:
                totals[name].append(spent[name])
            for name, b in banks.items():
                d = {k: b.stats[k] - before[name][k] for k in b.stats}
                shares[name] = {"padded_share": d["padded_samples"] / max(1, d["window_samples"]), "net_launches_per_second": d["launches"]}
    out = {name: {"device_ms_per_second_of_audio": stat(v), **shares.get(name, {})} for name, v in totals.items()}
    ref = statistics.median(totals["three_lockstep_sessions"])
    for name, _ in PAD_LIMITS:
        out[name]["over_three_lockstep_sessions"] = statistics.median(totals[name]) / ref
    out["three_lockstep_sessions"]["spread_ms"] = max(totals["three_lockstep_sessions"]) - min(totals["three_lockstep_sessions"])
    return out


def kernel(wv, reps):
    dev, S, nb, hop, G, ring = wv.device, 64, 16, 320, 2, 64
    sb, eb = ops.segment_track_bytes(S, nb, G, ring)
    state, events = torch.zeros(sb, dtype=torch.uint8, device=dev), torch.zeros(eb, dtype=torch.uint8, device=dev)
    fsum = torch.rand((S, nb + 1, 1), device=dev) * hop
    fsum[:, nb] = hop                                                 # every frame on: the open runs grow, nothing closes
    tk = []
    for rep in range(reps + 1):
        state.zero_()
        events.zero_()
        pk = []
        for i in range(PUSHES):
            desc = torch.tensor([[s, s * (nb + 1), 1, 0, 1, i, hop, 0] for s in range(S)], dtype=torch.int64, device=dev)
            pk.append(timed(lambda: ops.bank_segment_track(fsum.reshape(-1), desc, S, S, nb, hop, 0.5, G, 5, state, events, ring)))
        if rep:
            tk.append(statistics.median(pk))
    return {"bank_segment_track_64x1_frame_16_bits_ms": stat(tk)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "segment_bank_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segmentbankbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "equal": {}, "mixed": {}, "kernel": kernel(wv, a.reps)}
    for precision in ("f32", "f16"):
        wv.set_precision(precision)
        for S in (1, 16, 64):
            res["equal"][f"S{S}_{precision}"] = equal(wv, S, a.reps)
        res["mixed"][precision] = mixed(wv, a.reps)
        print(json.dumps({k: v for k, v in res.items() if k in ("equal", "mixed")}), flush=True)
    wv.set_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
