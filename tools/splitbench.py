"""Cost of splitting runs where the decoded id changes (localize.SplitRule) -> profiles/segment_split_bench.json.

    python tools/splitbench.py [--reps 15] [--out profiles/segment_split_bench.json]

The default full-size nets with seeded random weights, exact and f16, the default rule (window_frames 25), a caller's gate in place of
the random locator (which would open no run to follow).  Every time is the
host clock around one call that ends in a device synchronise; each repetition opens its sessions and banks afresh, repetition 0 warms up,
and the figures are medians over the repetitions with their min and max.  Within a repetition the contenders take turns call by call
(interleaved).  The yardstick is always the same call without a rule, in the same run.
    (a) tick    S = 1, 16, 64 streams that all push 20 ms (320 samples): SegmentSession.push and SegmentBank.push after set_split(rule)
                against the same push without a rule, 110 pushes of which the last 50 are timed.  A caller's gate of ones keeps one run open
                in every stream (the random locator would open none), so from push 50 on every split tick evaluates one boundary per
                stream: the busy path, not an idle one.
    (b) batch   detect_segments_batch on 32 clips of 30 s with and without the rule (a caller's gate of three stretches per clip, so that
                the trackers have runs to follow whatever the random locator would mark).
    (c) kernel  wv_segment_track_split and wv_bank_segment_track_split alone beside the plain kernels: 64 streams of one new frame each
                inside a long run (every tick evaluates one boundary: two windows of 25 frames), and one launch over 32 x 1500 frames.
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
from waveverify_amd.localize import SplitRule  # noqa: E402

PUSH, PUSHES, SKIP = 320, 110, 60
RULE = SplitRule()


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


def versus(split, plain):
    s, p = statistics.median(split), statistics.median(plain)
    return {"split_ms": stat(split), "plain_ms": stat(plain), "split_minus_plain_ms": s - p, "split_over_plain": s / p,
            "plain_spread_ms": max(plain) - min(plain)}


def tick(wv, S, reps):
    x = audio(S, PUSH * PUSHES, 0)
    ones = torch.ones((S, PUSH), device=x.device)
    t = {k: [] for k in ("session_split", "session_plain", "bank_split", "bank_plain")}
    for rep in range(reps + 1):
        sess = {"session_split": wv.open_segment_session(S), "session_plain": wv.open_segment_session(S)}
        bank = {"bank_split": wv.open_segment_bank(S, gated=True), "bank_plain": wv.open_segment_bank(S, gated=True)}
        sess["session_split"].set_split(RULE)
        bank["bank_split"].set_split(RULE)
        for b in bank.values():
            assert [b.open() for _ in range(S)] == list(range(S))
        p = {k: [] for k in t}
        for i in range(PUSHES):
            xi = x[:, i * PUSH:(i + 1) * PUSH]
            for k, s in sess.items():
                p[k].append(timed(lambda: s.push(xi, ones)))
            for k, b in bank.items():
                p[k].append(timed(lambda: b.push({s: (xi[s], ones[s]) for s in range(S)})))
        if rep:
            for k in t:
                t[k].append(statistics.median(p[k][SKIP:]))
    return {"session": versus(t["session_split"], t["session_plain"]), "bank": versus(t["bank_split"], t["bank_plain"])}


def batch(wv, reps, B=32, seconds=30):
    T = seconds * 16000
    x = audio(B, T, 2).unsqueeze(1)
    gate = torch.zeros((B, T), device=x.device)
    for a, b in ((1, 9), (11, 18), (20, 29)):
        gate[:, a * 16000:b * 16000] = 1
    ts, tp = [], []
    for rep in range(reps + 1):
        a = timed(lambda: wv.detect_segments_batch(x, gate=gate, split=RULE))
        b = timed(lambda: wv.detect_segments_batch(x, gate=gate))
        if rep:
            ts.append(a)
            tp.append(b)
    return versus(ts, tp)


def kernel(wv, reps):
    dev, S, nb, hop, G, ring, W = wv.device, 64, 16, 320, 2, 64, RULE.window_frames
    out = {}
    # one new frame per stream inside a long run
    fsum = torch.rand((S, nb + 1, 1), device=dev) * hop
    fsum[:, nb] = hop
    bufs = {}
    for name, (sb, eb) in (("plain", ops.segment_track_bytes(S, nb, G, ring)), ("split", ops.segment_split_bytes(S, nb, G, W, ring))):
        bufs[name] = (torch.zeros(sb, dtype=torch.uint8, device=dev), torch.zeros(eb, dtype=torch.uint8, device=dev))
    t = {k: [] for k in ("lockstep_plain", "lockstep_split", "bank_plain", "bank_split")}
    for form in ("lockstep", "bank"):
        for rep in range(reps + 1):
            for st, ev in bufs.values():
                st.zero_()
                ev.zero_()
            p = {"plain": [], "split": []}
            for i in range(3 * W + 50):
                desc = torch.tensor([[s, s * (nb + 1), 1, 0, 1, i, hop, 0] for s in range(S)], dtype=torch.int64, device=dev)
                if form == "lockstep":
                    a = timed(lambda: ops.segment_track(fsum, 0, 1, i, hop, hop, False, 0.5, G, 5, *bufs["plain"], ring))
                    b = timed(lambda: ops.segment_track_split(fsum, 0, 1, i, hop, hop, False, 0.5, G, 5, RULE, *bufs["split"], ring))
                else:
                    a = timed(lambda: ops.bank_segment_track(fsum.reshape(-1), desc, S, S, nb, hop, 0.5, G, 5, *bufs["plain"], ring))
                    b = timed(lambda: ops.bank_segment_track_split(fsum.reshape(-1), desc, S, S, nb, hop, 0.5, G, 5, RULE, *bufs["split"], ring))
                if i >= 3 * W:                                        # every timed tick evaluates one boundary per stream
                    p["plain"].append(a)
                    p["split"].append(b)
            if rep:
                t[form + "_plain"].append(statistics.median(p["plain"]))
                t[form + "_split"].append(statistics.median(p["split"]))
    out["one_frame_64_streams_16_bits"] = {"lockstep": versus(t["lockstep_split"], t["lockstep_plain"]),
                                           "bank": versus(t["bank_split"], t["bank_plain"])}
    # one launch over whole clips: 32 x 1500 frames, ids changing every 150 frames
    B, Fr = 32, 1500
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, (B, nb, Fr // 150)).repeat(150, axis=2)
    whole = np.concatenate([(0.2 + 0.6 * bits) * hop, np.full((B, 1, Fr), float(hop))], axis=1).astype(np.float32)
    whole = torch.from_numpy(whole).to(dev)
    desc = torch.tensor([[b, b * (nb + 1) * Fr, Fr, 0, Fr, 0, hop, 1] for b in range(B)], dtype=torch.int64, device=dev)
    big = {"plain": ops.segment_track_bytes(B, nb, G, Fr), "split": ops.segment_split_bytes(B, nb, G, W, Fr)}
    big = {k: (torch.zeros(sb, dtype=torch.uint8, device=dev), torch.zeros(eb, dtype=torch.uint8, device=dev)) for k, (sb, eb) in big.items()}
    ts, tp = [], []
    for rep in range(reps + 1):
        for st, ev in big.values():
            st.zero_()
            ev.zero_()
        a = timed(lambda: ops.bank_segment_track(whole.reshape(-1), desc, B, B, nb, hop, 0.5, G, 5, *big["plain"], Fr))
        b = timed(lambda: ops.bank_segment_track_split(whole.reshape(-1), desc, B, B, nb, hop, 0.5, G, 5, RULE, *big["split"], Fr))
        if rep:
            tp.append(a)
            ts.append(b)
    n = ops.split_events(big["split"][1], B, nb, Fr)[0]
    out["whole_clips_32x1500_frames"] = {**versus(ts, tp), "pieces_per_clip": float(n.mean())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "segment_split_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splitbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rule": {"window_frames": RULE.window_frames, "threshold": RULE.threshold,
                                                                             "min_bits": RULE.min_bits},
           "kernel": kernel(wv, a.reps), "tick": {}, "batch": {}}
    print(json.dumps(res["kernel"]), flush=True)
    for precision in ("f32", "f16"):
        wv.set_precision(precision)
        for S in (1, 16, 64):
            res["tick"][f"S{S}_{precision}"] = tick(wv, S, a.reps)
        res["batch"][precision] = batch(wv, a.reps)
        print(json.dumps({k: res[k] for k in ("tick", "batch")}), flush=True)
    wv.set_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
