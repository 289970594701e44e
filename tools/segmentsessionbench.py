"""Cost of one push of a live segment session -> profiles/segment_session_bench.json.

    python tools/segmentsessionbench.py [--reps 15] [--out profiles/segment_session_bench.json]

20 ms pushes (320 samples at 16 kHz), 1 and 16 streams in lockstep, the default full-size detector and locator with seeded random weights, exact
and f16.  Fed the same audio, push after push:
    segment  WaveVerify.open_segment_session(S).push: one history, one window for both nets, the frames kernel gated by the locator's logits,
             one wv_segment_track; nothing read back;
    pair     what a live user had before: LocateSession.push, then DetectSession.push on the same samples (two histories, two windows; the pair
             cannot decode per segment at all, so this is a cost comparison only);
    tracker  the wv_segment_track launch alone on one new frame of frame sums.
Each repetition opens the sessions afresh and pushes 1 s of audio (50 pushes) -- segment push i, then pair push i, then tracker tick i -- keeping
the per-push host-clock times, each ending in a device synchronise; the first 10 pushes (the halo still filling) are left out.  Recorded: the
medians over repetitions of each repetition's median push with their min and max over repetitions (the spread), and segment - pair.  No bar:
nobody had measured this before."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd.core import WaveVerify  # noqa: E402
from waveverify_amd.session import HipSegmentTracker  # noqa: E402

PUSH, PUSHES, SKIP = 320, 50, 10


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "segment_session_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segmentsessionbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    res = {"device": torch.cuda.get_device_name(0), "samples_per_push": PUSH, "pushes_per_repetition": PUSHES, "pushes_left_out": SKIP,
           "reps": a.reps, "cases": {}}
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    for S in (1, 16):
        rng = np.random.default_rng([16000, S])
        x = torch.from_numpy(np.clip(0.1 * rng.standard_normal((S, PUSH * PUSHES), dtype=np.float32), -1, 1)).cuda()
        fsum = torch.rand((S, 17, 1), device="cuda") * 320.0
        for precision in ("f32", "f16"):
            wv.set_precision(precision)
            ts, tp, tt = [], [], []
            for rep in range(a.reps + 1):                                  # repetition 0 warms up
                seg, loc, det = wv.open_segment_session(S), wv.open_locate_session(S), wv.open_detect_session(S)
                trk = HipSegmentTracker(S, 16, 320, 0.5, 2, 5, 64, wv.device)
                ps, pp, pt = [], [], []
                for i in range(PUSHES):                                    # interleaved
                    xi = x[:, i * PUSH:(i + 1) * PUSH]
                    ps.append(timed(lambda: seg.push(xi)))
                    pp.append(timed(lambda: (loc.push(xi), det.push(xi))))
                    pt.append(timed(lambda: trk.advance(fsum, 0, 1)))
                if rep:
                    ts.append(statistics.median(ps[SKIP:]))
                    tp.append(statistics.median(pp[SKIP:]))
                    tt.append(statistics.median(pt[SKIP:]))
            s_, p_ = statistics.median(ts), statistics.median(tp)
            res["cases"][f"S{S}_{precision}"] = {"segment_push_ms": stat(ts), "locate_plus_detect_push_ms": stat(tp), "tracker_launch_ms": stat(tt),
                                                 "segment_minus_pair_ms": s_ - p_, "segment_over_pair": s_ / p_,
                                                 "pair_spread_ms": max(tp) - min(tp)}
        wv.set_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
