"""Cost of the per-channel SNR floor at a file's own rate -> profiles/channel_floor_bench.json.

    python tools/channelfloorbench.py [--reps 15] [--out profiles/channel_floor_bench.json]

The default full-size generator with seeded random weights.  Every time is the host clock around one call that ends in a device
synchronise; repetition 0 warms up, and the figures are medians over the repetitions with their min and max (the spread).  The yardstick of
every workload is the floor-less call in the same run; within a repetition the two take turns (interleaved).
    back end             native.upsample_add_floor against native.upsample_add alone on 32 stereo clips x 10 s, at 48 kHz and at 44.1 kHz,
                         the residual a generator's; the fused call's workspace comes from torch's caching allocator, as in the route
    embed_native_batch   the whole route on the same clips with the channel floor on against off
No bar is set on any of these: they are recorded.  `over` is floor / no floor by medians; `beyond_spread` says whether the difference of the
medians is larger than the floor-less form's own max - min."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import native  # noqa: E402
from waveverify_amd.core import WaveVerify  # noqa: E402

DB = 20.0
RATES = (48000, 44100)
CLIPS, CHANNELS, SECONDS = 32, 2, 10


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def audio(shape, seed):
    rng = np.random.default_rng([16000, seed])
    return torch.from_numpy(np.clip(0.1 * rng.standard_normal(shape, dtype=np.float32), -1, 1)).cuda()


def pair(off, on, reps):
    """off / on: the call without and with the floor -> their statistics, interleaved."""
    a, b = [], []
    for rep in range(reps + 1):
        t_off, t_on = timed(off), timed(on)
        if rep:
            a.append(t_off)
            b.append(t_on)
    so, sn = stat(a), stat(b)
    return {"no_floor_ms": so, "floor_ms": sn, "over": sn["median"] / so["median"],
            "beyond_spread": bool(sn["median"] - so["median"] > so["max"] - so["min"])}


def switched(wv, db, fn):
    def run():
        wv.set_channel_snr_floor(db)
        try:
            fn()
        finally:
            wv.set_channel_snr_floor(None)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "channel_floor_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("channelfloorbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    hop = wv.configs["generator"].hop_length
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "min_snr_db": DB, "hop": hop,
           "clips": f"{CLIPS} x {CHANNELS} channels x {SECONDS} s"}
    msg = wv._messages(0xBEEF)
    for sr in RATES:
        x = audio((CLIPS, CHANNELS, SECONDS * sr), sr)
        delta = wv.model.generator.generator(wv.to_model_rate(x, sr), msg, add_input=False, precision=wv.generator_precision)
        out = torch.empty_like(x)
        _, g = native.upsample_add_floor(x, delta, sr, DB, hop=hop, return_gains=True)
        back = pair(lambda: native.upsample_add(x, delta, sr, 1.0, out=out), lambda: native.upsample_add_floor(x, delta, sr, DB, hop=hop, out=out),
                    a.reps)
        back["frames_turned_down"] = float((g < 1).float().mean())
        res[f"back_end_{sr}"] = back
        print(json.dumps({sr: back}), flush=True)
        del delta, out
        route = pair(lambda: wv.embed_native_batch(x, sr, msg), switched(wv, DB, lambda: wv.embed_native_batch(x, sr, msg)), a.reps)
        res[f"embed_native_batch_{sr}"] = route
        print(json.dumps({sr: route}), flush=True)
        del x
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
