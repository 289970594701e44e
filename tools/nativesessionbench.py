"""Cost of one push of a native-rate live session -> profiles/native_session_bench.json.

    python tools/nativesessionbench.py [--reps 15] [--out profiles/native_session_bench.json]

20 ms pushes of stereo audio at 48 kHz (960 samples) and at 44.1 kHz (882 samples), 1 and 16 streams in lockstep, the default full-size generator
with seeded random weights, exact and f16.  Two sessions are fed the same audio, push after push:
    native   WaveVerify.open_embed_session(ids, sample_rate, channels=2): front stage, 16 kHz session, back stage;
    model    the 16 kHz EmbedSession of the same build given the same audio already down-mixed and resampled (320 samples per push): the model
             tick a native session cannot go below.
Each repetition opens both sessions afresh, pushes 1 s of audio (50 pushes) through each in turn -- native push i, then model push i -- and keeps
the per-push host-clock times, each ending in a device synchronise; the first 10 pushes (the halo still filling) are left out.  Recorded: the
medians over repetitions of each repetition's median push, and the native overhead (native - model, and native / model).  No bar: nobody had
measured a session tick on these kernels before."""
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

CHANNELS, PUSH_MS, PUSHES, SKIP = 2, 20, 50, 10


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "native_session_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nativesessionbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    res = {"device": torch.cuda.get_device_name(0), "channels": CHANNELS, "push_ms": PUSH_MS, "pushes_per_repetition": PUSHES,
           "pushes_left_out": SKIP, "reps": a.reps, "cases": {}}
    for sr in (48000, 44100):
        n = sr * PUSH_MS // 1000
        for S in (1, 16):
            rng = np.random.default_rng([sr, S])
            x = torch.from_numpy(np.clip(0.1 * rng.standard_normal((S, CHANNELS, n * PUSHES), dtype=np.float32), -1, 1)).cuda()
            x16 = native.downmix_resample(x, sr)[:, 0]
            n16 = x16.shape[1] // PUSHES
            ids = list(range(1, S + 1))
            for precision in ("f32", "f16"):
                wv.set_precision(precision)
                tn, tm = [], []
                for rep in range(a.reps + 1):                              # repetition 0 warms up
                    nat = wv.open_embed_session(ids, sample_rate=sr, channels=CHANNELS)
                    mod = wv.open_embed_session(ids)
                    pn, pm = [], []
                    for i in range(PUSHES):                                # interleaved
                        pn.append(timed(lambda: nat.push(x[:, :, i * n:(i + 1) * n])))
                        pm.append(timed(lambda: mod.push(x16[:, i * n16:(i + 1) * n16])))
                    if rep:
                        tn.append(statistics.median(pn[SKIP:]))
                        tm.append(statistics.median(pm[SKIP:]))
                nm, mm = statistics.median(tn), statistics.median(tm)
                res["cases"][f"{sr}Hz_S{S}_{precision}"] = {
                    "samples_per_push": n, "model_samples_per_push": n16, "latency_samples": nat.latency_samples,
                    "native_push_ms": {"median": nm, "min": min(tn), "max": max(tn)}, "model_push_ms": {"median": mm, "min": min(tm), "max": max(tm)},
                    "native_overhead_ms": nm - mm, "native_over_model": nm / mm}
            wv.set_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
