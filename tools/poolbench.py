"""Cost of drawing a training batch from the device-resident clip pool against the host route it replaces, and of a fit() step
against a step() on a ready tensor -> profiles/clip_pool_bench.json.

    python tools/poolbench.py [--reps 15] [--out profiles/clip_pool_bench.json]

The corpus: 200 clips of 10 s at 16 kHz, speech-shaped noise (an amplitude-modulated low-passed gaussian) of which every third clip is
silent for its first 70 %, so that the gate has work to do.  Per repetition, one after the other (interleaved, after a warm-up), each
timed on the host clock and ending in a device synchronise:
A: pool.sample(64, 1.0), 8 tries: the draws, one wv_loudness over 512 candidates, one wv_pool_sample, info read back.
B: pool.sample(64, 1.0, loudness_cutoff=None): the draws and the copy alone.
C: the host route: the same draws, numpy slices of a host copy of the corpus, the float64 host loudness (loudness.loudness_numpy: scipy's
   sosfilt where installed) try by try until one is above the cutoff, as a data loader does it, then ONE upload of the [64,1,16000] batch.
Then, with the default full-size nets at batch 64 and fewer repetitions: one fit() step (A inside it) against one step() on a tensor
that is already on the device, alternating.  Medians; the minimum and maximum are kept beside them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import loudness as L  # noqa: E402
from waveverify_amd.data import ClipPool  # noqa: E402

FS, T, B, TRIES, CUTOFF = 16000, 16000, 64, 8, -40.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def corpus(n=200, seconds=10, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = seconds * FS
        x = np.convolve(rng.standard_normal(m + 16), np.hanning(17) / 8, mode="valid")[:m]
        env = np.abs(np.sin(np.pi * np.arange(m) / (FS * (0.7 + 0.1 * (i % 5))))) ** 2
        x = 0.3 * x * env
        if i % 3 == 0:
            x[: int(0.7 * m)] = 0.0
        out.append(x.astype(np.float32))
    return out


def host_route(clips, lengths, rng):
    """The draws of ClipPool.sample, then try by try on the host; -> (the uploaded batch, tries used)."""
    clip, offset, lens = L.draw(rng, lengths, B, T, TRIES)
    batch = np.zeros((B, 1, T), np.float32)
    used = np.zeros(B, np.int64)
    for b in range(B):
        for k in range(TRIES):
            w = clips[clip[b]][offset[b, k]: offset[b, k] + T]
            used[b] = k + 1
            if L.loudness_numpy(np.pad(w, (0, T - len(w))), FS) > CUTOFF:
                break
        batch[b, 0, : len(w)] = w
    return torch.from_numpy(batch).cuda(), used


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "clip_pool_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("poolbench needs the GPU: nothing is measured without one")
    clips = corpus()
    pool = ClipPool(clips, FS)
    lengths = pool.lengths
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": FS, "batch": B, "duration_s": 1.0, "num_tries": TRIES, "cutoff_lufs": CUTOFF,
           "pool_clips": len(pool), "pool_seconds": pool.seconds, "reps": a.reps}
    rngs = [np.random.default_rng(s) for s in (1, 2, 3)]
    # the two routes agree on what they pick (same generator state -> same draws)
    x, info = pool.sample(B, 1.0, rng=np.random.default_rng(9))
    xh, used = host_route(clips, lengths, np.random.default_rng(9))
    res["routes_agree"] = bool(torch.equal(x, xh) and np.array_equal(info["tries_used"], used))
    res["tries_used_mean"] = float(info["tries_used"].mean())
    for _ in range(a.warmup):
        pool.sample(B, 1.0, rng=rngs[0]); pool.sample(B, 1.0, rng=rngs[1], loudness_cutoff=None); host_route(clips, lengths, rngs[2])
    ta, tb, tc = [], [], []
    for _ in range(a.reps):                                      # interleaved A / B / C
        ta.append(timed(lambda: pool.sample(B, 1.0, rng=rngs[0])))
        tb.append(timed(lambda: pool.sample(B, 1.0, rng=rngs[1], loudness_cutoff=None)))
        tc.append(timed(lambda: host_route(clips, lengths, rngs[2])))
    res["sample_gated"], res["sample_ungated"], res["host_route"] = spread(ta), spread(tb), spread(tc)
    res["host_over_gated"] = statistics.median(tc) / statistics.median(ta)

    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import WatermarkTrainer
    cfgs = [default_config(k) for k in ("generator", "detector", "locator")]
    sds = [random_state_dict(c, 0, parametrized=True) for c in cfgs]
    tr = WatermarkTrainer(cfgs[0], sds[0], cfgs[1], sds[1], cfgs[2], sds[2])
    ready, _ = pool.sample(B, 1.0, rng=4)
    msg = (torch.rand(B, 16, device="cuda") < 0.5).float()
    for _ in range(2):
        tr.fit(pool, steps=1, batch=B, seed=5); tr.step(ready, msg)
    tf, ts = [], []
    for i in range(max(5, a.reps // 2)):
        tf.append(timed(lambda: tr.fit(pool, steps=1, batch=B, seed=6 + i))); ts.append(timed(lambda: tr.step(ready, msg)))
    res["fit_step"], res["step_ready_tensor"] = spread(tf), spread(ts)
    res["fit_added_ms_median"] = statistics.median(tf) - statistics.median(ts)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
