"""Cost of STOI on the GPU against the float64 numpy route on the host, and of validate(stoi=True) against validate()
-> profiles/stoi_bench.json.

    python tools/stoibench.py [--reps 15] [--out profiles/stoi_bench.json]

For 16 x 1 s and 64 x 1 s at 16 kHz (speech-shaped noise: an amplitude-modulated low-passed gaussian, so that some frames fall silent):
A: metrics.STOI on device tensors, one fused call, ending in the copy of the [B] results to the host.
B: the same clips copied to the host and put through the float64 numpy route clip by clip (waveverify_amd/stoi.py), the only other
   implementation in this tree and the shape of what the reference does through pystoi.
A and B alternate inside one loop after a warm-up; medians of per-iteration host-clock times, each ending in a device synchronise.  Then
one whole validate(stoi=True) against validate() of the default full-size nets at 16 x 1 s, alternating the same way."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import metrics  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def clips(B, T, seed):
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((B, T + 64))
    x = np.stack([np.convolve(r, np.hanning(17) / 8, mode="valid")[:T] for r in n])
    env = np.abs(np.sin(np.pi * np.arange(T)[None] / (T / (2 + np.arange(B)[:, None] % 3)))) ** 4
    x = (0.3 * x * env).astype(np.float32)
    y = (x + 0.01 * rng.standard_normal((B, T))).astype(np.float32)
    return torch.from_numpy(x)[:, None].cuda(), torch.from_numpy(y)[:, None].cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "stoi_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stoibench needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)
    res = {"device": torch.cuda.get_device_name(0), "sample_rate": 16000, "samples": 16000, "reps": a.reps, "batches": {}}
    m = metrics.STOI()
    for B in (16, 64):
        x, y = clips(B, 16000, B)

        def fused():
            return m(y, x, 16000).cpu().numpy()

        def host():
            return metrics.STOI()(y.cpu(), x.cpu(), 16000).numpy()

        da, db = fused(), host()
        for _ in range(a.warmup):
            fused(); host()
        ta, tb = [], []
        for _ in range(a.reps):                                  # interleaved A / B
            ta.append(timed(fused)); tb.append(timed(host))
        res["batches"][str(B)] = {"max_abs_difference": float(np.abs(da - db).max()), "frames_kept_min": int(m.last_frames[:, 0].min()),
                                  "frames": int(m.last_frames[0, 1]),
                                  "fused_ms_median": statistics.median(ta), "fused_ms_min": min(ta), "fused_ms_max": max(ta),
                                  "host_f64_ms_median": statistics.median(tb), "host_f64_ms_min": min(tb), "host_f64_ms_max": max(tb),
                                  "host_over_fused": statistics.median(tb) / statistics.median(ta)}

    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import WatermarkTrainer
    cfgs = [default_config(k) for k in ("generator", "detector", "locator")]
    sds = [random_state_dict(c, 0, parametrized=True) for c in cfgs]
    tr = WatermarkTrainer(cfgs[0], sds[0], cfgs[1], sds[1], cfgs[2], sds[2], spectral_losses=True)
    x, _ = clips(16, 16000, 16)
    msg = (torch.rand(16, 16, device="cuda") < 0.5).float()
    for _ in range(2):
        tr.validate(x, msg); tr.validate(x, msg, stoi=True)
    tv, ts = [], []
    for _ in range(max(3, a.reps // 3)):
        tv.append(timed(lambda: tr.validate(x, msg))); ts.append(timed(lambda: tr.validate(x, msg, stoi=True)))
    res["validate"] = {"batch": 16, "validate_ms_median": statistics.median(tv), "validate_stoi_ms_median": statistics.median(ts),
                       "validate_ms_min": min(tv), "validate_stoi_ms_min": min(ts),
                       "added_ms_median": statistics.median(ts) - statistics.median(tv)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
