"""Cost of localized detection on the GPU -> profiles/localized_detect_bench.json.

    python tools/localizedbench.py [--reps 10] [--out profiles/localized_detect_bench.json]

Workloads 256 x 1 s and 32 x 30 s, each in the exact and the f16 mode; per workload three routes, timed interleaved in one loop after a
warm-up (host clock around a device synchronise, medians):
  plain         detect_batch + locate_batch: the whole-clip mean and the locator's mask side by side (no masked decode at all)
  materialised  the masked decode as it had to be done before: net.locator, net.detector logits [B, 16, T], metrics.ber_per_clip with
                the locator's mask
  fused         detect_localized_batch: locator logits as the gate of the frames kernel, then wv_frames_reduce
and torch.cuda.max_memory_allocated of each route on its own (peak above the resident nets and the input)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import WaveVerify, metrics  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "localized_detect_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("localizedbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    det, loc = wv.model.detector, wv.model.locator
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for B, T in ((256, 16000), (32, 480000)):
        x = 0.1 * torch.randn(B, 1, T, device="cuda", generator=g)
        bits0 = torch.zeros(B, 16, device="cuda")
        for precision in ("f32", "f16"):
            wv.set_precision(precision)

            def plain():
                wv.detect_batch(x)
                wv.locate_batch(x)

            def materialised():
                mask = (loc.locator(x, precision=precision) > 0).float()
                return metrics.ber_per_clip(det.detector(x, precision=precision), bits0, mask)[2]

            def fused():
                return wv.detect_localized_batch(x)[1]

            routes = {"plain": plain, "materialised": materialised, "fused": fused}
            same = bool(torch.equal(materialised() >= 0.5, fused() >= 0.5))
            for _ in range(a.warmup):
                for fn in routes.values():
                    fn()
            times = {k: [] for k in routes}
            for _ in range(a.reps):                              # interleaved
                for k, fn in routes.items():
                    times[k].append(timed(fn))
            row = {"batch": B, "samples": T, "precision": precision, "reps": a.reps, "same_bits": same, "logits_bytes": B * 16 * T * 4}
            for k, fn in routes.items():
                row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = statistics.median(times[k]), min(times[k]), max(times[k])
                row[k + "_peak_bytes"] = peak(fn)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")


if __name__ == "__main__":
    main()
