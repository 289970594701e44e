#!/usr/bin/env python3
"""Time of the time-domain effect kernels (csrc/wv_fx_time.hip) through their Python wrappers, at the trainer's per-clip call
[1,1,16000] and at the training batch [64,1,16000].  A record, not a gate: at one clip every one of them is launch-bound.

    python tools/fxtimebench.py [--out profiles/fx_time_bench.json]

For each effect: microseconds per call (device events around `reps` calls after a warm-up, the median of `rounds` such windows), the
bytes the algorithm must move (2 * 4 * B * T for the single-pass ones: one read and one write of the audio; more where a mask, a
keep mask, a noise tensor or a second pass is part of the contract) and the achieved TB/s = those bytes over that time.  The time is
the wrapper's: output allocation and, where the effect has them, the host-side draws and uploads are inside it (pink_noise's host
loop is excluded: the noise is generated once, outside the window, and only the add is timed)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import _lib, effects as E  # noqa: E402


def window(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def cases(B, T):
    g = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn(B, 1, T, device="cuda", generator=g) * 0.1
    d = torch.randn(B, 1, T, device="cuda", generator=g)
    mask = torch.ones_like(x)
    noise = torch.randn(B, 1, T, device="cuda", generator=g)
    n = 4 * B * T
    _, keep, _ = E.shush_forward(x, T // 10, mask)
    _, rec = E.echo_forward(x, 4000, 0.3)
    idx = torch.from_numpy(E.suppression_indices(B, 1, T, 0.1)).cuda()
    y = x.clone()
    return [
        ("amplitude_scaling", lambda: E.pointwise(x, E.OP_SCALE, 0.7), 2 * n),
        ("noise add (random / white / pink, noise given)", lambda: E.pointwise(x, E.OP_ADD_NOISE, 0.001, noise), 3 * n),
        ("random_noise (randn_like + add)", lambda: E.AudioEffects.random_noise(x, 0.001), 2 * n),
        ("quantization 16 bit", lambda: E.pointwise(x, E.OP_QUANTIZE, 32767.0), 2 * n),
        ("median_filter k=3", lambda: E.median(x, 3), 2 * n),
        ("median_filter k=7", lambda: E.median(x, 7), 2 * n),
        ("median_filter k=31", lambda: E.median(x, 31), 2 * n),
        ("median_filter k=33 (rank counting)", lambda: E.median(x, 33), 2 * n),
        ("shush 10% (audio, keep, mask)", lambda: E.shush_forward(x, T // 10, mask), 5 * n),
        ("shush backward (gradient * keep)", lambda: E.pointwise(d, E.OP_MUL, 0.0, keep), 3 * n),
        ("echo n=4000 (peaks + apply)", lambda: E.echo_forward(x, 4000, 0.3), 3 * n),
        ("echo backward", lambda: E.echo_backward(x, d, rec, 4000, 0.3), 5 * n),
        ("smooth w=6 (audio, mask)", lambda: E.smooth_forward(x, 6, mask), 4 * n),
        ("smooth backward w=6", lambda: E.smooth_backward(d, 6), 2 * n),
        ("scatter-zero 10% (audio, mask; in place)", lambda: E.scatter_zero(y, idx, mask), 3 * 4 * idx.numel()),
        ("sample_suppression 10% (randperm on the host, upload, copy, scatter)", lambda: E.AudioEffects.sample_suppression(x, 0.1, mask=mask), 4 * n),
        ("linear stretch 20000 -> 16000", (lambda xs: (lambda: E.stretch_linear(xs, T)))(torch.randn(B, 1, T * 5 // 4, device="cuda") * 0.1), 9 * n // 4),
        ("speed 0.8 (resample 4:5 + stretch)", lambda: E.AudioEffects.speed(x, 0.8), 2 * n + 2 * 5 * n // 4),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "fx_time_bench.json"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fxtimebench needs the GPU (a CPU run measures nothing)")
    lib = _lib.load()
    rows = []
    for B in (1, 64):
        for name, f, nbytes in cases(B, 16000):
            reps = max(5, a.reps // 10) if "host" in name else a.reps
            window(f, a.warmup)
            us = [window(f, reps) for _ in range(a.rounds)]
            med = statistics.median(us)
            rows.append({"effect": name, "shape": [B, 1, 16000], "us_per_call": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                         "bytes": int(nbytes), "tb_per_s": round(nbytes / med / 1e6, 4)})
            print(f"[{B:2d},1,16000] {name:70s} {med:9.1f} us  (min {min(us):8.1f} max {max(us):8.1f})  {nbytes / 1e6:8.3f} MB  {nbytes / med / 1e6:7.3f} TB/s")
    out = {"device": torch.cuda.get_device_name(0), "library": lib.wv_version().decode(), "warmup": a.warmup, "reps": a.reps, "rounds": a.rounds,
           "note": "wrapper time per call, median of `rounds` windows of `reps` calls between device events; bytes = what the algorithm must move; "
                   "at [1,1,16000] every effect is launch-bound, so the TB/s there measures the launch, not the kernel", "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
