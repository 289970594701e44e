"""Cost of the native-rate embed route -> profiles/native_embed_bench.json.

    python tools/nativebench.py [--reps 15] [--out profiles/native_embed_bench.json]

32 stereo clips of 10 s at 48 kHz and at 44.1 kHz (seeded noise at the level of the suite's synthetic clips), default full-size nets with
seeded random weights:
(a) the two fused calls (native.downmix_resample, native.upsample_add) against the same work composed from the calls that existed before
    them: the channel mean, effects.resample_waveform down, effects.resample_waveform up, the broadcast add.  Same residual both ways.
(b) one whole embed_native_batch against embed_batch on the already down-mixed 16 kHz input (what the native rate adds to an embed).
(c) peak device memory above what is resident before the call, for each way of (a) and (b).
(d) what the detector sees: ||down(up(d)) - d|| / ||d|| for the residual d this generator produces, and the largest change of the
    detector's mean probabilities between x16 + d and the 16 kHz copy of the native-rate result.  Recorded, not judged: no trained
    checkpoint ships.
The two ways of (a) and of (b) alternate inside one loop after a warm-up; medians of per-iteration host-clock times, each ending in a
device synchronise.  Condition on (a): fused_over_composed <= 1 at both rates."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import effects, native  # noqa: E402
from waveverify_amd.core import WaveVerify  # noqa: E402

CLIPS, SECONDS, CHANNELS = 32, 10, 2


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def peak_above_resident(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def stats(ts):
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "native_embed_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nativebench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    gen = wv.model.generator
    msg = (torch.rand(CLIPS, 16, generator=torch.Generator().manual_seed(1)) < 0.5).float().cuda()
    res = {"device": torch.cuda.get_device_name(0), "clips": CLIPS, "seconds": SECONDS, "channels": CHANNELS, "reps": a.reps, "rates": {}}
    for sr in (48000, 44100):
        Tn = sr * SECONDS
        rng = np.random.default_rng(sr)
        x = torch.from_numpy(np.clip(0.1 * rng.standard_normal((CLIPS, CHANNELS, Tn), dtype=np.float32), -1, 1)).cuda()
        x16 = native.downmix_resample(x, sr)
        delta = gen.generator(x16, msg, add_input=False, precision=wv.generator_precision)

        def fused():
            return native.downmix_resample(x, sr), native.upsample_add(x, delta, sr)

        def composed():
            y = effects.resample_waveform(x.mean(dim=1, keepdim=True), sr, native.MODEL_RATE)
            up = effects.resample_waveform(delta, native.MODEL_RATE, sr)[..., :Tn]
            return y, x + up

        def embed_native():
            return wv.embed_native_batch(x, sr, msg)

        def embed_16k():
            return wv.embed_batch(x16, msg)

        (yf, of), (yc, oc) = fused(), composed()
        same = {"front_max_abs_difference": float((yf - yc).abs().max()), "back_max_abs_difference": float((of - oc).abs().max())}
        del yf, of, yc, oc
        for _ in range(a.warmup):
            fused(); composed(); embed_native(); embed_16k()
        tf, tc, tn, te = [], [], [], []
        for _ in range(a.reps):                                  # interleaved
            tf.append(timed(fused)); tc.append(timed(composed))
        for _ in range(a.reps):
            tn.append(timed(embed_native)); te.append(timed(embed_16k))
        # (d) what the detector sees
        wm_native = embed_native()
        back16 = native.downmix_resample(wm_native, sr)                                    # = x16 + down(up(delta)) up to rounding
        rt = native.downmix_resample(native.upsample_add(torch.zeros(CLIPS, 1, Tn, device=x.device), delta, sr), sr)
        ratio = float((rt - delta).double().norm() / delta.double().norm())
        _, mp_direct = wv.detect_batch(x16 + delta)
        _, mp_native = wv.detect_batch(back16)
        del wm_native, back16, rt
        nbytes = 4 * CLIPS * Tn
        res["rates"][str(sr)] = {
            "samples": Tn, "model_samples": int(x16.shape[-1]), "fused_equals_composed": same,
            "a_fused": stats(tf), "a_composed": stats(tc), "a_fused_over_composed": statistics.median(tf) / statistics.median(tc),
            "a_algorithmic_MB": {"fused": (3 * CHANNELS + 2 / 3) * nbytes / 1e6, "composed": (5 * CHANNELS + 2 / 3) * nbytes / 1e6},
            "b_embed_native": stats(tn), "b_embed_16k_mono": stats(te), "b_native_over_16k": statistics.median(tn) / statistics.median(te),
            "c_peak_MB_above_resident": {"fused": peak_above_resident(fused), "composed": peak_above_resident(composed),
                                         "embed_native": peak_above_resident(embed_native), "embed_16k_mono": peak_above_resident(embed_16k)},
            "d_round_trip_relative_error": ratio,
            "d_residual_rms_over_input_rms": float(delta.double().norm() / x16.double().norm()),
            "d_detector_mean_prob_max_change": float((mp_direct - mp_native).abs().max()),
            "d_detector_bits_changed": int(((mp_direct >= 0.5) != (mp_native >= 0.5)).sum()),
        }
        del x, x16, delta
        torch.cuda.empty_cache()
    res["condition_a_met"] = all(r["a_fused_over_composed"] <= 1.0 for r in res["rates"].values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
