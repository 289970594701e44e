"""Cost of the SNR floor of embedding -> profiles/snr_floor_bench.json.

    python tools/snrfloorbench.py [--reps 15] [--out profiles/snr_floor_bench.json]

The default full-size generator with seeded random weights.  Every time is the host clock around one call that ends in a device
synchronise; repetition 0 warms up, and the figures are medians over the repetitions with their min and max (the spread).  The yardstick of
every workload is the same call with the floor off, in the same run; within a repetition the two take turns (interleaved).
    embed_batch          256 clips x 1 s
    embed_native_batch   32 stereo clips x 10 s at 48 kHz
    bank tick            an EmbedBank push of 20 ms per stream with 1, 16 and 64 streams, exact and f16 (two banks, one under the floor, the
                         histories full)
    kernel               wv_snr_floor alone on 256 rows x 16 000 samples: achieved GB/s over 12 bytes per sample (x and r read, out written)
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
from waveverify_amd import _lib, snr_floor  # noqa: E402
from waveverify_amd.core import WaveVerify  # noqa: E402

FS = 16000
DB = 20.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def audio(shape, seed):
    rng = np.random.default_rng([FS, seed])
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
        wv.set_snr_floor(db)
        try:
            fn()
        finally:
            wv.set_snr_floor(None)
    return run


def bank_tick(wv, S, precision, reps):
    """Two banks of S streams, one under the floor; 40 warm-up ticks fill the histories, then every repetition pushes 20 ms per stream."""
    wv.set_precision(precision)
    banks = []
    for db in (None, DB):
        wv.set_snr_floor(db)
        bank = wv.open_embed_bank(capacity=S)
        wv.set_snr_floor(None)
        banks.append((bank, [bank.open(0x1000 + i) for i in range(S)]))
    x = audio((S, 320), S)
    push = lambda bank, slots: (lambda: bank.push({s: x[i] for i, s in enumerate(slots)}))      # noqa: E731
    for _ in range(40):
        for bank, slots in banks:
            push(bank, slots)()
    res = pair(push(*banks[0]), push(*banks[1]), reps)
    wv.set_precision("f32")
    return res


def kernel(reps, B=256, T=16000, L=320):
    dev = torch.device("cuda")
    x, r, out = audio((B * T,), 7), audio((B * T,), 8), torch.empty(B * T, device=dev)
    table = np.zeros((B, snr_floor.DESC), np.int64)
    table[:, 0] = table[:, 1] = table[:, 2] = np.arange(B) * T
    table[:, 3], table[:, 4], table[:, 5], table[:, 6], table[:, 7] = T, snr_floor.strength_bits(1.0), -1, 1, -1
    desc, ramp = torch.from_numpy(table).to(dev), torch.from_numpy(snr_floor.floor_ramp(L)).to(dev)
    lib, rho = _lib.load(), snr_floor.rho_of(DB)
    call = lambda: _lib.check(lib.wv_snr_floor(x.data_ptr(), B * T, r.data_ptr(), B * T, out.data_ptr(), B * T, desc.data_ptr(), B, T, None, 0, None,   # noqa: E731
                                               0, ramp.data_ptr(), L, rho, 1, _lib.stream()), "wv_snr_floor")
    ts = []
    for rep in range(reps + 1):
        p = [timed(call) for _ in range(20)]
        if rep:
            ts.append(statistics.median(p))
    s = stat(ts)
    return {f"snr_floor_{B}x{T}_ms": s, "GB_per_s_over_12_bytes_per_sample": 12.0 * B * T / (s["median"] * 1e-3) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "snr_floor_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("snrfloorbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "min_snr_db": DB, "frame": wv.configs["generator"].hop_length}
    res["kernel"] = kernel(a.reps)
    print(json.dumps(res["kernel"]), flush=True)
    msg = wv._messages(0xBEEF)
    clips = audio((256, 1, FS), 1)
    res["embed_batch_256x1s"] = pair(lambda: wv.embed_batch(clips, msg), switched(wv, DB, lambda: wv.embed_batch(clips, msg)), a.reps)
    print(json.dumps(res["embed_batch_256x1s"]), flush=True)
    del clips
    stereo = audio((32, 2, 10 * 48000), 2)
    res["embed_native_batch_32x10s_48k_stereo"] = pair(lambda: wv.embed_native_batch(stereo, 48000, msg),
                                                       switched(wv, DB, lambda: wv.embed_native_batch(stereo, 48000, msg)), a.reps)
    print(json.dumps(res["embed_native_batch_32x10s_48k_stereo"]), flush=True)
    del stereo
    res["bank_tick_20ms"] = {}
    for precision in ("f32", "f16"):
        for S in (1, 16, 64):
            res["bank_tick_20ms"][f"{S}_streams_{precision}"] = bank_tick(wv, S, precision, a.reps)
    print(json.dumps(res["bank_tick_20ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
