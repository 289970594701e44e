"""Cost of span embedding against watermarking whole clips and splicing -> profiles/span_embed_bench.json.

    python tools/spanbench.py [--reps 15] [--out profiles/span_embed_bench.json]

The default full-size generator with seeded random weights, exact and f16.  Every time is the host clock around one call that ends in a
device synchronise; repetition 0 warms up, and the figures are medians over the repetitions with their min and max (the spread).  Within a
repetition the contenders take turns (interleaved).
    (a) inserts   32 clips x 30 s with one 2 s span each (one id)
    (b) items     one 600 s clip with six 5 s spans of six ids
Each: embed_spans_clips against the only route there was before it: embed_clips once per distinct id over the whole clips, then a
torch.where splice per id on the device.  Both routes are checked against each other once (largest difference inside the spans, equality
outside).  expected_share = sum(H + span) / (ids x sum T), the share of samples the span route runs; peak memory is the allocator's peak
above what is resident before the call (the nets).
    (c) kernels   wv_span_gather and wv_span_scatter_add alone on scenario (a)'s one launch.
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
from waveverify_amd import _lib, window  # noqa: E402
from waveverify_amd.core import WaveVerify  # noqa: E402

FS = 16000


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def audio(B, n, seed):
    rng = np.random.default_rng([FS, B, seed])
    return torch.from_numpy(np.clip(0.1 * rng.standard_normal((B, 1, n), dtype=np.float32), -1, 1)).cuda()


def scenarios():
    """-> {name: (clips [B,1,T], spans per clip [(start, end, id)])}."""
    a = [[((3 + b % 20) * FS + 37 * b, (5 + b % 20) * FS + 37 * b, 0xBEEF)] for b in range(32)]
    b = [[((40 + 95 * i) * FS + 11 * i, (45 + 95 * i) * FS + 11 * i, 0x1000 + i) for i in range(6)]]
    return {"inserts_32x30s_one_2s_span": (audio(32, 30 * FS, 0), a), "items_600s_six_5s_spans": (audio(1, 600 * FS, 1), b)}


def splice(wv, clips, spans):
    """The route of before: one whole-clip embed per distinct id, then the spans cut in."""
    out = clips.clone()
    t = torch.arange(clips.shape[-1], device=clips.device)
    for wid in sorted({w for sp in spans for _, _, w in sp}):
        wm = wv.embed_clips(clips, wid)
        mask = torch.zeros(clips.shape, dtype=torch.bool, device=clips.device)
        for b, sp in enumerate(spans):
            for s, e, w in sp:
                if w == wid:
                    mask[b, 0] |= (t >= s) & (t < e)
        out = torch.where(mask, wm, out)
    return out


def peak_above_resident(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def scenario(wv, clips, spans, reps):
    H = window.halo(wv.configs["generator"])
    ids = len({w for sp in spans for _, _, w in sp})
    share = sum(H + e - s for sp in spans for s, e, _ in sp) / (ids * clips.shape[0] * clips.shape[-1])
    got, ref = wv.embed_spans_clips(clips, spans), splice(wv, clips, spans)
    inside = torch.zeros(clips.shape, dtype=torch.bool, device=clips.device)
    for b, sp in enumerate(spans):
        for s, e, _ in sp:
            inside[b, 0, s:e] = True
    res = {"expected_share": share, "max_abs_difference_inside_spans": float((got - ref)[inside].abs().max()),
           "equal_outside_spans": bool(torch.equal(got[~inside], ref[~inside])),
           "launches": len(window.plan_spans([clips.shape[-1]] * clips.shape[0], [[(s, e, 0) for s, e, _ in sp] for sp in spans],
                                             wv._window_samples(30.0), wv.configs["generator"]))}
    del got, ref
    res["span_peak_MiB"] = peak_above_resident(lambda: wv.embed_spans_clips(clips, spans))
    res["splice_peak_MiB"] = peak_above_resident(lambda: splice(wv, clips, spans))
    ts, tw, th = [], [], []
    for rep in range(reps + 1):
        a = timed(lambda: wv.embed_spans_clips(clips, spans))
        b = timed(lambda: splice(wv, clips, spans))
        t0 = time.perf_counter()                                     # the host planning alone: no device work
        lengths = [clips.shape[-1]] * clips.shape[0]
        window.plan_spans(lengths, [[(s, e, 0) for s, e, _ in sp] for sp in spans], wv._window_samples(30.0), wv.configs["generator"])
        wv._span_messages(spans)
        c = (time.perf_counter() - t0) * 1e3
        if rep:
            ts.append(a)
            tw.append(b)
            th.append(c)
    res.update({"span_ms": stat(ts), "splice_ms": stat(tw), "host_planning_ms": stat(th),
                "span_over_splice": statistics.median(ts) / statistics.median(tw)})
    return res


def kernels(wv, clips, spans, reps):
    lib, dev, cfg = _lib.load(), wv.device, wv.configs["generator"]
    B, T = clips.shape[0], clips.shape[-1]
    wins = [w for g in window.plan_spans([T] * B, [[(s, e, 0) for s, e, _ in sp] for sp in spans], wv._window_samples(30.0), cfg, float("inf"))
            for w in g]
    bases = [b * T for b in range(B)]
    A, Lmax = len(wins), max(w.length for w in wins)
    gd = torch.tensor(window.span_gather_desc(wins, bases), dtype=torch.int64, device=dev)
    sd = torch.tensor(window.span_scatter_desc(wins, bases), dtype=torch.int64, device=dev)
    packed, out = clips.reshape(-1), clips.reshape(-1).clone()
    xw, y = torch.empty((A, 1, Lmax), device=dev), torch.randn((A, 1, Lmax), device=dev)
    ramp = torch.from_numpy(window.span_ramp(160)).to(dev)
    ga = lambda: _lib.check(lib.wv_span_gather(packed.data_ptr(), packed.numel(), gd.data_ptr(), xw.data_ptr(), A, Lmax, _lib.stream()))
    sc = lambda: _lib.check(lib.wv_span_scatter_add(y.data_ptr(), out.data_ptr(), sd.data_ptr(), ramp.data_ptr(), 160, 1.0, out.data_ptr(), out.numel(),
                                                    A, Lmax, _lib.stream()))
    tg, tsc = [], []
    for rep in range(reps + 1):
        pg, ps = [], []
        for _ in range(50):
            pg.append(timed(ga))
            ps.append(timed(sc))
        if rep:
            tg.append(statistics.median(pg))
            tsc.append(statistics.median(ps))
    return {f"span_gather_{A}x{Lmax}_ms": stat(tg), f"span_scatter_add_{A}x{Lmax}_fade160_ms": stat(tsc)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "span_embed_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spanbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    sc = scenarios()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "halo": window.halo(wv.configs["generator"]), "scenarios": {}}
    res["kernels"] = kernels(wv, *sc["inserts_32x30s_one_2s_span"], a.reps)
    for precision in ("f32", "f16"):
        wv.set_precision(precision)
        for name, (clips, spans) in sc.items():
            res["scenarios"][f"{name}_{precision}"] = scenario(wv, clips, spans, a.reps)
            print(json.dumps(res["scenarios"]), flush=True)
    wv.set_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
