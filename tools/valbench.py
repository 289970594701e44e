"""Cost of the validation metrics and of one whole validate() on the GPU -> profiles/validate_bench.json.

    python tools/valbench.py [--batch 16] [--samples 16000] [--reps 30] [--out profiles/validate_bench.json]

A: the three fused per-clip calls (metrics.ber_per_clip, metrics.iou_counts, metrics.SISNR) for the seven evaluation effects, with the
   one copy of the counts to the host that validate() makes.
B: the same numbers the way the package got them before: metrics.BER + metrics.MIOU per effect (each ends in a host copy) and a torch
   restatement of SI-SNR.
A and B alternate inside one loop after a warm-up; the medians of the per-iteration host-clock times (each ending in a device
synchronise) and their ratio are written, with one whole validate() of the default full-size nets next to them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import metrics  # noqa: E402
from waveverify_amd.effects import EVAL_EFFECTS  # noqa: E402


def torch_sisnr(est, ref, eps=1e-8):
    out, ref = est.squeeze(1), ref.squeeze(1)
    ref = ref - ref.mean(dim=1, keepdim=True)
    out = out - out.mean(dim=1, keepdim=True)
    e = (ref ** 2).sum(dim=1, keepdim=True) + eps
    proj = (ref * out).sum(dim=1, keepdim=True) * ref / e
    noise = out - proj
    return (10 * torch.log10((proj ** 2).sum(dim=1) / ((noise ** 2).sum(dim=1) + eps) + eps)).mean()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "validate_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("valbench needs the GPU: nothing is measured without one")
    B, T, E = a.batch, a.samples, len(EVAL_EFFECTS)
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = [torch.randn(B, 16, T, device="cuda", generator=g) for _ in range(E)]
    loc = [torch.randn(B, 1, T, device="cuda", generator=g) + 0.5 for _ in range(E)]
    mask = [(torch.rand(B, 1, T, device="cuda", generator=g) < 0.8).float() for _ in range(E)]
    msg = (torch.rand(B, 16, device="cuda", generator=g) < 0.5).float()
    x = 0.1 * torch.randn(B, 1, T, device="cuda", generator=g)
    wm = x + 1e-3 * torch.randn(B, 1, T, device="cuda", generator=g)
    ber, miou, sisnr = metrics.BER(), metrics.MIOU(), metrics.SISNR()

    def fused():
        e, v, c = [], [], []
        for i in range(E):
            ei, vi, _ = metrics.ber_per_clip(logits[i], msg, mask[i])
            e.append(ei); v.append(vi); c.append(metrics.iou_counts(loc[i], mask[i]))
        s = sisnr(wm, x)
        e, v, c, s = (t.cpu().numpy() for t in (torch.stack(e), torch.stack(v), torch.stack(c), s))
        return [float(e[i].sum() / max(v[i].sum(), 1)) for i in range(E)], list(metrics.miou_from_counts(c.astype(np.int64).sum(axis=1))), float(s.mean())

    def classes():
        b = [float(ber(logits[i], msg, mask[i])) for i in range(E)]
        m = [miou((loc[i] > 0.5).float(), mask[i]) for i in range(E)]
        return b, m, float(torch_sisnr(wm, x))

    fa, fb = fused(), classes()
    same = bool(np.allclose(fa[0], fb[0], atol=1e-7) and fa[1] == fb[1] and abs(fa[2] - fb[2]) < 1e-2)
    for _ in range(a.warmup):
        fused(); classes()
    ta, tb = [], []
    for _ in range(a.reps):                                      # interleaved A / B
        ta.append(timed(fused)); tb.append(timed(classes))
    res = {"batch": B, "samples": T, "effects": E, "reps": a.reps, "device": torch.cuda.get_device_name(0), "same_numbers": same,
           "fused_ms_median": statistics.median(ta), "fused_ms_min": min(ta), "fused_ms_max": max(ta),
           "classes_ms_median": statistics.median(tb), "classes_ms_min": min(tb), "classes_ms_max": max(tb),
           "classes_over_fused": statistics.median(tb) / statistics.median(ta),
           "logits_bytes_read_once": E * B * 16 * T * 4}

    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import WatermarkTrainer
    cfgs = [default_config(k) for k in ("generator", "detector", "locator")]
    sds = [random_state_dict(c, 0, parametrized=True) for c in cfgs]
    tr = WatermarkTrainer(cfgs[0], sds[0], cfgs[1], sds[1], cfgs[2], sds[2], spectral_losses=True)
    for _ in range(2):
        tr.validate(x, msg)
    tv = [timed(lambda: tr.validate(x, msg)) for _ in range(max(3, a.reps // 6))]
    res.update({"validate_ms_median": statistics.median(tv), "validate_ms_min": min(tv), "validate_ms_max": max(tv),
                "fused_share_of_validate": statistics.median(ta) / statistics.median(tv),
                "classes_share_of_validate_before": statistics.median(tb) / (statistics.median(tv) - statistics.median(ta) + statistics.median(tb))})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
