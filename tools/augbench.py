#!/usr/bin/env python3
"""Bandwidth of the fused augmentation launch (csrc/wv_aug.hip) against the HBM roof, and the reference-style CPU
loop beside it (the oracle's restatement, 1 thread).

    python tools/augbench.py [--batches 64 1024 8192]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import augment as A          # noqa: E402

PEAK = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1024, 8192])
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    T = 16000
    for B in a.batches:
        x = torch.randn(B, 1, T, device="cuda")
        w = x + 1e-3
        aug = A.TemporalAugmenter(16000, 0.1)
        np.random.seed(0)
        plan = aug.localization_augmenter.draw_plan(B, T)
        for name, sm in (("loc+reverse", A.SeqMap(A.SEQ_REVERSE, t_out=T)), ("loc+roll", A.SeqMap(A.SEQ_ROLL, a=4321, t_out=T)),
                         ("loc+shuffle", A.SeqMap(A.SEQ_PERMUTE, a=8000, perm=np.array([1, 0], np.int32), t_out=T))):
            plan_d = torch.from_numpy(plan).cuda()
            lib = A._lib.load()
            outs = [torch.empty_like(x) for _ in range(3)]
            perm_d = torch.from_numpy(sm.perm).cuda() if sm.perm is not None else None

            def launch():
                rc = lib.wv_aug_localize_sequence(x.data_ptr(), w.data_ptr(), plan_d.data_ptr(), plan.shape[1], 1600, sm.mode, sm.a,
                                                  sm.b, sm.c, perm_d.data_ptr() if perm_d is not None else None, outs[0].data_ptr(),
                                                  outs[1].data_ptr(), outs[2].data_ptr(), B, 1, T, T, A._lib.stream())
                assert rc == 0
            for _ in range(5):
                launch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / a.reps * 1e3
            gb = 4.0 * B * T * 5 / 1e9
            print(f"B={B:5d} {name:12s} {us:9.1f} us  {gb / (us * 1e-6):8.1f} GB/s  frac {gb / (us * 1e-6) / PEAK:.3f}")
        if B <= 64:
            from oracle import wv_oracle_aug as OA
            xn, wn = x.cpu().numpy(), w.cpu().numpy()
            t0 = time.perf_counter()
            np.random.seed(0)
            o = OA.localization_forward(xn, wn, 1600)
            OA.sequence_forward(o[2], o[0], o[1], 16000)
            print(f"B={B:5d} CPU loop (oracle, 1 thread) {(time.perf_counter() - t0) * 1e6:9.1f} us")


if __name__ == "__main__":
    main()
