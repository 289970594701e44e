"""Windowed execution measured.

    python tools/windowbench.py longform [--seconds 60 300 1200] [--window-seconds 30] [--max-windows 8]
    python tools/windowbench.py session [--sessions 1 64 512] [--ticks-ms 20 100 1000] [--seconds 4]

longform: one clip, embed -> detect -> locate, whole-clip forwards vs the windowed path: ms and torch.cuda.max_memory_allocated.
session:  S lockstep sessions fed ticks of the given length, exact and f16 mode: ms per tick and the real-time factor
          (audio seconds per wall second, per session).  One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from waveverify_amd import window  # noqa: E402
from waveverify_amd.config import default_config  # noqa: E402
from waveverify_amd.init import random_state_dict  # noqa: E402
from waveverify_amd.nets import HipNet  # noqa: E402
from waveverify_amd.session import DetectSession, EmbedSession, LocateSession  # noqa: E402

SR = 16000


def _nets():
    return {k: HipNet(default_config(k), random_state_dict(default_config(k), 0)) for k in ("generator", "detector", "locator")}


def _timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, torch.cuda.max_memory_allocated()


def longform(a):
    msg = torch.randint(0, 2, (1, 16), device="cuda").float()
    for sec in a.seconds:
        x = (0.1 * torch.randn(1, 1, int(sec * SR), device="cuda")).clamp(-1, 1)
        W = a.window_seconds * SR
        modes = {
            "whole": lambda n: (lambda wm: (n["detector"].detector_mean_prob(wm), n["locator"].locator(wm)))(
                n["generator"].generator(x, msg, add_input=True)),
            "windowed": lambda n: (lambda wm: (window.windowed_detector_mean_prob(n["detector"], wm, W, max_windows=a.max_windows),
                                               window.windowed_locator(n["locator"], wm, W, max_windows=a.max_windows)))(
                window.windowed_generator(n["generator"], x, msg, W, max_windows=a.max_windows)),
        }
        for name, fn in modes.items():
            nets = _nets()                      # fresh workspaces per mode: the peak is this mode's own
            fn(nets)                            # warm-up (workspace allocation, first launches)
            ms = []
            for _ in range(a.reps):
                t, peak = _timed(lambda: fn(nets))
                ms.append(t)
            print(json.dumps({"bench": "longform", "seconds": sec, "mode": name, "ms": min(ms), "ms_all": ms,
                              "max_memory_allocated_GiB": round(peak / 2 ** 30, 3)}), flush=True)
            del nets
            torch.cuda.empty_cache()


def session(a):
    nets = _nets()
    for prec in ("f32", "f16"):
        for S in a.sessions:
            for tick_ms in a.ticks_ms:
                n = tick_ms * SR // 1000
                ticks = max(3, int(a.seconds * 1000 // tick_ms))
                x = (0.1 * torch.randn(S, n * ticks, device="cuda")).clamp(-1, 1)
                msg = torch.randint(0, 2, (S, 16), device="cuda").float()
                for kind, make in (("embed", lambda: EmbedSession(nets["generator"], msg, prec)),
                                   ("detect", lambda: DetectSession(nets["detector"], S, prec)),
                                   ("locate", lambda: LocateSession(nets["locator"], S, prec))):
                    sess = make()
                    for i in range(2):                          # warm-up ticks (workspace growth)
                        sess.push(x[:, i * n: (i + 1) * n])
                    sess.reset()
                    torch.cuda.synchronize()
                    per = []
                    for i in range(ticks):
                        t = time.perf_counter()
                        sess.push(x[:, i * n: (i + 1) * n])
                        torch.cuda.synchronize()
                        per.append((time.perf_counter() - t) * 1e3)
                    steady = sorted(per[len(per) // 2:])            # ticks past the halo warm-up
                    med = steady[len(steady) // 2]
                    print(json.dumps({"bench": "session", "kind": kind, "precision": prec, "S": S, "tick_ms": tick_ms,
                                      "ticks": ticks, "median_tick_ms": round(med, 3), "max_tick_ms": round(max(per), 3),
                                      "real_time_factor": round(tick_ms / med, 2)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="cmd", required=True)
    lf = sub.add_parser("longform")
    lf.add_argument("--seconds", type=float, nargs="+", default=[60, 300, 1200])
    lf.add_argument("--window-seconds", type=int, default=30)
    lf.add_argument("--max-windows", type=int, default=8)
    lf.add_argument("--reps", type=int, default=2)
    ss = sub.add_parser("session")
    ss.add_argument("--sessions", type=int, nargs="+", default=[1, 64, 512])
    ss.add_argument("--ticks-ms", type=int, nargs="+", default=[20, 100, 1000])
    ss.add_argument("--seconds", type=float, default=4.0)
    a = p.parse_args()
    torch.manual_seed(0)
    with torch.no_grad():
        longform(a) if a.cmd == "longform" else session(a)


if __name__ == "__main__":
    main()
