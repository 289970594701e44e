"""Time what spec_learnable adds to a training step on B clips of T samples (default 64 x 1 s): the five basis-gradient calls
(wv_stft_plan_basis_grad), the five plan refreshes (wv_stft_plan_set_basis_device), and one WatermarkTrainer.step with the switch
off and on.

    python tools/specbasisbench.py [--batch 64] [--samples 16000] [--iters 20] [--out profiles/spec_learnable_bench.json]
                                   [--parent DIR]

Times are medians over --iters calls, each bracketed by device events after --warmup untimed calls.  One JSON document to stdout
and to --out.  The step with the switch off runs the same launches as before the switch existed; --parent DIR (a built checkout of
the parent commit) times that commit's step the same way in a child process, as `step_ms.parent`, to show it."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("WV_SPECBASISBENCH_ROOT") or HERE           # the child of --parent imports the package from DIR
sys.path.insert(0, ROOT)

from waveverify_amd.config import default_config  # noqa: E402
from waveverify_amd.init import random_state_dict  # noqa: E402
from waveverify_amd.train import StftFeatures, WatermarkTrainer  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def step_ms(cfgs, x, msg, iters, warmup, **kw):
    sds = [random_state_dict(c, 0, parametrized=True) for c in cfgs]
    tr = WatermarkTrainer(cfgs[0], sds[0], cfgs[1], sds[1], cfgs[2], sds[2], **kw)
    np.random.seed(0)
    torch.manual_seed(0)
    return timed(lambda: tr.step(x, msg), iters, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "spec_learnable_bench.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its step is timed too")
    ap.add_argument("--step-only", action="store_true", help=argparse.SUPPRESS)        # the child of --parent
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("specbasisbench needs the GPU")
    B, T = a.batch, a.samples
    rng = np.random.default_rng(0)
    x = torch.from_numpy((0.1 * rng.standard_normal((B, 1, T))).astype(np.float32)).cuda()
    msg = torch.from_numpy(rng.integers(0, 2, (B, 16)).astype(np.float32)).cuda()
    cfgs = [default_config(k) for k in ("generator", "detector", "locator")]
    if a.step_only:
        print(json.dumps({"step_ms": step_ms(cfgs, x, msg, a.iters, a.warmup)}))
        return
    from waveverify_amd.init import stft_basis_keys
    res = {"batch": B, "samples": T, "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "basis_grad_ms": {},
           "refresh_ms": {}, "step_ms": {}}
    plans, stride, flops = [], 1, 0.0
    for s, (key, n_fft) in enumerate(stft_basis_keys(cfgs[0]).items()):
        st = StftFeatures(n_fft, stride, cfgs[0].spec_means[s], cfgs[0].spec_stds[s])
        Tf = -(-T // stride)
        dP = torch.randn(B, n_fft // 2 + 1, Tf, device="cuda")
        basis, d = torch.randn(n_fft + 2, n_fft, device="cuda"), torch.empty(n_fft + 2, n_fft, device="cuda")
        plans.append((st, dP, basis, d))
        res["basis_grad_ms"][f"n{n_fft}_hop{stride}"] = timed(lambda: st.basis_grad(x, dP, d), a.iters, a.warmup)
        # (leaves the plan on a random basis: the gradient's time does not depend on the values)
        res["refresh_ms"][f"n{n_fft}"] = timed(lambda: st.set_basis_device(basis), a.iters, a.warmup)
        flops += 2 * 2.0 * (n_fft + 2) * n_fft * B * Tf                        # the forward recompute and the time-contracting product
        if s < len(cfgs[0].strides):
            stride *= cfgs[0].strides[s]
    res["basis_grad_ms"]["all"] = timed(lambda: [st.basis_grad(x, dP, d) for st, dP, _, d in plans], a.iters, a.warmup)
    res["refresh_ms"]["all"] = timed(lambda: [st.set_basis_device(b) for st, _, b, _ in plans], a.iters, a.warmup)
    res["basis_grad_gflop"] = flops / 1e9
    res["basis_grad_tflops_achieved"] = flops / (res["basis_grad_ms"]["all"] * 1e-3) / 1e12
    del plans
    for name, on in (("off", False), ("on", True)):
        res["step_ms"][name] = step_ms(cfgs, x, msg, a.iters, a.warmup, spec_learnable=on)
    if a.parent:
        import subprocess
        env = dict(os.environ, WV_SPECBASISBENCH_ROOT=os.path.abspath(a.parent))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-only", "--batch", str(B), "--samples", str(T), "--iters", str(a.iters),
                              "--warmup", str(a.warmup)], env=env, check=True, capture_output=True, text=True).stdout
        res["step_ms"]["parent"] = json.loads(out.strip().splitlines()[-1])["step_ms"]
        res["step_ms"]["off_over_parent"] = res["step_ms"]["off"] / res["step_ms"]["parent"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
