#!/usr/bin/env python3
"""Generate tests/golden/effects_time.npz by running the REFERENCE's own apply_effect (/root/reference/utils/effect_augmentation.py)
on the CPU for its plain-arithmetic time-domain effects, forward and autograd, under fixed torch / numpy / random seeds (build
container only).

The module imports torchaudio and julius at module level (both absent here), so it is loaded by path with stand-ins registered in
sys.modules, like make_golden_aug.py does: `torchaudio` is empty (unused by the effects that are run), and `julius` holds only
    fft_conv1d = torch.nn.functional.conv1d
SUBSTITUTION: julius.fft_conv1d(x, w) is the cross-correlation of x with w, no padding, computed through an FFT; conv1d computes the
same cross-correlation directly.  The two differ by the FFT's rounding only (about 1e-6 of the peak), which is why `echo` and
`smooth` audio are held to the filter bar and not bit for bit.

For every case the file holds the inputs, the parameters the reference drew (replayed from the same seed with the reference's own
draw calls), the output audio and mask, and the gradient of the fixed linear functional (y * r).sum() towards the input (<case>_grad, or the flag
<case>_grad_is_r where that gradient is r itself bit for bit, which keeps the file small).  For echo
the same gradient is also taken in float64 and the float32-versus-float64 difference, relative to the gradient's peak, is stored
as <case>_grad_f32_f64.  AudioProcessor.adjust_audio_length(mode='stretch') is recorded for a few (Tin, Tout) pairs.
Only data is written.

Usage (from repo root, in the build container):  python tests/golden/make_golden_effects_time.py"""
from __future__ import annotations

import importlib.util
import json
import logging
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SR = 16000
LENGTHS = (2000, 1001, 37)

# (effect, params, lengths)
CASES = [
    ("median_filter", {"kernel_size": 3}, LENGTHS), ("median_filter", {"kernel_size": 5}, LENGTHS), ("median_filter", {"kernel_size": 31}, LENGTHS),
    ("median_filter", {"kernel_size": 4}, LENGTHS), ("median_filter", {"kernel_size": 33}, LENGTHS),
    ("quantization", {"bit_depth": 2}, LENGTHS), ("quantization", {"bit_depth": 8}, LENGTHS), ("quantization", {"bit_depth": 16}, LENGTHS),
    ("quantization", {"bit_depth": 24}, LENGTHS), ("quantization", {"bit_depth": 1}, (37,)),
    ("amplitude_scaling", {"scale": 0.7}, LENGTHS), ("amplitude_scaling", {"scale": -1.3}, (1001,)),
    ("shush", {"fraction": 0.1}, LENGTHS), ("shush", {"fraction": 0.5}, LENGTHS), ("shush", {"fraction": 0.0}, (1001, 37)),
    ("shush", {"fraction": 1.0}, (37,)),
    ("sample_suppression", {"suppression_percentage": 0.1}, LENGTHS), ("sample_suppression", {"suppression_percentage": 0.3}, (1001,)),
    ("pink_noise", {"noise_std": 0.01}, (1001, 37)),
    ("random_noise", {"noise_std": 0.001}, LENGTHS), ("white_noise", {"noise_std": 0.01}, (1001,)),
    ("smooth", {"window_size_range": (2, 10)}, LENGTHS), ("smooth", {"window_size_range": (2, 3)}, LENGTHS),
    ("smooth", {"window_size_range": (7, 8), "valid_threshold": 0.7}, (1001, 37)),
    ("echo", {}, LENGTHS), ("echo", {"volume_range": (0.3, 0.9), "duration_range": (0.001, 0.01)}, LENGTHS),
]
STRETCH = [(2500, 2000), (1252, 1001), (47, 37), (1001, 2000), (37, 1001)]


def _load():
    sys.dont_write_bytecode = True
    logging.disable(logging.CRITICAL)
    import torch
    sys.modules["torchaudio"] = types.ModuleType("torchaudio")
    j = types.ModuleType("julius")
    j.fft_conv1d = torch.nn.functional.conv1d          # the same cross-correlation, computed directly (see the module docstring)
    sys.modules["julius"] = j
    spec = importlib.util.spec_from_file_location("ref_effect_augmentation", f"{REF}/utils/effect_augmentation.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def inputs(T: int):
    """x [2,1,T] with distinct magnitudes, one unique peak and two exact zeros per row; a mask with a zero stretch; the functional r."""
    rng = np.random.default_rng(1000 + T)
    x = (0.1 * rng.standard_normal((2, 1, T))).astype(np.float32)
    x[0, 0, T // 3], x[1, 0, T // 2] = 0.9, -0.6
    x[:, :, 5], x[:, :, T - 9] = 0.0, 0.0
    for row in x.reshape(2, T):
        while True:                                        # nudge repeated magnitudes apart by one ulp
            _, first = np.unique(np.abs(row), return_index=True)
            dup = np.setdiff1d(np.arange(T), first)
            dup = dup[row[dup] != 0]
            if not len(dup):
                break
            row[dup] = np.nextafter(row[dup], np.float32(1.0))
        mags = np.abs(row[row != 0])
        assert len(np.unique(mags)) == len(mags) and (row == 0).sum() == 2
    mask = np.ones((2, 1, T), dtype=np.float32)
    mask[0, 0, T // 4: T // 4 + max(3, T // 10)] = 0.0
    mask[1, 0, : 4] = 0.0
    r = rng.standard_normal((2, 1, T)).astype(np.float32)
    return x, mask, r


def seed_all(seed: int):
    import torch
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def drawn(name, params, x, seed):
    """The parameters the reference draws for this call, replayed from the same seed with its own draw calls
    (effect_augmentation.py:1558-1567 echo, :1947 smooth, :2088-2091 sample_suppression, :2125 / :2360 the noises, :1645-1663 pink)."""
    import torch
    seed_all(seed)
    T = x.shape[-1]
    if name == "echo":
        duration = torch.FloatTensor(1).uniform_(*params.get("duration_range", (0.1, 0.5))).item()
        duration = min(duration, T / SR * 0.5)
        volume = torch.FloatTensor(1).uniform_(*params.get("volume_range", (0.1, 0.5))).item()
        return {"n": np.array(max(int(SR * duration), 2)), "volume": np.array(volume, dtype=np.float64)}
    if name == "smooth":
        return {"w": np.array(int(torch.FloatTensor(1).uniform_(*params["window_size_range"])))}
    if name == "sample_suppression":
        num = int(T * params["suppression_percentage"])
        return {"idx": np.stack([torch.randperm(T)[:num].numpy() for _ in range(x.shape[0] * x.shape[1])]).astype(np.int32)}
    if name in ("random_noise", "white_noise"):
        return {"noise": torch.randn_like(torch.from_numpy(x)).numpy()}
    return {}


def main():
    import torch
    ea = _load()
    out = {}
    listing = []
    for T in LENGTHS:
        out[f"x_{T}"], out[f"mask_{T}"], out[f"r_{T}"] = inputs(T)
    for ci, (name, params, lengths) in enumerate(CASES):
        for T in lengths:
            key, seed = f"c{ci}_{T}", 100 * ci + T
            x, mask, r = out[f"x_{T}"], out[f"mask_{T}"], out[f"r_{T}"]
            for k, v in drawn(name, params, x, seed).items():
                out[f"{key}_{k}"] = v
            grads = {}
            for dt in (torch.float32, torch.float64):
                seed_all(seed)
                xt = torch.from_numpy(x).to(dt).requires_grad_(True)
                y, m = ea.apply_effect(xt, name, sample_rate=SR, mask=torch.from_numpy(mask).to(dt), **params)
                (y * torch.from_numpy(r).to(dt)).sum().backward()
                grads[dt] = xt.grad.numpy()
                if dt == torch.float32:
                    out[f"{key}_y"], out[f"{key}_m"] = y.detach().numpy(), m.numpy()
                    if np.array_equal(grads[dt], r):       # a straight-through gradient: recorded as such, not as a second copy of r
                        out[f"{key}_grad_is_r"] = np.array(True)
                    else:
                        out[f"{key}_grad"] = grads[dt]
                if name != "echo":
                    break
            if name == "echo":
                g64 = grads[torch.float64]
                out[f"{key}_grad_f32_f64"] = np.array(np.abs(grads[torch.float32] - g64).max() / np.abs(g64).max())
                assert not out[f"{key}_y"][..., T - int(out[f"{key}_n"]) + 1:].any()          # the drawn n is the one the reference used
            if name == "pink_noise":                       # the noise itself, as the reference's generator returns it: 0 + noise * 1.0
                seed_all(seed)
                out[f"{key}_noise"] = ea.AudioEffects.pink_noise(torch.zeros(x.shape), noise_std=1.0)[0].numpy()
            assert out[f"{key}_y"].dtype == np.float32 and out[f"{key}_y"].shape == x.shape
            listing.append({"key": key, "name": name, "params": params, "T": T, "seed": seed})
            print(key, name, params, {k: (v.tolist() if v.size == 1 else v.shape) for k, v in out.items() if k.startswith(key + "_") and k[len(key) + 1:] in ("n", "volume", "w", "idx", "grad_f32_f64")})
    for tin, tout in STRETCH:
        x = (0.1 * np.random.default_rng(tin + tout).standard_normal((2, 1, tin))).astype(np.float32)
        out[f"stretch_{tin}_{tout}_x"] = x
        out[f"stretch_{tin}_{tout}_y"] = ea.AudioProcessor.adjust_audio_length(torch.from_numpy(x), tout, mode="stretch").numpy()
    out["cases"] = np.array(json.dumps(listing))
    out["stretch"] = np.array(STRETCH, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "effects_time.npz"), **out)
    print("wrote effects_time.npz", os.path.getsize(os.path.join(HERE, "effects_time.npz")), "bytes")


if __name__ == "__main__":
    main()
