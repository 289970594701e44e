"""Time the multi-scale STFT and mel reconstruction losses, forward + backward towards wm, on B clips of T samples (default 64 x 1 s),
scale by scale and together, on the HIP path (waveverify_amd.spectral_loss) and -- for comparison only -- a torch restatement on the
same GPU (torch.stft + autograd, float32 and float64).

    python tools/specloss_bench.py [--batch 64] [--samples 16000] [--iters 20] [--out profiles/specloss_bench.json]

Times are medians over --iters calls, each bracketed by device events after --warmup untimed calls.  One JSON document to stdout
(and to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from waveverify_amd import spectral_loss as SL  # noqa: E402


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


def torch_losses(wm, x, stft_w, mel, sr=16000):
    """The same objective in torch (for comparison only): sum of the STFT terms and of the mel terms, d(10 stft + 20 mel)/dwm."""
    T = wm.shape[-1]
    wm = wm.detach().requires_grad_(True)

    def mag(s, w):
        win = torch.hann_window(w, periodic=True, dtype=s.dtype, device=s.device)
        return torch.stft(s.reshape(-1, T), n_fft=w, hop_length=w // 4, window=win, center=True, pad_mode="reflect", return_complex=True).abs()

    def l1log(a, b, p):
        return (torch.log10(a.clamp(1e-5) ** p) - torch.log10(b.clamp(1e-5) ** p)).abs().mean()
    stft = sum((l1log(mag(wm, w), mag(x, w), 2.0) + (mag(wm, w) - mag(x, w)).abs().mean() for w in stft_w), torch.zeros((), dtype=wm.dtype,
                                                                                                             device=wm.device))
    melv = torch.zeros((), dtype=wm.dtype, device=wm.device)
    for n, w, fb in mel:
        melv = melv + l1log(fb @ mag(wm, w), fb @ mag(x, w), 1.0)
    (10.0 * stft + 20.0 * melv).backward()
    return stft, melv, wm.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("specloss_bench needs the GPU")
    rng = np.random.default_rng(0)
    x = torch.from_numpy((0.1 * rng.standard_normal((a.batch, 1, a.samples))).astype(np.float32)).cuda()
    wm = x + torch.from_numpy((0.01 * rng.standard_normal((a.batch, 1, a.samples))).astype(np.float32)).cuda()
    res = {"batch": a.batch, "samples": a.samples, "iters": a.iters, "device": torch.cuda.get_device_name(0), "hip_ms": {}, "torch_ms": {}}
    # the whole objective through one plan (2048 and 512 shared by both losses)
    both = SL.SpectralLosses()
    out = torch.zeros_like(wm)
    res["hip_ms"]["both_fwd_bwd"] = timed(lambda: both(wm, x, 10.0, 20.0, out=out), a.iters, a.warmup)
    res["hip_ms"]["both_fwd"] = timed(lambda: both(wm, x, want_grad=False), a.iters, a.warmup)
    # scale by scale: the mel term alone, and where the STFT loss shares the window, both terms on one transform
    for n, w in zip(SL.MEL_N_MELS, SL.MEL_WINDOW_LENGTHS):
        mel_one = SL.MelSpectrogramLoss(n_mels=[n], window_lengths=[w])
        res["hip_ms"][f"w{w}_mel_fwd_bwd"] = timed(lambda: mel_one(wm, x, 20.0, out=out), a.iters, a.warmup)
        if w in SL.STFT_WINDOW_LENGTHS:
            pair = SL.SpectralLosses(SL.MultiScaleSTFTLoss(window_lengths=[w]), SL.MelSpectrogramLoss(n_mels=[n], window_lengths=[w]))
            res["hip_ms"][f"w{w}_mel_stft_fwd_bwd"] = timed(lambda: pair(wm, x, 10.0, 20.0, out=out), a.iters, a.warmup)
    # torch restatement on the same GPU, for comparison only
    for dt in (torch.float32, torch.float64):
        mel = [(n, w, torch.from_numpy(SL.mel_filters(16000, w, n)).to(device="cuda", dtype=dt))
               for n, w in zip(SL.MEL_N_MELS, SL.MEL_WINDOW_LENGTHS)]
        wmd, xd = wm.to(dt), x.to(dt)
        res["torch_ms"][f"both_fwd_bwd_{str(dt).split('.')[-1]}"] = timed(lambda: torch_losses(wmd, xd, SL.STFT_WINDOW_LENGTHS, mel), a.iters,
                                                                           a.warmup)
    # the two agree (float64 torch as the yardstick)
    ls, lm, d = both(wm, x, 10.0, 20.0)
    mel64 = [(n, w, torch.from_numpy(SL.mel_filters(16000, w, n)).to(device="cuda", dtype=torch.float64))
             for n, w in zip(SL.MEL_N_MELS, SL.MEL_WINDOW_LENGTHS)]
    rs, rm, rd = torch_losses(wm.double(), x.double(), SL.STFT_WINDOW_LENGTHS, mel64)
    res["check"] = {"stft_rel": abs(float(ls.item()) / float(rs) - 1), "mel_rel": abs(float(lm.item()) / float(rm) - 1),
                    "grad_rel_max": float((d.double() - rd).abs().max() / rd.abs().max())}
    flops = 0.0
    T, B = a.samples, a.batch
    for w in SL.MEL_WINDOW_LENGTHS:
        F, Tf = w // 2 + 1, T // (w // 4) + 1
        flops += 2.0 * (2 * F) * w * Tf * B * 3                                # forward for wm and x, backward for wm
    res["dft_gemm_gflop_fwd_bwd"] = flops / 1e9
    res["dft_gemm_tflops_achieved"] = flops / (res["hip_ms"]["both_fwd_bwd"] * 1e-3) / 1e12
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
