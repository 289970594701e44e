"""Torch restatement of the multi-scale STFT and mel reconstruction losses (waveverify_amd/spectral_loss.py's documented semantics),
general in everything the C ABI of csrc/wv_specloss.hip is general in.

    res = spectral_oracle(wm, x, scales, dtype=torch.float64, stft_grad_scale=10.0, mel_grad_scale=20.0)

`scales` are the dicts `spectral_loss._Plan` takes: {w, stft: (log_w, mag_w, pow, eps) | None, mel: (...) | None, n_mels, fmin, fmax,
sr}.  Per scale:  S = |torch.stft(center=True, pad_mode="reflect", periodic Hann of length w, hop = w // 4)|, for a mel term projected
onto `slaney_filters` rounded to float32 the way librosa stores them, and

    term = log_w * mean|log10(clamp(S_wm, eps)^pow) - log10(clamp(S_x, eps)^pow)| + mag_w * mean|S_wm - S_x|

(a part whose weight is 0 is not computed).  Gradients come from autograd, each term's on its own.  dtype float64 is the oracle;
dtype float32 evaluates the same formulas in float32 and is the arithmetic floor a float32 kernel can be held against.

Nothing here imports waveverify_amd: the filters are restated per value, not taken from spectral_loss.mel_filters (code under test).
tests/test_oracle_specloss.py pins the float64 evaluation to tests/golden/spectral_loss.npz (the reference's own classes)."""
import math

import numpy as np
import scipy.signal
import torch

MEL_N, MEL_W, STFT_W = [5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048], [2048, 512]
STFT_TERM, MEL_TERM = (1.0, 1.0, 2.0, 1e-5), (1.0, 0.0, 1.0, 1e-5)          # (log_weight, mag_weight, pow, clamp_eps)


def _mel_points(sr, n_mels, fmin, fmax):
    step = math.log(6.4) / 27.0
    hz2mel = lambda f: 15.0 + math.log(f / 1000.0) / step if f >= 1000.0 else 3.0 * f / 200.0      # noqa: E731
    mel2hz = lambda m: 1000.0 * math.exp(step * (m - 15.0)) if m >= 15.0 else 200.0 * m / 3.0      # noqa: E731
    lo, hi = hz2mel(float(fmin)), hz2mel(sr / 2.0 if fmax is None else float(fmax))
    return [mel2hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]


def slaney_filters(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """librosa.filters.mel defaults written out: Slaney mel scale (linear to 1 kHz at 200/3 Hz per mel, then log-spaced with step
    ln(6.4)/27), n_mels + 2 equally spaced mel points from fmin to fmax (None: sr/2), triangles over the bin frequencies k sr / n_fft,
    each scaled by 2 / (upper edge - lower edge) in Hz; float64, not rounded."""
    edges = _mel_points(sr, n_mels, fmin, fmax)
    W = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        lo, mid, hi = edges[m], edges[m + 1], edges[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * sr / n_fft
            W[m, k] = max(0.0, min((f - lo) / (mid - lo), (hi - f) / (hi - mid))) * 2.0 / (hi - lo)
    return W


def slaney_filters_f32(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """The same filters as librosa stores them: the triangle is written into a float32 array and that array is then scaled by the
    float64 area normalisation (float32(float32(triangle) * norm)).  float32."""
    edges = _mel_points(sr, n_mels, fmin, fmax)
    W = np.zeros((n_mels, n_fft // 2 + 1), np.float32)
    for m in range(n_mels):
        lo, mid, hi = edges[m], edges[m + 1], edges[m + 2]
        tri = np.array([max(0.0, min((k * sr / n_fft - lo) / (mid - lo), (hi - k * sr / n_fft) / (hi - mid))) for k in range(n_fft // 2 + 1)])
        W[m] = (tri.astype(np.float32).astype(np.float64) * (2.0 / (hi - lo))).astype(np.float32)
    return W


def empty_bands(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """Indices of the bands of the restated filters that hold no spectrum bin (every weight 0)."""
    return [m for m, row in enumerate(slaney_filters_f32(sr, n_fft, n_mels, fmin, fmax)) if not row.any()]


def magnitude(s, w, dtype=torch.float64):
    """|STFT| of s [B, 1, T] (or [B, T]): centred, reflect padding of w // 2, periodic Hann, hop w // 4 -> [B, w // 2 + 1, T // hop + 1]."""
    win = torch.from_numpy(scipy.signal.get_window("hann", w)).to(dtype)
    return torch.stft(s.reshape(-1, s.shape[-1]), n_fft=w, hop_length=w // 4, window=win, center=True, pad_mode="reflect",
                      return_complex=True).abs()


def term_value(a, b, term):
    """One loss term on two spectrograms of equal shape; None when both weights are 0."""
    log_w, mag_w, p, eps = term
    out = None
    if log_w != 0:
        out = log_w * (torch.log10(a.clamp(eps) ** p) - torch.log10(b.clamp(eps) ** p)).abs().mean()
    if mag_w != 0:
        m = mag_w * (a - b).abs().mean()
        out = m if out is None else out + m
    return out


def unsafe_elements(a, b, term):
    """How many elements sit so close to a jump of the term's gradient that a float32 transform may land on its other side: the
    L1 kinks (|a - b| for the magnitude part, the log difference for the log part) and the clamp's edge a = eps.  A float32 DFT carries
    an absolute error of about 1e-6 of the typical magnitude; the margin asked for is ten times that on either side."""
    log_w, mag_w, p, eps = term
    a, b = a.detach().double(), b.detach().double()
    delta = 1e-6 * float(b.mean())
    bad = torch.zeros_like(a, dtype=torch.bool)
    if mag_w != 0:
        bad |= ((a - b).abs() <= 20 * delta) & ~((a == 0) & (b == 0))      # both exactly 0 (an empty band, silence): sign(0) either way
    if log_w != 0:
        ca, cb = a.clamp(eps), b.clamp(eps)
        live = (a >= eps) | (b >= eps)
        d = (p * torch.log10(ca) - p * torch.log10(cb)).abs()
        bad |= live & (d <= 10 * p * 0.4343 * delta * (1 / ca + 1 / cb))
        bad |= (a - eps).abs() <= 10 * delta
    return int(bad.sum())


def spectral_oracle(wm, x, scales, dtype=torch.float64, stft_grad_scale=1.0, mel_grad_scale=1.0, want_bins=False):
    """wm, x: [B, 1, T] arrays or tensors.  -> dict:
      scales: one dict per scale with `stft` / `mel` (the term, float, or None), `d_stft` / `d_mel` (d term / d wm, [B, 1, T] numpy in
              `dtype`, or None), `unsafe` (unsafe_elements over the scale's terms); with want_bins also `dmag_stft` / `dmag_mel`
              (d term / d|X_wm| per bin, [B, F, Tf]) and `mag_wm` / `mag_x`;
      stft_total, mel_total (floats), d_stft, d_mel (sums over scales), d_total = stft_grad_scale * d_stft + mel_grad_scale * d_mel."""
    as_t = lambda v: (v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(dtype)   # noqa: E731
    wm_t, x_t = as_t(wm).clone().requires_grad_(True), as_t(x)
    zero = np.zeros(tuple(wm_t.shape), wm_t.detach().numpy().dtype)
    out = {"scales": [], "stft_total": 0.0, "mel_total": 0.0, "d_stft": zero.copy(), "d_mel": zero.copy()}
    for s in scales:
        w = int(s["w"])
        a, b = magnitude(wm_t, w, dtype), magnitude(x_t, w, dtype)
        rec = {"w": w, "stft": None, "mel": None, "d_stft": None, "d_mel": None, "unsafe": 0}
        parts = []
        if s.get("stft"):
            parts.append(("stft", a, b, s["stft"]))
        if s.get("mel"):
            fb = torch.from_numpy(slaney_filters_f32(s["sr"], w, s["n_mels"], s.get("fmin", 0.0), s.get("fmax"))).to(dtype)
            parts.append(("mel", fb @ a, fb @ b, s["mel"]))
        for name, pa, pb, term in parts:
            v = term_value(pa, pb, term)
            rec["unsafe"] += unsafe_elements(pa, pb, term)
            if v is None:
                continue
            d_wm, d_mag = torch.autograd.grad(v, [wm_t, a], retain_graph=True)
            rec[name], rec["d_" + name] = float(v.detach()), d_wm.numpy()
            out[name + "_total"] += rec[name]
            out["d_" + name] = out["d_" + name] + rec["d_" + name]
            if want_bins:
                rec["dmag_" + name] = d_mag.numpy()
        if want_bins:
            rec["mag_wm"], rec["mag_x"] = a.detach().numpy(), b.detach().numpy()
        out["scales"].append(rec)
    out["d_total"] = stft_grad_scale * out["d_stft"] + mel_grad_scale * out["d_mel"]
    return out


def default_scales(sr=16000):
    """The default configuration as separate losses: (the two STFT scales, the seven mel scales)."""
    stft = [{"w": w, "stft": STFT_TERM, "mel": None} for w in STFT_W]
    mel = [{"w": w, "stft": None, "mel": MEL_TERM, "n_mels": n, "fmin": 0.0, "fmax": None, "sr": sr} for n, w in zip(MEL_N, MEL_W)]
    return stft, mel


def spectral_restatement(wm, x, sr=16000):
    """float64 torch: the STFT and mel losses of the default configuration as differentiable scalars (torch.stft centred, reflect
    padding, periodic Hann; Slaney filters as written above)."""
    def l1log(a, b, p):
        return (torch.log10(a.clamp(1e-5) ** p) - torch.log10(b.clamp(1e-5) ** p)).abs().mean()
    stft = sum(l1log(magnitude(wm, w), magnitude(x, w), 2.0) + (magnitude(wm, w) - magnitude(x, w)).abs().mean() for w in STFT_W)
    mel = 0.0
    for n, w in zip(MEL_N, MEL_W):
        fb = torch.from_numpy(slaney_filters(sr, w, n).astype(np.float32).astype(np.float64))
        mel = mel + l1log(fb @ magnitude(wm, w), fb @ magnitude(x, w), 1.0)
    return stft, mel
