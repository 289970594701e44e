"""BER and MIoU, the two metrics parity is reported in.

Restated from /root/reference/scripts/evaluate.py: BER.forward :442-516 (mask-weighted
time-averaged sigmoid, >= threshold, errors over valid bits) and MIOU.forward :591-665
(mean of foreground and background IoU on binary masks; an empty union counts as IoU 1).
Note model/watermarking.py:717,797 binarises the *raw* locator output at 0.5 before MIOU.

Per-clip forms for a validation pass, fused on the GPU (csrc/wv_metrics.hip), one read of the inputs each:

    errors, valid, avg = ber_per_clip(logits, bits, mask)      # BER of the batch = errors.sum() / valid.sum()
    miou = miou_per_clip(locator_out, mask)                    # [B] float64, from iou_counts(...) -> [B,4] int32
    sisnr = SISNR()(estimate, reference)                       # [B] float64 dB; SISNR().mean(...) is the reference's scalar
    stoi = STOI()(estimate, reference, sample_rate=16000)      # [B] float64 (csrc/wv_stoi.hip; the algorithm in stoi.py)
    lufs = Loudness()(x, sample_rate=16000)                    # [B] float64 LUFS (csrc/wv_loudness.hip; the algorithm in loudness.py)

Device tensors go through the kernels; CPU tensors take a torch route with the same arithmetic (f64 sums, then the reference's f32
finish for the bit decision), so host-only callers need no GPU.  `BER` and `MIOU` above stay the reference's own formulation.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _lib


class BER:
    def __init__(self, threshold: float = 0.5, eps: float = 1e-8):
        self.threshold, self.eps = threshold, eps

    def __call__(self, decoded_logits: torch.Tensor, original_bits: torch.Tensor,
                 presence_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, W, T = decoded_logits.shape
        if tuple(original_bits.shape) != (B, W):
            raise RuntimeError("BER computation failed")        # reference wraps the ValueError
        probs = torch.sigmoid(decoded_logits)
        if presence_mask is not None:
            if presence_mask.shape[0] != B or presence_mask.shape[2] != T:
                raise RuntimeError("BER computation failed")
            mask = presence_mask.expand(-1, W, -1)
            valid = mask.sum(dim=2) > 0
            avg = (probs * mask).sum(dim=2) / (mask.sum(dim=2) + self.eps)
        else:
            avg = probs.mean(dim=2)
            valid = torch.ones((B, W), dtype=torch.bool, device=decoded_logits.device)
        decoded = (avg >= self.threshold).float()
        errors = ((decoded != original_bits.float()) * valid).sum()
        total = valid.sum()
        if total > 0:
            return errors / total
        return torch.tensor(0.0, device=decoded_logits.device)


class MIOU:
    def __call__(self, predicted_mask: Union[torch.Tensor, np.ndarray],
                 ground_truth_mask: Union[torch.Tensor, np.ndarray]) -> float:
        p = predicted_mask.detach().cpu().numpy() if torch.is_tensor(predicted_mask) else np.asarray(predicted_mask)
        g = ground_truth_mask.detach().cpu().numpy() if torch.is_tensor(ground_truth_mask) else np.asarray(ground_truth_mask)
        if p.shape != g.shape or not np.isin(np.unique(p), [0, 1]).all() or not np.isin(np.unique(g), [0, 1]).all():
            raise RuntimeError("MIOU computation failed")
        out = []
        for cls in (1, 0):
            inter = np.logical_and(p == cls, g == cls).sum()
            union = np.logical_or(p == cls, g == cls).sum()
            out.append((1.0 if inter == 0 else 0.0) if union == 0 else inter / union)
        return float(sum(out) / 2)


# ---- per-clip metrics (the validation pass) --------------------------------------------------------------------------------------
def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


def ber_per_clip(logits: torch.Tensor, bits: torch.Tensor, mask: Optional[torch.Tensor] = None, threshold: float = 0.5,
                 eps: float = 1e-8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """BER.forward (scripts/evaluate.py:442-516) split per clip -> (errors [B] int32, valid [B] int32, avg [B,W] float32) on the
    logits' device: `valid` counts the bits of a clip whose mask has a live sample, `errors` those of them decoded wrongly, and the
    reference's scalar is errors.sum() / valid.sum() (0 when nothing is valid).  Per (clip, bit) the masked sums of sigmoid(logits)
    and of the mask are taken in float64 and rounded to float32; the decision is then the reference's own float32 expression,
    avg = S / (N + eps) >= threshold (S / T without a mask), so a tie such as all-zero logits decodes as it does there."""
    if logits.dim() != 3:
        raise ValueError(f"logits must be [B, W, T], got {tuple(logits.shape)}")
    B, W, T = logits.shape
    if tuple(bits.shape) != (B, W):
        raise ValueError(f"bits must be [B, W] = [{B}, {W}], got {tuple(bits.shape)}")
    if mask is not None and (mask.dim() != 3 or mask.shape[0] != B or mask.shape[1] != 1 or mask.shape[2] != T):
        raise ValueError(f"mask must be [B, 1, T] = [{B}, 1, {T}], got {tuple(mask.shape)}")
    z, g = _f32(logits), _f32(bits).to(logits.device)
    m = None if mask is None else _f32(mask).to(logits.device)
    if z.is_cuda:
        lib = _lib.load()
        avg = torch.empty(B, W, dtype=torch.float32, device=z.device)
        errors = torch.empty(B, dtype=torch.int32, device=z.device)
        valid = torch.empty(B, dtype=torch.int32, device=z.device)
        ws = _lib.scratch(int(lib.wv_metrics_decode_workspace_bytes(B, W, T)), z.device)
        _lib.check(lib.wv_metrics_decode(z.data_ptr(), g.data_ptr(), _lib.ptr(m), float(threshold), float(eps), B, W, T,
                                         avg.data_ptr(), errors.data_ptr(), valid.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _lib.stream(z.device)), "wv_metrics_decode")
        return errors, valid, avg
    p = torch.sigmoid(z.double())
    if m is not None:
        md = m.double().expand(-1, W, -1)
        s, n = (p * md).sum(dim=2).float(), md.sum(dim=2).float()
        avg = s / (n + torch.tensor(eps, dtype=torch.float32))
        ok = n > 0
    else:
        avg = p.sum(dim=2).float() / torch.tensor(float(T), dtype=torch.float32)
        ok = torch.ones(B, W, dtype=torch.bool)
    decoded = (avg >= torch.tensor(threshold, dtype=torch.float32)).float()
    errors = ((decoded != g) & ok).sum(dim=1).to(torch.int32)
    return errors, ok.sum(dim=1).to(torch.int32), avg


def iou_counts(locator_out: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """-> [B,4] int32 on the inputs' device: per clip |p & g1|, |p | g1|, |~p & g0|, |~p | g0| with p = locator_out > 0.5 (the RAW
    locator output, as watermarking.py:797 binarises it), g1 = mask == 1, g0 = mask == 0.  Summed over clips they are the counts MIOU
    takes on the whole batch tensor."""
    if locator_out.shape != mask.shape or locator_out.dim() != 3 or locator_out.shape[1] != 1:
        raise ValueError(f"locator output and mask must both be [B, 1, T], got {tuple(locator_out.shape)} and {tuple(mask.shape)}")
    B, _, T = locator_out.shape
    p, g = _f32(locator_out), _f32(mask).to(locator_out.device)
    if p.is_cuda:
        lib = _lib.load()
        counts = torch.empty(B, 4, dtype=torch.int32, device=p.device)
        ws = _lib.scratch(int(lib.wv_metrics_iou_workspace_bytes(B, T)), p.device)
        _lib.check(lib.wv_metrics_iou(p.data_ptr(), g.data_ptr(), B, T, counts.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream(p.device)), "wv_metrics_iou")
        return counts
    fg, g1, g0 = (p > 0.5)[:, 0], (g == 1)[:, 0], (g == 0)[:, 0]
    return torch.stack([(fg & g1).sum(1), (fg | g1).sum(1), (~fg & g0).sum(1), (~fg | g0).sum(1)], dim=1).to(torch.int32)


def miou_from_counts(counts) -> np.ndarray:
    """[..., 4] integer counts -> float64 mIoU: the mean of the foreground and the background IoU, an empty union counting as IoU 1
    (MIOU.forward, scripts/evaluate.py:591-665)."""
    c = (counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)).astype(np.float64)
    out = np.zeros(c.shape[:-1], np.float64)
    for k in (0, 2):
        inter, union = c[..., k], c[..., k + 1]
        out += np.where(union == 0, 1.0, inter / np.where(union == 0, 1.0, union))
    return out / 2


def miou_per_clip(locator_out: torch.Tensor, mask: torch.Tensor) -> np.ndarray:
    """MIOU of every clip of a batch -> [B] float64 (host): exact integer counts from one pass over the RAW locator output and the
    0 / 1 mask (`iou_counts`), the ratio formed on the host in float64."""
    return miou_from_counts(iou_counts(locator_out, mask))


class SISNR:
    """The reference's scale-invariant signal-to-noise ratio (scripts/evaluate.py:146-229), per clip, in dB:

        x0, y0 = estimate - mean, reference - mean;  proj = y0 <x0, y0> / (|y0|^2 + eps)
        SI-SNR = 10 log10(|proj|^2 / (|x0 - proj|^2 + eps) + eps)

    with all three eps of the reference; a silent reference gives 10 log10(eps).  One pass gathers the five moments sum x, sum y,
    sum xx, sum xy, sum yy in float64 (`last_moments`, [B,5]); the rest is algebra on them in float64.  The noise power is taken as
    (<x0,x0> - <x0,y0>^2 / |y0|^2) + (<x0,y0> eps)^2 / (|y0|^2 (|y0|^2 + eps)^2), which is the same number without the cancellation.
    Calling returns [B] float64 on the inputs' device; `.mean(...)` is the scalar the reference's module returns."""

    def __init__(self, eps: float = 1e-8):
        self.eps = float(eps)
        self.last_moments: Optional[torch.Tensor] = None

    def __call__(self, estimates: torch.Tensor, references: torch.Tensor) -> torch.Tensor:
        if estimates.shape != references.shape or estimates.dim() != 3 or estimates.shape[1] != 1:
            raise ValueError(f"estimates and references must both be [B, 1, T], got {tuple(estimates.shape)} and {tuple(references.shape)}")
        B, _, T = estimates.shape
        y = _f32(references)
        x = _f32(estimates).to(y.device)                        # the reference moves the estimate to the reference's device
        if y.is_cuda:
            lib = _lib.load()
            out = torch.empty(B, dtype=torch.float64, device=y.device)
            mom = torch.empty(B, 5, dtype=torch.float64, device=y.device)
            ws = _lib.scratch(int(lib.wv_metrics_sisnr_workspace_bytes(B, T)), y.device)
            _lib.check(lib.wv_metrics_sisnr(x.data_ptr(), y.data_ptr(), B, T, self.eps, out.data_ptr(), mom.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _lib.stream(y.device)), "wv_metrics_sisnr")
            self.last_moments = mom
            return out
        xd, yd = x.double()[:, 0], y.double()[:, 0]
        mom = torch.stack([xd.sum(1), yd.sum(1), (xd * xd).sum(1), (xd * yd).sum(1), (yd * yd).sum(1)], dim=1)
        self.last_moments = mom
        return self.from_moments(mom, T)

    def from_moments(self, moments: torch.Tensor, T: int) -> torch.Tensor:
        """[B,5] float64 moments of T-sample clips -> [B] float64 dB (the arithmetic the kernel's second launch runs)."""
        m, eps, n = moments.double(), self.eps, float(T)
        xx = (m[:, 2] - (m[:, 0] * m[:, 0]) / n).clamp_min(0.0)
        xy = m[:, 3] - (m[:, 0] * m[:, 1]) / n
        yy = (m[:, 4] - (m[:, 1] * m[:, 1]) / n).clamp_min(0.0)
        e = yy + eps
        a = xy / e
        live = yy > 0
        yys = torch.where(live, yy, torch.ones_like(yy))
        k = xy * eps / (yys * e)
        noise = torch.where(live, (xx - (xy / yys) * xy).clamp_min(0.0) + yy * k * k, xx)
        return 10.0 * torch.log10((a * a * yy) / (noise + eps) + eps)

    def mean(self, estimates: torch.Tensor, references: torch.Tensor) -> torch.Tensor:
        return self(estimates, references).mean()


class STOI:
    """Short-time objective intelligibility (Taal et al. 2011), per clip, the third number next to BER / mIoU and SI-SNR the reference
    reports on a validation batch (scripts/evaluate.py:65-144, there through the pystoi package, clip by clip on the host).  The
    algorithm, its constants and the frame-range switch are in waveverify_amd/stoi.py; parity with an installed `pystoi` stays unpinned.

        STOI()(estimates, references, sample_rate=16000) -> [B] float64 on the inputs' device

    in the reference's own argument order: the REFERENCE clip is the algorithm's x (its silent frames are the ones dropped) and the
    measure is not symmetric.  `.mean(...)` is the scalar the reference's module returns; `.last_frames` ([B,2] int32) holds the frames
    kept and the frames of each clip.  A clip left with fewer than 30 frames gives 1e-5, pystoi's answer; the CPU route also raises pystoi's
    RuntimeWarning, the device route does not (it would cost a trip to the host: `last_frames` says which clips, and validate() warns
    from the copy it makes anyway).  Device tensors go through csrc/wv_stoi.hip (one call; tables cached per sample rate and device),
    CPU tensors through the float64 numpy route."""

    def __init__(self, extended: bool = False):
        if extended:
            raise NotImplementedError("extended STOI is not implemented")
        self.last_frames: Optional[torch.Tensor] = None

    def __call__(self, estimates: torch.Tensor, references: torch.Tensor, sample_rate: int = 16000) -> torch.Tensor:
        import warnings
        from . import stoi as S
        if estimates.shape != references.shape or estimates.dim() != 3 or estimates.shape[1] != 1:
            raise ValueError(f"estimates and references must both be [B, 1, T], got {tuple(estimates.shape)} and {tuple(references.shape)}")
        if int(sample_rate) < 1:
            raise ValueError(f"sample_rate must be positive, got {sample_rate}")
        B, _, T = estimates.shape
        x = _f32(references)
        y = _f32(estimates).to(x.device)
        if x.is_cuda:
            lib = _lib.load()
            kern, up, down, L, width, basis = S.device_tables(sample_rate, x.device)
            out = torch.empty(B, dtype=torch.float64, device=x.device)
            frames = torch.empty(B, 2, dtype=torch.int32, device=x.device)
            ws = _lib.scratch(int(lib.wv_metrics_stoi_workspace_bytes(B, T, up, down, L, width)), x.device)
            _lib.check(lib.wv_metrics_stoi(x.data_ptr(), y.data_ptr(), B, T, _lib.ptr(kern), up, down, L, width, basis.data_ptr(), out.data_ptr(),
                                           frames.data_ptr(), None, None, ws.data_ptr(), ws.numel(), _lib.stream(x.device)), "wv_metrics_stoi")
            self.last_frames = frames
            short = None                                        # known on the device only: no trip to the host for a warning
        else:
            res = [S.stoi_numpy(x[b, 0].numpy(), y[b, 0].numpy(), int(sample_rate)) for b in range(B)]
            out = torch.tensor([r[0] for r in res], dtype=torch.float64)
            self.last_frames = torch.tensor([[r[1], r[2]] for r in res], dtype=torch.int32).reshape(B, 2)
            short = any(r[1] - 1 < S.N_SEG for r in res)
        if short:
            warnings.warn(S.SHORT_MESSAGE, RuntimeWarning)
        return out

    def mean(self, estimates: torch.Tensor, references: torch.Tensor, sample_rate: int = 16000) -> torch.Tensor:
        return self(estimates, references, sample_rate).mean()


def loudness_windows(arena: torch.Tensor, starts: torch.Tensor, lens: torch.Tensor, T: int, sample_rate: int,
                     want_filtered: bool = False):
    """wv_loudness on N windows of T samples of one flat float32 device arena -> (lufs [N] float64, sub [N, T // (fs / 10)] float64,
    filtered [N, T] float32 or None).  starts [N] int64 sample offsets, lens [N] int32 valid samples (the rest of a window counts as
    zeros and is not read), both on the arena's device."""
    from . import loudness as L
    lib = _lib.load()
    N, T, fs = int(starts.numel()), int(T), int(sample_rate)
    h = L.sub_block(fs)
    if T < L.BLOCK_SUBS * h:
        raise ValueError(f"loudness: {T} samples at {fs} Hz are fewer than one gating block of {L.BLOCK_SUBS} sub-blocks ({L.BLOCK_SUBS * h})")
    if not (arena.is_cuda and arena.dtype == torch.float32 and arena.is_contiguous() and starts.dtype == torch.int64 and lens.dtype == torch.int32
            and starts.device == arena.device and lens.device == arena.device and lens.numel() == N and starts.is_contiguous() and lens.is_contiguous()):
        raise ValueError("loudness_windows: a contiguous float32 device arena with int64 starts and int32 lens [N] on its device is required")
    table = L.device_table(fs, arena.device)
    lufs = torch.empty(N, dtype=torch.float64, device=arena.device)
    sub = torch.empty(N, T // h, dtype=torch.float64, device=arena.device)
    filtered = torch.empty(N, T, dtype=torch.float32, device=arena.device) if want_filtered else None
    ws = _lib.scratch(int(lib.wv_loudness_workspace_bytes(N, T, fs)), arena.device)
    _lib.check(lib.wv_loudness(arena.data_ptr(), starts.data_ptr(), lens.data_ptr(), N, T, fs, table.data_ptr(), lufs.data_ptr(), sub.data_ptr(),
                               _lib.ptr(filtered), ws.data_ptr(), ws.numel(), _lib.stream(arena.device)), "wv_loudness")
    return lufs, sub, filtered


class Loudness:
    """Gated loudness of every clip in LUFS per ITU-R BS.1770-4 (one channel): K-weighting, 400 ms blocks at 75 % overlap, the
    absolute gate at -70 LUFS and the relative gate 10 LU under the gated mean; loudness.MIN_LOUDNESS (-70.0) where nothing passes the
    absolute gate.  It is the level measure next to SI-SNR and STOI -- how much did embed() change a file's level -- and the gate of
    data.ClipPool.sample.  The constants and the algorithm are in waveverify_amd/loudness.py: a restatement of the published standard,
    parity with audiotools' `Meter` (what the reference's data loader measures with) stays unpinned.

        Loudness()(x, sample_rate=16000) -> [B] float64 on x's device,  x [B, 1, T], T >= 0.4 s, sample_rate % 10 == 0

    Device tensors go through csrc/wv_loudness.hip (one launch; the table cached per sample rate and device), CPU tensors through the
    float64 host route.  `.last_sub` holds the [B, T // (fs / 10)] sub-block energies."""

    def __init__(self):
        self.last_sub: Optional[torch.Tensor] = None

    def __call__(self, x: torch.Tensor, sample_rate: int = 16000) -> torch.Tensor:
        from . import loudness as L
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"x must be [B, 1, T], got {tuple(x.shape)}")
        B, _, T = x.shape
        h = L.sub_block(sample_rate)
        if T < L.BLOCK_SUBS * h:
            raise ValueError(f"loudness: {T} samples at {sample_rate} Hz are fewer than one gating block of {L.BLOCK_SUBS} sub-blocks ({L.BLOCK_SUBS * h})")
        x = _f32(x)
        if x.is_cuda:
            starts = torch.arange(B, dtype=torch.int64, device=x.device) * T
            lens = torch.full((B,), T, dtype=torch.int32, device=x.device)
            out, self.last_sub, _ = loudness_windows(x.reshape(-1), starts, lens, T, sample_rate)
            return out
        sub = L.sub_block_energies(L.k_filter(x[:, 0].numpy(), int(sample_rate)), int(sample_rate))
        self.last_sub = torch.from_numpy(sub)
        return torch.tensor([L.gate(s, int(sample_rate)) for s in sub], dtype=torch.float64)

    def mean(self, x: torch.Tensor, sample_rate: int = 16000) -> torch.Tensor:
        return self(x, sample_rate).mean()
