"""Localized detection, host side (NOT in the reference's package API; its evaluation decodes this way, scripts/evaluate.py:442-516 with
the mask of model/watermarking.py:793-801): which frames count as watermarked, and how runs of them become segments.

The kernels (head_frames_kernel, head16_frames_kernel, wv_frames_reduce) give per FRAME the gated sigmoid sums and the gated sample
count; everything here is pure Python / numpy on those small arrays, so it runs without a GPU."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .watermark_id import WatermarkID


@dataclass(frozen=True)
class Segment:
    start_s: float                      # first sample of the segment, in seconds
    end_s: float                        # one past its last sample, in seconds
    watermark: WatermarkID              # decoded over the segment's gated samples only
    confidence: float                   # mean of the per-bit masked mean probabilities, as detect()'s confidence is
    coverage: float                     # gated samples / samples of the segment
    prob: Optional[np.ndarray] = None   # [nbits] float32, the masked mean probability of every bit
    frames: Tuple[int, int] = (0, 0)    # [f_lo, f_hi) in detector frames


def gate_threshold(p: float) -> float:
    """The locator-LOGIT threshold equivalent to sigmoid(logit) > p, in double: log(p / (1 - p))."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"threshold must lie strictly between 0 and 1, got {p}")
    return math.log(p / (1.0 - p))


def frame_valid(T: int, hop: int) -> np.ndarray:
    """Samples per frame of a T-sample clip: hop everywhere but the (possibly partial) last frame."""
    Fr = -(-int(T) // hop)
    v = np.full(Fr, hop, np.int64)
    v[-1] = int(T) - (Fr - 1) * hop
    return v


def segments_from_counts(count: Sequence[float], valid: Sequence[float], min_on: float = 0.5, min_gap_frames: int = 2,
                         min_len_frames: int = 5) -> List[Tuple[int, int]]:
    """Runs [f_lo, f_hi) of watermarked frames.  A frame is on when count / valid >= min_on (count = its gated samples, valid = its
    samples); gaps SHORTER than min_gap_frames are merged first, then runs shorter than min_len_frames are dropped.  With the default
    min_gap_frames = 2 two segments never touch the same frame or adjacent ones; min_len_frames = 5 is 100 ms at the default hop."""
    count, valid = np.asarray(count, np.float64).reshape(-1), np.asarray(valid, np.float64).reshape(-1)
    if count.shape != valid.shape:
        raise ValueError("count and valid need one entry per frame each")
    on = (valid > 0) & (count >= min_on * valid)
    runs: List[List[int]] = []
    f, n = 0, len(on)
    while f < n:
        if not on[f]:
            f += 1
            continue
        g = f
        while g < n and on[g]:
            g += 1
        if runs and f - runs[-1][1] < min_gap_frames:
            runs[-1][1] = g
        else:
            runs.append([f, g])
        f = g
    return [(lo, hi) for lo, hi in runs if hi - lo >= min_len_frames]
