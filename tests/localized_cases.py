"""Localized detection: the float64 restatement the GPU tests compare against, and the CPU tests' case lists (a plain module).

frame_sums_ref is what head_frames_kernel / head16_frames_kernel promise: per detector frame the sum of sigmoid(logit) over the gated
samples, and their number.  reduce_ref is wv_frames_reduce: frames of a segment added in f64, prob = S / (float32(N) + float32(eps)) with
the quotient rounded once to float32, 0 where N == 0.  With one whole-clip segment the two are the reference's masked BER decode
(scripts/evaluate.py:442-516), which tests/golden/metrics.npz records."""
import numpy as np

from validation_cases import MET_BER


def sigmoid64(x):
    with np.errstate(over="ignore"):                              # exp(+huge) = inf -> probability 0, as intended
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def gated(gate, thr, B, T):
    """[B, T] bool: gate > thr (strict), everything without a gate."""
    if gate is None:
        return np.ones((B, T), bool)
    return np.asarray(gate).reshape(B, T) > thr


def frame_sums_from_probs(p, gate, thr, hop, T):
    """p [B, nb, >= T] float64 probabilities -> fsum [B, nb + 1, Fr] float64."""
    p = np.asarray(p, np.float64)[:, :, :T]
    B, nb, _ = p.shape
    Fr = -(-T // hop)
    on = gated(gate, thr, B, T)
    pad = Fr * hop - T
    pm = np.pad(p * on[:, None, :], ((0, 0), (0, 0), (0, pad)))
    out = np.zeros((B, nb + 1, Fr), np.float64)
    out[:, :nb] = pm.reshape(B, nb, Fr, hop).sum(-1)
    out[:, nb] = np.pad(on, ((0, 0), (0, pad))).reshape(B, Fr, hop).sum(-1)
    return out


def frame_sums_ref(logits64, gate, thr, hop, T):
    return frame_sums_from_probs(sigmoid64(logits64), gate, thr, hop, T)


def reduce_ref(fsum, segs, eps=1e-8):
    """-> (prob [n, nb] float32, count [n] float64, exact float64 quotient [n, nb])."""
    fsum = np.asarray(fsum, np.float64)
    nb = fsum.shape[1] - 1
    prob, count, exact = np.zeros((len(segs), nb), np.float32), np.zeros(len(segs), np.float64), np.zeros((len(segs), nb), np.float64)
    for i, (b, lo, hi) in enumerate(segs):
        S, N = fsum[b, :nb, lo:hi].sum(-1), fsum[b, nb, lo:hi].sum()
        count[i] = N
        if N > 0:
            prob[i] = (S / np.float64(np.float32(N) + np.float32(eps))).astype(np.float32)
            exact[i] = S / (N + eps)
    return prob, count, exact


def decide(prob, thr=0.5):
    return (np.asarray(prob, np.float32) >= np.float32(thr)).astype(np.int32)


# the reference's own BER records that carry a mask (masks there are 0 / 1: the gate is mask > 0.5)
MASKED_BER = [c for c in MET_BER if c["mask"] is not None]

# segments_from_counts on hand-built counts, hop 10: (name, count, valid, kwargs, expected)
_V = [10] * 12
SEGMENT_CASES = [
    ("empty", [0] * 12, _V, {}, []),
    ("all on", [10] * 12, _V, {}, [(0, 12)]),
    ("a short blip is dropped", [0, 0, 10, 10, 10, 10, 0, 0, 0, 0, 0, 0], _V, {}, []),
    ("two runs merged across a 1-frame gap", [10, 10, 10, 0, 10, 10, 10, 0, 0, 0, 0, 0], _V, {}, [(0, 7)]),
    ("two runs kept apart across a 2-frame gap", [10, 10, 10, 10, 10, 0, 0, 10, 10, 10, 10, 10], _V, {}, [(0, 5), (7, 12)]),
    ("a 2-frame gap, the second run too short", [10, 10, 10, 10, 10, 0, 0, 10, 10, 10, 10, 0], _V, {}, [(0, 5)]),
    ("a partial last frame is on by its own length", [0] * 7 + [10, 10, 10, 10, 2], [10] * 11 + [3], {}, [(7, 12)]),
    ("a partial last frame below min_on", [0] * 6 + [10, 10, 10, 10, 10, 1], [10] * 11 + [3], {}, [(6, 11)]),
    ("a run touching both ends", [5] * 12, _V, {}, [(0, 12)]),
    ("just below min_on", [4] * 12, _V, {}, []),
    ("min_len 1 keeps the blip", [0, 0, 10, 0, 0, 0, 0, 0, 0, 0, 0, 0], _V, {"min_len_frames": 1}, [(2, 3)]),
    ("min_gap 1 merges nothing", [10, 10, 10, 0, 10, 10, 10, 0, 0, 0, 0, 0], _V, {"min_gap_frames": 1, "min_len_frames": 3}, [(0, 3), (4, 7)]),
]
