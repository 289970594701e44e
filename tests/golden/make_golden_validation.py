#!/usr/bin/env python3
"""Generate tests/golden/validation_metrics.npz by running the REFERENCE's own SISNR and BER classes (scripts/evaluate.py:146-229,
419-516; build container only), loaded the way make_golden_metrics.py loads that file.  SISNR takes audiotools' AudioSignal, which is
not installed: a stand-in with the two attributes it reads (`audio_data`, `device`) and the `to` it calls is passed in its place.
Only data is written: inputs, the reference's outputs.

SI-SNR cases (one clip each, so the reference's batch mean IS the per-clip value; signals live on a 2^-15 grid and are stored as
int16 steps, the estimate as its difference from the reference plus a DC step count, so the file stays small and every float32 input
is reproduced exactly): T in {1, 63, 64, 65, 400, 4097, 16000}; estimate = reference + noise at about 10, 30 and 60 dB; identical
signals; a silent reference; a large DC offset; and one batch of three for the mean.

Per-clip BER cases: B <= 4, W in {1, 8, 16}, partial masks, clips whose mask is all zero, exact ties.  The reference only returns the
scalar of a batch, so it is also run on every clip and on every (clip, bit) slice on its own: that is its own decision for that bit.
Every case is redrawn until, for each (clip, bit), the float64 margin |avg - thr| is at least (log2 T + 2) 2^-24 -- the bound of a
pairwise float32 sum of T terms -- or the bit is an exact tie (every live sample's probability is exactly 0.5 and thr = 0.5): the
reference's float32 answer is then unambiguous, whatever order it summed in.

Usage (from repo root, in the build container):  python tests/golden/make_golden_validation.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_metrics import _import_evaluate  # noqa: E402

GRID = 32768.0


class _Audio:
    """What SISNR.forward reads of an AudioSignal."""

    def __init__(self, audio_data):
        self.audio_data, self.device = audio_data, audio_data.device

    def to(self, device):
        return self


def main():
    import torch
    ev = _import_evaluate()
    rng = np.random.default_rng(20261)
    out = {}

    # ---------------------------------------------------------------- SI-SNR
    sisnr = ev.SISNR()

    def signals(ref_q, diff_q, dc):
        est = ((ref_q.astype(np.int64) + diff_q + dc[0]) / GRID).astype(np.float32)
        ref = ((ref_q.astype(np.int64) + dc[1]) / GRID).astype(np.float32)
        return est, ref

    def ref_value(est, ref):
        return float(sisnr(_Audio(torch.from_numpy(est).reshape(-1, 1, est.shape[-1])), _Audio(torch.from_numpy(ref).reshape(-1, 1, ref.shape[-1]))))

    n = 0

    def si_case(T, kind, level_db=None):
        nonlocal n
        ref_q = np.clip(np.rint(rng.standard_normal(T) * 0.2 * GRID), -32000, 32000).astype(np.int16)
        diff_q, dc = np.zeros(T, np.int16), np.zeros(2, np.int32)
        if kind == "noise":
            amp = 0.2 * 10.0 ** (-level_db / 20.0)
            diff_q = np.rint(rng.standard_normal(T) * amp * GRID).astype(np.int16)
        elif kind == "silent":
            diff_q, ref_q = ref_q.copy(), np.zeros(T, np.int16)          # estimate = a signal, reference = silence
        elif kind == "dc":
            diff_q = np.rint(rng.standard_normal(T) * 0.2 * 10.0 ** (-30 / 20.0) * GRID).astype(np.int16)
            dc[:] = (8 * 32768, 5 * 32768)                                # estimate rides on +8.0, reference on +5.0
        est, ref = signals(ref_q, diff_q, dc)
        out[f"si{n}_ref"], out[f"si{n}_diff"], out[f"si{n}_dc"] = ref_q, diff_q, dc
        out[f"si{n}_kind"] = np.array(kind)
        out[f"si{n}_out"] = np.float64(ref_value(est, ref))
        n += 1

    for T in (1, 63, 64, 65):
        si_case(T, "noise", 30)
    for T in (400, 4097):
        for db in (10, 30, 60):
            si_case(T, "noise", db)
        si_case(T, "identical")
        si_case(T, "silent")
        si_case(T, "dc")
    si_case(16000, "noise", 30)
    si_case(1, "identical")
    out["n_si"] = np.int64(n)
    batch = [i for i in range(n) if out[f"si{i}_ref"].shape[0] == 400][:3]
    pairs = [signals(out[f"si{i}_ref"], out[f"si{i}_diff"], out[f"si{i}_dc"]) for i in batch]
    out["si_batch_cases"] = np.array(batch, np.int64)
    out["si_batch_mean"] = np.float64(ref_value(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])))

    # ---------------------------------------------------------------- per-clip BER
    def margins_ok(logits, mask, thr):
        B, W, T = logits.shape
        p = 1.0 / (1.0 + np.exp(-logits.astype(np.float32).astype(np.float64)))
        m = np.ones((B, 1, T)) if mask is None else mask.astype(np.float64)
        cnt = np.broadcast_to(m.sum(axis=2), (B, W))
        avg = (p * m).sum(axis=2) / (cnt + 1e-8) if mask is not None else p.mean(axis=2)
        tie = np.array([[thr == 0.5 and bool(np.all(p[b, w][m[b, 0] != 0] == 0.5)) for w in range(W)] for b in range(B)])
        bound = (np.log2(T) + 2) * 2.0 ** -24
        return bool(np.all((np.abs(avg - thr) >= bound) | tie | (cnt == 0)))

    ber = ev.BER

    def run_ber(logits, bits, mask, thr):
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
        return float(ber(threshold=thr)(t(logits), t(bits), t(mask)))

    nb = 0

    def ber_case(draw, thr=0.5):
        nonlocal nb
        assert thr > 0
        for attempt in range(1000):
            logits, bits, mask = draw()
            logits = logits.astype(np.float32)
            if margins_ok(logits, mask, thr):
                break
        else:
            raise RuntimeError("no draw with unambiguous margins")
        B, W, T = logits.shape
        valid = np.ones((B, W), bool) if mask is None else np.broadcast_to(mask.sum(axis=2) > 0, (B, W)).copy()
        wrong = np.zeros((B, W), np.int32)
        clip = np.zeros(B, np.float64)
        for b in range(B):
            mb = None if mask is None else mask[b:b + 1]
            clip[b] = run_ber(logits[b:b + 1], bits[b:b + 1], mb, thr)
            for w in range(W):
                wrong[b, w] = int(round(run_ber(logits[b:b + 1, w:w + 1], bits[b:b + 1, w:w + 1], mb, thr)))
        # the reference's decoded bit: where the bit is valid, the stored bit flipped when the reference counts an error; where it is
        # not, avg = 0 / (0 + eps) = 0 < thr decodes 0
        decoded = np.where(valid, bits.astype(np.int32) ^ wrong, 0).astype(np.int32)
        out[f"ber{nb}_logits"], out[f"ber{nb}_bits"], out[f"ber{nb}_thr"] = logits, bits.astype(np.float32), np.float32(thr)
        if mask is not None:
            out[f"ber{nb}_mask"] = mask.astype(np.float32)
        out[f"ber{nb}_out"] = np.float64(run_ber(logits, bits, mask, thr))
        out[f"ber{nb}_clip"], out[f"ber{nb}_wrong"], out[f"ber{nb}_decoded"], out[f"ber{nb}_valid"] = clip, wrong, decoded, valid
        assert abs(out[f"ber{nb}_out"] - (wrong.sum() / max(valid.sum(), 1))) < 1e-6
        nb += 1

    def drawer(B, W, T, mask_kind, scale=0.3):
        def draw():
            logits = rng.standard_normal((B, W, T)) * scale
            bits = rng.integers(0, 2, (B, W)).astype(np.float32)
            if mask_kind == "none":
                mask = None
            elif mask_kind == "partial":
                mask = (rng.random((B, 1, T)) < 0.5).astype(np.float32)
            elif mask_kind == "dead_clip":
                mask = (rng.random((B, 1, T)) < 0.6).astype(np.float32)
                mask[B // 2] = 0.0
            elif mask_kind == "block":
                mask = np.zeros((B, 1, T), np.float32)
                mask[:, :, T // 5: T // 2] = 1.0
            return logits, bits, mask
        return draw

    ber_case(drawer(1, 1, 1, "none", 1.0))
    ber_case(drawer(2, 8, 63, "partial"))
    ber_case(drawer(3, 16, 65, "dead_clip"))
    ber_case(drawer(4, 16, 130, "partial"), thr=0.45)
    ber_case(drawer(4, 1, 400, "none"))
    ber_case(drawer(3, 8, 400, "block", 2.0))
    ber_case(drawer(2, 16, 40, "dead_clip"))

    def ties(masked):
        def draw():
            B, W, T = 2, 16, 40
            logits = np.zeros((B, W, T))
            bits = rng.integers(0, 2, (B, W)).astype(np.float32)
            mask = None
            if masked:
                mask = (rng.random((B, 1, T)) < 0.5).astype(np.float32)
                logits = np.where(mask != 0, 0.0, rng.standard_normal((B, W, T)))   # only the live samples sit at p = 0.5
            return logits, bits, mask
        return draw
    ber_case(ties(False))
    ber_case(ties(True))
    out["n_ber"] = np.int64(nb)

    path = os.path.join(HERE, "validation_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {n} SI-SNR cases, {nb} BER cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
