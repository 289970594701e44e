"""Localized detection without a GPU: segments_from_counts on hand-built counts, the float64 restatement of the frames kernels and the
segment reduce (tests/localized_cases.py) against the reference's own masked BER records, and the frame-unit scatter descriptors of the
windowed route."""
import numpy as np
import pytest
import torch

from localized_cases import MASKED_BER, SEGMENT_CASES, decide, frame_sums_ref, reduce_ref
from waveverify_amd import localize, metrics, window
from waveverify_amd.config import default_config


@pytest.mark.parametrize("name,count,valid,kw,want", SEGMENT_CASES, ids=[c[0] for c in SEGMENT_CASES])
def test_segments_from_counts(name, count, valid, kw, want):
    assert localize.segments_from_counts(count, valid, **kw) == want


def test_segments_from_counts_refuses_mismatched_rows():
    with pytest.raises(ValueError):
        localize.segments_from_counts([1, 2], [1])


def test_gate_threshold_and_frame_valid():
    assert localize.gate_threshold(0.5) == 0.0
    assert localize.gate_threshold(0.9) == pytest.approx(np.log(9.0), rel=1e-15)
    for p in (0.0, 1.0, -1.0):
        with pytest.raises(ValueError):
            localize.gate_threshold(p)
    assert localize.frame_valid(641, 320).tolist() == [320, 320, 1]
    assert localize.frame_valid(640, 320).tolist() == [320, 320]


@pytest.mark.parametrize("hop", [1, 7, 64])
@pytest.mark.parametrize("case", MASKED_BER, ids=[c["name"] for c in MASKED_BER])
def test_whole_clip_segment_is_the_references_masked_ber(case, hop):
    """One segment {b, 0, Fr} per clip: the decoded bits equal those of metrics.ber_per_clip (itself held to these records), and the
    BER they give is the reference's scalar -- the all-invalid clips and the all-zero-logits case (a tie at the threshold) included."""
    lg, mask, thr = case["logits"], case["mask"], case["thr"]
    B, W, T = lg.shape
    assert set(np.unique(mask)) <= {0.0, 1.0}
    Fr = -(-T // hop)
    fsum = frame_sums_ref(lg.astype(np.float64), mask[:, 0], 0.5, hop, T)
    assert np.array_equal(fsum[:, W].sum(-1), mask[:, 0].sum(-1))
    prob, count, _ = reduce_ref(fsum, [(b, 0, Fr) for b in range(B)])
    bits = decide(prob, thr)
    errors, valid, avg = metrics.ber_per_clip(torch.from_numpy(lg), torch.from_numpy(case["bits"]), torch.from_numpy(mask), threshold=thr)
    live = count > 0
    assert np.array_equal(live * W, valid.numpy())
    assert np.array_equal(bits[live], (avg.numpy() >= np.float32(thr)).astype(np.int32)[live])
    assert (prob[~live] == 0).all() and (bits[~live] == 0).all()
    wrong = int(((bits != case["bits"].astype(np.int32)) & live[:, None]).sum())
    total = int(live.sum()) * W
    assert abs((wrong / total if total else 0.0) - case["out"]) < 1e-7


@pytest.mark.parametrize("extra", [0, 1, 319, 320, 321, 3 * 320 + 7])
def test_frame_scatter_descriptors_tile_every_clip_once(extra):
    """For window.plan's outputs on the default detector -- one window, two windows, several, ragged tails, T % hop != 0 -- the kept
    frame ranges of the frame-unit descriptors tile [0, Fr) of every clip exactly once, inside each window's own frame count."""
    cfg = default_config("detector")
    hop, H = cfg.hop_length, window.halo(cfg)
    L = H + 2 * hop
    lengths = [L - extra if extra < L else L, L + extra, 2 * L + extra, 900, L + 3 * hop + 7, 5 * L - 1]
    frames = [-(-T // hop) for T in lengths]
    fbases = np.concatenate([[0], np.cumsum(frames)[:-1]]).tolist()
    C_ = cfg.head_bits + 1
    hits = [np.zeros(f, int) for f in frames]
    for wins in window.plan(lengths, L, cfg, max_windows=4):
        FrW = -(-wins[0].length // hop)
        for w, (off, stride, lo, hi) in zip(wins, window.frame_scatter_desc(wins, fbases, frames, hop, C_)):
            assert stride == frames[w.clip] and 0 <= lo < hi <= FrW
            f0 = off - C_ * fbases[w.clip]
            assert f0 * hop == w.start
            hits[w.clip][f0 + lo: f0 + hi] += 1
            assert (f0 + lo) * hop == w.keep_lo and min((f0 + hi) * hop, lengths[w.clip]) == w.keep_hi
    for h in hits:
        assert (h == 1).all()


def test_frame_scatter_descriptors_refuse_an_edge_off_the_hop():
    with pytest.raises(ValueError):
        window.frame_scatter_desc([window.Window(0, 0, 700, 5, 700)], [0], [3], 320, 17)
