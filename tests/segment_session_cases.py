"""Live segment sessions: the reference arithmetic and the case lists of tests/test_segment_session_cpu.py and
tests/test_gpu_segment_session.py (a plain module, fixed seeds, importable without a GPU).

What a streaming tracker (localize.SegmentTracker, wv_segment_track) must give is what the file route gives on the whole array of frame sums:
localize.segments_from_counts for the frames, localized_cases.reduce_ref for count and prob.  reduce_ref adds with numpy's pairwise sum, the
trackers and wv_frames_reduce add frame by frame in ascending order; the two are the same number, bit for bit, exactly when no add rounds.  So
the patterns compared with reduce_ref hold QUANTIZED sums (multiples of 2^-12 no larger than the hop: at most 200 frames of at most 2^9 need
9 + 8 + 12 = 29 bits, far inside float64's 53 and each value inside float32's 24), where every order of addition is exact.  The order itself is
pinned separately by ascending_ref on float32 sums spread over twelve decades (float32 values of like size add exactly in float64, so only
such a spread makes an add round): one float64 add per frame, lo first."""
from __future__ import annotations

import zlib

import numpy as np

from localized_cases import reduce_ref
from waveverify_amd.localize import segments_from_counts

Q = 2.0 ** -12

NBS = (1, 16)
GAPS = (1, 2, 5)
LENS = (1, 5)
CHUNKINGS = ("whole", "frames", "random")


def seed_of(*what):
    return zlib.crc32(repr(what).encode())


# ---- references ---------------------------------------------------------------------------------------------------------------------------
def valid_of(n_frames, hop, last_valid):
    v = np.full(n_frames, hop, np.int64)
    if n_frames:
        v[-1] = last_valid
    return v


def whole_ref(fsum, hop, last_valid, min_on, min_gap_frames, min_len_frames, eps=1e-8):
    """fsum [S, nb + 1, Fr] -> per stream [(lo, hi, count, prob float32 [nb])]: segments_from_counts, then reduce_ref."""
    S, nb1, Fr = fsum.shape
    out = []
    for s in range(S):
        runs = segments_from_counts(fsum[s, nb1 - 1], valid_of(Fr, hop, last_valid), min_on, min_gap_frames, min_len_frames)
        prob, count, _ = reduce_ref(fsum, [(s, lo, hi) for lo, hi in runs], eps)
        out.append([(lo, hi, float(count[i]), prob[i]) for i, (lo, hi) in enumerate(runs)])
    return out


def ascending_ref(fsum, s, lo, hi, eps=1e-8):
    """(count, prob) of frames [lo, hi) of stream s, one float64 add per frame in ascending order (np.cumsum adds that way)."""
    nb = fsum.shape[1] - 1
    tot = np.cumsum(np.asarray(fsum[s, :, lo:hi], np.float64), axis=1)[:, -1]
    N = tot[nb]
    if not N > 0:
        return float(N), np.zeros(nb, np.float32)
    return float(N), (tot[:nb] / np.float64(np.float32(N) + np.float32(eps))).astype(np.float32)


def same_events(got, want):
    """None, or the first difference between two per-stream event lists, bit for bit in frames, count and prob."""
    if len(got) != len(want):
        return f"{len(got)} streams against {len(want)}"
    for s, (g, w) in enumerate(zip(got, want)):
        if [(a[0], a[1]) for a in g] != [(a[0], a[1]) for a in w]:
            return f"stream {s}: frames {[(a[0], a[1]) for a in g]} against {[(a[0], a[1]) for a in w]}"
        for a, b in zip(g, w):
            if np.float64(a[2]).tobytes() != np.float64(b[2]).tobytes():
                return f"stream {s} segment {a[:2]}: count {a[2]!r} against {b[2]!r}"
            if np.asarray(a[3], np.float32).tobytes() != np.asarray(b[3], np.float32).tobytes():
                return f"stream {s} segment {a[:2]}: prob {a[3]} against {b[3]}"
    return None


# ---- chunkings ----------------------------------------------------------------------------------------------------------------------------
def chunks_of(n_frames, kind, rng, partial=False):
    """-> [(f_lo, f_hi)] covering [0, n_frames) in order; "random" has empty ticks too.  The last tick is the final one; with a partial last
    frame it holds that frame (a session meets a partial frame only in flush), else it may be empty."""
    if kind == "whole":
        return [(0, n_frames)]
    if kind == "frames":
        return [(f, f + 1) for f in range(n_frames)] or [(0, 0)]
    out, f = [], 0
    body = n_frames - 1 if partial and n_frames else n_frames
    while f < body:
        m = int(rng.integers(0, 8))
        m = 0 if m > 5 else m                                          # 0 three times in eight
        out.append((f, min(body, f + m)))
        f = min(body, f + m)
    if body < n_frames:
        out.append((body, n_frames))
    elif int(rng.integers(0, 2)) or not out:
        out.append((n_frames, n_frames))                               # a final tick without frames
    return out


def run_tracker(tracker, fsum, chunks, last_valid, poll_each=False):
    """Feed fsum [S, nb + 1, Fr] to a tracker tick by tick -> per stream the events in the order they came out."""
    out = [[] for _ in range(fsum.shape[0])]
    for i, (lo, hi) in enumerate(chunks):
        final = i == len(chunks) - 1
        ends_here = final and hi == fsum.shape[2] and hi > lo
        tracker.advance(fsum, lo, hi, last_valid if ends_here else tracker.hop, final)
        if poll_each or final:
            for s, evs in enumerate(tracker.poll()):
                out[s] += evs
    return out


# ---- patterns -----------------------------------------------------------------------------------------------------------------------------
def sums_for(count, nb, rng, quantized=True):
    """count [Fr] -> fsum [nb + 1, Fr] float32: bit rows drawn in [0, count] (a sum of sigmoids over `count` samples).  quantized: multiples
    of Q; else count * 10^-12u, twelve decades (sigmoids of strongly negative logits), where float64 adds of float32 values do round."""
    count = np.asarray(count, np.float64)
    u = rng.random((nb, len(count)))
    rows = np.floor(u * count / Q) * Q if quantized else count * 10.0 ** (-12.0 * u)
    return np.concatenate([rows, count[None]]).astype(np.float32)


def random_counts(rng, hop, min_on, n_frames, last_valid):
    """Runs of on and off frames of random lengths 1 .. 7, on counts in [ceil(min_on * hop), hop], off counts below; now and then a count exactly
    on the rule's edge.  The last frame holds at most last_valid samples."""
    edge = min_on * hop
    on_lo = int(np.ceil(edge))
    count, on = [], bool(rng.integers(0, 2))
    while len(count) < n_frames:
        for _ in range(int(rng.integers(1, 8))):
            if on:
                c = on_lo if rng.integers(0, 4) == 0 else int(rng.integers(on_lo, hop + 1))
            else:
                c = int(rng.integers(0, on_lo)) if on_lo > 0 else 0
            count.append(c)
        on = not on
    count = count[:n_frames]
    count[-1] = min(count[-1], last_valid) if rng.integers(0, 2) else int(rng.integers(0, last_valid + 1))
    return count


def random_case(i):
    """Seeded case i of the CPU fuzz -> (nb, min_gap_frames, min_len_frames, hop, min_on, last_valid, fsum [1, nb + 1, Fr])."""
    rng = np.random.default_rng(seed_of("segment-fuzz", i))
    nb, G, ml = NBS[i % 2], GAPS[(i // 2) % 3], LENS[(i // 6) % 2]
    hop = int(rng.choice([10, 32, 320]))
    min_on = float(rng.choice([0.5, 0.25, 0.7]))
    n_frames = int(rng.integers(1, 60))
    last_valid = hop if (i // 12) % 2 == 0 else int(rng.integers(1, hop))
    count = random_counts(rng, hop, min_on, n_frames, last_valid)
    return nb, G, ml, hop, min_on, last_valid, sums_for(count, nb, rng)[None]


# the GPU tracker test's named patterns, built for given (hop, min_on, G, min_len): on = a full frame, off = 0 gated samples
def named_patterns(hop, min_on, G, min_len):
    """-> [(name, count list, last_valid, anchor)]; every pattern is at most 200 frames.  anchor: the end of the recording the pattern is
    about ("start" / "end"), so padding goes to the other one."""
    on, off, L = hop, 0, max(min_len, 1)
    edge = int(min_on * hop) if float(int(min_on * hop)) == min_on * hop else None
    lv = max(2, hop // 3)                                               # a partial last frame
    lv_on = int(np.ceil(min_on * lv))
    pats = [
        ("a run from frame 0", [on] * (L + 2) + [off] * (G + 1), hop, "start"),
        ("a run open at final", [off] * 3 + [on] * (L + 1), hop, "end"),
        ("a gap of G - 1 merges", [off] + [on] * L + [off] * (G - 1) + [on] * L + [off] * G, hop, "end"),
        ("a gap of G splits", [off] + [on] * L + [off] * G + [on] * L + [off] * G, hop, "end"),
        ("a short run merges into a long one", [off] * 2 + [on] + [off] * (G - 1) + [on] * (L + 3) + [off] * (G + 2), hop, "end"),
        ("a short run alone is dropped", [off] * 2 + [on] * max(L - 1, 0) + [off] * (G + 2) + [on] * L, hop, "end"),
        ("a partial last frame on", [off] * 2 + [on] * L + [lv_on], lv, "end"),
        ("a partial last frame just off", [off] * 2 + [on] * L + [max(lv_on - 1, 0)], lv, "end"),
        ("a partial last frame that opens a run", [off] * (G + 1) + [lv], lv, "end"),
        ("twelve runs", ([on] * L + [off] * G) * 12, hop, "end"),
        ("empty", [off] * 7, hop, "end"),
        ("all on", [on] * 40, hop, "end"),
    ]
    if edge is not None:
        pats.append(("a count exactly min_on * valid", [off] * 2 + [edge] * (L + 1) + [edge - 1] * G + [edge] * L, hop, "end"))
    assert all(len(c) <= 200 for _, c, _, _ in pats)
    return pats


def stream_patterns(S, hop, min_on, G, min_len, nb, salt=0):
    """A different named pattern per stream, padded with off frames to one length at the end it is not about -> (names, fsum [S, nb + 1, Fr] float32, last_valid).  The streams of one batch share last_valid, so the batch takes its
    patterns from one of the two groups (full last frame, partial last frame) in turn."""
    pats = named_patterns(hop, min_on, G, min_len)
    full = [p for p in pats if p[2] == hop]
    part = [p for p in pats if p[2] != hop]
    group = part if salt % 2 else full
    chosen = [group[(salt // 2 + s) % len(group)] for s in range(S)]
    Fr = max(len(c) for _, c, _, _ in chosen)
    pad = lambda c, anchor: list(c) + [0] * (Fr - len(c)) if anchor == "start" else [0] * (Fr - len(c)) + list(c)
    rng = np.random.default_rng(seed_of("stream-patterns", S, hop, G, min_len, nb, salt))
    fsum = np.stack([sums_for(pad(c, a), nb, rng) for _, c, _, a in chosen])
    return [n for n, _, _, _ in chosen], fsum, chosen[0][2]


# ---- the locator-driven recording of the GPU tests (test_segment_session_cpu.test_locator_recording_margin_on_the_oracle) ---------------------
# Randomly initialised nets: WaveVerify.random_init(LOC_SEED).  Such a locator fires on about 55 % of the samples of a noisy stretch at this
# threshold and on about 30 % of a silent one, so silences cut the recording into segments.  The three values were chosen on the float64 oracle
# so that no frame's count comes near min_on * valid (the margin test states the figures).
LOC_SEED = 3
LOC_THRESHOLD = 0.93
LOC_MIN_ON = 0.43
LOC_T = 16001
LOC_EXPECTED_FRAMES = [[(0, 10), (17, 30), (38, 51)], [(7, 40)]]
LOC_SILENCES = (((3200, 5440), (9600, 12000)), ((0, 2240), (8000, 8320), (12800, 16001)))


def locator_recording():
    """-> x [2, 1, LOC_T] float32: synthetic clips with silent stretches (a 1-frame silence in stream 1 is bridged; its end is silent)."""
    from waveverify_amd.init import synthetic_clips
    x = synthetic_clips(len(LOC_SILENCES), LOC_T, seed=11)[0].copy()
    for s, cuts in enumerate(LOC_SILENCES):
        for a, b in cuts:
            x[s, 0, a:b] = 0.0
    return x
