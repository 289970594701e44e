"""Live segment sessions without a GPU: the streaming tracker's host twin against the file route's arithmetic, the session's state machine
on the float64 oracle of small nets, the margin that lets the GPU's locator-driven recording have one right answer, and the new exports.

The references are segment_session_cases.whole_ref (localize.segments_from_counts + localized_cases.reduce_ref on the whole array) and
ascending_ref; why the bit-for-bit comparison with reduce_ref uses quantized sums is said there."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import segment_session_cases as SC
import window_cases as W
from localized_cases import SEGMENT_CASES, frame_sums_ref
from waveverify_amd.localize import BankSegmentTracker, Segment, SegmentTracker, gate_threshold
from waveverify_amd.session import SegmentStreamBank, SegmentStreamSession, cut_rows, numpy_advance, segment_halo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tracker(fsum, hop, min_on, G, ml, dtype=np.float32):
    return SegmentTracker(fsum.shape[0], fsum.shape[1] - 1, hop, min_on, G, ml, dtype=dtype)


def _all_chunkings(fsum, hop, last_valid, min_on, G, ml, what):
    want = SC.whole_ref(fsum, hop, last_valid, min_on, G, ml)
    for kind in SC.CHUNKINGS:
        rng = np.random.default_rng(SC.seed_of("chunks", what, kind))
        for poll_each in (False, True):
            got = SC.run_tracker(_tracker(fsum, hop, min_on, G, ml), fsum, SC.chunks_of(fsum.shape[2], kind, rng, last_valid < hop), last_valid, poll_each)
            diff = SC.same_events(got, want)
            assert diff is None, (what, kind, poll_each, diff)
    return want


# ---- 1. the host twin against segments_from_counts + reduce_ref -------------------------------------------------------------------------
@pytest.mark.parametrize("nb", SC.NBS)
def test_tracker_equals_the_file_route_on_the_hand_built_cases(nb):
    for name, count, valid, kw, expected in SEGMENT_CASES:
        hop, last_valid = valid[0], valid[-1]
        assert list(valid[:-1]) == [hop] * (len(valid) - 1)
        rng = np.random.default_rng(SC.seed_of("hand", name, nb))
        fsum = SC.sums_for(count, nb, rng)[None]
        G, ml = kw.get("min_gap_frames", 2), kw.get("min_len_frames", 5)
        want = _all_chunkings(fsum, hop, last_valid, 0.5, G, ml, (name, nb))
        assert [(a[0], a[1]) for a in want[0]] == expected, name
        for G2 in SC.GAPS:                                                  # the same counts under every gap and length rule
            for ml2 in SC.LENS:
                _all_chunkings(fsum, hop, last_valid, 0.5, G2, ml2, (name, nb, G2, ml2))


def test_tracker_equals_the_file_route_on_1000_random_patterns():
    seen = set()
    n_seg = 0
    for i in range(1000):
        nb, G, ml, hop, min_on, last_valid, fsum = SC.random_case(i)
        want = _all_chunkings(fsum, hop, last_valid, min_on, G, ml, ("fuzz", i))
        seen.add((nb, G, ml, last_valid < hop))
        n_seg += len(want[0])
    assert seen == {(nb, G, ml, p) for nb in SC.NBS for G in SC.GAPS for ml in SC.LENS for p in (False, True)}
    assert n_seg > 1000                                                      # the patterns do hold segments


def test_tracker_adds_frame_by_frame_in_ascending_order():
    """Float32 sums over twelve decades, where the order of the float64 adds shows in the last bits: the tracker's count and prob are those of one
    ascending pass over [lo, hi), gap frames included, in every chunking."""
    differs = 0
    for i in range(200):
        nb, G, ml, hop, min_on, last_valid, q = SC.random_case(i)
        rng = np.random.default_rng(SC.seed_of("order", i))
        fsum = SC.sums_for(q[0, nb], nb, rng, quantized=False)[None]
        for kind in SC.CHUNKINGS:
            got = SC.run_tracker(_tracker(fsum, hop, min_on, G, ml), fsum,
                                 SC.chunks_of(fsum.shape[2], kind, np.random.default_rng(SC.seed_of("order-chunks", i, kind)), last_valid < hop), last_valid)
            want = [[(lo, hi) + SC.ascending_ref(fsum, 0, lo, hi) for lo, hi, _, _ in SC.whole_ref(fsum, hop, last_valid, min_on, G, ml)[0]]]
            diff = SC.same_events(got, want)
            assert diff is None, (i, kind, diff)
        for lo, hi, _, _ in want[0]:
            back = np.cumsum(np.asarray(fsum[0, :, lo:hi], np.float64)[:, ::-1], axis=1)[:, -1]
            differs += int((back != np.cumsum(np.asarray(fsum[0, :, lo:hi], np.float64), axis=1)[:, -1]).any())
    assert differs > 20                                                      # the data can tell one order from another


def test_tracker_open_runs_and_lifecycle():
    hop, nb = 10, 16
    rng = np.random.default_rng(5)
    fsum = SC.sums_for([0, 10, 10, 10, 0, 10, 10, 0, 0, 0], nb, rng)[None]
    t = SegmentTracker(1, nb, hop, 0.5, 2, 5)
    assert t.open_runs() == [None] and t.poll() == [[]]
    t.advance(fsum, 0, 2)
    lo, hi, cnt, prob = t.open_runs()[0]                                     # an opening shows at once
    assert (lo, hi, cnt) == (1, 2, 10.0) and prob.dtype == np.float32
    t.advance(fsum, 2, 8)
    assert t.open_runs()[0][:3] == (1, 7, 50.0) and t.poll() == [[]]        # the gap frame 4 is inside, the trailing off frame 7 is not
    t.advance(fsum, 8, 9)                                                    # the second off frame closes it: known min_gap_frames frames late
    assert t.open_runs() == [None]
    (ev,), = t.poll()
    assert ev[:3] == (1, 7, 50.0) and t.poll() == [[]]
    t.advance(fsum, 9, 10, final=True)
    with pytest.raises(RuntimeError, match="reset"):
        t.advance(fsum, 0, 0)
    t.reset()
    assert t.frames_seen == 0 and t.open_runs() == [None]
    with pytest.raises(ValueError):
        t.advance(np.zeros((2, nb + 1, 3), np.float32))


# ---- 2. the session's state machine on the float64 oracle of small nets -----------------------------------------------------------------
def _pushes(hop, T):
    base = [1, hop - 1, hop, 3 * hop + 7, 0]
    out, k = [], 0
    while sum(out) < T:
        out.append(min(base[k % len(base)], T - sum(out)))
        k += 1
    return out + [0]


@pytest.mark.parametrize("det_id,loc_id,gated", [("x1.detector", "x3.locator", False), ("x7.detector", "x3.locator", False),
                                                 ("x1.detector", "x3.locator", True)])
def test_session_state_machine_on_the_oracle(det_id, loc_id, gated):
    cases = {c[0]: c for c in W.net_cases()}
    dcfg, _, dnet = W.oracle_net(cases[det_id])
    lcfg, _, lnet = W.oracle_net(cases[loc_id])
    hop, nb, H = dcfg.hop_length, dcfg.head_bits, segment_halo(dcfg, lcfg)
    assert H % hop == 0 and hop % lcfg.hop_length == 0
    S, T = 2, 40 * hop + 5
    x = np.concatenate([W.clip_data(cases[det_id], T, s)[0] for s in range(S)])                  # [S, 1, T]
    env = np.ones(T, np.float32)
    env[7 * hop: 13 * hop] = 0.0
    env[22 * hop + 3: 29 * hop] = 0.0
    x[1] *= env
    dlog = W.oracle_forward(dcfg, dnet, x)
    if gated:
        gate = np.zeros((S, T), np.float32)
        gate[0, 3 * hop + 5: 17 * hop] = 1.0
        gate[0, 20 * hop: 21 * hop + hop // 2] = 1.0                                                # exactly min_on of frame 21
        gate[1, 30 * hop:] = 1.0
        gsrc, thr, min_on = gate, 0.5, 0.5
    else:
        llog = W.oracle_forward(lcfg, lnet, x)[:, 0]
        srt = np.sort(llog[0])
        thr = float(0.5 * (srt[T // 2 - 1] + srt[T // 2]))                                         # the random locator fires on half of stream 0
        p = 1.0 / (1.0 + np.exp(-thr))
        assert abs(gate_threshold(p) - thr) < 1e-9
        gate, gsrc, min_on = None, llog, 0.5
        near = np.abs(llog - thr) < 1e-9
        assert not near.any()                                                                      # no gate decision hangs on the stitching error
    whole = frame_sums_ref(dlog, gsrc, thr, hop, T)
    G, ml = 2, 2
    ref_t = SegmentTracker(S, nb, hop, min_on, G, ml, dtype=np.float64)
    ref_t.advance(whole, 0, whole.shape[2], T - (whole.shape[2] - 1) * hop, True)
    want = ref_t.poll()
    assert sum(len(w) for w in want) >= 3, [[e[:2] for e in w] for w in want]

    def frame_sums(win, gwin):
        L = win.shape[-1]
        g = gwin if gwin is not None else W.oracle_forward(lcfg, lnet, win)[:, 0]
        return frame_sums_ref(W.oracle_forward(dcfg, dnet, win), g, thr, hop, L)

    sess = SegmentStreamSession(S, hop, H, frame_sums, SegmentTracker(S, nb, hop, min_on, G, ml, dtype=np.float64), numpy_advance,
                                sample_rate=16000, capacity=2, min_gap_frames=G, min_len_frames=ml)
    got = [[] for _ in range(S)]
    seen = 0
    for k, n in enumerate(_pushes(hop, T)):
        assert sess.push(x[:, 0, seen: seen + n], None if gate is None else gate[:, seen: seen + n]) is None
        seen += n
        if k % 4 == 0:
            for s, segs in enumerate(sess.poll()):
                got[s] += segs
    assert seen == T
    opened = sess.open_segments()
    for s, segs in enumerate(sess.flush()):
        got[s] += segs
    with pytest.raises(RuntimeError, match="reset"):
        sess.flush()
    worst = 0.0
    for s in range(S):
        assert [g.frames for g in got[s]] == [(lo, hi) for lo, hi, _, _ in want[s]], s
        for g, (lo, hi, cnt, prob) in zip(got[s], want[s]):
            assert isinstance(g, Segment)
            end = min(hi * hop, T)
            assert g.start_s == lo * hop / 16000 and g.end_s == end / 16000 and g.coverage == cnt / (end - lo * hop)
            worst = max(worst, float(np.abs(g.prob.astype(np.float64) - prob).max()))
        if opened[s] is not None:                                                                  # what was open before the flush came out of it
            assert got[s] and got[s][-1].frames[0] == opened[s].frames[0]
    # windows against the whole clip in float64 differ by the stitching error (1e-12 of the logits, test_window_cases_cpu), so the float32
    # prob may round the other way: one float32 ulp below 1
    assert worst <= 2.0 ** -24 * 1.01, worst
    sess.reset()
    assert sess.samples_seen == 0 and sess.poll() == [[] for _ in range(S)] and sess.flush() == [[] for _ in range(S)]


def test_session_refusals():
    cases = {c[0]: c for c in W.net_cases()}
    dcfg, _ = W.net_config(cases["x7.detector"])
    lcfg, _ = W.net_config(cases["x4.locator"])
    with pytest.raises(ValueError, match="does not divide"):
        segment_halo(dcfg, lcfg)                                             # hops 32 and 20
    fs = lambda win, gwin: np.zeros((1, 2, -(-win.shape[-1] // 4)), np.float32)
    sess = SegmentStreamSession(1, 4, 8, fs, SegmentTracker(1, 1, 4), numpy_advance)
    sess.push(np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError, match="gated on every push or on none"):
        sess.push(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError, match="shape"):
        sess.push(np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="capacity"):
        SegmentStreamSession(1, 4, 8, fs, SegmentTracker(1, 1, 4), numpy_advance, capacity=0)


def test_session_automatic_poll_loses_nothing_at_capacity_one():
    """A gate-only session on a count-only 'net' (frame sums straight from the gate): twelve runs per stream through an event ring of one or
    two records, pushed whole, frame by frame and ragged, with no poll before the flush."""
    hop, G, ml = 4, 1, 1
    counts = ([hop] + [0]) * 12 + [hop]
    gate = np.repeat(np.asarray(counts, np.float32) / hop, hop)[None]
    T = gate.shape[1]

    class Ring(SegmentTracker):
        def __init__(self, cap):
            super().__init__(1, 1, hop, 0.5, G, ml)
            self.cap, self.waiting = cap, 0

        def advance(self, *a, **k):
            before = self.events_total[0]
            super().advance(*a, **k)
            self.waiting += self.events_total[0] - before
            assert self.waiting <= self.cap, "an event would have been overwritten"

        def poll(self):
            self.waiting = 0
            return super().poll()

    def fs(win, gwin):
        c = np.pad(gwin, ((0, 0), (0, -gwin.shape[1] % hop))).reshape(1, -1, hop).sum(-1)
        return np.stack([c * 0.75, c], axis=1).astype(np.float32)

    for cap in (1, 2):
        for sizes in ([T], [hop] * (T // hop), [1, 7, 0, 13, 2] * 20):
            sess = SegmentStreamSession(1, hop, 2 * hop, fs, Ring(cap), numpy_advance, capacity=cap, min_gap_frames=G, min_len_frames=ml)
            seen = 0
            for n in sizes:
                n = min(n, T - seen)
                sess.push(np.zeros((1, n), np.float32), gate[:, seen: seen + n])
                seen += n
            assert seen == T
            segs = sess.flush()[0]
            assert [s.frames for s in segs] == [(2 * i, 2 * i + 1) for i in range(13)], (cap, sizes[:3])
            assert all(s.coverage == 1.0 and s.prob[0] == np.float32(0.75) for s in segs)


def test_a_ring_of_one_with_period_one_terminates_and_equals_the_bank():
    """capacity = 1 with min_gap_frames + min_len_frames = 1: ring * period - 1 = 0 frames, the step a lockstep session once cut its ticks by
    without the bank's floor of one frame, so its loop never advanced.  The tracker here refuses a second advance in a row that brings no
    frame and is not final, so the old behaviour fails instead of hanging.  The session's segments are those of a bank of one slot."""
    hop, nb = 4, 2

    class Progress(SegmentTracker):
        idle = 0

        def advance(self, fsum, f_lo=0, f_hi=None, last_valid=None, final=False):
            n = (fsum.shape[2] if f_hi is None else f_hi) - f_lo
            self.idle = self.idle + 1 if n == 0 and not final else 0
            assert self.idle < 2, "two advances in a row without a frame: the cut makes no progress"
            super().advance(fsum, f_lo, f_hi, last_valid, final)

    def fs(win, gwin):                                                       # the "locator" is the sign of x
        on = np.pad(win[:, 0] > 0, ((0, 0), (0, -win.shape[-1] % hop))).reshape(win.shape[0], -1, hop).sum(-1)
        return np.stack([on * 0.75, on * 0.25, on], axis=1).astype(np.float32)

    for frames, want in (([1, 1, 0], [(0, 2)]), ([1, 1, 1], [(0, 3)]), ([1, 0, 1], [(0, 1), (2, 3)])):
        x = np.repeat(np.asarray(frames, np.float32), hop)
        sess = SegmentStreamSession(1, hop, 2 * hop, fs, Progress(1, nb, hop, 0.5, 1, 0), capacity=1, min_gap_frames=1, min_len_frames=0)
        assert sess.push(x[None]) is None
        got = sess.flush()[0]
        bank = SegmentStreamBank(1, hop, 2 * hop, fs, BankSegmentTracker(1, nb, hop, 0.5, 1, 0, ring=1), ring=1, min_gap_frames=1, min_len_frames=0)
        slot = bank.open()
        bank.push({slot: x})
        ref = bank.close(slot)
        assert [g.frames for g in got] == [r.frames for r in ref] == want, (frames, got, ref)
        for g, r in zip(got, ref):
            assert (g.start_s, g.end_s, g.coverage, g.confidence) == (r.start_s, r.end_s, r.coverage, r.confidence) and g.prob.tobytes() == r.prob.tobytes()
            assert g.coverage == 1.0 and g.prob.tolist() == [0.75, 0.25]


def _lockstep_cut_before(capacity, period, hop, unread, f_lo, f_hi, last_valid, final):
    """The lockstep session's own loop as it stood before cut_rows, the tracker's advance and the ring's read replaced by a log."""
    log = []
    step = capacity * period - 1                                             # frames // period + 1 <= capacity
    while True:
        m = min(step, f_hi - f_lo)
        last = f_lo + m == f_hi
        drained = False
        if unread and (unread + m) // period + 1 >= capacity:
            drained, unread = True, 0
        log.append((drained, f_lo, f_lo + m, last_valid if last else hop, final and last))
        unread += m
        f_lo += m
        if last:
            return log, unread


def test_the_shared_cut_rule_is_the_lockstep_rule_wherever_that_one_terminates():
    hop, f_lo, n, multi, drains = 4, 3, 0, 0, 0
    for ring in (1, 2, 3, 64):
        for period in (1, 2, 7):
            step = ring * period - 1
            if step < 1:
                continue                                                     # the old loop does not end there (the test above)
            for unread in sorted({0, 1, ring * period - 2} - {-1}):
                for frames in sorted({0, 1, step - 1, step, step + 1, 3 * step + 2}):
                    for last_valid, final in ((hop, False), (hop - 1, True)):
                        want, left = _lockstep_cut_before(ring, period, hop, unread, f_lo, f_lo + frames, last_valid, final)
                        pieces, after = cut_rows([[0, 5, 9, f_lo, f_lo + frames, 11, last_valid, int(final)]], [unread], ring, period, hop)
                        got = [(drain, lo, hi, lv, bool(fin)) for drain, ((_, _, _, lo, hi, _, lv, fin),) in pieces]
                        assert got == want and after == [left], (ring, period, unread, frames, final, got, want)
                        at = 11
                        for _, ((s, off, Fr, lo, hi, f0, _, _),) in pieces:   # what names the stream's rows goes through; frame0 moves on
                            assert (s, off, Fr, f0) == (0, 5, 9, at)
                            at += hi - lo
                        n, multi, drains = n + 1, multi + (len(got) > 1), drains + sum(g[0] for g in got)
    assert n > 300 and multi > 50 and drains > 100, (n, multi, drains)


# ---- 3. the margin of the GPU tests' locator-driven recording ----------------------------------------------------------------------------
def test_locator_recording_margin_on_the_oracle():
    """The GPU test compares a live session (windows) with detect_segments_batch (one forward) on SC.locator_recording().  Their locator logits
    differ in the last bits, so a sample whose logit lies within 1e-4 of the threshold may be gated in one and not in the other; a frame
    holding m_f such samples may differ by m_f in its count.  For the frames to have one right answer every frame's count must lie more than
    m_f from min_on * valid.  Checked here on the float64 oracle for the values fixed in segment_session_cases (seed, threshold, min_on):
    measured: the nearest full frame lies 3.6 samples from the rule's edge with m_f <= 1; the 1-sample last frame lies 0.57 from it with
    m_f = 0 (its one logit is far from the threshold)."""
    from oracle import wv_oracle as O
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    cfg = default_config("locator")
    onet = O._Net(cfg, random_state_dict(cfg, SC.LOC_SEED), np.float64)
    x = SC.locator_recording()
    S, _, T = x.shape
    hop = default_config("detector").hop_length
    lg = O.locator_forward(cfg, onet, x, dtype=np.float64)[:, 0]
    thr = gate_threshold(SC.LOC_THRESHOLD)
    Fr = -(-T // hop)
    pad = ((0, 0), (0, Fr * hop - T))
    count = np.pad(lg > thr, pad).reshape(S, Fr, hop).sum(-1)
    m = np.pad(np.abs(lg - thr) <= 1e-4, pad).reshape(S, Fr, hop).sum(-1)
    valid = SC.valid_of(Fr, hop, T - (Fr - 1) * hop)
    dist = np.abs(count - SC.LOC_MIN_ON * valid[None])
    print(f"MEASURE locator recording: max m_f = {int(m.max())}, nearest count {float(dist.min()):.2f} samples from min_on * valid")
    assert (dist > m).all(), (np.argwhere(dist <= m), count, m)
    from waveverify_amd.localize import segments_from_counts
    runs = [segments_from_counts(count[s], valid, SC.LOC_MIN_ON, 2, 5) for s in range(S)]
    assert runs == SC.LOC_EXPECTED_FRAMES, runs


# ---- 4. the exports -----------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("wv_segment_track", "wv_segment_track_bytes")


def test_new_exports_are_declared_listed_and_bound():
    from waveverify_amd import _lib
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    declared = set(re.findall(r"\b(wv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert "WV_SEGMENT_MAX_GAP" in header and "frame j in slot" in header        # the limit and the layout are stated for callers
    zero = {C.c_int: 0, C.c_int64: 0, C.c_size_t: 0, C.c_float: 0.0, C.c_double: 0.0}
    for name in NEW_EXPORTS:
        rc = getattr(lib, name)(*[zero.get(t) for t in _lib.SIGNATURES[name][1]])
        msg = lib.wv_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":"), (name, rc, msg)
    sb, eb = C.c_size_t(), C.c_size_t()
    assert lib.wv_segment_track_bytes(3, 16, 2, 64, C.byref(sb), C.byref(eb)) == 0
    assert sb.value == 3 * (32 + 8 * 17 + 4 * 17 + 4) and eb.value == 3 * (8 + 64 * (24 + 64))
    assert lib.wv_segment_track_bytes(3, 16, 65, 64, C.byref(sb), C.byref(eb)) == -1 and b"min_gap_frames outside [1, 64]" in lib.wv_last_error()
    assert lib.wv_segment_track_bytes(65536, 16, 2, 64, C.byref(sb), C.byref(eb)) == -1 and b"[1, 65535]" in lib.wv_last_error()
    from waveverify_amd.core import WaveVerify
    import inspect
    sig = inspect.signature(WaveVerify.open_segment_session)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == dict(
        n=1, threshold=0.5, min_on=0.5, min_gap_frames=2, min_len_frames=5, sample_rate=16000, channels=1, capacity=64)
