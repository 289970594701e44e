"""Live segment sessions on the MI355X: wv_segment_track against its host twin on guarded buffers, and session.SegmentSession /
native_session.NativeSegmentSession against the file route (WaveVerify.detect_segments_batch) on the full-size nets.

Bars.  Tracker against twin: bit for bit (the same float64 adds in the same order).  Session against detect_segments_batch: frames, start_s,
end_s and coverage equal; prob within 1e-5, the project's bar for windowed against whole-clip sums (test_gpu_localized); bits equal wherever
the reference probability is more than 1e-5 from 0.5.  The locator-driven recording and its margin: segment_session_cases.LOC_* and
test_segment_session_cpu.test_locator_recording_margin_on_the_oracle; that margin is worked out for the exact path's agreement between a
windowed and a whole-clip locator (1e-4 on a logit), so the locator-driven comparisons run the exact path.  The native-rate session is compared
with a 16 kHz session fed the front stage's own pieces, which makes the two runs the same launches on the same numbers.

Measured on the MI355X (MEASURE lines, pytest -s): tracker against twin 0 differences over 6260 launches; session prob against
detect_segments_batch 6.0e-8 at most on the exact path (gate mask and locator-driven, every chunking), 0 in the f16 mode, 0 between the native
and the 16 kHz session; the locator-driven frames are those the float64 oracle gives (segment_session_cases.LOC_EXPECTED_FRAMES)."""
import numpy as np
import pytest
import torch

import segment_session_cases as SC
from guard import Guards
from waveverify_amd import native, ops
from waveverify_amd import native_session as NS
from waveverify_amd.localize import Segment, SegmentTracker
from waveverify_amd.session import HipSegmentTracker, SegmentSession

pytestmark = pytest.mark.gpu

BAR = 1e-5
HOP = 320


# ================================================================== 1. the tracker kernel against its host twin
class GuardedTracker(HipSegmentTracker):
    """HipSegmentTracker with fsum, state and events between guard bands."""

    def __init__(self, fsum, hop, min_on, G, ml, capacity):
        self.g = Guards()
        self.fsum = self.g.input(fsum, "fsum")
        S, nb1, _ = fsum.shape
        sb, eb = ops.segment_track_bytes(S, nb1 - 1, G, capacity)
        self._state_arena = self.g.output((sb,), torch.uint8, "state")
        self._events_arena = self.g.output((eb,), torch.uint8, "events")
        super().__init__(S, nb1 - 1, hop, min_on, G, ml, capacity, torch.device("cuda", torch.cuda.current_device()))

    def reset(self):
        super().reset()
        self.state, self.events = self._state_arena.t.zero_(), self._events_arena.t.zero_()

    def advance(self, fsum, *a, **k):
        super().advance(self.fsum.t, *a, **k)

    def check(self):
        torch.cuda.synchronize()
        self.fsum.check()                                                       # guards and data untouched
        bad = self._state_arena.guard_report() + self._events_arena.guard_report()
        assert not bad, bad


@pytest.mark.parametrize("nb", SC.NBS)
@pytest.mark.parametrize("S", [1, 3, 65])
def test_tracker_kernel_equals_the_twin(S, nb):
    hop, min_on = 10, 0.5
    n_names, n_events, n_launch = set(), 0, 0
    for G, ml in ((2, 5), (1, 1), (5, 5), (3, 1)):
        n_pat = len(SC.named_patterns(hop, min_on, G, ml))
        for salt in range(2 * n_pat if S == 1 else 8 if S == 3 else 2):
            names, fsum, last_valid = SC.stream_patterns(S, hop, min_on, G, ml, nb, salt)
            assert fsum.shape[2] <= 200
            n_names |= set(names)
            want = SC.whole_ref(fsum, hop, last_valid, min_on, G, ml)
            for kind in SC.CHUNKINGS:
                chunks = SC.chunks_of(fsum.shape[2], kind, np.random.default_rng(SC.seed_of("gpu-chunks", S, nb, G, ml, salt)), last_valid < hop)
                twin = SC.run_tracker(SegmentTracker(S, nb, hop, min_on, G, ml), fsum, chunks, last_valid)
                assert SC.same_events(twin, want) is None
                dev = GuardedTracker(fsum, hop, min_on, G, ml, 16)
                got = SC.run_tracker(dev, fsum, chunks, last_valid, poll_each=(salt % 2 == 1))
                dev.check()
                diff = SC.same_events(got, twin)
                assert diff is None, (names, G, ml, kind, diff)
                n_events += sum(len(e) for e in got)
                n_launch += len(chunks)
    if S == 1:
        assert len(n_names) == len(SC.named_patterns(hop, min_on, 2, 5))        # every named pattern ran
    print(f"MEASURE tracker S={S} nb={nb}: {n_launch} launches, {n_events} events, all bit-equal to the twin")
    assert n_events > 0


def test_tracker_open_run_on_the_way_equals_the_twin():
    """The provisional open run, the held gap frames across ticks and a run that outlives many ticks: state read back after every tick."""
    hop, nb, G, ml = 10, 16, 5, 1
    rng = np.random.default_rng(9)
    count = [0, 10, 10, 0, 0, 0, 0, 7, 0, 0, 0, 0, 0, 10, 0, 0, 5, 5, 4, 0, 0, 0, 0, 10]
    fsum = np.stack([SC.sums_for(count, nb, rng, quantized=False), SC.sums_for(count[::-1], nb, rng, quantized=False)])
    twin, dev = SegmentTracker(2, nb, hop, 0.5, G, ml), GuardedTracker(fsum, hop, 0.5, G, ml, 4)
    for f in range(len(count)):
        twin.advance(fsum, f, f + 1, final=f == len(count) - 1)
        dev.advance(fsum, f, f + 1, final=f == len(count) - 1)
        a, b = twin.open_runs(), dev.open_runs()
        for u, v in zip(a, b):
            assert (u is None) == (v is None), f
            if u is not None:
                assert u[:3] == v[:3] and u[3].tobytes() == v[3].tobytes(), (f, u, v)
        assert SC.same_events(dev.poll(), twin.poll()) is None, f
    dev.check()


def test_tracker_takes_garbage_state_as_closed():
    """Buffers of 0xFF bytes (never cleared): open = -1, lo = hi = -1, counter -1, NaN sums.  The header promises that such a state is taken as
    closed with no events; the tick then gives what a fresh tracker gives and nothing outside the buffers is touched."""
    hop, nb, G, ml = 10, 16, 3, 1
    names, fsum, last_valid = SC.stream_patterns(3, hop, 0.5, G, ml, nb, 0)
    want = SC.whole_ref(fsum, hop, last_valid, 0.5, G, ml)
    dev = GuardedTracker(fsum, hop, 0.5, G, ml, 16)
    dev.state.fill_(0xFF)
    dev.events.fill_(0xFF)
    got = SC.run_tracker(dev, fsum, [(0, fsum.shape[2])], last_valid)
    dev.check()
    assert SC.same_events(got, want) is None


def test_tracker_refusals():
    fsum = torch.zeros((2, 17, 4), device="cuda")
    sb, eb = ops.segment_track_bytes(2, 16, 2, 4)
    state, events = torch.zeros(sb, dtype=torch.uint8, device="cuda"), torch.zeros(eb, dtype=torch.uint8, device="cuda")
    call = lambda **k: ops.segment_track(**{**dict(fsum=fsum, f_lo=0, f_hi=4, frame0=0, hop=10, last_valid=10, final=False, min_on=0.5,
                                                   min_gap_frames=2, min_len_frames=5, state=state, events=events, capacity=4), **k})
    call()
    for kw, what in ((dict(min_gap_frames=65), "min_gap_frames outside"), (dict(state=state[:-8]), "shorter than"),
                     (dict(events=events[:-8]), "shorter than"), (dict(f_hi=5), "outside"), (dict(last_valid=11), "last_valid"),
                     (dict(capacity=0), "capacity"), (dict(min_gap_frames=3), "shorter than")):
        with pytest.raises(RuntimeError, match="wv_segment_track.*" + what):
            call(**kw)
    with pytest.raises(RuntimeError, match=r"wv_segment_track_bytes.*\[1, 65535\]"):
        ops.segment_track_bytes(65536, 16, 2, 4)


# ================================================================== the full-size nets
@pytest.fixture(scope="module")
def wv():
    from waveverify_amd import WaveVerify
    return WaveVerify.random_init(seed=SC.LOC_SEED)


def _pieces(T, kind, hop=HOP):
    if kind == "whole":
        return [T]
    if kind == "hop":
        return [hop] * (T // hop) + ([T % hop] if T % hop else [])
    out, base, k = [], [1, hop - 1, 0, hop, 3 * hop + 7, 5 * hop - 1, 2], 0
    while sum(out) < T:
        out.append(min(base[k % len(base)], T - sum(out)))
        k += 1
    return out


def _run(sess, x, gate, kind, poll_every=3):
    """Push x [S, T] (and its gate) in pieces, polling now and then -> per stream every Segment, in the order it came out."""
    got = [[] for _ in range(x.shape[0])]
    at = 0
    for i, n in enumerate(_pieces(x.shape[-1], kind)):
        assert sess.push(x[..., at:at + n], None if gate is None else gate[:, at:at + n]) is None
        at += n
        if i % poll_every == poll_every - 1:
            for s, segs in enumerate(sess.poll()):
                got[s] += segs
    for s, segs in enumerate(sess.flush()):
        got[s] += segs
    return got


def _compare(got, want, what, exact_prob=False):
    """Frames, times and coverage equal; prob within BAR; bits equal away from 0.5 -> the largest prob difference."""
    worst = 0.0
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert [a.frames for a in g] == [b.frames for b in w], (what, s, [a.frames for a in g], [b.frames for b in w])
        for a, b in zip(g, w):
            assert isinstance(a, Segment)
            assert (a.start_s, a.end_s, a.coverage) == (b.start_s, b.end_s, b.coverage), (what, s, a, b)
            d = float(np.abs(a.prob.astype(np.float64) - b.prob.astype(np.float64)).max())
            worst = max(worst, d)
            far = np.abs(b.prob.astype(np.float64) - 0.5) > BAR
            assert ((a.prob >= 0.5) == (b.prob >= 0.5))[far].all(), (what, s, a.frames)
            if far.all():
                assert a.watermark == b.watermark and abs(a.confidence - b.confidence) <= BAR
    assert worst <= BAR, (what, worst)
    if exact_prob:
        assert worst == 0.0, (what, worst)
    return worst


# ================================================================== 2. capacity 2, twelve segments per stream
def test_automatic_poll_at_capacity_two_loses_nothing(wv):
    S, L, G = 2, 5, 2
    Fr = 12 * (L + G) + 1
    T = Fr * HOP
    gate = np.zeros((S, Fr), np.float32)
    for i in range(12):
        gate[0, i * (L + G): i * (L + G) + L] = 1
        gate[1, 1 + i * (L + G): 1 + i * (L + G) + L] = 1
    gate = torch.from_numpy(np.repeat(gate, HOP, axis=1)).cuda()
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((S, T)).astype(np.float32) * 0.1).cuda()
    want = wv.detect_segments_batch(x.unsqueeze(1), gate=gate)
    assert [len(w) for w in want] == [12, 12]
    for kind in ("whole", "hop", "ragged"):
        sess = wv.open_segment_session(S, capacity=2)
        got = _run(sess, x, gate, kind, poll_every=10 ** 9)                     # no poll but the session's own
        worst = _compare(got, want, ("capacity 2", kind))
        print(f"MEASURE capacity 2, {kind}: 12 segments per stream in order, prob within {worst:.2e}")


# ================================================================== 3. the gate-mask session
@pytest.fixture(scope="module")
def gate_case():
    T, S = 16001, 3
    from waveverify_amd.init import synthetic_clips
    x = torch.from_numpy(synthetic_clips(S, T, seed=53)[0][:, 0]).cuda()
    gate = torch.zeros((S, T), device="cuda")
    gate[0, 5 * HOP: 15 * HOP] = 1
    gate[0, 40 * HOP: 48 * HOP] = 1
    gate[1] = 1
    return x, gate


@pytest.mark.parametrize("kind", ["whole", "hop", "ragged"])
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_gate_mask_session_equals_detect_segments_batch(wv, gate_case, precision, kind):
    x, gate = gate_case
    wv.set_precision(precision)
    try:
        want = wv.detect_segments_batch(x.unsqueeze(1), gate=gate)
        assert [[s.frames for s in w] for w in want] == [[(5, 15), (40, 48)], [(0, 51)], []]
        assert want[1][0].end_s == 16001 / 16000                                 # the true length on the final frame
        sess = wv.open_segment_session(3)
        assert type(sess) is SegmentSession and sess.precision == precision and sess.locator_precision == precision
        got = _run(sess, x, gate, kind)
        worst = _compare(got, want, (precision, kind))
        print(f"MEASURE gate-mask session {precision} {kind}: prob against detect_segments_batch {worst:.2e}")
    finally:
        wv.set_precision("f32")


# ================================================================== 4. the locator-driven session
@pytest.mark.parametrize("kind", ["whole", "hop", "ragged"])
def test_locator_driven_session_equals_detect_segments_batch(wv, kind):
    x = torch.from_numpy(SC.locator_recording()[:, 0]).cuda()
    kw = dict(threshold=SC.LOC_THRESHOLD, min_on=SC.LOC_MIN_ON)
    want = wv.detect_segments_batch(x.unsqueeze(1), **kw)
    assert all(len(w) >= 1 for w in want), [[s.frames for s in w] for w in want]
    got = _run(wv.open_segment_session(x.shape[0], **kw), x, None, kind)
    worst = _compare(got, want, ("locator", kind))
    print(f"MEASURE locator-driven session {kind}: frames {[[s.frames for s in g] for g in got]}, prob against detect_segments_batch {worst:.2e}")


def test_open_segments_shows_an_opening_at_once_and_a_close_two_frames_late(wv, gate_case):
    x, gate = gate_case
    sess = wv.open_segment_session(3)
    sess.push(x[:, :6 * HOP], gate[:, :6 * HOP])
    o = sess.open_segments()
    assert o[0].frames == (5, 6) and o[1].frames == (0, 6) and o[2] is None and o[0].start_s == 5 * HOP / 16000
    sess.push(x[:, 6 * HOP: 16 * HOP], gate[:, 6 * HOP: 16 * HOP])             # one off frame: still open, nothing closed
    assert sess.open_segments()[0].frames == (5, 15) and sess.poll()[0] == []
    sess.push(x[:, 16 * HOP: 17 * HOP], gate[:, 16 * HOP: 17 * HOP])           # the second: closed
    assert sess.open_segments()[0] is None and [s.frames for s in sess.poll()[0]] == [(5, 15)]


# ================================================================== 5. the native-rate session
def test_native_48k_stereo_session_is_the_16k_session_behind_the_front_stage(wv):
    sr, Cn = 48000, 2
    x16 = SC.locator_recording()[:, 0]
    left = np.repeat(x16, 3, axis=1)
    x = torch.from_numpy(np.stack([left, 0.5 * left], axis=1).astype(np.float32)).cuda()      # [S, 2, 3 T]
    S, _, Tn = x.shape
    kw = dict(threshold=SC.LOC_THRESHOLD, min_on=SC.LOC_MIN_ON)
    m16 = wv.to_model_rate(x, sr)[:, 0]
    nat, ref = wv.open_segment_session(S, sample_rate=sr, channels=Cn, **kw), wv.open_segment_session(S, **kw)
    assert isinstance(nat, NS.NativeSegmentSession) and type(ref) is SegmentSession
    with pytest.raises(ValueError, match="gate"):
        nat.push(x[:, :, :10], gate=torch.zeros((S, 10), device="cuda"))
    plan = NS.StagePlan(*native.table_geometry(sr, native.MODEL_RATE))
    got, want = [[] for _ in range(S)], [[] for _ in range(S)]
    at = at16 = 0
    for i, n in enumerate(_pieces(Tn, "ragged", 3 * HOP)):
        assert nat.push(x[:, :, at:at + n]) is None
        k = plan.push(n).n_out
        ref.push(m16[:, at16:at16 + k])
        at, at16 = at + n, at16 + k
        if i % 3 == 2:
            a, b = nat.poll(), ref.poll()
            for s in range(S):
                got[s] += a[s]
                want[s] += b[s]
    assert at == Tn
    k = plan.flush().n_out
    ref.push(m16[:, at16:at16 + k])
    assert at16 + k == m16.shape[1]
    for s, (a, b) in enumerate(zip(nat.flush(), ref.flush())):
        got[s] += a
        want[s] += b
    worst = _compare(got, want, "native 48 kHz stereo", exact_prob=True)
    n_seg = sum(len(g) for g in got)
    print(f"MEASURE native 48 kHz stereo session: {n_seg} segments, frames {[[s.frames for s in g] for g in got]}, prob difference {worst:.2e}")
    assert n_seg >= 1
    whole = wv.detect_segments_batch(m16.unsqueeze(1), **kw)                      # and the file route on to_model_rate of the recording
    assert [[s.frames for s in g] for g in got] == [[s.frames for s in w] for w in whole]
    _compare(got, whole, "native against the file route")


# ================================================================== 6. lifecycle
def test_lifecycle(wv, gate_case):
    x, gate = gate_case
    sess = wv.open_segment_session(3)
    assert sess.flush() == [[], [], []]
    with pytest.raises(RuntimeError, match="reset"):
        sess.flush()
    with pytest.raises(RuntimeError, match="reset"):
        sess.push(x[:, :10])
    sess.reset()
    first = _run(sess, x, gate, "ragged")
    sess.reset()
    assert sess.samples_seen == 0 and sess.open_segments() == [None] * 3 and sess.poll() == [[], [], []]
    again = _run(sess, x, gate, "ragged")
    assert [len(f) for f in first] == [2, 1, 0]
    _compare(again, first, "rerun", exact_prob=True)
    with pytest.raises(ValueError, match="gated on every push or on none"):
        s2 = wv.open_segment_session(3)
        s2.push(x[:, :10], gate[:, :10])
        s2.push(x[:, 10:20])
    with pytest.raises(ValueError, match="capacity"):
        wv.open_segment_session(1, capacity=0)
    with pytest.raises(RuntimeError, match="min_gap_frames outside"):
        wv.open_segment_session(1, min_gap_frames=65)
