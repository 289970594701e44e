"""Segment banks on the MI355X: wv_bank_segment_track against its numpy twin on guarded buffers, and session.SegmentBank
against the lockstep SegmentSession, the float64 and f16 oracles and the file route (WaveVerify.detect_segments_batch).

Bars.  Kernel against twin, bank against lockstep session, reused slot against fresh bank, alone against beside others: bit for bit.  Bank
against the oracles on the small session nets (gate-mask form): frames and counts equal, prob within test_gpu_session_bank's bars for
DetectBank's mean probability: 1e-6 on the exact path, det_mean_bar(n) in the f16 mode with n the segment's own gated sample count.  Bank
against detect_segments_batch: frames, times and coverage equal, prob within test_gpu_segment_session's BAR (1e-5).

Every figure is printed as a MEASURE line before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import bank_cases as BK
import segment_bank_cases as SB
import segment_session_cases as SC
from guard import Guards
from localized_cases import frame_sums_from_probs, frame_sums_ref, sigmoid64
from test_gpu_h16 import det_mean_bar
from test_gpu_segment_session import BAR, HOP, _compare
from waveverify_amd import ops
from waveverify_amd.localize import BankSegmentTracker
from waveverify_amd.session import HipBankSegmentTracker, SegmentBank, SegmentSession, bank_track_row_ok

pytestmark = pytest.mark.gpu

W = SB.W
MEAN_BAR = 1e-6                                                    # tests/test_gpu_session_bank.py, exact DetectBank mean probability
CAP = SB.KERNEL_CAPACITY
ARENA = 1 << 15                                                    # floats: the largest tick of the kernel cases needs far fewer


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ================================================================== 1. the kernel against its twin
class GuardedBank(HipBankSegmentTracker):
    """HipBankSegmentTracker with fsum, desc, state and events between guard bands.  One fsum arena serves every tick: it is NaN beyond the
    tick's n_fsum floats, which the kernel is told of, so a read past the tick's arena shows as it would past the buffer."""

    def __init__(self, nb, hop, min_on, G, ml, ring):
        super().__init__(CAP, nb, hop, min_on, G, ml, ring, torch.device("cuda", torch.cuda.current_device()))
        self.g = Guards()
        self._fsum = self.g.output((ARENA,), torch.float32, "fsum")
        self._desc = self.g.output((CAP + 16, 8), torch.int64, "desc")
        self._state = self.g.output((self.state.numel(),), torch.uint8, "state")
        self._events = self.g.output((self.events.numel(),), torch.uint8, "events")
        self.state, self.events = self._state.t.zero_(), self._events.t.zero_()

    def tick(self, arena, desc):
        """One call on host arrays -> (state, events) bytes as they were before it."""
        assert arena.size <= ARENA and len(desc) <= CAP + 16
        self._fsum.t.fill_(float("nan"))
        self._fsum.t[:arena.size].copy_(cu(arena))
        self._desc.t[:len(desc)].copy_(cu(np.asarray(desc, np.int64).reshape(-1, 8)))
        before = (self.state.clone(), self.events.clone())
        self.advance(self._fsum.t[:arena.size], self._desc.t, len(desc))
        return before

    def untouched(self, before, named):
        """The state and event sections of every slot outside `named` are byte-equal to `before`."""
        changed = ((self.state != before[0]).view(CAP, -1).any(1) | (self.events != before[1]).view(CAP, -1).any(1)).cpu().numpy()
        assert not set(np.flatnonzero(changed).tolist()) - set(named), (np.flatnonzero(changed), named)

    def check(self):
        torch.cuda.synchronize()
        bad = [m for a in self.g.arenas for m in a.guard_report()]
        assert not bad, bad


def _same_runs(a, b, what):
    for s in a:
        assert (a[s] is None) == (b[s] is None), (what, s)
        if a[s] is not None:
            assert a[s][:3] == b[s][:3] and a[s][3].tobytes() == b[s][3].tobytes(), (what, s, a[s], b[s])


@pytest.mark.parametrize("G", SC.GAPS)
@pytest.mark.parametrize("nb", SC.NBS)
@pytest.mark.parametrize("P", [1, 3, 9])
def test_bank_kernel_equals_the_twin(P, nb, G):
    hop, min_on, ml = SB.HOP, 0.5, 5 if G == 2 else 1
    kinds = {1: ("random",), 3: ("random", "frames"), 9: ("whole", "random")}[P]
    n_ticks = n_events = n_empty = n_partial = 0
    for kind in kinds:
        rng = np.random.default_rng(SC.seed_of("gpu-bank", P, nb, G, kind))
        for batch in SB.pattern_streams(nb, G, ml, kind, rng, capacity=P + 1):
            twin, dev = BankSegmentTracker(CAP, nb, hop, min_on, G, ml, ring=16), GuardedBank(nb, hop, min_on, G, ml, 16)
            slots = [b[0] for b in batch]
            for arena, desc in SB.bank_ticks(batch, nb, hop, rng):
                assert all(bank_track_row_ok(r, CAP, nb, hop, arena.size) for r in desc)
                n_empty += sum(1 for r in desc if r[3] == r[4])
                n_partial += sum(1 for r in desc if r[7] and r[6] < hop)
                twin.advance(arena, desc)
                before = dev.tick(arena, desc)
                dev.untouched(before, [int(r[0]) for r in desc])
                _same_runs(twin.open_runs(slots), dev.open_runs(slots), (kind, n_ticks))             # state and events read back after every tick
                a, b = twin.poll(slots), dev.poll(slots)
                for s in slots:
                    diff = SC.same_events([b[s]], [a[s]])
                    assert diff is None, (kind, s, diff)
                    n_events += len(a[s])
                n_ticks += 1
            dev.check()
    print(f"MEASURE bank tracker P={P} nb={nb} G={G}: {n_ticks} launches, {n_events} events, {n_empty} empty ranges, {n_partial} partial last "
          f"frames, all bit-equal to the twin")
    assert n_events > 0 and n_empty > 0 and n_partial > 0


def test_bank_kernel_skips_bad_rows_serves_the_good_and_takes_garbage_as_closed():
    hop, nb, G, ml = SB.HOP, 16, 3, 1
    rng = np.random.default_rng(11)
    twin, dev = BankSegmentTracker(CAP, nb, hop, 0.5, G, ml, ring=16), GuardedBank(nb, hop, 0.5, G, ml, 16)
    held = SC.sums_for([hop] * 3, nb, rng)
    for t in (twin, dev):
        (t.advance if t is twin else dev.tick)(held.reshape(-1), np.array([[4, 0, 3, 0, 3, 0, hop, 0]], np.int64))
    ss, es = dev._strides
    dev.state[6 * ss:7 * ss].fill_(0xFF)                                        # slot 6 was never cleared: open = -1, lo = hi = -1, NaN sums
    dev.events[6 * es:7 * es].fill_(0xFF)
    batch = [(6, SC.sums_for([0, hop, hop, 0, 0, 0, hop, hop], nb, rng), hop, [(0, 3), (3, 8)], 0),
             (1, SC.sums_for([hop, hop, 0, hop], nb, rng), 3, [(0, 2), (2, 4)], 0)]
    for arena, desc in SB.bank_ticks(batch, nb, hop, rng):
        good = [4] + [int(v) for v in desc[0][1:]]
        bads = [b for _, b in SB.bad_track_rows(good, CAP, nb, hop, arena.size) if b[0] == 4]
        assert len(bads) >= 10 and not any(bank_track_row_ok(b, CAP, nb, hop, arena.size) for b in bads)
        desc = np.concatenate([np.array(bads[:5], np.int64), desc, np.array(bads[5:], np.int64)])
        twin.advance(arena, desc)
        before = dev.tick(arena, desc)
        dev.untouched(before, [6, 1])                                           # slot 4, named by the bad rows alone, among them
    dev.check()
    _same_runs(twin.open_runs([4, 6, 1]), dev.open_runs([4, 6, 1]), "after bad rows")
    a, b = twin.poll([6, 1]), dev.poll([6, 1])
    assert [e[:2] for e in a[6]] == [(1, 3), (6, 8)] and len(a[1]) >= 1
    assert SC.same_events([b[6], b[1]], [a[6], a[1]]) is None


def test_bank_kernel_refusals():
    nb, hop = 16, 10
    sb, eb = ops.segment_track_bytes(4, nb, 2, 8)
    state, events = torch.zeros(sb, dtype=torch.uint8, device="cuda"), torch.zeros(eb, dtype=torch.uint8, device="cuda")
    fsum = torch.zeros(17 * 4, device="cuda")
    desc = cu(np.array([[1, 0, 4, 0, 4, 0, hop, 0]], np.int64))
    base = dict(fsum=fsum, desc=desc, P=1, capacity=4, nb=nb, hop=hop, min_on=0.5, min_gap_frames=2, min_len_frames=5, state=state, events=events,
                ring=8)
    call = lambda **k: ops.bank_segment_track(**{**base, **k})
    call()
    call(P=0)
    for kw, what in ((dict(capacity=0), "capacity outside"), (dict(capacity=1048577), "capacity outside"), (dict(nb=0), "nb outside"),
                     (dict(nb=256), "nb outside"), (dict(hop=0), "hop < 1"), (dict(min_gap_frames=0), "min_gap_frames outside"),
                     (dict(min_gap_frames=65), "min_gap_frames outside"), (dict(min_len_frames=-1), "min_len_frames < 0"),
                     (dict(ring=0), "ring < 1"), (dict(min_on=float("nan")), "not a number"), (dict(state=state[:-8]), "shorter than"),
                     (dict(events=events[:-8]), "shorter than"), (dict(capacity=5), "shorter than"), (dict(ring=9), "shorter than"),
                     (dict(min_gap_frames=3), "shorter than"), (dict(state=state[1:]), "8-byte aligned"), (dict(events=events[4:]), "8-byte aligned")):
        with pytest.raises(RuntimeError, match="wv_bank_segment_track.*" + what):
            call(**kw)
    from waveverify_amd import _lib
    lib, st = _lib.load(), _lib.stream()
    raw = lambda a: lib.wv_bank_segment_track(a[0], a[1], a[2], a[3], 4, nb, hop, 0.5, 2, 5, 1e-8, a[4], sb, a[5], eb, 8, st)
    args = [fsum.data_ptr(), fsum.numel(), desc.data_ptr(), 1, state.data_ptr(), events.data_ptr()]
    assert raw(args) == 0
    for i, v, what in ((0, None, "frame sums without fsum"), (2, None, "null desc"), (4, None, "null desc, state"), (5, None, "null desc, state or events"),
                       (1, -1, "n_fsum < 0"), (3, -1, "P outside"), (3, 65536, "P outside")):
        a = list(args)
        a[i] = v
        assert raw(a) == -1
        msg = lib.wv_last_error().decode()
        assert msg.startswith("wv_bank_segment_track:") and what in msg, (i, msg)
    torch.cuda.synchronize()
    assert int(ops.segment_events(events, 4, nb, 8)[0].sum()) == 0


# ================================================================== the full-size nets
@pytest.fixture(scope="module")
def wv():
    from waveverify_amd import WaveVerify
    return WaveVerify.random_init(seed=SC.LOC_SEED)


def _run_bank(bank, streams, poll_every=3):
    """streams [(x [T], gate [T] or None, push sizes)] opened together and pushed in step, each in its own sizes, then closed in order
    -> per stream every Segment in the order it came out."""
    slots = [bank.open() for _ in streams]
    got, at = [[] for _ in streams], [0] * len(streams)
    for i in range(max(len(sz) for _, _, sz in streams)):
        items = {}
        for k, (x, g, sz) in enumerate(streams):
            if i < len(sz):
                a, b = at[k], at[k] + sz[i]
                items[slots[k]] = x[a:b] if g is None else (x[a:b], g[a:b])
                at[k] = b
        assert bank.push(items) is None
        if i % poll_every == poll_every - 1:
            for s, segs in bank.poll().items():
                got[slots.index(s)] += segs
    for k, (x, _, _) in enumerate(streams):
        assert at[k] == x.shape[0] and bank.samples_seen(slots[k]) == at[k] // bank.hop * bank.hop
        got[k] += bank.close(slots[k])
    return got


# ================================================================== 2. equal pushes are the lockstep session
@pytest.mark.parametrize("kind", ["hop", "ragged"])
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_equal_pushes_are_the_lockstep_session_bit_for_bit(wv, precision, kind):
    T, S = 16001, 4
    from waveverify_amd.init import synthetic_clips
    x = torch.from_numpy(synthetic_clips(S, T, seed=53)[0][:, 0]).cuda()
    gate = torch.zeros((S, T), device="cuda")
    gate[0, 5 * HOP: 15 * HOP] = 1
    gate[0, 40 * HOP: 48 * HOP] = 1
    gate[1] = 1
    gate[3, 2 * HOP + 7: 30 * HOP + 160] = 1
    wv.set_precision(precision)
    try:
        sess = wv.open_segment_session(S)
        bank = wv.open_segment_bank(capacity=S, gated=True)
        assert type(bank) is SegmentBank and type(sess) is SegmentSession and (bank.precision, bank.locator_precision) == (precision, precision)
        sizes = SB.pieces(T, kind, HOP)
        want, at = [[] for _ in range(S)], 0
        for n in sizes:
            sess.push(x[:, at:at + n], gate[:, at:at + n])
            at += n
        for s, segs in enumerate(sess.flush()):
            want[s] += segs
        got = _run_bank(bank, [(x[s], gate[s], sizes) for s in range(S)])
        assert sum(len(w) for w in want) >= 4 and bank.stats["padded_samples"] == 0
        worst = _compare(got, want, (precision, kind), exact_prob=True)          # frames, times, coverage (= count), prob: all equal
        print(f"MEASURE equal pushes {precision} {kind}: {sum(len(w) for w in want)} segments, prob difference {worst:.1e}")
    finally:
        wv.set_precision("f32")


# ================================================================== 3. the mixed schedule on the small session nets against the oracles
PAIRS = [("x6.detector", "x14.locator"), ("x9.detector", "x13.locator"), ("x0.detector", "x0.locator"), ("x13.detector", "x13.locator"),
         ("x14.detector", "x14.locator")]
F16_DETECTORS = ("h.detector", "h.nbits36.detector")
NETS = {c[0]: c for c in W.net_cases()}


@functools.lru_cache(maxsize=None)
def _hip(cid):
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    cfg, seed = W.net_config(NETS[cid])
    if NETS[cid][1] == "f32":
        cfg, sd, _ = W.oracle_net(NETS[cid])
    else:
        sd = random_state_dict(cfg, seed)
    return cfg, sd, HipNet(cfg, sd)


@functools.lru_cache(maxsize=None)
def _mixed_reference(det_id, loc_id):
    """-> (steps, xs, gates, {stream: the whole-recording tracker's events in float64}, hop): computed once for every pad_limit."""
    from waveverify_amd.session import segment_halo
    dcfg, sd, _ = _hip(det_id)
    hop, nb = dcfg.hop_length, dcfg.head_bits
    steps = BK.mixed_schedule(hop, segment_halo(dcfg, _hip(loc_id)[0]))
    xs = {n: W.clip_data(NETS[det_id], max(T, 1), 300 + i)[0][0, 0, :T] for i, (n, T) in enumerate(BK.stream_lengths(steps).items())}
    gates = {n: SB.stream_gate(len(x), hop) for n, x in xs.items()}
    want = {}
    for n, x in xs.items():
        if not x.size:
            want[n] = []
            continue
        if NETS[det_id][1] == "f32":
            whole = frame_sums_ref(W.oracle_forward(dcfg, W.oracle_net(NETS[det_id])[2], x[None, None]), gates[n][None], 0.5, hop, x.size)
        else:
            from oracle import wv_oracle_h16 as O16
            from oracle import wv_oracle_torch as OT
            onet = OT.Net(dcfg, sd)
            if O16.head16_gate(dcfg):
                p = O16.head16_probs(O16.encoder_latent(onet, OT._t(x[None, None]).double(), None), *O16.head_weights(onet))
            else:
                p = sigmoid64(O16.detect_logits(onet, x[None, None]).double().numpy())
            whole = frame_sums_from_probs(p, gates[n][None], 0.5, hop, x.size)
        want[n] = SB.lockstep_events(whole[0], hop, x.size - (whole.shape[2] - 1) * hop, 0.5, 1, 1, dtype=np.float64)
    return steps, xs, gates, want, hop


def _check_mixed(det_id, loc_id, precision, what):
    steps, xs, gates, want, hop = _mixed_reference(det_id, loc_id)
    det, loc = _hip(det_id)[2], _hip(loc_id)[2]
    xt, gt = {n: cu(x) for n, x in xs.items()}, {n: cu(g) for n, g in gates.items()}
    worst, stats = 0.0, []
    for pad in BK.PAD_LIMITS:
        bank = SegmentBank(det, loc, BK.CAPACITY, pad, min_gap_frames=1, min_len_frames=1, ring=4, gated=True, precision=precision)
        got, _ = SB.play(bank, steps, xt, gt, poll_every=3)
        assert bank.open_slots() == []
        stats.append(bank.stats)
        for n, x in xs.items():
            assert [g.frames for g in got[n]] == [(lo, hi) for lo, hi, _, _ in want[n]], (what, pad, n)
            for g, (lo, hi, cnt, prob) in zip(got[n], want[n]):
                end = min(hi * hop, x.size)
                assert g.coverage == cnt / (end - lo * hop) and g.end_s == end / 16000, (what, pad, n, g.frames)       # the count, exactly
                err = float(np.abs(g.prob.astype(np.float64) - prob).max())
                bar = MEAN_BAR if precision == "f32" else det_mean_bar(int(cnt))
                worst = max(worst, err / bar)
                print(f"MEASURE {what} pad_limit {pad} stream {n} segment {g.frames}: prob {err:.2e} (bar {bar:.1e})")
                assert err <= bar, (what, pad, n, g.frames, err, bar)
    assert stats[0]["launches"] > stats[2]["launches"] and stats[0]["padded_samples"] == 0 < stats[2]["padded_samples"]
    assert sum(len(w) for w in want.values()) >= 12
    print(f"MEASURE {what}: worst prob error {worst:.2f} of its bar")


@pytest.mark.parametrize("det_id,loc_id", PAIRS, ids=[d for d, _ in PAIRS])
def test_mixed_schedule_vs_float64(det_id, loc_id):
    assert NETS[det_id][3][1] in BK.SESSION_NETS and NETS[loc_id][3][1] in BK.SESSION_NETS
    _check_mixed(det_id, loc_id, "f32", f"exact {det_id}")


@pytest.mark.parametrize("det_id", F16_DETECTORS)
def test_mixed_schedule_f16_vs_its_oracle(det_id):
    assert det_id in BK.F16_BANKS
    _check_mixed(det_id, "h.locator", "f16", f"f16 {det_id}")


# ================================================================== 4. the gate-mask bank against detect_segments_batch
@pytest.mark.parametrize("pad", BK.PAD_LIMITS)
def test_gate_mask_bank_equals_detect_segments_batch(wv, pad):
    from waveverify_amd.init import synthetic_clips
    Ts = (16001, 9600, 12345)
    kinds = ("ragged", "hop", "whole")
    packets = (HOP // 2, HOP, 3 * HOP)                                           # 10 / 20 / 60 ms
    x = torch.from_numpy(synthetic_clips(3, max(Ts), seed=53)[0][:, 0]).cuda()
    streams, want = [], []
    for s, T in enumerate(Ts):
        gate = torch.zeros(T, device="cuda")
        gate[(3 + s) * HOP: (14 + s) * HOP] = 1
        gate[20 * HOP + 11 * s: T - s * 1000] = 1
        want += wv.detect_segments_batch(x[s:s + 1, None, :T], gate=gate[None])
        sizes = [packets[s]] * (T // packets[s]) + ([T % packets[s]] if T % packets[s] else [])
        streams.append((x[s, :T], gate, sizes if s else SB.pieces(T, kinds[s], HOP)))
    assert [len(w) for w in want] == [2, 2, 2]
    bank = wv.open_segment_bank(capacity=4, pad_limit=pad, gated=True)
    got = _run_bank(bank, streams)
    worst = _compare(got, want, ("gate-mask bank", pad))
    print(f"MEASURE gate-mask bank pad_limit {pad}: prob against detect_segments_batch {worst:.2e}; {bank.stats}")


# ================================================================== 5. the locator-driven bank
def test_locator_driven_bank_equals_detect_segments_batch(wv):
    x = torch.from_numpy(SC.locator_recording()[:, 0]).cuda()
    kw = dict(threshold=SC.LOC_THRESHOLD, min_on=SC.LOC_MIN_ON)
    want = wv.detect_segments_batch(x.unsqueeze(1), **kw)
    bank = wv.open_segment_bank(capacity=2, **kw)
    assert not bank.gated and bank.precision == bank.locator_precision == "f32"
    T = x.shape[1]
    got = _run_bank(bank, [(x[0], None, SB.pieces(T, "hop", HOP)), (x[1], None, SB.pieces(T, "ragged", HOP))])
    assert [[s.frames for s in g] for g in got] == SC.LOC_EXPECTED_FRAMES
    worst = _compare(got, want, "locator-driven bank")
    print(f"MEASURE locator-driven bank: frames {[[s.frames for s in g] for g in got]}, prob against detect_segments_batch {worst:.2e}")


# ================================================================== 6. ring and reuse
def test_ring_two_reuse_and_alone_beside_others(wv):
    L, G, n = 5, 2, 12
    gate_np, frames = SB.ring_gates(HOP, L, G, n, slots=4)
    T = gate_np.shape[1]
    gate = cu(gate_np)
    x = cu(np.random.default_rng(2).standard_normal((4, T)).astype(np.float32) * 0.1)
    sizes = SB.pieces(T, "ragged", HOP)
    bank = wv.open_segment_bank(capacity=4, ring=2, gated=True)
    reads = [0]
    poll = bank._tracker.poll
    bank._tracker.poll = lambda slots: (reads.__setitem__(0, reads[0] + 1), poll(slots))[1]
    beside = _run_bank(bank, [(x[s], gate[s], sizes) for s in range(4)], poll_every=10 ** 9)   # no poll but the bank's own
    assert reads[0] > 4                                                         # it read the rings itself
    assert [[g.frames for g in b] for b in beside] == frames                    # twelve per slot through a ring of two, none lost
    whole = _run_bank(wv.open_segment_bank(capacity=4, ring=2, gated=True), [(x[s], gate[s], [T]) for s in range(4)], poll_every=10 ** 9)
    assert [[g.frames for g in b] for b in whole] == frames                     # one long push: tracked in pieces
    # a stream alone equals the same stream beside three others with equal window lengths
    alone = _run_bank(wv.open_segment_bank(capacity=4, ring=2, gated=True), [(x[1], gate[1], sizes)], poll_every=10 ** 9)
    _compare(alone, [beside[1]], "alone against beside three others", exact_prob=True)
    # slot 0 closed mid-run, reopened: the new stream equals a fresh bank's
    used = wv.open_segment_bank(capacity=2, ring=2, gated=True)
    p = used.open()
    used.push({p: (x[0, :11 * HOP + 5], gate[0, :11 * HOP + 5])})
    assert used.open_segments()[p].frames == (7, 11)
    assert [s.frames for s in used.close(p)] == [(0, 5), (7, 12)]               # the open run comes back from close, the partial frame in it
    got = _run_bank(used, [(x[2], gate[2], sizes)], poll_every=10 ** 9)
    want = _run_bank(wv.open_segment_bank(capacity=2, ring=2, gated=True), [(x[2], gate[2], sizes)], poll_every=10 ** 9)
    _compare(got, want, "reused slot against a fresh bank", exact_prob=True)
    assert [g.frames for g in got[0]] == frames[2]


# ================================================================== 7. lifecycle
def test_lifecycle(wv):
    bank = wv.open_segment_bank(capacity=2, gated=True)
    x, on, off = torch.zeros(HOP, device="cuda"), torch.ones(HOP, device="cuda"), torch.zeros(HOP, device="cuda")
    a, b = bank.open(), bank.open()
    with pytest.raises(RuntimeError, match="slots"):
        bank.open()
    bank.push({a: (x, on)})
    assert bank.open_segments()[a].frames == (0, 1) and bank.open_segments()[b] is None               # an opening shows at once
    bank.push({a: (x, off), b: (x[:7], on[:7])})
    assert bank.open_segments()[a].frames == (0, 1) and bank.poll() == {a: [], b: []}                  # one off frame: still open
    bank.push({a: (x, off)})
    assert bank.open_segments()[a] is None and bank.poll()[a] == []                                    # closed min_gap_frames late; too short to report
    for bad in ({a: x}, {a: (x, on[:-1])}, {a: (x.view(2, -1), on.view(2, -1))}, {5: (x, on)}):
        with pytest.raises(ValueError):
            bank.push(bad)
    assert bank.samples_seen(a) == 3 * HOP and bank.samples_seen(b) == 0
    segs = bank.close(b)                                                        # seven gated samples of seven: one partial frame, too short
    assert segs == [] and bank.open_slots() == [a] and sorted(bank.poll()) == [a] and sorted(bank.open_segments()) == [a]
    assert bank.open() == b
    with pytest.raises(ValueError, match="gated"):
        plain = wv.open_segment_bank(capacity=2)
        plain.push({plain.open(): (x, on)})
    with pytest.raises(ValueError, match="ring"):
        wv.open_segment_bank(ring=0)
    with pytest.raises(RuntimeError, match="min_gap_frames outside"):
        wv.open_segment_bank(min_gap_frames=65)
