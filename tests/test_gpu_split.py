"""Splitting a run where the decoded id changes, on the MI355X: wv_segment_track_split and
wv_bank_segment_track_split against their numpy twins on guarded buffers, against the plain kernels where no rule fires, and the routes
(detect_segments_batch(split=), the file route, SegmentSession, SegmentBank, a native-rate bank) on the small session nets.

Bars.  Kernel against twin: events (lo, hi, flags, count, prob) and the readable state bit for bit.  Routes with a caller's gate against the
float64 oracle's frame sums put through the float64 twin (the f16 mode: its own oracle's): frames, flags and counts equal, prob within 1e-5 on
the exact path (test_gpu_segment_session.BAR) and det_mean_bar(count) in the f16 mode (test_gpu_segment_bank); the margins that make frames
and flags comparable are asserted in test_split_cases_cpu.  A route is also held, bit for bit, to the float32 twin fed the frame sums the GPU
itself computed on the whole clip.  The route nets are untrained (split_cases explains their zeroed head bias): these tests check the
plumbing and the arithmetic, not that an id is decoded.  The locator-driven forms are held to the oracle in the same way on the same
recordings, the locator's threshold in a gap of the oracle's logits (split_cases.LOC_*; the f16 detector behind the exact locator), and
are also compared route against route.  On the full-size random nets no bit's mean crosses 1/2, so no rule fires: the span test asserts it.

Every figure is printed as a MEASURE line before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import segment_bank_cases as SB
import segment_session_cases as SC
import split_cases as X
import window_cases as W
from guard import Guards
from test_gpu_h16 import det_mean_bar
from waveverify_amd import ops
from waveverify_amd.localize import BankSegmentTracker, SegmentTracker, SplitRule
from waveverify_amd.session import HipBankSegmentTracker, HipSegmentTracker, SegmentBank, SegmentSession, bank_track_row_ok

pytestmark = pytest.mark.gpu

BAR = 1e-5
CAP = 5
ARENA = 1 << 15


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poison_rings(state, n, nb):
    """0xFF (NaN) in every ring slot of zeroed state sections: a slot is read only after the kernel wrote it, so this changes nothing."""
    state.view(n, -1)[:, 64 + 8 * (nb + 1):].fill_(0xFF)


# ================================================================== 1. the kernels against their twins
class GuardedSplit(HipSegmentTracker):
    """HipSegmentTracker under a rule with fsum, state and events between guard bands and the unused ring slots poisoned."""

    def __init__(self, fsum, hop, min_on, G, ml, capacity, rule):
        self.g = Guards()
        self.fsum = self.g.input(fsum, "fsum")
        S, nb1, _ = fsum.shape
        sb, eb = ops.segment_split_bytes(S, nb1 - 1, G, rule.window_frames, capacity)
        self._arenas = (self.g.output((sb,), torch.uint8, "state"), self.g.output((eb,), torch.uint8, "events"))
        super().__init__(S, nb1 - 1, hop, min_on, G, ml, capacity, torch.device("cuda", torch.cuda.current_device()))
        self.set_split(rule)

    def _clear(self):
        super()._clear()
        if self.split is not None:
            self.state, self.events = self._arenas[0].t.zero_(), self._arenas[1].t.zero_()
            _poison_rings(self.state, self.S, self.nb)

    def advance(self, fsum, *a, **k):
        super().advance(self.fsum.t, *a, **k)

    def check(self):
        torch.cuda.synchronize()
        self.fsum.check()
        bad = self._arenas[0].guard_report() + self._arenas[1].guard_report()
        assert not bad, bad


def _run_both(twin, dev, fsum, chunks, last_valid, what, state_every=1):
    """Tick by tick: events and the readable state of the device equal the twin's, bit for bit -> the events."""
    out = [[] for _ in range(fsum.shape[0])]
    for i, (lo, hi) in enumerate(chunks):
        final = i == len(chunks) - 1
        lv = last_valid if final and hi == fsum.shape[2] and hi > lo else twin.hop
        twin.advance(fsum, lo, hi, lv, final)
        dev.advance(fsum, lo, hi, lv, final)
        if i % state_every == 0 or final:
            a, b = twin.poll(), dev.poll()
            diff = X.same_events(b, a)
            assert diff is None, (what, i, diff)
            for s, evs in enumerate(a):
                out[s] += evs
            for s, (u, (_, v)) in enumerate(zip(twin.split_state(), dev.split_state(range(fsum.shape[0])))):
                assert X.same_state(v, u) is None, (what, i, s, X.same_state(v, u))
            for u, v in zip(twin.open_runs(), dev.open_runs()):
                assert (u is None) == (v is None) and (u is None or (u[:3] == v[:3] and u[3].tobytes() == v[3].tobytes() and u[4] == v[4])), (what, i)
    return out


@pytest.mark.parametrize("nb", (4, 16))
def test_split_kernel_equals_the_twin_on_the_synthetic_cases(nb):
    n_launch = n_events = 0
    for Wf in (3, 4, 5, 6):
        for case in X.synthetic_cases(nb, Wf):
            f = case["fsum"][None]
            args = (X.HOP, case["min_on"], case["G"], case["ml"])
            whole = SC.run_tracker(SegmentTracker(1, nb, *args, split=case["rule"]), f, [(0, f.shape[2])], case["last_valid"])
            assert [(e[0], e[1], e[4]) for e in whole[0]] == [w[:3] for w in case["want"]]
            cuts = [e[1] for e in whole[0] if e[4][1]]
            parts = X.partitions(f.shape[2], cuts, Wf, ("gpu", nb, Wf, case["name"]), case["last_valid"] < X.HOP)
            for name in [p for p in parts if not p.startswith("random") or p == "random0"]:
                dev = GuardedSplit(f, *args, 8, case["rule"])
                got = _run_both(SegmentTracker(1, nb, *args, split=case["rule"]), dev, f, parts[name], case["last_valid"], (Wf, case["name"], name))
                dev.check()
                assert X.same_events(got, whole) is None
                n_launch += len(parts[name])
                n_events += len(got[0])
    print(f"MEASURE split tracker on the synthetic cases nb={nb}: {n_launch} launches, {n_events} events, events and state bit-equal to the twin")
    assert n_events > 0


@pytest.mark.parametrize("Wf,G", [(2, 1), (5, 2), (25, 4)])
@pytest.mark.parametrize("S,nb", [(1, 4), (3, 16)])
def test_split_kernel_equals_the_twin_on_random_frame_sums(S, nb, Wf, G):
    hop, ml, rule = 10, min(Wf, 5), SplitRule(Wf, 0.3, 1)
    n_launch = n_events = n_cuts = 0
    for seed in range(2):
        fsum, lv = X.random_fsum(S, nb, 120 if Wf < 25 else 200, Wf, G, hop, seed)
        Fr = fsum.shape[2]
        whole = SC.run_tracker(SegmentTracker(S, nb, hop, 0.5, G, ml, split=rule), fsum, [(0, Fr)], lv)
        cuts = [e[1] for e in whole[0] if e[4][1]][:1]
        parts = X.partitions(Fr, cuts, Wf, ("gpu-rand", S, nb, Wf, seed), lv < hop)
        for name in ("whole", "frames", "random0") + tuple(p for p in parts if p.startswith("all@")):
            dev = GuardedSplit(fsum, hop, 0.5, G, ml, 64, rule)
            got = _run_both(SegmentTracker(S, nb, hop, 0.5, G, ml, split=rule), dev, fsum, parts[name], lv, (seed, name), state_every=7)
            dev.check()
            assert X.same_events(got, whole) is None, (seed, name)
            n_launch += len(parts[name])
            n_events += sum(len(g) for g in got)
            n_cuts += sum(e[4][1] for g in got for e in g)
    print(f"MEASURE split tracker S={S} nb={nb} W={Wf} G={G}: {n_launch} launches, {n_events} events, {n_cuts} cuts, all bit-equal to the twin")
    assert n_cuts > 0


class GuardedSplitBank(HipBankSegmentTracker):
    """HipBankSegmentTracker under a rule with fsum, desc, state and events between guard bands, ring slots poisoned."""

    def __init__(self, nb, hop, min_on, G, ml, ring, rule):
        super().__init__(CAP, nb, hop, min_on, G, ml, ring, torch.device("cuda", torch.cuda.current_device()))
        self.set_split(rule)
        self.g = Guards()
        self._fsum = self.g.output((ARENA,), torch.float32, "fsum")
        self._desc = self.g.output((CAP + 16, 8), torch.int64, "desc")
        self._state = self.g.output((self.state.numel(),), torch.uint8, "state")
        self._events = self.g.output((self.events.numel(),), torch.uint8, "events")
        self.state, self.events = self._state.t.zero_(), self._events.t.zero_()
        _poison_rings(self.state, CAP, nb)

    def tick(self, arena, desc):
        assert arena.size <= ARENA and len(desc) <= CAP + 16
        self._fsum.t.fill_(float("nan"))
        self._fsum.t[:arena.size].copy_(cu(arena))
        self._desc.t[:len(desc)].copy_(cu(np.asarray(desc, np.int64).reshape(-1, 8)))
        before = (self.state.clone(), self.events.clone())
        self.advance(self._fsum.t[:arena.size], self._desc.t, len(desc))
        return before

    def untouched(self, before, named):
        changed = ((self.state != before[0]).view(CAP, -1).any(1) | (self.events != before[1]).view(CAP, -1).any(1)).cpu().numpy()
        assert not set(np.flatnonzero(changed).tolist()) - set(named), (np.flatnonzero(changed), named)

    def check(self):
        torch.cuda.synchronize()
        bad = [m for a in self.g.arenas for m in a.guard_report()]
        assert not bad, bad


def _bank_streams(nb, Wf, G, hop, rng, seed):
    """Four streams of unequal lengths on scattered slots that start at different ticks; slot 3's stream is empty (a final tick alone)."""
    out = []
    for i, (slot, Fr) in enumerate(((4, 90), (0, 61), (2, 37))):
        fsum, lv = X.random_fsum(1, nb, Fr, Wf, G, hop, seed + i)
        out.append((slot, fsum[0], lv, SC.chunks_of(Fr, "random", rng, lv < hop), i))
    out.append((3, np.zeros((nb + 1, 0), np.float32), hop, [(0, 0)], 1))
    return out


@pytest.mark.parametrize("nb,Wf,G", [(4, 2, 1), (16, 5, 2), (16, 5, 4)])
def test_split_bank_kernel_equals_the_twin(nb, Wf, G):
    hop, ml, rule = 10, min(Wf, 5), SplitRule(Wf, 0.3, 1)
    n_ticks = n_events = n_cuts = n_final = 0
    for seed in range(2):
        rng = np.random.default_rng(SC.seed_of("gpu-split-bank", nb, Wf, G, seed))
        batch = _bank_streams(nb, Wf, G, hop, rng, 10 * seed)
        slots = [b[0] for b in batch]
        twin, dev = BankSegmentTracker(CAP, nb, hop, 0.5, G, ml, ring=32, split=rule), GuardedSplitBank(nb, hop, 0.5, G, ml, 32, rule)
        got = {s: [] for s in slots}
        for arena, desc in SB.bank_ticks(batch, nb, hop, rng):
            assert all(bank_track_row_ok(r, CAP, nb, hop, arena.size) for r in desc)
            n_final += sum(1 for r in desc if r[7])
            twin.advance(arena, desc)
            before = dev.tick(arena, desc)
            dev.untouched(before, [int(r[0]) for r in desc])
            a, b = twin.poll(slots), dev.poll(slots)
            st_a, st_b = twin.split_state(slots), dict(dev.split_state(slots))
            for s in slots:
                assert X.same_events([b[s]], [a[s]]) is None, (seed, s, X.same_events([b[s]], [a[s]]))
                assert X.same_state(st_b[s], st_a[s]) is None, (seed, s, X.same_state(st_b[s], st_a[s]))
                got[s] += a[s]
            n_ticks += 1
        dev.check()
        for slot, fsum, lv, _, _ in batch:                               # and each slot is the lockstep twin on its whole array
            if fsum.shape[1]:
                whole = SC.run_tracker(SegmentTracker(1, nb, hop, 0.5, G, ml, split=rule), fsum[None], [(0, fsum.shape[1])], lv)
                assert X.same_events([got[slot]], whole) is None
        n_events += sum(len(g) for g in got.values())
        n_cuts += sum(e[4][1] for g in got.values() for e in g)
    print(f"MEASURE split bank nb={nb} W={Wf} G={G}: {n_ticks} launches, {n_events} events, {n_cuts} cuts, {n_final} final rows, bit-equal to the twin")
    assert n_cuts > 0 and n_final >= 8


def test_split_bank_skips_bad_rows_and_takes_garbage_as_closed():
    hop, nb, G, ml, rule = 10, 16, 2, 5, SplitRule(5, 0.3, 1)
    rng = np.random.default_rng(11)
    twin, dev = BankSegmentTracker(CAP, nb, hop, 0.5, G, ml, ring=16, split=rule), GuardedSplitBank(nb, hop, 0.5, G, ml, 16, rule)
    ss, es = dev._strides
    dev.state[1 * ss:2 * ss].fill_(0xFF)                                 # slot 1 was never cleared: open = -1, lo = hi = plo = -1, NaN sums
    dev.events[1 * es:2 * es].fill_(0xFF)
    fa, lva = X.random_fsum(1, nb, 70, 5, G, hop, 3)
    fb, lvb = X.random_fsum(1, nb, 50, 5, G, hop, 4)
    batch = [(1, fa[0], lva, [(0, 33), (33, 70)], 0), (4, fb[0], lvb, [(0, 20), (20, 50)], 0)]
    for arena, desc in SB.bank_ticks(batch, nb, hop, rng):
        good = [2] + [int(v) for v in desc[0][1:]]
        bads = [b for _, b in SB.bad_track_rows(good, CAP, nb, hop, arena.size) if b[0] == 2]
        assert len(bads) >= 10 and not any(bank_track_row_ok(b, CAP, nb, hop, arena.size) for b in bads)
        desc = np.concatenate([np.array(bads[:5], np.int64), desc, np.array(bads[5:], np.int64)])
        twin.advance(arena, desc)
        before = dev.tick(arena, desc)
        dev.untouched(before, [1, 4])                                     # slot 2, named by the bad rows alone, among the untouched
    dev.check()
    a, b = twin.poll([1, 4]), dev.poll([1, 4])
    assert len(a[1]) >= 2 and len(a[4]) >= 2
    assert X.same_events([b[1], b[4]], [a[1], a[4]]) is None
    # a header that says "open" with a pending cut outside the piece: closed, and the tick is a fresh tracker's
    dev2 = GuardedSplit(fa, hop, 0.5, G, ml, 16, rule)
    hdr = np.array([1, 0, 40, 40, 0, 1, 39], np.int64)                    # cg = 39 > hi - W
    dev2.state[:56].copy_(cu(hdr.view(np.uint8)))
    dev2.frames_seen = 40
    dev2.advance(fa, 40, 70, lva, True)
    dev2.check()
    want = SegmentTracker(1, nb, hop, 0.5, G, ml, split=rule)
    want.frames_seen = 40
    want.advance(fa, 40, 70, lva, True)
    assert X.same_events(dev2.poll(), want.poll()) is None


def test_split_refusals_leave_the_buffers_untouched():
    nb, hop, rule = 16, 10, SplitRule(5, 0.5, 1)
    sb, eb = ops.segment_split_bytes(4, nb, 2, 5, 8)
    g = Guards()
    state, events = g.output((sb,), torch.uint8, "state"), g.output((eb,), torch.uint8, "events")
    st, ev = state.t.zero_(), events.t.zero_()
    fsum = torch.ones((4, 17, 4), device="cuda")
    desc = cu(np.array([[1, 0, 4, 0, 4, 0, hop, 0]], np.int64))
    bank = dict(fsum=fsum.reshape(-1), desc=desc, P=1, capacity=4, nb=nb, hop=hop, min_on=0.5, min_gap_frames=2, min_len_frames=5, rule=rule,
                state=st, events=ev, ring=8)
    lock = dict(fsum=fsum, f_lo=0, f_hi=4, frame0=0, hop=hop, last_valid=hop, final=False, min_on=0.5, min_gap_frames=2, min_len_frames=5,
                rule=rule, state=st, events=ev, capacity=8)
    R = lambda **k: type("R", (), {**dict(window_frames=5, threshold=0.5, min_bits=1), **k})   # a rule the dataclass would refuse
    common = ((dict(min_gap_frames=0), "min_gap_frames outside"), (dict(min_gap_frames=65), "min_gap_frames outside"),
              (dict(min_len_frames=-1), "min_len_frames < 0"), (dict(min_on=float("nan")), "not a number"),
              (dict(rule=R(window_frames=1)), "window_frames outside"), (dict(rule=R(window_frames=257)), "window_frames outside"),
              (dict(min_len_frames=6), "window_frames outside"), (dict(min_gap_frames=6), "window_frames outside"),
              (dict(rule=R(threshold=0.0)), "threshold not above 0"), (dict(rule=R(threshold=float("nan"))), "threshold not above 0"),
              (dict(rule=R(min_bits=0)), "min_bits outside"), (dict(rule=R(min_bits=17)), "min_bits outside"),
              (dict(state=st[:-8]), "shorter than"), (dict(events=ev[:-8]), "shorter than"), (dict(state=st[1:]), "8-byte aligned"),
              (dict(rule=R(window_frames=6)), "shorter than"))
    for base, fn, name, more in ((bank, ops.bank_segment_track_split, "wv_bank_segment_track_split",
                                  ((dict(capacity=0), "capacity outside"), (dict(nb=0), "nb outside"), (dict(nb=256), "nb outside"),
                                   (dict(hop=0), "hop < 1"), (dict(ring=0), "ring < 1"), (dict(capacity=5), "shorter than"),
                                   (dict(ring=9), "shorter than"))),
                                 (lock, ops.segment_track_split, "wv_segment_track_split",
                                  ((dict(f_hi=5), "outside"), (dict(last_valid=11), "last_valid"), (dict(capacity=0), "capacity"),
                                   (dict(frame0=-1), "frame0 < 0"), (dict(capacity=9), "shorter than")))):
        for kw, what in common + more:
            with pytest.raises(RuntimeError, match=name + ".*" + what):
                fn(**{**base, **kw})
    ops.bank_segment_track_split(**{**bank, "P": 0})                      # success without a launch
    ops.segment_track_split(**{**lock, "f_hi": 0})
    from waveverify_amd import _lib
    lib, stream = _lib.load(), _lib.stream()
    raw = lambda a: lib.wv_bank_segment_track_split(a[0], a[1], a[2], a[3], 4, nb, hop, 0.5, 2, 5, 1e-8, 5, 0.5, 1, a[4], sb, a[5], eb, 8, stream)
    args = [fsum.data_ptr(), fsum.numel(), desc.data_ptr(), 1, st.data_ptr(), ev.data_ptr()]
    for i, v, what in ((0, None, "frame sums without fsum"), (2, None, "null desc"), (4, None, "null desc, state"),
                       (5, None, "null desc, state or events"), (1, -1, "n_fsum < 0"), (3, -1, "P outside"), (3, 65536, "P outside")):
        a = list(args)
        a[i] = v
        assert raw(a) == -1
        msg = lib.wv_last_error().decode()
        assert msg.startswith("wv_bank_segment_track_split:") and what in msg, (i, msg)
    torch.cuda.synchronize()
    assert not state.guard_report() + events.guard_report()
    assert int(st.count_nonzero()) == 0 and int(ev.count_nonzero()) == 0     # nothing was written by any refused call
    assert raw(args) == 0
    with pytest.raises(RuntimeError, match=r"wv_segment_split_bytes.*\[1, 65535\]"):
        ops.segment_split_bytes(65536, 16, 2, 5, 4)


# ================================================================== 2. where no rule fires: the existing kernels, bit for bit
@pytest.mark.parametrize("nb", SC.NBS)
@pytest.mark.parametrize("S", [1, 3])
def test_a_rule_that_never_fires_gives_the_plain_kernels_events(S, nb):
    hop, min_on, dev = 10, 0.5, torch.device("cuda", torch.cuda.current_device())
    n_events = 0
    for G, ml in ((2, 5), (1, 1), (5, 5), (3, 1)):
        rule = SplitRule(max(2, G, ml), 1e9, 1)
        for salt in range(6):
            names, fsum, lv = SC.stream_patterns(S, hop, min_on, G, ml, nb, salt)
            chunks = SC.chunks_of(fsum.shape[2], SC.CHUNKINGS[salt % 3], np.random.default_rng(salt), lv < hop)
            f = cu(fsum)
            plain = SC.run_tracker(HipSegmentTracker(S, nb, hop, min_on, G, ml, 16, dev), f, chunks, lv)
            split = HipSegmentTracker(S, nb, hop, min_on, G, ml, 16, dev)
            split.set_split(rule)
            got = SC.run_tracker(split, f, chunks, lv)
            assert SC.same_events(got, plain) is None, (names, G, ml, SC.same_events(got, plain))
            assert all(e[4] == (False, False) for g in got for e in g)
            # the bank form, every stream a slot with the same ticks
            b_plain, b_split = HipBankSegmentTracker(S, nb, hop, min_on, G, ml, 16, dev), HipBankSegmentTracker(S, nb, hop, min_on, G, ml, 16, dev)
            b_split.set_split(rule)
            Fr = fsum.shape[2]
            for i, (lo, hi) in enumerate(chunks):
                final = i == len(chunks) - 1
                desc = cu(np.array([[s, s * (nb + 1) * Fr, Fr, lo, hi, lo, lv if final and hi == Fr and hi > lo else hop, int(final)]
                                    for s in range(S)], np.int64))
                b_plain.advance(f.reshape(-1), desc)
                b_split.advance(f.reshape(-1), desc)
            a, b = b_plain.poll(range(S)), b_split.poll(range(S))
            assert SC.same_events([b[s] for s in range(S)], [a[s] for s in range(S)]) is None
            assert SC.same_events([a[s] for s in range(S)], plain) is None
            n_events += sum(len(g) for g in got)
    print(f"MEASURE never-firing rule S={S} nb={nb}: {n_events} events equal to wv_segment_track's and wv_bank_segment_track's, bit for bit")
    assert n_events > 0


# ================================================================== 3. the routes on the small session nets
NETS = {c[0]: c for c in W.net_cases()}


@functools.lru_cache(maxsize=None)
def _route(det_id):
    """-> (WaveVerify on the route's detector and its locator, x, gate on the device, the oracle's events, precision)."""
    from waveverify_amd import WaveVerify
    from waveverify_amd.init import random_state_dict
    cfg, sd, x, gate, whole = X.route_reference(det_id)
    events, _ = X.route_events(det_id, whole)
    loc_case = NETS[X.ROUTE_LOCATORS[det_id]]
    lcfg, lseed = W.net_config(loc_case)
    lsd = W.oracle_net(loc_case)[1] if loc_case[1] == "f32" else random_state_dict(lcfg, lseed)
    wv = WaveVerify.__new__(WaveVerify)
    wv.device = torch.device("cuda", torch.cuda.current_device())
    wv._build({"detector": sd, "locator": lsd}, {"detector": cfg, "locator": lcfg})
    wv.sample_rate, wv.watermark_bits = 16000, 16
    precision = NETS[det_id][1]
    wv.set_precision(precision)
    return wv, cu(x), cu(gate), events, precision


def _against_oracle(got, events, hop, T, precision, what):
    """Frames and flags equal; the count exactly; prob within the bar -> the worst prob error over its bar."""
    worst = 0.0
    assert len(got) == len(events)
    for s, (g, w) in enumerate(zip(got, events)):
        assert [(a.frames, a.change) for a in g] == [((e[0], e[1]), e[4]) for e in w], (what, s, [(a.frames, a.change) for a in g])
        for a, (lo, hi, cnt, prob, _) in zip(g, w):
            end = min(hi * hop, T)
            assert a.coverage == cnt / (end - lo * hop) and a.end_s == end / 16000 and a.start_s == lo * hop / 16000, (what, s, a.frames)
            err = float(np.abs(a.prob.astype(np.float64) - prob).max())
            bar = BAR if precision == "f32" else det_mean_bar(int(cnt))
            print(f"MEASURE {what} stream {s} piece {a.frames} {a.change}: prob {err:.2e} (bar {bar:.1e})")
            assert err <= bar, (what, s, a.frames, err, bar)
            worst = max(worst, err / bar)
    return worst


def _same_segments(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [(a.frames, a.change, a.start_s, a.end_s, a.coverage, a.confidence) for a in g] == \
               [(a.frames, a.change, a.start_s, a.end_s, a.coverage, a.confidence) for a in w], (what, g, w)
        assert all(a.prob.tobytes() == b.prob.tobytes() and a.watermark == b.watermark for a, b in zip(g, w)), what


def _close_segments(got, want, what):
    """Frames, flags and times equal, prob within BAR: two routes whose windows differ (a flush runs the partial last frame on its own)."""
    assert len(got) == len(want)
    worst = 0.0
    for g, w in zip(got, want):
        assert [(a.frames, a.change, a.start_s, a.end_s) for a in g] == [(a.frames, a.change, a.start_s, a.end_s) for a in w], (what, g, w)
        for a, b in zip(g, w):
            worst = max(worst, float(np.abs(a.prob.astype(np.float64) - b.prob.astype(np.float64)).max()))
    print(f"MEASURE {what}: prob difference {worst:.2e}")
    assert worst <= BAR, (what, worst)


def _twin_on_gpu_sums(wv, x, gate, rule, kw):
    """The float32 twin fed the frame sums the GPU computes on the whole clips -> its events."""
    det = wv._need("detector")
    g, thr = wv._gate(x[:, None], kw.get("threshold", 0.5), gate)
    fsum = det.detector_frame_sums(x[:, None], g, thr, wv.detector_precision).cpu().numpy()
    hop, T = det.hop_length, x.shape[1]
    t = SegmentTracker(fsum.shape[0], fsum.shape[1] - 1, hop, kw.get("min_on", 0.5), X.ROUTE_G, X.ROUTE_ML, split=rule)
    t.advance(fsum, 0, fsum.shape[2], T - (fsum.shape[2] - 1) * hop, True)
    return t.poll()


def _push_all(sess, x, gate, sizes, poll_every=3):
    got, at = [[] for _ in range(x.shape[0])], 0
    for i, n in enumerate(sizes):
        sess.push(x[:, at:at + n], None if gate is None else gate[:, at:at + n])
        at += n
        if i % poll_every == poll_every - 1:
            for s, segs in enumerate(sess.poll()):
                got[s] += segs
    for s, segs in enumerate(sess.flush()):
        got[s] += segs
    return got


@pytest.mark.parametrize("det_id", X.ROUTE_NETS + X.ROUTE_F16)
def test_gated_routes_against_the_oracle(det_id):
    wv, x, gate, events, precision = _route(det_id)
    rule, kw = X.route_rule(det_id), dict(min_gap_frames=X.ROUTE_G, min_len_frames=X.ROUTE_ML)
    det, loc = wv._need("detector"), wv._need("locator")
    hop, (S, T) = det.hop_length, x.shape
    assert sum(e[4][1] for evs in events for e in evs) >= S                  # every stream's run is cut on the oracle
    # the batch route: one launch for all clips
    batch = wv.detect_segments_batch(x[:, None], gate=gate, split=rule, **kw)
    worst = _against_oracle(batch, events, hop, T, precision, f"{det_id} batch")
    plain = wv.detect_segments_batch(x[:, None], gate=gate, **kw)
    assert [[a.frames for a in p] for p in plain] == [[X.ROUTE_ON]] * S       # without a rule: one segment, the whole stretch
    twin = _twin_on_gpu_sums(wv, x, gate, rule, {})
    for b, evs in zip(batch, twin):                                           # and bit for bit the f32 twin on the GPU's own sums
        assert [(a.frames, a.change) for a in b] == [((e[0], e[1]), e[4]) for e in evs]
        assert all(a.prob.tobytes() == e[3].tobytes() for a, e in zip(b, evs))
    # the live session, three partitions of the samples
    for kind in ("whole", "hop", "ragged"):
        sess = SegmentSession(det, loc, S, precision=precision, **kw)
        sess.set_split(rule)
        got = _push_all(sess, x, gate, SB.pieces(T, kind, hop))
        worst = max(worst, _against_oracle(got, events, hop, T, precision, f"{det_id} session {kind}"))
        if kind == "whole":
            _close_segments(got, batch, "a session fed the clip in one push against the batch route")
        if kind == "ragged":
            lockstep = got
    # the bank: equal pushes are the lockstep session, bit for bit
    bank = SegmentBank(det, loc, S, gated=True, precision=precision, **kw)
    bank.set_split(rule)
    slots = [bank.open() for _ in range(S)]
    got, at = [[] for _ in range(S)], 0
    for i, n in enumerate(SB.pieces(T, "ragged", hop)):
        bank.push({slots[s]: (x[s, at:at + n], gate[s, at:at + n]) for s in range(S)})
        at += n
        if i % 3 == 2:
            for s, segs in bank.poll().items():
                got[slots.index(s)] += segs
    mid = bank.open_segments()
    assert all(v is None for v in mid.values())                               # the stretch ended before the recording did
    for s in range(S):
        got[s] += bank.close(slots[s])
    _same_segments(got, lockstep, "bank with equal pushes against the lockstep session")
    worst = max(worst, _against_oracle(got, events, hop, T, precision, f"{det_id} bank"))
    # unequal pushes: slot by slot still the oracle's pieces
    bank = SegmentBank(det, loc, S, gated=True, precision=precision, **kw)
    bank.set_split(rule)
    slots = [bank.open() for _ in range(S)]
    sizes = [SB.pieces(T, ("hop", "ragged")[s % 2], hop) for s in range(S)]
    at, got = [0] * S, [[] for _ in range(S)]
    for i in range(max(len(z) for z in sizes)):
        items = {}
        for s in range(S):
            if i < len(sizes[s]):
                items[slots[s]] = (x[s, at[s]:at[s] + sizes[s][i]], gate[s, at[s]:at[s] + sizes[s][i]])
                at[s] += sizes[s][i]
        bank.push(items)
    for s in range(S):
        got[s] += bank.close(slots[s])
    worst = max(worst, _against_oracle(got, events, hop, T, precision, f"{det_id} bank, unequal pushes"))
    print(f"MEASURE {det_id} ({precision}): worst prob error {worst:.2f} of its bar")


@pytest.mark.parametrize("det_id", X.ROUTE_NETS + X.ROUTE_F16)
def test_locator_driven_routes_against_the_oracle(det_id):
    """No caller's gate: the locator decides every sample (threshold in a gap of the oracle's logits) and, at min_on = 0.5, every frame.
    Batch route, session and bank under three partitions against the oracle's locator-gated frame sums put through the float64 twin."""
    wv, x, _, _, precision = _route(det_id)
    cfg, sd, lcfg, lsd, x_np, lg, whole = X.loc_reference(det_id)
    events, _ = X.loc_events(det_id, whole)
    assert np.array_equal(x_np, x.cpu().numpy())
    rule = X.loc_rule(det_id)
    kw = dict(threshold=X.LOC_P[det_id], min_on=X.LOC_MIN_ON, min_gap_frames=X.ROUTE_G, min_len_frames=X.ROUTE_ML)
    det, loc = wv._need("detector"), wv._need("locator")
    hop, (S, T) = det.hop_length, x.shape
    assert sum(e[4][1] for evs in events for e in evs) >= 1
    before = wv.locator_precision
    wv.locator_precision = "f32"                                              # the exact locator, also behind the f16 detector (split_cases)
    try:
        batch = wv.detect_segments_batch(x[:, None], split=rule, **kw)
        worst = _against_oracle(batch, events, hop, T, precision, f"{det_id} locator-driven batch")
        lockstep = None
        for kind in ("whole", "hop", "ragged"):
            sess = SegmentSession(det, loc, S, precision=precision, locator_precision="f32", **kw)
            sess.set_split(rule)
            got = _push_all(sess, x, None, SB.pieces(T, kind, hop))
            worst = max(worst, _against_oracle(got, events, hop, T, precision, f"{det_id} locator-driven session {kind}"))
            lockstep = got
        for kinds in (("ragged", "ragged"), ("hop", "ragged"), ("whole", "hop")):
            bank = SegmentBank(det, loc, S, gated=False, precision=precision, locator_precision="f32", **kw)
            bank.set_split(rule)
            slots = [bank.open() for _ in range(S)]
            sizes = [SB.pieces(T, kinds[s % 2], hop) for s in range(S)]
            at, got = [0] * S, [[] for _ in range(S)]
            for i in range(max(len(z) for z in sizes)):
                items = {}
                for s in range(S):
                    if i < len(sizes[s]):
                        items[slots[s]] = x[s, at[s]:at[s] + sizes[s][i]]
                        at[s] += sizes[s][i]
                bank.push(items)
                if i % 4 == 3:
                    for slot, segs in bank.poll().items():
                        got[slots.index(slot)] += segs
            for s in range(S):
                got[s] += bank.close(slots[s])
            worst = max(worst, _against_oracle(got, events, hop, T, precision, f"{det_id} locator-driven bank {kinds}"))
            if kinds == ("ragged", "ragged"):
                _same_segments(got, lockstep, "locator-driven bank with equal pushes against the lockstep session")
    finally:
        wv.locator_precision = before
    print(f"MEASURE {det_id} locator-driven ({precision} detector, exact locator): worst prob error {worst:.2f} of its bar")


def test_a_native_session_refuses_set_split_after_its_first_push():
    """Also after a push that releases no 16 kHz sample yet: the front stage hands the inner session an empty push."""
    det_id = X.ROUTE_NETS[0]
    wv, x, _, _, _ = _route(det_id)
    rule = X.route_rule(det_id)
    sess = wv.open_segment_session(1, sample_rate=48000, channels=2, min_gap_frames=X.ROUTE_G, min_len_frames=X.ROUTE_ML)
    sess.set_split(rule)
    sess.set_split(None)
    sess.set_split(rule)
    sess.push(torch.zeros((1, 2, 1), device=x.device))
    with pytest.raises(RuntimeError, match="before the first push"):
        sess.set_split(None)
    sess.reset()
    sess.set_split(rule)


def test_open_segments_is_the_current_piece_and_set_split_is_refused_after_a_push():
    det_id = X.ROUTE_NETS[0]
    wv, x, gate, events, precision = _route(det_id)
    rule, kw = X.route_rule(det_id), dict(min_gap_frames=X.ROUTE_G, min_len_frames=X.ROUTE_ML)
    det, loc = wv._need("detector"), wv._need("locator")
    hop = det.hop_length
    cut = events[0][0][1]                                                     # stream 0's first cut on the oracle
    sess = SegmentSession(det, loc, x.shape[0], **kw)
    sess.set_split(rule)
    n = (cut + 2 * X.ROUTE_W - 1) * hop                                       # one frame short of knowing it
    sess.push(x[:, :n], gate[:, :n])
    assert sess.open_segments()[0].frames == (X.ROUTE_ON[0], cut + 2 * X.ROUTE_W - 1) and sess.poll()[0] == []
    with pytest.raises(RuntimeError, match="before the first push"):
        sess.set_split(None)
    sess.push(x[:, n:n + hop], gate[:, n:n + hop])
    piece = sess.open_segments()[0]
    assert piece.frames == (cut, cut + 2 * X.ROUTE_W) and piece.change == (True, False)
    assert [(s.frames, s.change) for s in sess.poll()[0]] == [((X.ROUTE_ON[0], cut), (False, True))]
    bank = SegmentBank(det, loc, 2, gated=True, **kw)
    bank.set_split(rule)
    bank.open()
    with pytest.raises(RuntimeError, match="first open"):
        bank.set_split(None)
    with pytest.raises(ValueError, match="window_frames"):
        SegmentSession(det, loc, 1, min_len_frames=6).set_split(rule)
    with pytest.raises(ValueError, match="window_frames"):
        wv.detect_segments_batch(x[:, None], gate=gate, min_len_frames=6, split=rule)


def test_locator_driven_routes_agree_with_each_other(tmp_path):
    """File route, batch route, windowed route and one-push sessions on the small exact nets against each other, the locator gating
    (min_on = 0: every frame is on, so the whole clip is one run whatever the locator marks).  A flush runs the partial last frame as a window
    of its own, so a one-push session is compared within BAR in prob, frames, flags and times equal."""
    from waveverify_amd.utils import load_audio, save_audio
    det_id = X.ROUTE_NETS[0]
    wv, x, _, _, _ = _route(det_id)
    rule = X.route_rule(det_id)
    kw = dict(min_on=0.0, min_gap_frames=X.ROUTE_G, min_len_frames=X.ROUTE_ML)
    det, loc = wv._need("detector"), wv._need("locator")
    hop = det.hop_length
    path = str(tmp_path / "clip.wav")
    save_audio(x[0].cpu()[None], path, 16000)
    audio = load_audio(path, 16000)[0].to(x.device)
    if audio.dim() == 1:
        audio = audio[None]
    audio = audio[:1]
    T = audio.shape[-1]
    batch = wv.detect_segments_batch(audio[:, None], split=rule, **kw)
    twin = _twin_on_gpu_sums(wv, audio, None, rule, kw)
    assert [(a.frames, a.change) for a in batch[0]] == [((e[0], e[1]), e[4]) for e in twin[0]]
    assert all(a.prob.tobytes() == e[3].tobytes() for a, e in zip(batch[0], twin[0]))
    print(f"MEASURE locator-driven batch route: pieces {[(a.frames, a.change) for a in batch[0]]}")
    assert len(batch[0]) >= 2 and batch[0][0].frames[0] == 0 and batch[0][-1].frames[1] == -(-T // hop)
    sess = SegmentSession(det, loc, 1, **kw)
    sess.set_split(rule)
    sess.push(audio)
    _close_segments(sess.flush(), batch, "one-push session against the batch route")
    # WaveVerify.segments: the defaults of detect_segments_batch, so on these nets whatever the locator's runs are; the same through a session
    file_segs = wv.segments(path, split=SplitRule(5, rule.threshold, 1))
    sess = wv.open_segment_session(1)
    sess.set_split(SplitRule(5, rule.threshold, 1))
    sess.push(audio)
    _close_segments(sess.flush(), [file_segs], "file route against a session fed the clip in one push")
    # the windowed long-form route: frames and flags equal, prob within the windowed bar
    from waveverify_amd.session import segment_halo
    win = wv.detect_segments_clips(audio[:, None], window_seconds=(segment_halo(det.cfg, loc.cfg) + 6 * hop) / 16000, split=rule, **kw)
    assert [(a.frames, a.change) for a in win[0]] == [(a.frames, a.change) for a in batch[0]]
    err = max(float(np.abs(a.prob - b.prob).max()) for a, b in zip(win[0], batch[0]))
    print(f"MEASURE windowed route against the batch route: prob {err:.2e}")
    assert err <= BAR


def test_native_48k_stereo_bank_under_a_rule():
    """A native-rate bank at 48 kHz stereo, one push and close, against the batch route on to_model_rate of the recording."""
    det_id = X.ROUTE_NETS[0]
    wv, x, _, _, _ = _route(det_id)
    rule = X.route_rule(det_id)
    kw = dict(min_on=0.0, min_gap_frames=X.ROUTE_G, min_len_frames=X.ROUTE_ML)
    hop = wv._need("detector").hop_length
    left = torch.repeat_interleave(x[0], 3)
    xn = torch.stack([left, 0.5 * left])                                      # [2, 3 T]
    m16 = wv.to_model_rate(xn[None], 48000)[:, 0]
    want = wv.detect_segments_batch(m16[:, None], split=rule, **kw)
    bank = wv.open_native_segment_bank([48000], capacity=2, **kw)
    bank.set_split(rule)
    slot = bank.open(sample_rate=48000, channels=2)
    with pytest.raises(RuntimeError, match="first open"):
        bank.set_split(None)
    half = xn.shape[1] // 2
    bank.push({slot: xn[:, :half]})
    bank.push({slot: xn[:, half:]})
    got = bank.close(slot)
    print(f"MEASURE native 48 kHz stereo bank: pieces {[(a.frames, a.change) for a in got]} against {[(a.frames, a.change) for a in want[0]]}")
    assert [(a.frames, a.change) for a in got] == [(a.frames, a.change) for a in want[0]] and len(got) >= 2
    err = max(float(np.abs(a.prob - b.prob).max()) for a, b in zip(got, want[0]))
    print(f"MEASURE native 48 kHz stereo bank: prob against the batch route {err:.2e}")
    assert err <= BAR


# ================================================================== 4. the full-size nets: span embedding meets split detection
def test_embed_spans_then_detect_segments_with_a_rule():
    """Two abutting spans with different ids, then detect_segments_batch(split=).  With random full-size nets this checks plumbing, not
    decoding: such a detector's bits do not follow the embedded id, so the test holds the route to the float32 twin on the GPU's own frame
    sums (bit for bit), whatever the rule finds."""
    from waveverify_amd import WaveVerify
    from waveverify_amd.watermark_id import WatermarkID
    wv = WaveVerify.random_init(seed=SC.LOC_SEED)
    x = torch.from_numpy(SC.locator_recording()[:1, 0]).cuda()
    T = x.shape[1]
    spans = [[(0, 8000, WatermarkID.custom("1010101010101010")), (8000, T, WatermarkID.custom("0101010101010101"))]]
    wm = wv.embed_spans_clips([x[0]], spans)[0][None]
    rule = SplitRule(5, 0.05, 1)
    kw = dict(threshold=SC.LOC_THRESHOLD, min_on=SC.LOC_MIN_ON)
    got = wv.detect_segments_batch(wm[:, None], split=rule, **kw)
    plain = wv.detect_segments_batch(wm[:, None], **kw)
    det = wv._need("detector")
    g, thr = wv._gate(wm[:, None], SC.LOC_THRESHOLD, None)
    fsum = det.detector_frame_sums(wm[:, None], g, thr, "f32").cpu().numpy()
    t = SegmentTracker(1, 16, det.hop_length, SC.LOC_MIN_ON, 2, 5, split=rule)
    t.advance(fsum, 0, fsum.shape[2], T - (fsum.shape[2] - 1) * det.hop_length, True)
    twin = t.poll()[0]
    print(f"MEASURE spans then split: pieces {[(a.frames, a.change) for a in got[0]]}; without a rule {[a.frames for a in plain[0]]}")
    assert [(a.frames, a.change) for a in got[0]] == [((e[0], e[1]), e[4]) for e in twin] and len(got[0]) >= 1
    assert all(a.prob.tobytes() == e[3].tobytes() and a.watermark is not None for a, e in zip(got[0], twin))
    # no bit's mean crosses 1/2 on a random full-size detector, whatever was embedded: no cut, the unsplit route's runs with no flag set
    assert [(a.frames, a.change) for a in got[0]] == [(a.frames, (False, False)) for a in plain[0]]
    assert all(a.prob.tobytes() == b.prob.tobytes() for a, b in zip(got[0], plain[0]))
    runs = [a.frames for a in plain[0]]                                       # the pieces tile the unsplit route's runs
    assert [a.frames[0] for a in got[0] if not a.change[0]] == [r[0] for r in runs]
    assert [a.frames[1] for a in got[0] if not a.change[1]] == [r[1] for r in runs]
