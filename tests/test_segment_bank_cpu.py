"""Segment banks without a GPU: the numpy twin of wv_bank_segment_track against the lockstep twin slot by slot, the
bank's state machine (session.SegmentStreamBank) on the float64 oracle of small nets and on a count-only net, and the new export.

Bars.  Twin against lockstep twin: bit for bit.  State machine against the tracker on the whole-recording frame sums of what a slot pushed:
frames equal, count and prob within 1e-12 (test_bank_cases_cpu's bar for stitched windows against the whole clip in float64).  A Segment's
prob is float32, so a stitching error that moved a quotient across a float32 rounding boundary would show as 6e-8 and fail; measured:
2.8e-14 at most, 0 in three of the four runs.  The mixed schedule's shortest streams have two frames, where two segments do not fit: every
stream has a frame exactly at min_on, and every stream of three frames or more has at least two segments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import segment_bank_cases as SB
import segment_session_cases as SC
from bank_cases import CAPACITY, PAD_LIMITS, mixed_schedule, stream_lengths
from localized_cases import frame_sums_ref
from waveverify_amd.localize import BankSegmentTracker, Segment, SegmentTracker, gate_threshold
from waveverify_amd.session import NumpyArrays, SegmentStreamBank, bank_track_row_ok, numpy_bank_advance, segment_halo

W = SB.W
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STITCH_BAR = 1e-12


# ---- 1. the twin, slot by slot, against the lockstep twin ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", SC.NBS)
def test_bank_twin_equals_the_lockstep_twin_slot_by_slot(nb):
    hop, min_on, cap = SB.HOP, 0.5, SB.KERNEL_CAPACITY
    n_events, n_bad, strides, offsets, names = 0, 0, set(), set(), 0
    for G in SC.GAPS:
        for ml in SC.LENS:
            for kind in SC.CHUNKINGS:
                rng = np.random.default_rng(SC.seed_of("bank-twin", nb, G, ml, kind))
                for batch in SB.pattern_streams(nb, G, ml, kind, rng):
                    names += len(batch)
                    assert len({first for *_, first in batch}) > 1 or len(batch) == 1             # the slots start at different ticks
                    bank = BankSegmentTracker(cap, nb, hop, min_on, G, ml, ring=64)
                    spare = (set(range(cap)) - {b[0] for b in batch}).pop()
                    # the spare slot holds an open run that every bad row names: it must come through untouched
                    held = SC.sums_for([hop] * 3, nb, rng)
                    bank.advance(held.reshape(-1), [[spare, 0, 3, 0, 3, 0, hop, 0]])
                    before = bank.open_runs([spare])[spare]
                    got = {b[0]: [] for b in batch}
                    for arena, desc in SB.bank_ticks(batch, nb, hop, rng):
                        for row in desc:
                            assert bank_track_row_ok(row, cap, nb, hop, arena.size)
                            strides.add(int(row[2]))
                            offsets.add(int(row[1]))
                        if len(desc):
                            good = [spare] + [int(v) for v in desc[0][1:]]
                            for why, bad in SB.bad_track_rows(good, cap, nb, hop, arena.size):
                                assert not bank_track_row_ok(bad, cap, nb, hop, arena.size), why
                                if bad[0] != spare:
                                    continue
                                desc = np.concatenate([desc, np.array([bad], np.int64)])
                                n_bad += 1
                        bank.advance(arena, desc)
                        for s, evs in bank.poll(list(got)).items():
                            got[s] += evs
                    for slot, fsum, last_valid, _, _ in batch:
                        want = SB.lockstep_events(fsum, hop, last_valid, min_on, G, ml)
                        assert SC.same_events([want], SC.whole_ref(fsum[None], hop, last_valid, min_on, G, ml)) is None
                        diff = SC.same_events([got[slot]], [want])
                        assert diff is None, (G, ml, kind, slot, diff)
                        n_events += len(want)
                    after = bank.open_runs([spare])[spare]
                    assert after[:3] == before[:3] and after[3].tobytes() == before[3].tobytes() and bank.poll([spare])[spare] == []
    assert names == 3 * sum(len(SC.named_patterns(hop, min_on, G, ml)) for G in SC.GAPS for ml in SC.LENS)
    assert n_events > 100 and n_bad > 100 and len(strides) > 5 and len(offsets) > 20


def test_bank_twin_takes_an_impossible_state_as_closed_and_reports_a_lost_event():
    hop, nb = 10, 1
    bank = BankSegmentTracker(2, nb, hop, 0.5, 2, 1, ring=1)
    on = SC.sums_for([hop] * 2, nb, np.random.default_rng(0)).reshape(-1)
    bank.advance(on, [[0, 0, 2, 0, 2, 0, hop, 0]])
    assert bank.open_runs([0])[0][:2] == (0, 2)
    bank.advance(on, [[0, 0, 2, 0, 2, 40, hop, 0]])                          # frame0 far beyond the open run: taken as closed, no event
    assert bank.open_runs([0])[0][:2] == (40, 42) and bank.poll([0]) == {0: []}
    bank.advance(on, [[0, 0, 2, 0, 0, 42, hop, 1]])                          # final without a frame closes it
    assert bank.open_runs([0]) == {0: None} and [e[:2] for e in bank.poll([0])[0]] == [(40, 42)]
    bank.reset(0)
    two = SC.sums_for([hop, 0, 0, hop, 0, 0], nb, np.random.default_rng(1)).reshape(-1)
    bank.advance(two, [[0, 0, 6, 0, 6, 0, hop, 0]])                          # two closes into a ring of one, unread
    with pytest.raises(RuntimeError, match="events were lost"):
        bank.poll([0])


# ---- 2. the state machine on the float64 oracle of small nets ---------------------------------------------------------------------------------
def _close(got, want, hop, T, what):
    """One slot's Segments against the whole-recording tracker's events: frames equal, count and prob within the stitching bar."""
    assert [g.frames for g in got] == [(lo, hi) for lo, hi, _, _ in want], (what, [g.frames for g in got], [w[:2] for w in want])
    worst = 0.0
    for g, (lo, hi, cnt, prob) in zip(got, want):
        assert isinstance(g, Segment)
        end = min(hi * hop, T)
        assert g.start_s == lo * hop / 16000 and g.end_s == end / 16000, (what, g)
        worst = max(worst, abs(g.coverage * (end - lo * hop) - cnt), float(np.abs(g.prob.astype(np.float64) - prob).max()))
    return worst


@pytest.mark.parametrize("det_id,loc_id,gated", [("x1.detector", "x3.locator", False), ("x7.detector", "x3.locator", False),
                                                 ("x1.detector", "x3.locator", True), ("x7.detector", "x3.locator", True)])
def test_bank_state_machine_on_the_oracle(det_id, loc_id, gated):
    cases = {c[0]: c for c in W.net_cases()}
    dcfg, _, dnet = W.oracle_net(cases[det_id])
    lcfg, _, lnet = W.oracle_net(cases[loc_id])
    hop, nb, H = dcfg.hop_length, dcfg.head_bits, segment_halo(dcfg, lcfg)
    assert (hop, lcfg.hop_length) == (32, 16)
    steps = mixed_schedule(hop, H)
    lengths = stream_lengths(steps)
    xs = {n: W.clip_data(cases[det_id], max(T, 1), 300 + i)[0][0, 0, :T] for i, (n, T) in enumerate(lengths.items())}
    dlog = {n: W.oracle_forward(dcfg, dnet, x[None, None]) for n, x in xs.items() if x.size}
    min_on = 0.5
    if gated:
        G, ml, thr = 1, 1, 0.5
        gates = {n: SB.stream_gate(len(x), hop, min_on) for n, x in xs.items()}
        gsrc = {n: g[None] for n, g in gates.items()}
    else:
        G, ml, gates = 2, 2, None
        gsrc = {n: W.oracle_forward(lcfg, lnet, x[None, None])[:, 0] for n, x in xs.items() if x.size}
        srt = np.sort(np.concatenate([g[0] for g in gsrc.values()]))
        thr = float(0.5 * (srt[len(srt) // 2 - 1] + srt[len(srt) // 2]))                           # the random locator fires on half the samples
        assert abs(gate_threshold(1.0 / (1.0 + np.exp(-thr))) - thr) < 1e-9
        assert not any((np.abs(g - thr) < 1e-9).any() for g in gsrc.values())                      # no gate decision hangs on the stitching error
    want = {}
    for n, x in xs.items():
        if not x.size:
            want[n] = []
            continue
        whole = frame_sums_ref(dlog[n], gsrc[n], thr, hop, x.size)
        want[n] = SB.lockstep_events(whole[0], hop, x.size - (whole.shape[2] - 1) * hop, min_on, G, ml, dtype=np.float64)
        if gated:                                                                                   # the patterns do what they are there for
            Fr = whole.shape[2]
            assert whole[0, nb, 0] == min_on * min(hop, x.size) and want[n][0][0] == 0, n
            assert len(want[n]) >= (2 if Fr >= 3 else 1), (n, Fr, want[n])
    assert sum(len(w) for w in want.values()) >= (12 if gated else 3)

    def frame_sums(win, gwin):
        g = gwin if gwin is not None else W.oracle_forward(lcfg, lnet, win)[:, 0]
        return frame_sums_ref(W.oracle_forward(dcfg, dnet, win), g, thr, hop, win.shape[-1])

    worst, stats = 0.0, {}
    for pad in PAD_LIMITS:
        bank = SegmentStreamBank(CAPACITY, hop, H, frame_sums, BankSegmentTracker(CAPACITY, nb, hop, min_on, G, ml, ring=2, dtype=np.float64),
                                 numpy_bank_advance, NumpyArrays(np.float64), pad, gated, 16000, 2, G, ml)
        got, _ = SB.play(bank, steps, xs, gates, poll_every=3)
        assert bank.open_slots() == []
        for n, x in xs.items():
            worst = max(worst, _close(got[n], want[n], hop, x.size, (pad, n)))
        stats[pad] = bank.stats
    print(f"MEASURE segment bank on the oracle ({det_id}, {'gated' if gated else 'locator'}): count / prob within {worst:.1e} of the whole recording")
    assert worst <= STITCH_BAR, worst
    a, b, c = (stats[p] for p in PAD_LIMITS)
    assert a["launches"] > c["launches"] and a["padded_samples"] == 0 < c["padded_samples"]       # the groupings differed


# ---- 3. padding is never tracked -------------------------------------------------------------------------------------------------------------------
def _count_bank(hop, capacity=3, ring=64, G=1, ml=1, pad=float("inf"), frame_sums=None, advance=numpy_bank_advance, tracker=None):
    tracker = tracker or BankSegmentTracker(capacity, 1, hop, 0.5, G, ml, ring=ring)
    return SegmentStreamBank(capacity, hop, 2 * hop, frame_sums or SB.count_net(hop), tracker, advance, None, pad, True, 16000, ring, G, ml)


def _same_segments(a, b):
    assert [s.frames for s in a] == [s.frames for s in b], ([s.frames for s in a], [s.frames for s in b])
    for u, v in zip(a, b):
        assert (u.start_s, u.end_s, u.coverage, u.confidence) == (v.start_s, v.end_s, v.coverage, v.confidence) and u.prob.tobytes() == v.prob.tobytes()


def test_padding_is_never_tracked():
    """Slot a pushes one frame a tick, slot b three: at pad_limit = inf they share a launch three frames long, so two frame columns of a's row
    are computed on zero padding.  The wrapper gives every such column a full count and NaN sums: tracked, it would open or extend a run with
    a NaN probability."""
    hop = 8
    rows_now, padded = {}, [0]

    def advance(hist, x, desc, A, Lmax):
        rows_now["desc"] = np.array(desc)
        return numpy_bank_advance(hist, x, desc, A, Lmax)

    def poisoned(win, gwin):
        out = SB.count_net(hop)(win, gwin)
        for _, _, _, _, r, wlen, _, _ in rows_now["desc"]:
            if wlen:
                f = -(-int(wlen) // hop)
                padded[0] += out.shape[2] - f
                out[r, :-1, f:] = np.nan
                out[r, -1, f:] = hop
        return out

    ga = np.repeat(np.array([1, 1, 0, 1, 0, 0, 1, 1, 1, 0], np.float32), hop)
    gb = np.repeat(np.array([0, 1, 1, 0] * 7 + [1, 1], np.float32), hop)
    runs = []
    for fs, adv in ((None, numpy_bank_advance), (poisoned, advance)):
        bank = _count_bank(hop, frame_sums=fs, advance=adv)
        a, b = bank.open(), bank.open()
        for k in range(10):
            bank.push({a: (np.zeros(hop, np.float32), ga[k * hop:(k + 1) * hop]), b: (np.zeros(3 * hop, np.float32), gb[3 * k * hop:3 * (k + 1) * hop])})
        runs.append((bank.close(a), bank.close(b)))
        assert bank.stats["padded_samples"] >= 10 * hop and bank.stats["launches"] == 10   # one launch per tick, a's row padded
    assert padded[0] >= 20                                                      # the schedule did produce padded frame columns
    assert [s.frames for s in runs[0][0]] == [(0, 2), (3, 4), (6, 9)] and len(runs[0][1]) == 8
    _same_segments(runs[1][0], runs[0][0])
    _same_segments(runs[1][1], runs[0][1])


# ---- 4. slot reuse -------------------------------------------------------------------------------------------------------------------------------
def test_a_reused_slot_starts_from_nothing_and_close_returns_the_open_run():
    hop = 8
    gp = np.repeat(np.array([0, 1, 1, 0, 0, 1, 1, 1], np.float32), hop)                            # closed mid-run: frames 5 .. 8 are open
    gq = np.repeat(np.array([1, 0, 0, 1, 1, 0, 1], np.float32), hop)[:-3]
    z = lambda g: (np.zeros(len(g), np.float32), g)
    used, fresh = _count_bank(hop, G=2), _count_bank(hop, G=2)
    p = used.open()
    used.push({p: z(gp[:3 * hop + 1])})
    used.push({p: z(gp[3 * hop + 1:])})
    assert used.open_segments()[p].frames == (5, 8)
    left = used.close(p)
    assert [s.frames for s in left] == [(1, 3), (5, 8)] and used.open_slots() == []
    q, f = used.open(), fresh.open()
    assert q == p == f
    assert used.open_segments() == {q: None} and used.poll() == {q: []} and used.samples_seen(q) == 0
    for bank, s in ((used, q), (fresh, f)):
        bank.push({s: z(gq[:hop + 3])})
        bank.push({s: z(gq[hop + 3:])})
    a, b = used.close(q), fresh.close(f)
    assert [s.frames for s in a] == [(0, 1), (3, 7)] and a[-1].end_s == len(gq) / 16000            # the one-frame gap merges at G = 2
    _same_segments(a, b)


# ---- 5. the ring -----------------------------------------------------------------------------------------------------------------------------------
class _Ring(BankSegmentTracker):
    """A twin that knows its ring: an advance that leaves more unread events on a slot than the ring holds would have overwritten one."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.waiting, self.reads = [0] * self.capacity, 0

    def advance(self, fsum, desc):
        before = [t.events_total[0] for t in self._t]
        super().advance(fsum, desc)
        for s, t in enumerate(self._t):
            self.waiting[s] += t.events_total[0] - before[s]
            assert self.waiting[s] <= self.ring, f"slot {s}: an event would have been overwritten"

    def reset(self, slot):
        super().reset(slot)
        self.waiting[slot] = 0

    def poll(self, slots):
        self.reads += 1
        for s in slots:
            self.waiting[s] = 0
        return super().poll(slots)


@pytest.mark.parametrize("ring", [1, 2])
def test_the_automatic_read_loses_nothing_at_ring_one_and_two(ring):
    hop = 4
    gate, want = SB.ring_gates(hop)
    T = gate.shape[1]
    for sizes in ([T], [hop] * (T // hop), [1, 7, 0, 13, 2] * 30):
        tracker = _Ring(3, 1, hop, 0.5, 1, 1, ring=ring)
        bank = _count_bank(hop, ring=ring, tracker=tracker)
        slots = [bank.open() for _ in range(3)]
        seen = [0, 0, 0]
        for i, n in enumerate(sizes):
            items = {}
            for s in slots:
                m = min(n + s, T - seen[s]) if len(sizes) > 1 else T                                # the slots push different sizes
                items[s] = (np.zeros(m, np.float32), gate[s, seen[s]:seen[s] + m])
                seen[s] += m
            assert bank.push(items) is None
        reads = tracker.reads
        assert reads > 0                                                        # nobody polled: the bank read the rings itself
        for s in slots:
            segs = bank.close(s)
            assert seen[s] == T and [g.frames for g in segs] == want[s], (ring, sizes[:3], s)
            assert all(g.coverage == 1.0 and g.prob[0] == np.float32(0.75) for g in segs)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [True, False])
def test_refused_pushes_change_no_stream(gated):
    hop = 8
    fs = SB.count_net(hop)
    frame_sums = fs if gated else (lambda win, gwin: fs(win, (win[:, 0] > 0).astype(np.float32)))     # ungated: the "locator" is the sign of x
    ga = np.repeat(np.array([1, 1, 0, 1, 1, 1, 0, 0, 1], np.float32), hop)
    gb = np.repeat(np.array([0, 1, 0, 0, 1, 1], np.float32), hop)[:-2]
    item = (lambda g: (g, g)) if gated else (lambda g: g)
    sizes = [3, hop, 2 * hop + 1, hop - 1, 5 * hop]

    def run(misuse):
        tr = BankSegmentTracker(3, 1, hop, 0.5, 1, 1)
        bank = SegmentStreamBank(3, hop, 2 * hop, frame_sums, tr, numpy_bank_advance, None, 1.5, gated, 16000, 64, 1, 1)
        a, b = bank.open(), bank.open()
        out, at = {a: [], b: []}, 0
        for n in sizes:
            if misuse:
                x = ga[:hop]
                bads = [{2: item(x)}, {a: item(x), 7: item(x)}, {a: item(x.reshape(2, -1))}, {a: item(x), True: item(x)}]
                bads += [{a: item(x), b: x}, {b: (x, x[:-1])}, {b: (x, x, x)}] if gated else [{a: item(x), b: (x, x)}, {b: [x, x]}]
                for bad in bads:
                    with pytest.raises(ValueError):
                        bank.push(bad)
                with pytest.raises(ValueError):
                    bank.close(2)
            bank.push({a: item(ga[at:at + n]), b: item(gb[at:at + n])})
            at += n
            for s, segs in bank.poll().items():
                out[s] += segs
        assert (bank.samples_seen(a), bank.samples_seen(b)) == (len(ga) // hop * hop, len(gb) // hop * hop)
        return out[a] + bank.close(a), out[b] + bank.close(b)

    clean, misused = run(False), run(True)
    assert [s.frames for s in clean[0]] == [(0, 2), (3, 6), (8, 9)] and [s.frames for s in clean[1]] == [(1, 2), (4, 6)]
    _same_segments(misused[0], clean[0])
    _same_segments(misused[1], clean[1])
    with pytest.raises(ValueError, match="ring"):
        SegmentStreamBank(3, hop, 2 * hop, fs, None, ring=0)
    with pytest.raises(ValueError, match="does not divide"):
        cases = {c[0]: c for c in W.net_cases()}
        segment_halo(W.net_config(cases["x7.detector"])[0], W.net_config(cases["x4.locator"])[0])


def test_lifecycle_on_the_host():
    hop = 8
    bank = _count_bank(hop, capacity=2, G=2)
    a, b = bank.open(), bank.open()
    with pytest.raises(RuntimeError, match="slots"):
        bank.open()
    on = np.ones(hop, np.float32)
    bank.push({a: (on, on)})
    assert bank.open_segments()[a].frames == (0, 1) and bank.open_segments()[b] is None            # an opening shows at once
    bank.push({a: (on, 0 * on)})
    assert bank.open_segments()[a].frames == (0, 1) and bank.poll() == {a: [], b: []}                # one off frame: still open
    bank.push({a: (on, 0 * on)})
    assert bank.open_segments()[a] is None and [s.frames for s in bank.poll()[a]] == [(0, 1)]       # the second closes it
    assert bank.close(b) == [] and bank.open_slots() == [a] and sorted(bank.poll()) == [a] and bank.open() == b


# ---- 7. the export -------------------------------------------------------------------------------------------------------------------------------
def test_the_new_export_is_declared_listed_and_bound():
    from waveverify_amd import _lib
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    declared = set(re.findall(r"\b(wv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    name = "wv_bank_segment_track"
    assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert "{slot, fsum_off, Fr_stride, f_lo, f_hi, frame0, last_valid, final}" in header          # the descriptor is stated for callers
    zero = {C.c_int: 0, C.c_int64: 0, C.c_size_t: 0, C.c_float: 0.0, C.c_double: 0.0}
    rc = getattr(lib, name)(*[zero.get(t) for t in _lib.SIGNATURES[name][1]])
    msg = lib.wv_last_error().decode()
    assert rc == -1 and msg.startswith(name + ": null"), (rc, msg)
    from waveverify_amd.core import WaveVerify
    import inspect
    sig = inspect.signature(WaveVerify.open_segment_bank)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == dict(
        capacity=64, pad_limit=1.5, threshold=0.5, min_on=0.5, min_gap_frames=2, min_len_frames=5, ring=64, gated=False)
