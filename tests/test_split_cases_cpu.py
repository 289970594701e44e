"""Splitting a run where the decoded id changes, without a GPU (localize.SplitRule, split_points and the streaming twins; DESIGN.md section
7d-10): the rule's definition on hand-written dyadic cases, the twins against the whole-array statement and against themselves under every
tick partition, the unsplit tracker where no rule fires, the margins of the route cases on the oracles, and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import segment_session_cases as SC
import split_cases as X
from waveverify_amd.localize import (WV_SPLIT_MAX_WINDOW, BankSegmentTracker, Segment, SegmentTracker, SplitRule, segments_from_counts,
                                     split_points, split_scores)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (4, 16)
WS = (3, 4, 5, 6)


def run(case, chunks=None, split=True):
    f = case["fsum"]
    t = SegmentTracker(1, f.shape[0] - 1, X.HOP, case["min_on"], case["G"], case["ml"], split=case["rule"] if split else None)
    return SC.run_tracker(t, f[None], chunks or [(0, f.shape[1])], case["last_valid"])[0], t


# ---- 1. the definition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("nb", NBS)
def test_two_ids_in_one_run_come_out_as_two_events(nb, W):
    case = X.synthetic_cases(nb, W)[0]
    ids = X.IDS4 if nb == 4 else X.IDS16
    assert case["name"] == "two ids"
    (one,), _ = run(case, split=False)                                  # today's tracker: one event, the mixed mean, neither id
    assert (one[0], one[1]) == (2, 2 + 6 * W) and len(one) == 4
    mixed = [(7 + 1) / 16 if a != b else (7 / 8 if a == "1" else 1 / 8) for a, b in zip(ids["A"], ids["B"])]
    assert one[3].tolist() == np.float32(mixed).tolist() and X.bits_of(one[3]) not in (ids["A"], ids["B"])
    got, _ = run(case)                                                  # the rule: two events, cut exactly at the boundary
    assert [(e[0], e[1], e[4]) for e in got] == [(2, 2 + 3 * W, (False, True)), (2 + 3 * W, 2 + 6 * W, (True, False))]
    assert [X.bits_of(e[3]) for e in got] == [ids["A"], ids["B"]]
    for e, bits in zip(got, (ids["A"], ids["B"])):
        assert e[2] == 3 * W * X.HOP and e[3].tolist() == np.float32([7 / 8 if b == "1" else 1 / 8 for b in bits]).tolist()


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("nb", NBS)
def test_synthetic_cases(nb, W):
    names = set()
    for case in X.synthetic_cases(nb, W):
        got, twin = run(case)
        names.add(case["name"])
        assert [(e[0], e[1], e[4]) for e in got] == [w[:3] for w in case["want"]], (case["name"], got)
        for e, w in zip(got, case["want"]):
            assert w[3] is None or X.bits_of(e[3]) == w[3], (case["name"], e)
            assert e[1] - e[0] >= W                                      # every piece has at least W frames
        # the streaming twin is the whole-array statement, run by run
        f = case["fsum"]
        valid = SC.valid_of(f.shape[1], X.HOP, case["last_valid"])
        want = []
        for lo, hi in segments_from_counts(f[nb], valid, case["min_on"], case["G"], case["ml"]):
            cuts = [lo] + [lo + g for g in split_points(f[:, lo:hi], case["rule"])] + [hi]
            for a, b in zip(cuts, cuts[1:]):
                cnt, prob = SC.ascending_ref(f[None], 0, a, b)
                want.append((a, b, cnt, prob, (a > lo, b < hi)))
        assert X.same_events([got], [want]) is None, (case["name"], X.same_events([got], [want]))
        if case.get("largest"):
            (lo, hi), = segments_from_counts(f[nb], valid, case["min_on"], case["G"], case["ml"])
            gs, S, d, ok, _, _ = split_scores(f[:, lo:hi], W)
            assert len(got) == 2 and got[0][1] == lo + int(gs[int(np.nanargmax(S))])
            assert (S[ok] >= 0.5).sum() > 1                              # several boundaries qualified
    assert len(names) >= 11 and (W != 4 or "equal S at two boundaries" in names)


def test_equal_S_keeps_the_earlier_boundary():
    case = [c for c in X.synthetic_cases(16, 4) if c["name"] == "equal S at two boundaries"][0]
    gs, S, d, ok, _, _ = split_scores(case["fsum"][:, 2:2 + 6 * 4 + 1], 4)
    i = int(np.flatnonzero(gs == 12)[0])
    assert S[i] == S[i + 1] == S.max() and d[i] >= 1                    # the same S, bit for bit, before and after the middle frame
    assert split_points(case["fsum"][:, 2:2 + 6 * 4 + 1], case["rule"]) == [12]


def test_a_cut_is_known_once_frame_g_plus_2W_minus_1_has_arrived():
    W = 5
    case = X.synthetic_cases(16, W)[0]
    f, g = case["fsum"], 2 + 3 * W
    t = SegmentTracker(1, 16, X.HOP, 0.5, 2, 5, split=case["rule"])
    t.advance(f[None], 0, g + 2 * W - 1)
    assert t.poll() == [[]] and t.open_runs()[0][:2] == (2, g + 2 * W - 1) and t.split_state()[0][3] == g      # pending, not yet known
    t.advance(f[None], g + 2 * W - 1, g + 2 * W)
    (e,), = t.poll()
    assert (e[0], e[1], e[4]) == (2, g, (False, True))
    piece = t.open_runs()[0]                                            # the open piece starts at the cut and says so
    assert piece[:2] == (g, g + 2 * W) and piece[4] == (True, False) and X.bits_of(piece[3]) == X.IDS16["B"]


# ---- 2. the equalities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("nb", NBS)
def test_every_tick_partition_gives_the_one_tick_events(nb, W):
    n = 0
    for case in X.synthetic_cases(nb, W):
        whole, _ = run(case)
        cuts = [e[1] for e in whole if e[4][1]]
        for name, chunks in X.partitions(case["fsum"].shape[1], cuts, W, (nb, W, case["name"]), case["last_valid"] < X.HOP).items():
            got, _ = run(case, chunks)
            assert X.same_events([got], [whole]) is None, (case["name"], name, X.same_events([got], [whole]))
            n += 1
    assert n > 100


@pytest.mark.parametrize("seed", range(6))
def test_random_frame_sums_twin_partitions_and_bank(seed):
    """The kernel fuzz's inputs on the host: the lockstep twin in one tick, under partitions, and behind the bank twin's descriptors."""
    S, nb, W, G = (1, 3)[seed % 2], NBS[seed % 2], (2, 5, 25)[seed % 3], (1, 2, 4)[seed % 3]
    hop, ml = 10, min(W, 5)
    rule = SplitRule(W, 0.3, 1)
    fsum, lv = X.random_fsum(S, nb, 120 if W < 25 else 200, W, G, hop, seed)
    Fr = fsum.shape[2]
    one = SegmentTracker(S, nb, hop, 0.5, G, ml, split=rule)
    whole = SC.run_tracker(one, fsum, [(0, Fr)], lv)
    assert sum(e[4][1] for evs in whole for e in evs) >= 1              # some run was cut
    for evs in whole:
        assert all(e[1] - e[0] >= W for e in evs if e[4] != (False, False))
    cuts = [e[1] for e in whole[0] if e[4][1]][:2]
    for name, chunks in X.partitions(Fr, cuts, W, ("rand", seed), lv < hop).items():
        got = SC.run_tracker(SegmentTracker(S, nb, hop, 0.5, G, ml, split=rule), fsum, chunks, lv)
        assert X.same_events(got, whole) is None, (name, X.same_events(got, whole))
    bank = BankSegmentTracker(S + 1, nb, hop, 0.5, G, ml, ring=64, split=rule)
    for lo, hi in SC.chunks_of(Fr, "random", np.random.default_rng(seed), lv < hop):
        final = hi == Fr
        desc = [[s + 1, s * (nb + 1) * Fr, Fr, lo, hi, lo, lv if final and hi > lo else hop, int(final)] for s in range(S)]
        bank.advance(fsum.reshape(-1), np.array(desc, np.int64))
        if final:
            break
    else:
        bank.advance(fsum.reshape(-1), np.array([[s + 1, 0, 0, 0, 0, Fr, hop, 1] for s in range(S)], np.int64))
    got = bank.poll(range(1, S + 1))
    assert X.same_events([got[s + 1] for s in range(S)], whole) is None


@pytest.mark.parametrize("i", range(48))
def test_no_rule_or_a_rule_that_never_fires_is_todays_tracker(i):
    nb, G, ml, hop, min_on, lv, fsum = SC.random_case(i)
    W = max(2, G, ml) + i % 3
    rng = np.random.default_rng(i)
    chunks = SC.chunks_of(fsum.shape[2], SC.CHUNKINGS[i % 3], rng, lv < hop)
    today = SC.run_tracker(SegmentTracker(1, nb, hop, min_on, G, ml), fsum, chunks, lv)
    none = SC.run_tracker(SegmentTracker(1, nb, hop, min_on, G, ml, split=None), fsum, chunks, lv)
    never = SC.run_tracker(SegmentTracker(1, nb, hop, min_on, G, ml, split=SplitRule(W, 1e9, 1)), fsum, chunks, lv)
    assert SC.same_events(none, today) is None
    assert all(len(e) == 4 for e in none[0]) and all(len(e) == 5 and e[4] == (False, False) for e in never[0])
    assert SC.same_events(never, today) is None                          # frames, count and prob bit for bit


def test_not_quantized_sums_are_one_ascending_pass_per_piece():
    """Twelve decades of values, where float64 adds of float32 values do round: a piece's sums are ascending_ref's over its own frames."""
    rng = np.random.default_rng(5)
    nb, W, hop = 16, 4, 10
    f = SC.sums_for([hop] * 40, nb, rng, quantized=False)
    f[:nb, 20:] = (hop - f[:nb, 20:]).astype(np.float32)                # the second half's bits flipped
    t = SegmentTracker(1, nb, hop, 0.5, 2, 4, split=SplitRule(W, 0.5, 1))
    for lo in range(0, 40, 3):
        t.advance(f[None], lo, min(40, lo + 3), final=lo + 3 >= 40)
    got = t.poll()[0]
    assert len(got) >= 2
    for e in got:
        cnt, prob = SC.ascending_ref(f[None], 0, e[0], e[1])
        assert e[2] == cnt and e[3].tobytes() == prob.tobytes()


# ---- 3. the margins of the cases that run against f32 sums on the GPU ---------------------------------------------------------------------
@pytest.mark.parametrize("det_id", X.ROUTE_NETS + X.ROUTE_F16)
def test_route_cases_keep_their_margins_on_the_oracle(det_id):
    cfg, sd, x, gate, whole = X.route_reference(det_id)
    events, margins = X.route_events(det_id, whole)
    print(f"MEASURE {det_id}: oracle events {[[(e[0], e[1], e[4]) for e in evs] for evs in events]}, margins {margins}")
    assert all(len(evs) >= 2 for evs in events)                          # every stream's run is cut
    assert set(margins) == {"threshold", "vote", "pending"}
    assert min(margins.values()) >= X.MARGIN, margins
    assert float(np.abs(np.asarray(sd["last_layer.bias"])).max()) == 0.0


@pytest.mark.parametrize("det_id", X.ROUTE_NETS + X.ROUTE_F16)
def test_locator_driven_cases_keep_their_margins_on_the_oracle(det_id):
    from waveverify_amd.localize import gate_threshold
    cfg, sd, lcfg, lsd, x, lg, whole = X.loc_reference(det_id)
    near = float(np.abs(lg - gate_threshold(X.LOC_P[det_id])).min())
    events, margins = X.loc_events(det_id, whole)
    hop = cfg.hop_length
    on = (whole[:, -1, :-1] >= X.LOC_MIN_ON * hop).sum(1)
    print(f"MEASURE {det_id}: nearest locator logit {near:.2e} from the threshold, gated share {float((lg > gate_threshold(X.LOC_P[det_id])).mean()):.2f}, "
          f"on frames {on.tolist()} of {whole.shape[2]}, oracle events {[[(e[0], e[1], e[4]) for e in evs] for evs in events]}, margins {margins}")
    assert near >= X.LOC_LOGIT_MARGIN
    assert sum(e[4][1] for evs in events for e in evs) >= 1 and all(len(evs) >= 1 for evs in events)
    assert min(margins.values()) >= X.MARGIN, margins
    counts = whole[:, -1]
    assert (counts == np.round(counts)).all() and 0 < (counts < hop).sum()      # the locator leaves samples out: it decides the sums


def test_margins_start_over_with_reset_and_set_split():
    case = X.synthetic_cases(4, 4)[0]
    _, t = run(case)
    assert t.margins
    t.reset()
    assert t.margins == {}
    run_again = SC.run_tracker(t, case["fsum"][None], [(0, case["fsum"].shape[1])], case["last_valid"])
    assert t.margins and run_again
    t.set_split(SplitRule(4, 0.25, 1))
    assert t.margins == {}


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_rule_fields_are_validated():
    assert SplitRule() == SplitRule(25, 0.5, 1)
    with pytest.raises(Exception):
        SplitRule().window_frames = 3                                    # frozen
    for kw in (dict(window_frames=1), dict(window_frames=WV_SPLIT_MAX_WINDOW + 1), dict(window_frames=2.5), dict(window_frames=True),
               dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(min_bits=0),
               dict(min_bits=1.5)):
        with pytest.raises(ValueError):
            SplitRule(**kw)
    SplitRule(2, 1e-9, 1), SplitRule(WV_SPLIT_MAX_WINDOW, 3.0, 255)


def test_rule_meets_the_tracker():
    for kw in (dict(min_gap_frames=6), dict(min_len_frames=6)):
        with pytest.raises(ValueError, match="window_frames"):
            SegmentTracker(1, 16, 10, **kw, split=SplitRule(5))
        with pytest.raises(ValueError, match="window_frames"):
            BankSegmentTracker(2, 16, 10, **kw, split=SplitRule(5))
    with pytest.raises(ValueError, match="min_bits"):
        SegmentTracker(1, 4, 10, split=SplitRule(5, 0.5, 5))
    SegmentTracker(1, 4, 10, min_gap_frames=5, min_len_frames=5, split=SplitRule(5, 0.5, 4))
    with pytest.raises(ValueError, match="min_bits"):
        split_points(np.ones((5, 30)), SplitRule(5, 0.5, 5))


def test_set_split_only_before_the_first_push():
    """The backend-independent session and bank on numpy arrays with a count-only net."""
    import segment_bank_cases as SB
    from waveverify_amd.session import SegmentStreamBank, SegmentStreamSession
    hop, rule = 10, SplitRule(5, 0.5, 1)
    fs = SB.count_net(hop)
    sess = SegmentStreamSession(1, hop, 20, lambda win, g: fs(win, g), SegmentTracker(1, 1, hop), capacity=8)
    sess.set_split(rule)
    sess.set_split(None)
    sess.set_split(rule)
    assert sess.split == rule
    x, g = np.zeros((1, 30), np.float32), np.ones((1, 30), np.float32)
    sess.push(x, g)
    with pytest.raises(RuntimeError, match="before the first push"):
        sess.set_split(None)
    assert sess.open_segments()[0].frames == (0, 3) and sess.open_segments()[0].change == (False, False)
    sess.reset()
    sess.set_split(None)                                                 # legal again
    with pytest.raises(ValueError, match="at least 6"):
        SegmentStreamSession(1, hop, 20, fs, SegmentTracker(1, 1, hop), capacity=5).set_split(rule)
    with pytest.raises(ValueError, match="window_frames"):
        SegmentStreamSession(1, hop, 20, fs, SegmentTracker(1, 1, hop, min_len_frames=6), capacity=8).set_split(rule)
    bank = SegmentStreamBank(2, hop, 20, fs, BankSegmentTracker(2, 1, hop), gated=True, ring=8)
    bank.set_split(rule)
    slot = bank.open()
    with pytest.raises(RuntimeError, match="first open"):
        bank.set_split(None)
    bank.push({slot: (x[0], g[0])})
    assert bank.open_segments()[slot].frames == (0, 3)


def test_segment_gains_a_last_field():
    import dataclasses
    f = dataclasses.fields(Segment)
    assert f[-1].name == "change" and f[-1].default == (False, False) and [x.name for x in f[:7]] == [
        "start_s", "end_s", "watermark", "confidence", "coverage", "prob", "frames"]


# ---- 5. the exports ------------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("wv_segment_split_bytes", "wv_segment_track_split", "wv_bank_segment_track_split")


def test_new_exports_are_declared_listed_and_bound():
    from waveverify_amd import _lib
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    declared = set(re.findall(r"\b(wv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    zero = {C.c_int: 0, C.c_int64: 0, C.c_size_t: 0, C.c_float: 0.0, C.c_double: 0.0}
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None
        rc = getattr(lib, name)(*[zero.get(t) for t in _lib.SIGNATURES[name][1]])
        msg = lib.wv_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":"), (name, rc, msg)
    assert "#define WV_SPLIT_MAX_WINDOW 256" in header and "split frame j in slot" in header
    sb, eb = C.c_size_t(), C.c_size_t()
    assert lib.wv_segment_split_bytes(3, 16, 2, 25, 64, C.byref(sb), C.byref(eb)) == 0
    assert sb.value == 3 * (64 + 8 * 17 + 4 * 52 * 17) and eb.value == 3 * (8 + 64 * (32 + 64))
    for args, what in (((3, 16, 2, 1, 64), "window_frames outside [2, 256]"), ((3, 16, 2, 257, 64), "window_frames outside [2, 256]"),
                       ((3, 16, 65, 25, 64), "min_gap_frames outside [1, 64]"), ((65536, 16, 2, 25, 64), "[1, 65535]")):
        assert lib.wv_segment_split_bytes(*args, C.byref(sb), C.byref(eb)) == -1 and what.encode() in lib.wv_last_error()
    import inspect
    from waveverify_amd.core import WaveVerify
    assert inspect.signature(WaveVerify.detect_segments_batch).parameters["split"].default is None
    p = inspect.signature(WaveVerify.segments).parameters["split"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
