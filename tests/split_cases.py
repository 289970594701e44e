"""Splitting a run where the decoded id changes (localize.SplitRule): the case lists of tests/test_split_cases_cpu.py
and tests/test_gpu_split.py (a plain module, fixed seeds, importable without a GPU).

synthetic_cases()   named runs of DYADIC frame sums (hop 8, a 1 bit sums to 7 per full frame and a 0 bit to 1, so every window mean is 7/8 or
                    1/8 or a dyadic mix and every sum is exact) with the events the rule must give, written down by hand
partitions()        the tick partitions every streaming tracker is run under
random_fsum()       seeded frame sums with several ids per run for the kernel fuzz: an event is bit-equal between kernel and twin whatever the
                    values, so these need no margin
route_reference()   the recording of the route tests on the small session nets: two unlike signals either side of a boundary inside one
                    gated stretch, and the rule whose comparisons keep the margins the CPU test asserts on the float64 oracle"""
from __future__ import annotations

import numpy as np

import segment_session_cases as SC
from waveverify_amd.localize import SplitRule

HOP = 8
ONE, ZERO = 7.0, 1.0                                               # a bit's sum over a full frame of 8 gated samples: p = 7/8 or 1/8
MARGIN = 1e-3

IDS4 = {"A": "1010", "B": "0110", "C": "0101", "A1": "1011"}
IDS16 = {"A": "1010101010101010", "B": "0110011001100110", "C": "0101010101010101", "A1": "1010101010101011"}


def frames_of(bits: str, n: int, count: float = HOP):
    """n frames of id `bits`, each with `count` gated samples -> [nb + 1, n] float64."""
    col = np.array([ONE if b == "1" else ZERO for b in bits] + [HOP], np.float64) * (count / HOP)
    return np.repeat(col[:, None], n, axis=1)


def off(nb: int, n: int):
    return np.zeros((nb + 1, n), np.float64)


def build(nb: int, parts):
    """parts: [("A", n) | ("off", n) | ("mid", n) | array] -> fsum [nb + 1, Fr] float32."""
    ids = IDS4 if nb == 4 else IDS16
    cols = []
    for p in parts:
        if isinstance(p, np.ndarray):
            cols.append(p)
        elif p[0] == "off":
            cols.append(off(nb, p[1]))
        elif p[0] == "mid":                                        # every bit at p = 1/2
            cols.append(np.repeat(np.array([4.0] * nb + [HOP])[:, None], p[1], axis=1))
        else:
            cols.append(frames_of(ids[p[0]], p[1]))
    return np.concatenate(cols, axis=1).astype(np.float32)


def bits_of(prob):
    return "".join("1" if p >= 0.5 else "0" for p in prob)


def synthetic_cases(nb: int, W: int):
    """-> [dict(name, fsum [nb + 1, Fr], rule, min_on, G, ml, last_valid, want [(lo, hi, (start, end) flags, bits or None)])], written down
    by hand; largest: the test also checks that the one cut lies at the largest S of the run.  Most runs start at frame 2."""
    ids = IDS4 if nb == 4 else IDS16
    nd = sum(a != b for a, b in zip(ids["A"], ids["B"]))
    rule = SplitRule(W, 0.5, 1)
    base = dict(rule=rule, min_on=0.5, G=2, ml=min(W, 5), last_valid=HOP)
    P = 2
    cases = [
        dict(base, name="two ids", fsum=build(nb, [("off", P), ("A", 3 * W), ("B", 3 * W), ("off", 3)]),
             want=[(P, P + 3 * W, (False, True), ids["A"]), (P + 3 * W, P + 6 * W, (True, False), ids["B"])]),
        dict(base, name="three ids", fsum=build(nb, [("off", P), ("A", 3 * W), ("B", 3 * W), ("C", 3 * W), ("off", 3)]),
             want=[(P, P + 3 * W, (False, True), ids["A"]), (P + 3 * W, P + 6 * W, (True, True), ids["B"]),
                   (P + 6 * W, P + 9 * W, (True, False), ids["C"])]),
        # one frame of A1 (one bit from A) at either edge: S(W) = 0.75 / W < 0.5, and no nearer boundary is a candidate
        dict(base, name="a change one frame from either edge", fsum=build(nb, [("off", P), ("A1", 1), ("A", 3 * W), ("A1", 1), ("off", 3)]),
             want=[(P, P + 3 * W + 2, (False, False), None)]),
        # a strong change W - 1 frames from the start: the nearest candidate is W, and that is where the cut falls; no piece is shorter than W
        dict(base, name="a strong change nearer than W to the start", fsum=build(nb, [("off", P), ("A", W - 1), ("B", 3 * W), ("off", 3)]),
             want=[(P, P + W, (False, True), None), (P + W, P + 4 * W - 1, (True, False), ids["B"])]),
        dict(base, name="the vote fails: min_bits above the differing bits", rule=SplitRule(W, 0.5, nd + 1),
             fsum=build(nb, [("off", P), ("A", 3 * W), ("B", 3 * W), ("off", 3)]), want=[(P, P + 6 * W, (False, False), None)]),
        # the gap's frame carries no gated sample, so the boundaries before and after it have the same two window means: a tie, the earlier stays
        dict(base, name="a change inside a merged gap", fsum=build(nb, [("off", P), ("A", 3 * W), ("off", 1), ("B", 3 * W), ("off", 3)]),
             want=[(P, P + 3 * W, (False, True), ids["A"]), (P + 3 * W, P + 6 * W + 1, (True, False), ids["B"])]),
        dict(base, name="the run closes with a cut pending", fsum=build(nb, [("off", P), ("A", 3 * W), ("B", W + 1), ("off", 3)]),
             want=[(P, P + 3 * W, (False, True), ids["A"]), (P + 3 * W, P + 4 * W + 1, (True, False), ids["B"])]),
        dict(base, name="final with a cut pending", fsum=build(nb, [("off", P), ("A", 3 * W), ("B", W + 1)]),
             want=[(P, P + 3 * W, (False, True), ids["A"]), (P + 3 * W, P + 4 * W + 1, (True, False), ids["B"])]),
        dict(base, name="a partial last frame", last_valid=3,
             fsum=build(nb, [("off", P), ("A", 3 * W), ("B", 3 * W - 1), frames_of(ids["B"], 1, 3.0)]),
             want=[(P, P + 3 * W, (False, True), ids["A"]), (P + 3 * W, P + 6 * W, (True, False), ids["B"])]),
        # min_on = 0: every frame is on, also those without a gated sample; a window of W such frames has no mean and its boundary cannot qualify
        dict(base, name="zero-count windows under min_on = 0", min_on=0.0,
             fsum=build(nb, [("A", 2 * W), ("off", W), ("B", 2 * W)]),
             want=[(0, 2 * W + 1, (False, True), ids["A"]), (2 * W + 1, 5 * W, (True, False), ids["B"])]),
        # two changes d < W apart, A -> A1 -> C: every boundary between them qualifies; ONE cut, at the largest S
        dict(base, name="two changes nearer than W", fsum=build(nb, [("off", P), ("A", 3 * W), ("A1", W - 1), ("C", 3 * W), ("off", 3)]),
             want=[(P, P + 4 * W - 1, (False, True), None), (P + 4 * W - 1, P + 7 * W - 1, (True, False), ids["C"])], largest=True),
    ]
    if W == 4:
        # a frame with every mean at 1/2 between A and B: with W a power of two the boundaries before and after it have the SAME S, bit for bit
        cases.append(dict(base, name="equal S at two boundaries", fsum=build(nb, [("off", P), ("A", 3 * W), ("mid", 1), ("B", 3 * W), ("off", 3)]),
                          want=[(P, P + 3 * W, (False, True), ids["A"]), (P + 3 * W, P + 6 * W + 1, (True, False), ids["B"])]))
    return cases


# ---- tick partitions ----------------------------------------------------------------------------------------------------------------------
def partitions(n_frames: int, cuts, W: int, seed, partial: bool):
    """-> {name: [(f_lo, f_hi)]}: one tick, one frame per tick, seeded random cuts (SC.chunks_of's, empty ticks among them) and, for every
    absolute boundary g in `cuts`, ticks that end at g, g - W, g + W and g + 2 W - 1 (the frame that makes the cut known) and one frame on."""
    rng = np.random.default_rng(SC.seed_of("split-partitions", seed))
    out = {"whole": [(0, n_frames)], "frames": SC.chunks_of(n_frames, "frames", rng, partial)}
    for i in range(3):
        out[f"random{i}"] = SC.chunks_of(n_frames, "random", rng, partial)
    for g in cuts:
        for name, e in (("g", g), ("g-W", g - W), ("g+W", g + W), ("g+2W-1", g + 2 * W - 1), ("g+2W", g + 2 * W)):
            if 0 < e < n_frames:
                out[f"{name}@{g}"] = [(0, e), (e, n_frames)]
        edges = sorted({e for e in (g - W, g, g + W, g + 2 * W - 1, g + 2 * W) if 0 < e < n_frames})
        out[f"all@{g}"] = list(zip([0] + edges, edges + [n_frames]))
    return out


def same_events(got, want):
    """SC.same_events, and the flags."""
    diff = SC.same_events(got, want)
    if diff is None:
        for s, (g, w) in enumerate(zip(got, want)):
            for a, b in zip(g, w):
                if tuple(a[4]) != tuple(b[4]):
                    return f"stream {s} piece {a[:2]}: flags {a[4]} against {b[4]}"
    return diff


def same_state(a, b):
    """None, or the difference between two split_state() tuples (lo, hi, plo, pending boundary, pending S, sums), bit for bit."""
    if (a is None) != (b is None):
        return f"open {a is not None} against {b is not None}"
    if a is None:
        return None
    if tuple(a[:4]) != tuple(b[:4]):
        return f"header {a[:4]} against {b[:4]}"
    if np.float64(a[4]).tobytes() != np.float64(b[4]).tobytes():
        return f"pending S {a[4]!r} against {b[4]!r}"
    if np.asarray(a[5], np.float64).tobytes() != np.asarray(b[5], np.float64).tobytes():
        return f"sums {a[5]} against {b[5]}"
    return None


# ---- the kernel fuzz ----------------------------------------------------------------------------------------------------------------------
def random_fsum(S: int, nb: int, Fr: int, W: int, G: int, hop: int, seed):
    """-> (fsum [S, nb + 1, Fr] float32, last_valid): per stream runs of 1 .. 5 W frames of one random id each (a bit's mean 0.1 .. 0.9 on its
    id's side, noisy frame by frame, not quantized: the adds round), abutting or parted by 1 .. G + 1 off frames; counts between hop / 2 and
    hop, now and then 0 inside a run; the last frame partial in every second case."""
    rng = np.random.default_rng(SC.seed_of("split-fuzz", S, nb, Fr, W, G, seed))
    last_valid = hop if seed % 2 == 0 else int(rng.integers(1, hop))
    out = np.zeros((S, nb + 1, Fr), np.float32)
    for s in range(S):
        f = int(rng.integers(0, 3))
        while f < Fr:
            n = int(rng.integers(1, 5 * W + 1))
            bits = rng.integers(0, 2, nb)
            strength = rng.uniform(0.1, 0.4)
            for j in range(f, min(Fr, f + n)):
                c = float(rng.integers(hop // 2 + 1, hop + 1)) if rng.integers(0, 12) else 0.0
                p = np.clip(0.5 + (2 * bits - 1) * strength + rng.normal(0, 0.08, nb), 0.0, 1.0)
                out[s, :nb, j] = (p * c).astype(np.float32)
                out[s, nb, j] = c
            f += n
            if rng.integers(0, 2):
                f += int(rng.integers(1, G + 2))
        out[s, nb, Fr - 1] = min(out[s, nb, Fr - 1], last_valid)
        out[s, :nb, Fr - 1] = np.minimum(out[s, :nb, Fr - 1], out[s, nb, Fr - 1])
    return out, last_valid


# ---- the routes' recording ----------------------------------------------------------------------------------------------------------------
# One gated stretch [ROUTE_ON) of each stream holds two unlike signals: quiet noise up to the boundary frame ROUTE_CUT, then loud noise over a low tone
# (broadband like the clips every other bar of the exact path was measured on: a pure loud tone alone costs the f32 nets more than 1e-5).
# The nets are the small session nets with random weights.  Such a detector's bits are set by the head's biases (every mean probability
# stays on its side of 1/2 whatever the input, so d(g) = 0 everywhere and no rule could fire); the route nets therefore have
# last_layer.bias set to ZERO, which leaves the input to decide the bits.  Nothing is decoded (the nets are untrained) and the cut need not
# fall on ROUTE_CUT: what the tests hold the routes to is the float64 oracle's frame sums put through the host twin.  The thresholds were
# read off the oracle's S curves (they lie in a gap of the values); test_split_cases_cpu recomputes every margin on that oracle.
ROUTE_FRAMES = 40
ROUTE_ON = (3, 35)
ROUTE_CUT = 19
ROUTE_W, ROUTE_G, ROUTE_ML = 5, 2, 3
ROUTE_LOCATORS = {"x0.detector": "x0.locator", "x9.detector": "x13.locator", "x13.detector": "x13.locator", "h.detector": "h.locator"}
ROUTE_THRESHOLDS = {"x0.detector": 0.37, "x9.detector": 0.30, "x13.detector": 0.35, "h.detector": 0.11}
# which route_signal streams a net is given, and whether their second signal is the pure tone: the full-size f16 detector tells a loud tone
# from noise but hardly one noise from another, and its bar (det_mean_bar) has room for what a pure tone costs
ROUTE_SIGNALS = {"x0.detector": ((0, 1), False), "x9.detector": ((2, 3), False), "x13.detector": ((0, 1), False), "h.detector": ((3, 4), True)}
ROUTE_NETS = ("x0.detector", "x9.detector", "x13.detector")
ROUTE_F16 = ("h.detector",)


def route_rule(det_id: str) -> SplitRule:
    return SplitRule(ROUTE_W, ROUTE_THRESHOLDS[det_id], 1)


def route_state_dict(sd: dict) -> dict:
    """A detector's state dict with the head's biases at zero (see above)."""
    sd = dict(sd)
    b = sd["last_layer.bias"]
    sd["last_layer.bias"] = b * 0
    return sd


def route_signal(hop: int, stream: int = 0, tone: bool = False):
    """-> (x [T] float32, gate [T] float32), T = ROUTE_FRAMES * hop + hop // 2: the last frame is partial."""
    T = ROUTE_FRAMES * hop + hop // 2
    rng = np.random.default_rng(SC.seed_of("split-route", stream))
    t = np.arange(T)
    cut = ROUTE_CUT * hop
    sine = np.sin(2 * np.pi * (0.011 + 0.002 * stream) * t)
    noise = rng.standard_normal(T)                                  # drawn either way, so that the quiet part does not depend on `tone`
    loud = 0.8 * sine if tone else np.clip(0.25 * noise, -1, 1) + 0.1 * sine
    x = np.where(t < cut, 0.05 * rng.standard_normal(T), loud).astype(np.float32)
    gate = np.zeros(T, np.float32)
    gate[ROUTE_ON[0] * hop:ROUTE_ON[1] * hop] = 1.0
    return x, gate


def route_reference(det_id: str):
    """-> (cfg, state dict, x [S, T] float32, gate [S, T] float32, oracle frame sums [S, nb + 1, Fr] float64): the float64 oracle for an exact
    net, the f16 mode's own oracle for an f16 net (tests/test_gpu_segment_bank._mixed_reference takes them the same way)."""
    import window_cases as W
    from localized_cases import frame_sums_from_probs, frame_sums_ref
    case = {c[0]: c for c in W.net_cases()}[det_id]
    cfg, seed = W.net_config(case)
    hop = cfg.hop_length
    streams, tone = ROUTE_SIGNALS[det_id]
    xs, gs = zip(*[route_signal(hop, s, tone) for s in streams])
    x, gate = np.stack(xs), np.stack(gs)
    if case[1] == "f32":
        from oracle import wv_oracle as O
        sd = route_state_dict(W.oracle_net(case)[1])
        whole = frame_sums_ref(W.oracle_forward(cfg, O._Net(cfg, sd, np.float64), x[:, None]), gate, 0.5, hop, x.shape[1])
    else:
        from waveverify_amd.init import random_state_dict
        sd = route_state_dict(random_state_dict(cfg, seed))
        whole = frame_sums_from_probs(_f16_probs(cfg, sd, x), gate, 0.5, hop, x.shape[1])
    return cfg, sd, x, gate, np.asarray(whole, np.float64)


def route_events(det_id: str, whole):
    """The oracle's frame sums through the float64 host twin -> (per stream events, the twin's margins)."""
    from waveverify_amd.localize import SegmentTracker
    import window_cases as W
    S, nb1, Fr = whole.shape
    hop = W.net_config({c[0]: c for c in W.net_cases()}[det_id])[0].hop_length
    t = SegmentTracker(S, nb1 - 1, hop, 0.5, ROUTE_G, ROUTE_ML, dtype=np.float64, split=route_rule(det_id))
    t.advance(whole, 0, Fr, hop // 2, True)
    return t.poll(), t.margins


# ---- the same recordings with the LOCATOR gating (no caller's gate) ---------------------------------------------------------------------------
# A sample is gated when its locator logit exceeds gate_threshold(p).  One sample that falls on the other side changes a frame's sums by a
# whole sigmoid, far more than any bar, so p sits in the middle of a GAP of the float64 oracle's logits over the recording (LOC_P, read off the
# sorted logits near their lower quintile, so that most frames are on at min_on = 0.5): test_split_cases_cpu asserts that no logit lies
# within LOC_LOGIT_MARGIN of the threshold, twice the 1e-4 by which a windowed exact locator may differ from the whole-clip one
# (segment_session_cases).  With every sample on its oracle's side the counts are the oracle's exactly, and so are the frames' on / off
# decisions.  The f16 detector runs behind the EXACT locator here: the f16 locator's logits are 1e-3 from their oracle's, more than any gap
# between 25 920 logits.  The rule's thresholds, again from the oracle's S curves; the CPU test recomputes their margins.
LOC_LOGIT_MARGIN = 2e-4
LOC_MIN_ON = 0.5
LOC_P = {"x0.detector": 0.037156, "x9.detector": 0.200781, "x13.detector": 0.172948, "h.detector": 0.067928}
LOC_THRESHOLDS = {"x0.detector": 0.42, "x9.detector": 0.32, "x13.detector": 0.49, "h.detector": 0.17}


def loc_rule(det_id: str) -> SplitRule:
    return SplitRule(ROUTE_W, LOC_THRESHOLDS[det_id], 1)


def loc_reference(det_id: str):
    """-> (cfg, detector state dict, locator cfg, locator state dict, x [S, T], the oracle's locator logits [S, T] float64, its frame sums
    [S, nb + 1, Fr] float64 under the gate logit > gate_threshold(LOC_P[det_id]))."""
    import window_cases as W
    from localized_cases import frame_sums_from_probs, frame_sums_ref
    from oracle import wv_oracle as O
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.localize import gate_threshold
    nets = {c[0]: c for c in W.net_cases()}
    cfg, sd, x, _, _ = route_reference(det_id)
    lcase = nets[ROUTE_LOCATORS[det_id]]
    lcfg, lseed = W.net_config(lcase)
    lsd = W.oracle_net(lcase)[1] if lcase[1] == "f32" else random_state_dict(lcfg, lseed)
    lg = O.locator_forward(lcfg, O._Net(lcfg, lsd, np.float64), x[:, None], dtype=np.float64)[:, 0]
    gate = (lg > gate_threshold(LOC_P[det_id])).astype(np.float32)
    hop = cfg.hop_length
    if nets[det_id][1] == "f32":
        whole = frame_sums_ref(W.oracle_forward(cfg, O._Net(cfg, sd, np.float64), x[:, None]), gate, 0.5, hop, x.shape[1])
    else:
        whole = frame_sums_from_probs(_f16_probs(cfg, sd, x), gate, 0.5, hop, x.shape[1])
    return cfg, sd, lcfg, lsd, x, lg, np.asarray(whole, np.float64)


def _f16_probs(cfg, sd, x):
    from localized_cases import sigmoid64
    from oracle import wv_oracle_h16 as O16
    from oracle import wv_oracle_torch as OT
    onet = OT.Net(cfg, sd)
    if O16.head16_gate(cfg):
        return O16.head16_probs(O16.encoder_latent(onet, OT._t(x[:, None]).double(), None), *O16.head_weights(onet))
    return sigmoid64(O16.detect_logits(onet, x[:, None]).double().numpy())


def loc_events(det_id: str, whole):
    """The oracle's locator-gated frame sums through the float64 host twin -> (per stream events, the twin's margins)."""
    import window_cases as W
    from waveverify_amd.localize import SegmentTracker
    S, nb1, Fr = whole.shape
    hop = W.net_config({c[0]: c for c in W.net_cases()}[det_id])[0].hop_length
    t = SegmentTracker(S, nb1 - 1, hop, LOC_MIN_ON, ROUTE_G, ROUTE_ML, dtype=np.float64, split=loc_rule(det_id))
    t.advance(whole, 0, Fr, hop // 2, True)
    return t.poll(), t.margins
