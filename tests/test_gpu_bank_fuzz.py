"""The bank layer on the MI355X under the generated schedules of tests/bank_fuzz_cases.py (tests/test_bank_fuzz_cases_cpu.py shows what they
cover): session banks, segment banks, native-rate banks, EmbedBank.set_message and set_split, each stream held to its own whole input.

a. Embed / Locate / Detect banks on every small session net against the FLOAT64 ORACLE on each stream's whole input, at pad_limit 1.0, 1.5 and
   infinite, at tests/test_gpu_session_bank.py's bars (its _check_bank plays the steps): GEN_BAR 5e-5 and LOGIT_BAR32 1e-4 of the
   reference's largest magnitude, MEAN_BAR 1e-6.
b. The f16 banks against oracle/wv_oracle_h16 at WM_BAR, LOGIT_BAR16 and det_mean_bar(T).
c. A host StreamBank with an identity forward played step for step beside the device bank: the device histories [capacity, hcap] (and a gated
   SegmentBank's gate histories) bit-equal to the host's over the whole array after every step, DetectBank._seen equal to the host's counts;
   open() on the full bank and a push to a closed slot raise before any launch and change none of it.
d. At pad_limit 1.0 every result of every stream bit-equal to the same stream replayed alone in a fresh bank of one slot: no neighbour and no
   earlier stream of the slot reaches it.
e. SegmentBank on test_gpu_segment_bank's small-net pairs, gated and locator-driven, event rings of 2 and 64, without a rule and under a
   SplitRule (rings of 6 and 64: set_split takes no smaller one): frames and counts equal to the float64 reference's, prob within MEAN_BAR.
   The locator-driven form's threshold lies in the widest gap of the reference's logits, wider than the locator's bar (asserted on the
   reference), so every gate decision is the reference's.  Held to the reference: no rule, and a rule that never fires (a random detector's
   bits are set by its head's biases).  Held to (d): a rule that does fire, on the detector with the head's biases at zero.
f. The four native banks in f32 and f16 under random_native_schedule: bit-equal to the 16 kHz bank behind the front stage, the embed bank also
   within test_gpu_native_bank's bars of embed_native_batch on each stream's whole recording.
g. EmbedBank under random_switch_plan against float64 span embedding at GEN_BAR, the input's bits outside the spans, no generator launch on a
   tick where only pass-through slots complete frames.
h. wv_bank_advance and wv_bank_detect_update on generated tables (guarded arenas at offsets 0 and 1) against numpy_bank_advance and the
   sequential f64 loop.

Every figure is printed as a MEASURE line before it is asserted (pytest -s).

MEASURED on the MI355X, the worst case per kind over the file (test_print_the_worst_cases prints them); no bar is wider than where it came from:
    exact    EmbedBank 6.2e-7 (GEN_BAR 5e-5) and LocateBank logits 6.4e-6 (LOGIT_BAR32 1e-4) of the reference's largest magnitude over the
             schedule's streams, DetectBank mean probability 1.6e-7 (MEAN_BAR 1e-6), EmbedBank with switches 1.2e-6 (GEN_BAR 5e-5)
    f16      EmbedBank 3.8e-5 absolute (WM_BAR 1e-4), LocateBank logits 1.2e-4 of max(1, |logits|max) (LOGIT_BAR16 1e-3), DetectBank mean
             probability 0.21 of det_mean_bar(T)
    segment  prob 1.2e-7 gated, 6.0e-8 locator-driven (MEAN_BAR 1e-6); the locator-driven thresholds sit in gaps of 2.3e-3 to 1.2e-2 of the
             reference's logits, 8 to 23 times the locator's bar; 14 to 160 segments per pair and form end or start at a cut in (d)
    native   embed bank against embed_native_batch 3.0e-7 in f32 and 0 in f16 (bar 2e-5), the f16 bank against the exact route 3.8e-5
             (WM_BAR 1e-4)
Everything else in the file is bit equality.  The slowest test takes 3.5 s (the f16 detector banks: an oracle run per checked state)."""
import functools

import numpy as np
import pytest
import torch

import bank_cases as BK
import bank_fuzz_cases as BF
import segment_bank_cases as SB
import span_cases as SP
import window_cases as W
from guard import Guards
from localized_cases import frame_sums_ref
from test_gpu_session_bank import (EXACT, F16, GEN_BAR, LOGIT_BAR32, MEAN_BAR, WORST, _abi, _bank, _check_bank, _inout, _net, _play, _same,
                                   _tick, bits, cu, measure)
from waveverify_amd.session import StreamBank, numpy_bank_advance
from waveverify_amd.window import halo

pytestmark = pytest.mark.gpu

TAG = "fuzz "
CAP = BF.CAPACITY
EXACT_PARAMS = [(c, s) for c in EXACT for s in BF.SEEDS]
F16_PARAMS = [(c, s) for c in F16 for s in BF.F16_SEEDS]


def _pid(params):
    return [f"{c[0]}-seed{s}" for c, s in params]


def _steps(cid, seed):
    cfg = _net(cid)[1]
    return BF.random_schedule(cfg.hop_length, halo(cfg), seed)


# =============================================================================================== a. / b. the banks against their oracles
def _vs_oracle(case, seed, precision):
    steps = _steps(case[0], seed)
    stats = [_check_bank(case[0], f"fuzz-seed{seed}", pad, precision, steps, CAP, TAG).stats for pad in BK.PAD_LIMITS]
    a, b, c = stats
    assert a["launches"] >= b["launches"] >= c["launches"] and a["padded_samples"] == 0 <= b["padded_samples"] <= c["padded_samples"]
    assert a["ticks"] == b["ticks"] == c["ticks"] > 0


@pytest.mark.parametrize("case,seed", EXACT_PARAMS, ids=_pid(EXACT_PARAMS))
def test_fuzz_banks_vs_float64(case, seed):
    _vs_oracle(case, seed, "f32")


@pytest.mark.parametrize("case,seed", F16_PARAMS, ids=_pid(F16_PARAMS))
def test_fuzz_banks_f16_vs_their_oracle(case, seed):
    _vs_oracle(case, seed, "f16")


# =============================================================================================== c. the state mirror
def _mirror(dev, host, steps, xs, ghost=None, gates=None, open_args=lambda n: ()):
    """Plays the steps on the device bank and on the host bank(s) side by side; after every step the device's histories are the host's."""
    slot, pos, n_full, n_closed = {}, {}, 0, 0

    def check(what):
        assert np.array_equal(bits(dev._hist), host._hist.view(np.int32)), what
        assert [(t.t_in, t.t_out, t.h0, t.closed) for t in dev._tickers] == [(t.t_in, t.t_out, t.h0, t.closed) for t in host._tickers], what
        if ghost is not None:
            assert np.array_equal(bits(dev._ghist), ghost._hist.view(np.int32)), what
        if hasattr(dev, "_seen"):
            assert dev._seen.cpu().tolist() == [t.t_out for t in host._tickers], what
    for i, (kind, arg) in enumerate(steps):
        what = f"step {i} {kind} {arg}"
        if kind == "open":
            slot[arg], pos[arg] = dev.open(*open_args(arg)), 0
            assert host.open() == slot[arg] and (ghost is None or ghost.open() == slot[arg])
        elif kind == "close":
            dev.close(slot[arg]), host.close(slot[arg])
            if ghost is not None:
                ghost.close(slot[arg])
            check(what)
            one = torch.zeros(1, device="cuda")
            with pytest.raises(ValueError, match="not open"):                     # raises before any launch
                dev.push({slot[arg]: one if gates is None else (one, one)})
            n_closed += 1
        else:
            if len(dev.open_slots()) == dev.capacity:
                with pytest.raises(RuntimeError, match="slots"):                  # raises before any launch
                    dev.open(*open_args("A"))
                n_full += 1
                check(what + " after the refused open")
            span = {n: (pos[n], pos[n] + m) for n, m in arg.items()}
            dev.push({slot[n]: (cu(xs[n][a:b]) if gates is None else (cu(xs[n][a:b]), cu(gates[n][a:b]))) for n, (a, b) in span.items()})
            host.push({slot[n]: xs[n][a:b] for n, (a, b) in span.items()})
            if ghost is not None:
                ghost.push({slot[n]: gates[n][a:b] for n, (a, b) in span.items()})
            for n, (a, b) in span.items():
                pos[n] = b
        check(what)
    assert dev.open_slots() == host.open_slots() == []
    return n_full, n_closed


MIRROR = ["x14.generator", "x0.detector", "x13.locator"]


@pytest.mark.parametrize("cid", MIRROR)
def test_device_histories_are_the_host_banks_bit_for_bit(cid):
    case, cfg, net, _ = _net(cid)
    hop, H = cfg.hop_length, halo(cfg)
    n_full = 0
    for seed in BF.SEEDS:
        steps = _steps(cid, seed)
        data = BK.stream_data(case, steps)
        xs = {n: x for n, (x, _) in data.items()}
        for pad in BK.PAD_LIMITS:
            dev = _bank(net, cfg.kind, "f32", pad, CAP)
            host = StreamBank(CAP, hop, H, lambda win, slots: win, numpy_bank_advance, None, pad)
            full, closed = _mirror(dev, host, steps, xs, open_args=(lambda n: (data[n][1],)) if cfg.kind == "generator" else (lambda n: ()))
            n_full += full
            assert closed == len(xs) and dev.stats == host.stats
    assert n_full > 0                                                              # the full bank did refuse an open


# =============================================================================================== d. isolation at pad_limit 1.0
def _alone(steps, name):
    return [(k, ({name: a[name]} if k == "push" else a)) for k, a in steps if (k == "push" and name in a) or (k != "push" and a == name)]


ISOLATION = EXACT_PARAMS + F16_PARAMS


@pytest.mark.parametrize("case,seed", ISOLATION, ids=_pid(ISOLATION))
def test_a_stream_beside_others_is_the_stream_alone_bit_for_bit(case, seed):
    """pad_limit 1.0: every row of a launch has one wlen, so only the number of rows differs between the bank and the stream alone."""
    case, cfg, net, _ = _net(case[0])
    kind, precision = cfg.kind, case[1]
    steps = _steps(case[0], seed)
    data = BK.stream_data(case, steps)
    out = _play(_bank(net, kind, precision, 1.0, CAP), kind, steps, data)
    compared = 0
    for name in data:
        alone = _play(_bank(net, kind, precision, 1.0, 1), kind, _alone(steps, name), data)[name]
        assert len(alone) == len(out[name])
        for i, ((k, p, got), (k2, p2, want)) in enumerate(zip(out[name], alone)):
            assert (k, p) == (k2, p2)
            _same(got, want, kind, f"{case[0]} seed {seed} stream {name} step {i} ({k} at {p}) beside others against alone")
            compared += 1
    assert compared > len(data)


# =============================================================================================== e. segment banks
from test_gpu_segment_bank import NETS, PAIRS, _hip as _seg_hip  # noqa: E402

SEG_SEED = BF.SEEDS[0]
FORMS = [(d, l, gated) for d, l in PAIRS for gated in (True, False)]


def _seg_key(s):
    return (s.frames, s.start_s, s.end_s, s.coverage, s.confidence, s.change, s.prob.tobytes())


@functools.lru_cache(maxsize=None)
def _segment_reference(det_id, loc_id, gated):
    """-> (steps, xs, gates or None, threshold as a probability, G, ml, {stream: the whole-recording tracker's events in float64}, hop)."""
    from waveverify_amd.session import segment_halo
    dcfg, lcfg = _seg_hip(det_id)[0], _seg_hip(loc_id)[0]
    hop = dcfg.hop_length
    steps = BF.random_schedule(hop, segment_halo(dcfg, lcfg), SEG_SEED)
    xs = {n: W.clip_data(NETS[det_id], max(T, 1), 300 + i)[0][0, 0, :T] for i, (n, T) in enumerate(BK.stream_lengths(steps).items())}
    dnet, lnet = W.oracle_net(NETS[det_id])[2], W.oracle_net(NETS[loc_id])[2]
    if gated:
        G, ml, thr, p = 1, 1, 0.5, 0.5
        gates = {n: BF.random_gate(len(x), hop, SEG_SEED) for n, x in xs.items()}
        gsrc = {n: g[None] for n, g in gates.items()}
    else:
        G, ml, gates = 2, 2, None
        gsrc = {n: W.oracle_forward(lcfg, lnet, x[None, None])[:, 0] for n, x in xs.items() if x.size}
        every = np.concatenate([g[0] for g in gsrc.values()])
        thr, margin = BF.gap_threshold(every)
        p = 1.0 / (1.0 + np.exp(-thr))
        from waveverify_amd.localize import gate_threshold
        bar = LOGIT_BAR32 * float(np.abs(every).max())
        print(f"MEASURE {det_id} locator-driven: threshold {thr:.6f} in a gap of +-{margin:.2e} of the reference's logits (the locator's bar: {bar:.2e})")
        assert margin > 2 * bar and abs(gate_threshold(p) - thr) < 1e-9            # on the reference alone: every gate decision is its own
    want = {}
    for n, x in xs.items():
        want[n] = []
        if x.size:
            whole = frame_sums_ref(W.oracle_forward(dcfg, dnet, x[None, None]), gsrc[n], thr, hop, x.size)
            want[n] = SB.lockstep_events(whole[0], hop, x.size - (whole.shape[2] - 1) * hop, 0.5, G, ml, dtype=np.float64)
    return steps, xs, gates, float(p), G, ml, want, hop


def _segment_bank(det, loc, pad, ring, gated, p, G, ml, rule, capacity=CAP):
    from waveverify_amd.session import SegmentBank
    bank = SegmentBank(det, loc, capacity, pad, threshold=p, min_gap_frames=G, min_len_frames=ml, ring=ring, gated=gated)
    if rule is not None:
        bank.set_split(rule)
    return bank


@pytest.mark.parametrize("det_id,loc_id,gated", FORMS, ids=[f"{d}-{'gated' if g else 'locator'}" for d, _, g in FORMS])
def test_fuzz_segment_banks_vs_float64(det_id, loc_id, gated):
    from waveverify_amd.localize import SplitRule
    steps, xs, gates, p, G, ml, want, hop = _segment_reference(det_id, loc_id, gated)
    det, loc = _seg_hip(det_id)[2], _seg_hip(loc_id)[2]
    xt, gt = {n: cu(x) for n, x in xs.items()}, None if gates is None else {n: cu(g) for n, g in gates.items()}
    never = SplitRule(2, 1e9, 1)                                  # the split kernels and their rings, and no cut: the same events
    what = TAG + f"segment bank prob ({'gated' if gated else 'locator-driven'})"
    for rule, rings in ((None, (2, 64)), (never, (6, 64))):
        for ring in rings:
            stats = []
            for pad in BK.PAD_LIMITS:
                bank = _segment_bank(det, loc, pad, ring, gated, p, G, ml, rule)
                got, _ = SB.play(bank, steps, xt, gt, poll_every=3)
                assert bank.open_slots() == []
                stats.append(bank.stats)
                for n, x in xs.items():
                    assert [g.frames for g in got[n]] == [(lo, hi) for lo, hi, _, _ in want[n]], (det_id, rule, ring, pad, n)
                    for g, (lo, hi, cnt, prob) in zip(got[n], want[n]):
                        end = min(hi * hop, x.size)
                        assert g.coverage == cnt / (end - lo * hop) and g.end_s == end / 16000 and g.change == (False, False), (pad, n, g.frames)
                        measure(what, float(np.abs(g.prob.astype(np.float64) - prob).max()), MEAN_BAR)
            assert stats[0]["launches"] >= stats[2]["launches"] and stats[0]["padded_samples"] == 0 <= stats[2]["padded_samples"]
    assert sum(len(w) for w in want.values()) >= 4


@pytest.mark.parametrize("det_id,loc_id,gated", FORMS, ids=[f"{d}-{'gated' if g else 'locator'}" for d, _, g in FORMS])
def test_a_segment_stream_beside_others_is_the_stream_alone(det_id, loc_id, gated):
    """(d) for segment banks at pad_limit 1.0, without a rule and under one that fires: the detector's head has its biases at zero so that
    the input decides the bits (tests/split_cases.py says why); nothing is held to a reference here, every Segment to the stream alone."""
    from split_cases import route_state_dict
    from waveverify_amd.localize import SplitRule
    from waveverify_amd.nets import HipNet
    steps, xs, gates, p, G, ml, _, hop = _segment_reference(det_id, loc_id, gated)
    dcfg, dsd, _ = _seg_hip(det_id)
    det, loc = HipNet(dcfg, route_state_dict(dsd)), _seg_hip(loc_id)[2]
    xt, gt = {n: cu(x) for n, x in xs.items()}, None if gates is None else {n: cu(g) for n, g in gates.items()}
    n_cut = 0
    for rule, ring in ((None, 2), (SplitRule(2, 0.05, 1), 6), (SplitRule(2, 0.05, 1), 64)):
        got, _ = SB.play(_segment_bank(det, loc, 1.0, ring, gated, p, G, ml, rule), steps, xt, gt, poll_every=3)
        for n in xs:
            alone, _ = SB.play(_segment_bank(det, loc, 1.0, ring, gated, p, G, ml, rule, 1), _alone(steps, n), xt, gt, poll_every=0)
            assert [_seg_key(s) for s in got[n]] == [_seg_key(s) for s in alone[n]], (det_id, gated, rule, ring, n)
            n_cut += sum(1 for s in got[n] if any(s.change))
    print(f"MEASURE {det_id} {'gated' if gated else 'locator-driven'}: {n_cut} segments at a cut, all bit-equal to the stream alone")


def test_a_gated_segment_banks_gate_history_is_the_host_banks():
    """(c) for the second history of a gated SegmentBank: it goes through wv_bank_advance with the samples' descriptor rows."""
    det_id, loc_id = PAIRS[0]
    steps, xs, gates, p, G, ml, _, hop = _segment_reference(det_id, loc_id, True)
    det, loc = _seg_hip(det_id)[2], _seg_hip(loc_id)[2]
    for pad in BK.PAD_LIMITS:
        dev = _segment_bank(det, loc, pad, 64, True, p, G, ml, None)
        host, ghost = (StreamBank(CAP, hop, dev.H, lambda win, slots: win, numpy_bank_advance, None, pad) for _ in range(2))
        _mirror(dev, host, steps, xs, ghost=ghost, gates=gates)


# =============================================================================================== f. native banks
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("kind", ["embed", "detect", "locate", "segment"])
@pytest.mark.parametrize("seed", BF.NATIVE_SEEDS[:2])
def test_fuzz_native_banks_are_the_16k_bank_behind_the_front_stage(seed, kind, precision):
    """tests/test_gpu_native_bank.py's two claims for its mixed schedule, on random_native_schedule."""
    import native_bank_cases as NBC
    from test_gpu_native_bank import (WM_BAR, RecordingEmbedBank, clip_data, counters_say_one_launch_per_stage_and_tick, message, nets, play_16k,
                                      same_state, seg_key, small_wv)
    from waveverify_amd import native
    from waveverify_amd import native_bank as NB
    from waveverify_amd.session import DetectBank, EmbedBank, LocateBank, SegmentBank, segment_halo
    gen, det, loc = nets(precision)
    net = {"embed": gen, "detect": det, "locate": loc, "segment": det}[kind]
    H = segment_halo(det.cfg, loc.cfg) if kind == "segment" else halo(net.cfg)
    steps, who = BF.random_native_schedule(net.cfg.hop_length, H, seed)
    xs = clip_data(steps, who, seed=20 + seed)
    Cm = NBC.MAX_CHANNELS
    cat = lambda a, b: torch.cat([a, b])                                      # noqa: E731
    if kind == "embed":
        gains = {n: (1.0, 0.37)[i % 2] for i, n in enumerate(who)}

        class Bank(RecordingEmbedBank):
            def open(self, name, **kw):
                return super().open(message(gen, name), strength=gains[name], **kw)
        bank = Bank(gen, NBC.RATES, CAP, Cm, precision)
        out, slot = NBC.run(bank, steps, xs, who, open_args=lambda n: (n,))
        ref = play_16k(EmbedBank(gen, CAP, precision, 1.5, None, add_input=False), steps, xs, who, lambda n: (message(gen, n),), cat)
        taken = {s: list(v) for s, v in bank.residuals.items()}                    # slots are reused: the residuals per slot in stream order
        w = small_wv("x6.generator" if precision == "f32" else "h.generator")
        for n in out:
            got_r = [taken[slot[n]].pop(0) for _ in out[n]]
            assert len(got_r) == len(ref[n])
            for i, (a, b) in enumerate(zip(got_r, ref[n])):
                assert a.shape == b.shape and torch.equal(a, b), f"embed {precision} stream {n} step {i}: not the 16 kHz bank's residual"
            y = torch.cat([r for _, _, r in out[n]], dim=1)
            assert y.shape == xs[n].shape
            if not xs[n].shape[1]:
                continue
            want = native.upsample_add(xs[n][None], torch.cat(got_r)[None], who[n][0], gains[n])[0]
            assert torch.equal(y, want), f"embed {precision} stream {n}: not upsample_add of its residual"
            msg = cu(message(gen, n)[None])
            w.set_precision(precision)
            try:
                e = float((y.double() - w.embed_native_batch(xs[n][None], who[n][0], msg, gains[n])[0].double()).abs().max())
                measure(TAG + f"native embed bank {precision} against embed_native_batch", e, 2e-5)
                if precision != "f32":
                    w.set_precision("f32")
                    e32 = float((y.double() - w.embed_native_batch(xs[n][None], who[n][0], msg, gains[n])[0].double()).abs().max())
                    measure(TAG + "native embed bank f16 against the exact embed_native_batch", e32, WM_BAR)
            finally:
                w.set_precision("f32")
        assert all(not v for v in taken.values())
        counters_say_one_launch_per_stage_and_tick(bank, True)
        return
    if kind == "segment":
        kw = dict(min_gap_frames=1, min_len_frames=1, precision=precision)
        bank, ref_bank = NB.NativeSegmentBank(det, loc, NBC.RATES, CAP, Cm, **kw), SegmentBank(det, loc, CAP, **kw)
        join = lambda a, b: b                                                 # noqa: E731
    else:
        cls_b, cls_r = (NB.NativeDetectBank, DetectBank) if kind == "detect" else (NB.NativeLocateBank, LocateBank)
        bank, ref_bank = cls_b(net, NBC.RATES, CAP, Cm, precision), cls_r(net, CAP, precision)
        join = (lambda a, b: b) if kind == "detect" else cat
    out, _ = NBC.run(bank, steps, xs, who)
    ref = play_16k(ref_bank, steps, xs, who, lambda n: (), join)
    for n in out:
        assert len(out[n]) == len(ref[n])
        for i, ((_, _, got), want) in enumerate(zip(out[n], ref[n])):
            what = f"{kind} {precision} seed {seed} stream {n} step {i}"
            if kind == "detect":
                same_state(got, want, what)
            elif kind == "locate":
                assert got.shape == want.shape and torch.equal(got, want), what
            elif got is not None or want is not None:
                assert [seg_key(v) for v in got] == [seg_key(v) for v in want], what
    counters_say_one_launch_per_stage_and_tick(bank, False)


# =============================================================================================== g. EmbedBank.set_message
SWITCH = [(cid, seed) for cid in SP.EXACT_IDS for seed in BF.SWITCH_SEEDS]


@pytest.mark.parametrize("cid,seed", SWITCH, ids=[f"{c}-seed{s}" for c, s in SWITCH])
def test_fuzz_embed_bank_with_switches_vs_float64_span_embedding(cid, seed):
    from waveverify_amd.nets import HipNet
    from waveverify_amd.session import EmbedBank
    case = SP.net_case(cid)
    cfg, sd, onet = W.oracle_net(case)
    net = HipNet(cfg, sd)
    hop, H = cfg.hop_length, halo(cfg)
    msgs = SP.messages(cid)
    steps, table = BF.split_msgs(BF.random_switch_plan(BF.random_schedule(hop, H, seed), hop, H, seed))
    data = BK.stream_data(case, steps)
    xs = {n: x for n, (x, _) in data.items()}
    ev, ticks, slot_of, _ = BF.events(steps, hop, H)
    for pad in SP.PAD_LIMITS:
        bank = EmbedBank(net, CAP, "f32", pad)
        state_msg = lambda st: None if st is None else msgs[st]                   # noqa: E731
        out, marks, launches, only = SP.run_switching(bank, steps, xs, table, lambda st: bank.open(state_msg(st)),
                                                      lambda slot, st: bank.set_message(slot, state_msg(st)), take=cu)
        assert len(launches) == len(ticks)
        for k, (now, _) in enumerate(ticks):                                      # a tick's launches, from the tickers and the plan
            who = [n for n, s in slot_of.items() if s in now and now[s].wlen > 0 and _open_at(steps, n, k)]
            net_rows = [n for n in who if table[n][k] is not None]
            assert (launches[k] == 0) == (not net_rows), (pad, k, who, net_rows, launches[k])
        assert all(n == 0 for n, o in zip(launches, only) if o)
        for n, x in xs.items():
            got = torch.cat([r.reshape(-1) for r in out[n]]).cpu().numpy() if out[n] else np.zeros(0, np.float32)
            assert got.shape == x.shape
            if not x.size:
                continue
            assert all(t % hop == 0 for t, _ in marks[n])
            sp = SP.spans_of(marks[n], x.size)
            deltas = {m: _delta(cid, seed, n, m, cfg, onet, x, msgs) for m in {m for _, _, m in sp}}
            ref = SP.reference(x, deltas, sp)
            measure(TAG + "EmbedBank with switches", float(np.abs(got - ref).max()) / float(np.abs(ref).max()), GEN_BAR)
            off = SP.outside(x.size, sp)
            assert np.array_equal(got[off].view(np.int32), x[off].view(np.int32)), (cid, seed, pad, n)   # outside the spans: the input's bits


_DELTAS = {}


def _delta(cid, seed, name, m, cfg, onet, x, msgs):
    """The float64 residual of a stream's whole input under message row m, computed once for the three pad_limits."""
    key = (cid, seed, name, m)
    if key not in _DELTAS:
        _DELTAS[key] = W.oracle_forward(cfg, onet, x[None, None], msgs[m:m + 1], add_input=False)[0, 0]
    return _DELTAS[key]


def _open_at(steps, name, k):
    """Whether stream `name` is open at push step k of the steps."""
    n_push, is_open = 0, False
    for kind, arg in steps:
        if kind == "push":
            if n_push == k:
                return is_open
            n_push += 1
        elif arg == name:
            is_open = kind == "open"
    return False


# =============================================================================================== h. raw tables
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("seed", BF.TABLE_SEEDS)
def test_bank_advance_on_generated_tables_vs_numpy(seed, offset):
    """Beyond each named slot's hv the history holds the guard's NaN pattern, so a read past hv shows in a window or a history; the rows
    taken from bank_cases.bad_rows are skipped whole beside the good ones (_tick compares the whole bank and every window row)."""
    capacity, hcap, A, Lmax, n_x, rows, bad = BF.random_advance_case(seed)
    hist_np, x_np = BK.advance_data((capacity, hcap, A, Lmax, n_x, tuple(r for i, r in enumerate(rows) if i not in bad)), 10 + offset)
    hist = _inout(hist_np, "hist", offset)
    ref_win = _tick(hist, x_np, rows, capacity, hcap, A, Lmax, offset, f"generated table {seed}")
    assert np.isfinite(ref_win).all()
    for i in bad:
        if 0 <= rows[i][0] < capacity:
            assert np.array_equal(bits(hist.t[rows[i][0]]), hist_np[rows[i][0]].view(np.int32)), (seed, rows[i])


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("seed", BF.TABLE_SEEDS)
def test_bank_detect_update_on_generated_tables_vs_a_sequential_f64_loop(seed, offset):
    capacity, nb, rows = BF.random_detect_case(seed)
    lib, st = _abi()
    A = len(rows)
    rng = np.random.default_rng(W.seed_of("bank-fuzz detect data", seed))
    acc_np = rng.uniform(0, 5000, (capacity, nb))
    seen_np = rng.integers(0, 10 ** 7, capacity).astype(np.int64)
    psum_np = (rng.uniform(0, 1, (A, nb)) * rng.integers(1, 5000, (A, 1))).astype(np.float32)
    acc, seen = _inout(acc_np.view(np.int64), "acc", offset), _inout(seen_np, "seen", offset)
    g = Guards(offset=offset)
    psum, desc = g.input(psum_np, "psum"), g.input(np.array(rows, np.int64), "desc")
    mp, bt = g.output((A, nb), name="mean_prob"), g.output((A, nb), torch.int32, name="bits")
    rc = lib.wv_bank_detect_update(acc.t.data_ptr(), seen.t.data_ptr(), capacity, nb, psum.t.data_ptr(), desc.t.data_ptr(), A, mp.t.data_ptr(),
                                   bt.t.data_ptr(), st)
    assert rc == 0, lib.wv_last_error()
    torch.cuda.synchronize()
    racc, rseen = acc_np.copy(), seen_np.copy()
    rmp, rbits, skipped = np.zeros((A, nb), np.float32), np.zeros((A, nb), np.int32), np.zeros((A, nb), bool)
    for r, (slot, samples) in enumerate(rows):
        if not 0 <= slot < capacity:
            skipped[r] = True
            continue
        rseen[slot] += samples
        for k in range(nb):
            racc[slot, k] = racc[slot, k] + float(psum_np[r, k])                  # one f64 add
            rmp[r, k] = np.float32(racc[slot, k] / float(max(int(rseen[slot]), 1)))
            rbits[r, k] = 1 if rmp[r, k] >= np.float32(0.5) else 0
    assert skipped.sum() == 2 * nb
    psum.check(), desc.check()
    mp.check(expect_unwritten=torch.from_numpy(skipped)), bt.check(expect_unwritten=torch.from_numpy(skipped))
    assert not acc.guard_report() and not seen.guard_report()
    assert np.array_equal(acc.t.cpu().numpy(), racc.view(np.int64)) and np.array_equal(seen.t.cpu().numpy(), rseen)   # unnamed slots untouched
    assert np.array_equal(bits(mp.t)[~skipped], rmp.view(np.int32)[~skipped]) and np.array_equal(bt.t.cpu().numpy()[~skipped], rbits[~skipped])


def test_print_the_worst_cases():
    """The last test of the file: the worst figure per kind over what ran before it (pytest -s)."""
    for what, err in sorted(WORST.items()):
        if what.startswith(TAG):
            print(f"WORST {what}: {err:.2e}")
