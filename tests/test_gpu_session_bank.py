"""Session banks (waveverify_amd/session.py EmbedBank / DetectBank / LocateBank, csrc/wv_window.hip wv_bank_advance / wv_bank_detect_update) on
the cases of tests/bank_cases.py.

1. wv_bank_advance through the C ABI on guarded arenas (tests/guard.py), every pointer on a 256-byte boundary and one element past it:
   bit-equal to session.numpy_bank_advance, zero fill to Lmax, unnamed history rows and everything beyond hv2 bit-identical, a history's tail
   never read back; every documented refusal -1 with its own reason and nothing written; every kind of bad row skipped beside good ones.
2. wv_bank_detect_update bit-equal to a sequential float64 loop for 1, 16 and 36 bits.
3. The three banks over every schedule at pad_limit 1.0, 1.5 and infinite against the FLOAT64 ORACLE ON EACH STREAM'S WHOLE INPUT, at the window
   fuzz's bars (5e-5 generator, 1e-4 logits of the reference's largest magnitude, 1e-6 mean probabilities); precision="f16" against
   oracle/wv_oracle_h16 at test_gpu_h16's WM_BAR / LOGIT_BAR / det_mean_bar(T); the 16-channel nets refuse.
4. Streams that push equal sizes: every output and DetectState bit-equal to the lockstep session of the same build, f32 and f16.
5. A stream alone in a bank bit-equal to the same stream beside others; a stream in a reused slot bit-equal to the same stream in a fresh bank.
6. Misuse raises and leaves the bank's other streams bit-equal.

Every figure is printed as a MEASURE line before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import bank_cases as BK
import window_cases as W
from guard import GuardedOutput, Guards
from localized_cases import sigmoid64
from test_gpu_h16 import LOGIT_BAR as LOGIT_BAR16, WM_BAR, det_mean_bar
from waveverify_amd.session import bank_row_ok, numpy_bank_advance

pytestmark = pytest.mark.gpu

GEN_BAR, LOGIT_BAR32 = 5e-5, 1e-4                                 # tests/test_gpu_window_fuzz.py (test_gpu_infer_fuzz.test_whole_nets_fuzz)
MEAN_BAR = 1e-6                                                   # tests/test_gpu_window.py

# MEASURED on the MI355X, the worst case per kind over the whole file (test_print_the_worst_cases prints them); no bar had to be widened.
#   exact   EmbedBank 6.5e-7 (bar 5e-5) and LocateBank logits 1.6e-6 (bar 1e-4) of the reference's largest magnitude over the schedule's
#           streams, DetectBank mean probability 1.2e-7 (bar 1e-6)
#   f16     EmbedBank 3.8e-5 absolute (WM_BAR 1e-4), LocateBank logits 1.1e-4 of max(1, |logits|max) (LOGIT_BAR 1e-3), DetectBank mean
#           probability 0.32 of det_mean_bar(T)
# Everything else in the file is bit equality.

EXACT, F16, F16_REFUSED = BK.net_cases()
NETS = EXACT + F16 + F16_REFUSED


def _ids(cases):
    return [c[0] for c in cases]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


WORST = {}


def measure(what, err, bar):
    WORST[what] = max(WORST.get(what, 0.0), err)
    print(f"MEASURE {what}: {err:.2e} (bar {bar:.1e}; worst so far {WORST[what]:.2e})")
    assert np.isfinite(err) and err <= bar, (what, err, bar)


def rel_err(got, ref, mag):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max()) / mag if ref.size else 0.0


def _abi():
    from waveverify_amd import _lib
    return _lib.load(), _lib.stream()


# =============================================================================================== 1. wv_bank_advance through the C ABI
ADVANCE = BK.advance_cases()


def _inout(array, name, offset):
    """An arena for a buffer the kernel reads AND writes: loaded bit for bit, its guards checked by guard_report()."""
    a = torch.from_numpy(np.ascontiguousarray(array))
    arena = GuardedOutput(tuple(a.shape), a.dtype, "cuda", name, offset)
    arena.tflat.copy_(a.reshape(-1).cuda())
    return arena


def _tick(hist, x_np, rows, capacity, hcap, A, Lmax, offset, what):
    """One call on the arena `hist`; everything it may and may not do, against the numpy restatement."""
    lib, st = _abi()
    rows_np = np.array(rows, np.int64).reshape(-1, 8)
    g = Guards(offset=offset)
    x, desc = g.input(x_np, "x"), g.input(rows_np, "desc")
    win = g.output((A, 1, Lmax), name="win")
    ref_hist = bits(hist.t).view(np.float32).copy()
    ref_win = numpy_bank_advance(ref_hist, x_np, rows_np, A, Lmax)
    rc = lib.wv_bank_advance(hist.t.data_ptr(), capacity, hcap, x.t.data_ptr(), x_np.size, desc.t.data_ptr(), len(rows_np), win.t.data_ptr(), A,
                             Lmax, st)
    assert rc == 0, (what, lib.wv_last_error())
    torch.cuda.synchronize()
    x.check(), desc.check()
    assert not hist.guard_report(), (what, hist.guard_report())
    named = np.zeros((A, 1, Lmax), bool)
    for r in rows_np:
        if bank_row_ok(r, capacity, hcap, x_np.size, A, Lmax) and r[5] > 0:
            named[r[4]] = True
    win.check(expect_unwritten=torch.from_numpy(~named))          # a named row is written up to Lmax, zeros included; no other row at all
    # the whole bank: named slots' [0, hv2) shifted, everything else (unnamed rows, tails beyond hv2) bit for bit as before
    assert np.array_equal(bits(hist.t), ref_hist.view(np.int32)), what
    got = bits(win.t)
    assert np.array_equal(got[named[:, 0, 0]], ref_win.view(np.int32)[named[:, 0, 0]]), what
    return ref_win


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", ADVANCE, ids=[f"hcap{c[1]}" for c in ADVANCE])
def test_bank_advance_vs_numpy(case, offset):
    """Two ticks on one bank.  Beyond each named slot's hv the history holds the guard's NaN pattern, and after the first tick whatever that
    tick left beyond hv2: a kernel that read either would carry it into a window or a history, which the bit comparison shows."""
    capacity, hcap, A, Lmax, n_x, rows, kinds = case
    hist_np, x_np = BK.advance_data(case, offset)
    hist = _inout(hist_np, "hist", offset)
    ref_win = _tick(hist, x_np, rows, capacity, hcap, A, Lmax, offset, f"hcap {hcap} first tick")
    by = dict(zip(kinds, rows))
    assert not ref_win[by["hop"][4], 0, 8:].any() and np.isfinite(ref_win).all()      # the short window beside the longest: zeros to Lmax
    capacity, hcap, A2, Lmax2, n_x2, rows2 = BK.second_tick(case)
    x2 = np.random.default_rng(W.seed_of("bank advance 2", hcap)).standard_normal(n_x2).astype(np.float32)
    ref_win2 = _tick(hist, x2, rows2, capacity, hcap, A2, Lmax2, offset, f"hcap {hcap} second tick")
    assert np.isfinite(ref_win2).all()


@pytest.mark.parametrize("offset", [0, 1])
def test_bank_advance_skips_bad_rows_and_serves_the_good(offset):
    case = BK.advance_case(257)
    capacity, hcap, A, Lmax, n_x, rows, kinds = case
    hist_np, x_np = BK.advance_data(case, 2 + offset)
    i = kinds.index("overlap")
    for why, bad in BK.bad_rows(case):
        hist = _inout(hist_np, "hist", offset)
        _tick(hist, x_np, rows[:i] + (bad,) + rows[i + 1:], capacity, hcap, A, Lmax, offset, why)
        if 0 <= bad[0] < capacity:
            assert np.array_equal(bits(hist.t[bad[0]]), hist_np[bad[0]].view(np.int32)), why


@pytest.mark.parametrize("offset", [0, 1])
def test_bank_advance_refusals(offset):
    """Each documented refusal returns -1 (WV_EINVAL), names itself in wv_last_error() and leaves history and window as they were."""
    lib, st = _abi()
    case = BK.advance_case(255)
    capacity, hcap, A, Lmax, n_x, rows, _ = case
    hist_np, x_np = BK.advance_data(case, 5)
    hist = _inout(hist_np, "hist", offset)
    g = Guards(offset=offset)
    x, desc = g.input(x_np, "x"), g.input(np.array(rows, np.int64), "desc")
    win = g.output((A, 1, Lmax), name="win")
    Hp, Xp, Dp, Wp = hist.t.data_ptr(), x.t.data_ptr(), desc.t.data_ptr(), win.t.data_ptr()
    ok = dict(hist=Hp, capacity=capacity, hcap=hcap, x=Xp, n_x=n_x, desc=Dp, P=len(rows), win=Wp, A=A, Lmax=Lmax)
    refusals = {
        "null hist": (dict(hist=None), "null"),
        "null desc": (dict(desc=None), "null"),
        "samples without x": (dict(x=None), "null"),
        "window rows without win": (dict(win=None), "null"),
        "capacity == 0": (dict(capacity=0), "capacity outside"),
        "capacity beyond the limit": (dict(capacity=(1 << 20) + 1), "capacity outside"),
        "hcap == 0": (dict(hcap=0), "capacity outside"),
        "n_x < 0": (dict(n_x=-1), "capacity outside"),
        "P < 0": (dict(P=-1), "capacity outside"),
        "P == 65536": (dict(P=65536), "capacity outside"),
        "A < 0": (dict(A=-1), "capacity outside"),
        "A == 65536": (dict(A=65536), "capacity outside"),
        "Lmax < 0": (dict(Lmax=-1), "capacity outside"),
        "window rows of no length": (dict(Lmax=0), "capacity outside"),
        "x inside hist": (dict(x=Hp + 4 * hcap), "overlap"),
        "win inside hist": (dict(win=Hp + 4), "overlap"),
        "hist inside win": (dict(hist=Wp, capacity=1, hcap=8), "overlap"),
        "win over x's end": (dict(win=Xp + 4 * (n_x - 1)), "overlap"),
    }
    call = lambda a: lib.wv_bank_advance(a["hist"], a["capacity"], a["hcap"], a["x"], a["n_x"], a["desc"], a["P"], a["win"], a["A"], a["Lmax"], st)
    for why, (change, word) in refusals.items():
        assert lib.wv_bank_detect_update(None, None, 0, 0, None, None, 0, None, None, st) == -1     # another call's reason stands there now
        assert b"wv_bank_detect_update" in lib.wv_last_error()
        rc = call(dict(ok, **change))
        msg = lib.wv_last_error().decode()
        assert rc == -1, (why, rc)
        assert msg.startswith("wv_bank_advance") and word in msg, (why, msg)
        torch.cuda.synchronize()
        win.check(expect_unwritten=torch.ones(win.t.shape, dtype=torch.bool))
        x.check(), desc.check()
        assert not hist.guard_report() and np.array_equal(bits(hist.t), hist_np.view(np.int32)), why
    assert call(dict(ok, P=0)) == 0                               # no rows: success, no launch
    torch.cuda.synchronize()
    win.check(expect_unwritten=torch.ones(win.t.shape, dtype=torch.bool))
    assert np.array_equal(bits(hist.t), hist_np.view(np.int32))
    assert call(ok) == 0                                          # and the call they were all derived from runs
    torch.cuda.synchronize()
    assert not np.array_equal(bits(hist.t), hist_np.view(np.int32))


# =============================================================================================== 2. wv_bank_detect_update
DETECT = BK.detect_cases()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", DETECT, ids=[f"nb{c[1]}" for c in DETECT])
def test_bank_detect_update_vs_a_sequential_f64_loop(case, offset):
    capacity, nb, rows = case
    lib, st = _abi()
    A = len(rows)
    rng = np.random.default_rng(W.seed_of("bank detect", nb))
    acc_np = rng.uniform(0, 5000, (capacity, nb))
    seen_np = rng.integers(1, 10 ** 7, capacity).astype(np.int64)
    acc_np[0], seen_np[0] = 0.0, 0                                # slot 0 has seen nothing and its row adds no samples: the divisor is max(0, 1)
    seen_np[7] = 3000                                             # mean probabilities on both sides of 0.5 ...
    acc_np[7] = 3040.0 * np.where(np.arange(nb) % 2 == 0, 0.75, 0.25)
    psum_np = (rng.uniform(0, 1, (A, nb)) * rng.integers(1, 5000, (A, 1))).astype(np.float32)
    psum_np[1] = psum_np[2] = 0.0
    acc_np[4] = (seen_np[4] + 8) * 0.5                            # ... and exactly on it: 0.5 >= 0.5f is a 1
    acc = _inout(acc_np.view(np.int64), "acc", offset)            # the guard patterns are integers and floats; f64 goes in as its bits
    seen = _inout(seen_np, "seen", offset)
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
            racc[slot, k] = racc[slot, k] + float(psum_np[r, k])   # one f64 add
            rmp[r, k] = np.float32(racc[slot, k] / float(max(int(rseen[slot]), 1)))
            rbits[r, k] = 1 if rmp[r, k] >= np.float32(0.5) else 0
    assert skipped.any() and (rbits == 1).any() and (rbits == 0).any()
    psum.check(), desc.check()
    mp.check(expect_unwritten=torch.from_numpy(skipped)), bt.check(expect_unwritten=torch.from_numpy(skipped))
    assert not acc.guard_report() and not seen.guard_report()
    assert np.array_equal(acc.t.cpu().numpy(), racc.view(np.int64))                  # named slots updated, every other slot untouched
    assert np.array_equal(seen.t.cpu().numpy(), rseen)
    assert np.array_equal(bits(mp.t)[~skipped], rmp.view(np.int32)[~skipped])
    assert np.array_equal(bt.t.cpu().numpy()[~skipped], rbits[~skipped])
    assert (bits(mp.t)[1] == 0).all()                             # 0 / max(0, 1)
    assert (mp.t[2] == 0.5).all() and (bt.t[2] == 1).all()
    for null in range(6):                                         # each null pointer refused, nothing written
        a = [acc.t.data_ptr(), seen.t.data_ptr(), psum.t.data_ptr(), desc.t.data_ptr(), mp.t.data_ptr(), bt.t.data_ptr()]
        a[null] = None
        assert lib.wv_bank_detect_update(a[0], a[1], capacity, nb, a[2], a[3], A, a[4], a[5], st) == -1
        assert b"wv_bank_detect_update: null" in lib.wv_last_error()
    for cap_, nb_, A_ in ((0, nb, A), (capacity, 0, A), (capacity, nb, -1), (capacity, nb, 65536)):
        assert lib.wv_bank_detect_update(acc.t.data_ptr(), seen.t.data_ptr(), cap_, nb_, psum.t.data_ptr(), desc.t.data_ptr(), A_, mp.t.data_ptr(),
                                         bt.t.data_ptr(), st) == -1
        assert b"wv_bank_detect_update: capacity" in lib.wv_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(acc.t.cpu().numpy(), racc.view(np.int64)) and np.array_equal(seen.t.cpu().numpy(), rseen)


# =============================================================================================== the nets
@functools.lru_cache(maxsize=None)
def _net(cid):
    """-> (case, cfg, HipNet, oracle net) of a case id, built once: the float64 numpy oracle for the exact cases, the torch net that
    oracle/wv_oracle_h16 runs in the f16 mode's arithmetic for the f16 ones."""
    from waveverify_amd.nets import HipNet
    case = next(c for c in NETS if c[0] == cid)
    if case[1] == "f32":
        cfg, sd, onet = W.oracle_net(case)
        return case, cfg, HipNet(cfg, sd), onet
    from oracle import wv_oracle_torch as OT
    from waveverify_amd.init import random_state_dict
    cfg, seed = W.net_config(case)
    sd = random_state_dict(cfg, seed)
    return case, cfg, HipNet(cfg, sd), OT.Net(cfg, sd)


def _bank(net, kind, precision, pad=1.5, capacity=BK.CAPACITY):
    from waveverify_amd.session import DetectBank, EmbedBank, LocateBank
    return {"generator": EmbedBank, "detector": DetectBank, "locator": LocateBank}[kind](net, capacity, precision, pad)


def _play(bank, kind, steps, data):
    """BK.run with a message per opened stream for an embed bank -> {stream: [(kind, samples so far, result)]}."""
    return BK.run(bank, steps, {n: cu(x) for n, (x, _) in data.items()}, (lambda n: (data[n][1],)) if kind == "generator" else (lambda n: ()))[0]


_REFERENCES = {}


def _references(cid, sched, steps=None):
    """-> (steps, data, {stream: whole-input reference [C, T] float64}) of a schedule, computed once for all pad_limits.  sched names one of
    bank_cases.schedules(cfg), or the `steps` themselves, which are then remembered under that name."""
    if (cid, sched) not in _REFERENCES:
        _REFERENCES[cid, sched] = _compute_references(cid, sched, steps)
    assert steps is None or steps == _REFERENCES[cid, sched][0], (cid, sched)
    return _REFERENCES[cid, sched]


def _compute_references(cid, sched, steps):
    case, cfg, net, onet = _net(cid)
    steps = dict(BK.schedules(cfg))[sched] if steps is None else steps
    data = BK.stream_data(case, steps)
    refs = {}
    for n, (x, m) in data.items():
        if not x.size:
            continue
        if case[1] == "f32":
            refs[n] = W.oracle_forward(cfg, onet, x[None, None], m[None])[0]
        else:
            from oracle import wv_oracle_h16 as O16
            refs[n] = (O16.embed(onet, x[None, None], m[None]) if cfg.kind == "generator" else O16.detect_logits(onet, x[None, None])).double().numpy()[0]
    return steps, data, refs


@functools.lru_cache(maxsize=None)
def _mean16(cid, sched, name, upto):
    """The f16 oracle's mean probabilities of a stream's first `upto` samples [nb] (its head has an arithmetic of its own)."""
    from oracle import wv_oracle_h16 as O16
    _, _, _, onet = _net(cid)
    x = _references(cid, sched)[1][name][0]
    return O16.detect_mean_prob(onet, x[None, None, :upto]).double().numpy()[0]


def _check_stream(cid, sched, name, events, x, ref, hop, kind, f16, what, tag=""):
    """One stream's results over a schedule: column counts, then the concatenation (or every DetectState) against its whole-input reference."""
    seen = [(pos // hop * hop if k == "push" else pos) for k, pos, _ in events]
    assert seen[-1] == x.size, what
    if kind == "detector":
        nb = ref.shape[0] if ref is not None else None
        prev, checks = None, []
        for i, ((k, pos, st), upto) in enumerate(zip(events, seen)):
            assert st.samples_seen == upto and st.mean_prob.dim() == 1 and torch.equal(st.bits, (st.mean_prob >= 0.5).to(torch.int32)), what
            if upto == 0:
                assert (st.mean_prob == 0).all(), what
            elif prev is not None and prev[1] == upto:
                assert torch.equal(st.mean_prob, prev[0].mean_prob), what             # nothing completed: the state stands
            else:
                checks.append((i, upto, st))
            prev = (st, upto)
        if f16 and checks:                                        # an oracle run per check: the first, the one after the largest step, the last
            big = max(checks, key=lambda c: c[1] - ([0] + seen)[c[0]])
            checks = [c for j, c in enumerate(checks) if j in (0, len(checks) - 1) or c is big]
        for _, upto, st in checks:
            if f16:
                measure(tag + "f16 DetectBank mean probability / det_mean_bar(T)", rel_err(st.mean_prob, _mean16(cid, sched, name, upto), 1.0) / det_mean_bar(upto), 1.0)
            else:
                measure(tag + "exact DetectBank mean probability", rel_err(st.mean_prob, sigmoid64(ref[:, :upto]).mean(axis=1), 1.0), MEAN_BAR)
        return None
    done = 0
    for (k, pos, r), upto in zip(events, seen):
        assert r.dim() == 1 and r.shape[0] == upto - done, (what, k, pos, tuple(r.shape))
        done = upto
    return torch.cat([r for _, _, r in events]) if x.size else None


def _check_bank(cid, sched, pad, precision, steps=None, capacity=BK.CAPACITY, tag=""):
    """A schedule by name, or the steps themselves under the name `sched` (tag: what their MEASURE lines start with)."""
    case, cfg, net, _ = _net(cid)
    kind, hop, f16 = cfg.kind, cfg.hop_length, precision == "f16"
    steps, data, refs = _references(cid, sched, steps)
    bank = _bank(net, kind, precision, pad, capacity)
    out = _play(bank, kind, steps, data)
    assert bank.open_slots() == []
    mag = max(float(np.abs(r).max()) for r in refs.values())      # the reference's largest magnitude over the schedule's streams
    for n, (x, _) in data.items():
        what = f"{cid} {sched} pad_limit {pad} stream {n}"
        got = _check_stream(cid, sched, n, out[n], x, refs.get(n), hop, kind, f16, what, tag)
        if got is None:
            continue
        ref = refs[n][0]
        if kind == "generator":
            measure(tag + ("f16 EmbedBank (absolute)" if f16 else "exact EmbedBank"), rel_err(got, ref, 1.0 if f16 else mag), WM_BAR if f16 else GEN_BAR)
        else:
            measure(tag + ("f16 LocateBank logits" if f16 else "exact LocateBank logits"), rel_err(got, ref, max(1.0, mag) if f16 else mag),
                    LOGIT_BAR16 if f16 else LOGIT_BAR32)
    return bank


# =============================================================================================== 3. the banks against the oracle
@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_banks_vs_float64(case):
    launches = {}
    for sched in ("mixed", "equal"):
        for pad in BK.PAD_LIMITS:
            launches[sched, pad] = _check_bank(case[0], sched, pad, "f32").stats
    for sched in ("mixed", "equal"):                              # the groupings differed, and every one met the bars
        a, b, c = (launches[sched, pad] for pad in BK.PAD_LIMITS)
        assert a["launches"] >= b["launches"] >= c["launches"] and a["padded_samples"] == 0 <= b["padded_samples"] <= c["padded_samples"]
    assert launches["mixed", 1.0]["launches"] > launches["mixed", float("inf")]["launches"] and launches["mixed", float("inf")]["padded_samples"] > 0
    assert launches["equal", 1.5]["padded_samples"] == 0


F16_PARAMS = [(c, pad) for c in F16 for pad in BK.PAD_LIMITS]


@pytest.mark.parametrize("case,pad", F16_PARAMS, ids=[f"{c[0]}-pad{p}" for c, p in F16_PARAMS])
def test_banks_f16_vs_their_oracle(case, pad):
    for sched in ("mixed", "equal"):
        _check_bank(case[0], sched, pad, "f16")


@pytest.mark.parametrize("case", F16_REFUSED, ids=_ids(F16_REFUSED))
def test_banks_f16_refuse_nets_without_a_plan(case):
    """The 16-channel nets have no f16 plan: a bank says so as the sessions do, and runs them on the exact path."""
    case, cfg, net, _ = _net(case[0])
    kind, hop = cfg.kind, cfg.hop_length
    x, msg = W.clip_data(case, 3 * hop, 0)
    args = (msg[0],) if kind == "generator" else ()
    bank = _bank(net, kind, "f16")
    slot = bank.open(*args)
    with pytest.raises(RuntimeError, match="f16"):
        bank.push({slot: cu(x[0, 0, :2 * hop])})
    exact = _bank(net, kind, "f32")
    slot = exact.open(*args)
    r = exact.push({slot: cu(x[0, 0, :2 * hop])})[slot]
    assert torch.isfinite(r.mean_prob if kind == "detector" else r).all()


# =============================================================================================== 4. / 5. bit equalities
def _same(a, b, kind, what):
    if kind == "detector":
        assert a.samples_seen == b.samples_seen and torch.equal(a.mean_prob, b.mean_prob) and torch.equal(a.bits, b.bits), what
    else:
        assert a.shape == b.shape and torch.equal(a, b), what


def _lockstep(net, kind, S, msg, precision):
    from waveverify_amd.session import DetectSession, EmbedSession, LocateSession
    if kind == "generator":
        return EmbedSession(net, cu(msg), precision)
    return (LocateSession if kind == "locator" else DetectSession)(net, S, precision)


def _of_stream(r, s, kind):
    """Stream s of a lockstep session's result, in the form a bank gives it."""
    from waveverify_amd.session import DetectState
    return DetectState(r.mean_prob[s], r.bits[s], r.samples_seen) if kind == "detector" else r[s, 0]


BIT_CASES = EXACT + F16


@pytest.mark.parametrize("case", BIT_CASES, ids=_ids(BIT_CASES))
def test_equal_pushes_are_the_lockstep_session_bit_for_bit(case):
    """Four streams that push the same sizes at the same ticks are one window batch per tick, the lockstep session's; and a stream of them
    alone in a bank (one row per launch) gets the same bits as beside the other three."""
    case, cfg, net, _ = _net(case[0])
    kind, precision = cfg.kind, case[1]
    steps, sizes = BK.equal_schedule(cfg)
    data = BK.stream_data(case, steps)
    names = list(data)
    out = _play(_bank(net, kind, precision), kind, steps, data)
    sess = _lockstep(net, kind, len(names), np.stack([data[n][1] for n in names]), precision)
    xt = cu(np.stack([data[n][0] for n in names]))
    seen, results = 0, []
    for n in sizes:
        results.append(sess.push(xt[:, seen: seen + n]))
        seen += n
    results.append(sess.flush())
    assert seen % cfg.hop_length and len(results) == len(out[names[0]])               # the close runs a partial frame
    for s, name in enumerate(names):
        for i, ((k, pos, got), r) in enumerate(zip(out[name], results)):
            _same(got, _of_stream(r, s, kind), kind, f"{case[0]} stream {name} step {i} ({k} at {pos}) against the lockstep session")
    alone = _play(_bank(net, kind, precision), kind, [(k, ({names[1]: a[names[1]]} if k == "push" else a)) for k, a in steps
                                                       if k == "push" or a == names[1]], data)
    for i, ((k, pos, got), (_, _, want)) in enumerate(zip(alone[names[1]], out[names[1]])):
        _same(got, want, kind, f"{case[0]} stream {names[1]} step {i} alone against beside three others")


REUSE = [c for c in EXACT if c[3][1] in (0, 14)] + F16


@pytest.mark.parametrize("case", REUSE, ids=_ids(REUSE))
def test_a_reused_slot_starts_from_nothing(case):
    """Slot 0's first stream pushes audio (a detect bank accumulates) and closes; the stream that takes the slot over gets, bit for bit, what
    it gets in a fresh bank.  A history or an accumulator left over would show."""
    case, cfg, net, _ = _net(case[0])
    kind, precision, hop = cfg.kind, case[1], cfg.hop_length
    from waveverify_amd.window import halo
    H = halo(cfg)
    first = [("open", "P"), ("push", {"P": H + 2 * hop + 3}), ("push", {"P": hop}), ("close", "P")]
    second = [("open", "Q"), ("push", {"Q": hop - 1}), ("push", {"Q": 1}), ("push", {"Q": hop + 5}), ("push", {"Q": H + hop + 3}), ("close", "Q")]
    data = BK.stream_data(case, first + second)
    assert float(np.abs(data["P"][0]).max()) > 0
    used, fresh = _bank(net, kind, precision, capacity=2), _bank(net, kind, precision, capacity=2)
    _play(used, kind, first, data)
    got, want = _play(used, kind, second, data), _play(fresh, kind, second, data)
    assert used.stats["ticks"] > fresh.stats["ticks"]
    for i, ((k, pos, a), (_, _, b)) in enumerate(zip(got["Q"], want["Q"])):
        _same(a, b, kind, f"{case[0]} step {i} ({k} at {pos}) in a reused slot against a fresh bank")


# =============================================================================================== 6. misuse
MISUSE = [c for c in EXACT if c[3][1] == 6]


@pytest.mark.parametrize("case", MISUSE, ids=_ids(MISUSE))
def test_misuse_raises_and_changes_no_stream(case):
    case, cfg, net, _ = _net(case[0])
    kind, hop = cfg.kind, cfg.hop_length
    steps = [("open", "A"), ("open", "B"), ("push", {"A": hop + 3, "B": 2 * hop - 1}), ("push", {"A": hop, "B": 1}), ("push", {"A": 3 * hop + 1}),
             ("close", "B"), ("close", "A")]
    data = BK.stream_data(case, steps)
    args = (data["A"][1],) if kind == "generator" else ()
    clean = _play(_bank(net, kind, "f32", capacity=3), kind, steps, data)
    bank = _bank(net, kind, "f32", capacity=3)
    x = cu(data["A"][0])

    def misuse():
        before = bank.open_slots()
        spares = [bank.open(*args) for _ in range(3 - len(before))]                    # every slot taken
        with pytest.raises(RuntimeError, match="slots"):
            bank.open(*args)
        for spare in spares:
            assert bank.close(spare) is not None
        for bad in ({spares[0]: x[:hop]}, {0: x[:hop], 7: x[:hop]}, {0: x[:2 * hop].view(2, hop)}, {0: x[:hop], spares[0]: x[None, :hop]}):
            with pytest.raises(ValueError):
                bank.push(bad)
        for bad in (spares[0], -1, 3, "0"):
            with pytest.raises(ValueError):
                bank.close(bad)
        assert bank.open_slots() == before and 0 in before

    slot, pos, out = {}, {"A": 0, "B": 0}, {"A": [], "B": []}
    for k, a in steps:                                            # BK.run, with the misuse before every push and close
        if k == "open":
            slot[a] = bank.open(*((data[a][1],) if kind == "generator" else ()))
            continue
        if len(slot) == 2:
            misuse()
        if k == "close":
            out[a].append(bank.close(slot[a]))
        else:
            res = bank.push({slot[n]: cu(data[n][0][pos[n]: pos[n] + m]) for n, m in a.items()})
            for n, m in a.items():
                pos[n] += m
                out[n].append(res[slot[n]])
    for n in "AB":
        assert len(out[n]) == len(clean[n])
        for i, (a, (_, _, b)) in enumerate(zip(out[n], clean[n])):
            _same(a, b, kind, f"{case[0]} stream {n} step {i} after misuse against a bank nobody misused")


def test_the_public_interface_opens_banks_at_the_nets_precision():
    """WaveVerify.open_*_bank: a watermark id per opened stream, the nets' current precision, equal to the lockstep sessions of the same object."""
    from waveverify_amd import WatermarkID, WaveVerify, session
    wv = WaveVerify.random_init(seed=0)
    ids = [WatermarkID.custom(0x1234), WatermarkID.custom(0xBEEF)]
    x = cu(W.clip_data(("api", "f32", "generator", None), 960, 0)[0][0, 0])
    for precision in ("f32", "f16"):
        wv.set_precision(precision)
        eb, db, lb = wv.open_embed_bank(capacity=2), wv.open_detect_bank(), wv.open_locate_bank(capacity=3, pad_limit=1.0)
        assert (type(eb), type(db), type(lb)) == (session.EmbedBank, session.DetectBank, session.LocateBank)
        assert (eb.precision, db.precision, lb.precision, db.capacity, lb.pad_limit) == (precision, precision, precision, 64, 1.0)
        slots = [eb.open(i) for i in ids]
        y = eb.push({slots[0]: x[:700], slots[1]: x[:700]})
        ref = wv.open_embed_session(ids).push(torch.stack([x[:700], x[:700]]))
        assert torch.equal(torch.stack([y[slots[0]], y[slots[1]]]), ref[:, 0]) and not torch.equal(y[slots[0]], y[slots[1]])
        d, l = db.open(), lb.open()
        st = db.push({d: y[slots[0]]})[d]
        rs = wv.open_detect_session(1).push(y[slots[0]][None])
        assert st.samples_seen == rs.samples_seen == 640 and torch.equal(st.mean_prob, rs.mean_prob[0])
        assert torch.equal(lb.push({l: y[slots[0]]})[l], wv.open_locate_session(1).push(y[slots[0]][None])[0, 0])
    wv.set_precision("f32")


def test_print_the_worst_cases():
    """The last test of the file: the worst figure per kind over what ran before it (pytest -s)."""
    for what, err in sorted(WORST.items()):
        print(f"WORST {what}: {err:.2e}")
