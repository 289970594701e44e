"""Span embedding on the CPU (tests/span_cases.py): the case list hits the edges it names; window.plan_spans keeps its geometry and grouping
rules on it; the numpy twins of wv_span_gather / wv_span_scatter_add keep their skip rules and the ramp's min; the planner's windows through
the float64 oracle generator and the twins are x + w * delta of the WHOLE clip to 1e-12; every span's residual is large enough for the GPU
bar to mean something; the bank's pass-through state machine on the float64 oracle is span embedding of each stream; every refusal; the two
exports.  No GPU."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import bank_cases as BK
import span_cases as SC
import window_cases as W
from waveverify_amd import window
from waveverify_amd.session import StreamBank, _Ticker, plan_tick
from waveverify_amd.window import halo, plan_spans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STITCH_BAR = 1e-12                                                # tests/test_window_cases_cpu.py holds stitching to it; it measured 6e-16
GPU_BAR = 5e-5                                                    # tests/test_gpu_span.py, exact path: of the reference's largest magnitude
F16_BAR = 1e-4                                                    # test_gpu_h16.WM_BAR, absolute
IDS = list(SC.EXACT_IDS)


def _oracle(cid):
    case = SC.net_case(cid)
    cfg, sd, onet = W.oracle_net(case)
    return case, cfg, onet


def _deltas(cfg, onet, x, msgs, rows):
    """{message row: the whole clip's residual under that message, float64 [T]}."""
    return {m: W.oracle_forward(cfg, onet, x[None, None], msgs[m:m + 1], add_input=False)[0, 0] for m in rows}


_SHARED = {}


def shared(cid):
    """-> (cfg, onet, L, lengths, spans, kinds, xs, msgs, deltas per clip), computed once and left unchanged."""
    if cid not in _SHARED:
        _, cfg, onet = _oracle(cid)
        L, lengths, spans, kinds = SC.cases(cid)
        xs, msgs = SC.clip_data(cid, lengths), SC.messages(cid)
        deltas = [_deltas(cfg, onet, x, msgs, {m for _, _, m in sp}) for x, sp in zip(xs, spans)]
        _SHARED[cid] = (cfg, onet, L, lengths, spans, kinds, xs, msgs, deltas)
    return _SHARED[cid]


# ---- the list hits its edges -------------------------------------------------------------------------------------------------------------
def test_nets_are_the_three_the_issue_names():
    cfgs = [W.net_config(SC.net_case(c))[0] for c in SC.EXACT_IDS]
    assert cfgs[0].dilation_base == 2 and len(cfgs[1].strides) == 4 and cfgs[2].n_residual_dec == 0
    assert all(SC.net_case(c)[1] == "f32" for c in SC.EXACT_IDS)
    f16 = SC.net_case(SC.F16_ID)
    assert f16[1] == "f16" and f16[2] == "generator" and f16[3][1].startswith("sweep")


@pytest.mark.parametrize("cid", IDS + [SC.F16_ID])
def test_clip_list_hits_the_edges_by_name(cid):
    cfg, _ = W.net_config(SC.net_case(cid))
    hop, H = cfg.hop_length, halo(cfg)
    L, lengths, spans, kinds = SC.cases(cid)
    assert len(lengths) == 5 and len(set(lengths)) == 5 and {k for ks in kinds for k in ks} == set(SC.SPAN_KINDS)
    by = {}
    for b, (sp, ks) in enumerate(zip(spans, kinds)):
        for span, k in zip(sp or [None], ks):
            by.setdefault(k, []).append((b, span))
    (b, (s, e, _)), = by["at-0"]
    assert s == 0
    (b, (s, e, _)), = by["ragged-end"]
    assert e == lengths[b] and lengths[b] % hop
    (b, (s, e, _)), = by["one-sample"]
    assert e - s == 1
    (b, (s, e, _)), = by["sub-hop"]
    assert e - s < hop and s % hop and e % hop
    (b, (s, e, _)), = by["off-grid"]
    assert s % hop and e % hop and e - s > hop
    (b0, (s0, e0, m0)), (b1, (s1, e1, m1)) = by["abutting"]
    assert b0 == b1 and e0 == s1 and m0 != m1
    (b, span), = by["three-pieces"]
    pieces = [w for g in plan_spans([lengths[b]], [[span]], L, cfg) for w in g]
    assert len(pieces) == 3 and span[1] - span[0] > L
    (b, (s, e, _)), = by["inside-halo"]
    assert 0 < s and e < H
    (b, span), = by["span-less"]
    assert span is None and spans[b] == ()
    assert {m for sp in spans for _, _, m in sp} == set(range(SC.N_MSG))


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS + [SC.F16_ID])
def test_plan_spans_properties(cid):
    cfg, _ = W.net_config(SC.net_case(cid))
    hop, H = cfg.hop_length, halo(cfg)
    L, lengths, spans, _ = SC.cases(cid)
    for window_ in (L, H + hop, 4 * L, 1):
        Lw = max(-(-window_ // hop) * hop, H + hop)
        for pad in SC.PAD_LIMITS:
            for mw in (1, 2, 64):
                launches = plan_spans(lengths, spans, window_, cfg, pad, mw)
                wins = [w for g in launches for w in g]
                for b, (T, sp) in enumerate(zip(lengths, spans)):
                    mine = [w for w in wins if w.clip == b]
                    assert bool(mine) == bool(sp)                  # a clip without spans has no window
                    for s, e, m in sp:
                        keeps = sorted((w.keep_lo, w.keep_hi) for w in mine if (w.span_lo, w.span_hi) == (s, e))
                        assert keeps[0][0] == s and keeps[-1][1] == e and all(a[1] == b_[0] for a, b_ in zip(keeps, keeps[1:]))
                        assert all(w.msg == m for w in mine if (w.span_lo, w.span_hi) == (s, e))
                for w in wins:
                    T = lengths[w.clip]
                    assert w.start % hop == 0 and (w.start == 0 or w.start <= w.keep_lo - H)
                    end = w.start + w.length
                    assert (end % hop == 0 or end == T) and end <= T and w.length <= Lw
                    assert w.start <= w.keep_lo < w.keep_hi <= end and w.span_lo <= w.keep_lo and w.keep_hi <= w.span_hi
                for g in launches:
                    assert 1 <= len(g) <= mw and [w.length for w in g] == sorted(w.length for w in g)
                    assert g[-1].length <= pad * g[0].length       # no row is padded beyond pad_limit
                    if any((w.start + w.length) % hop for w in g):
                        assert len({w.length for w in g}) == 1     # a ragged end shares a launch only with its own length
        assert any((w.start + w.length) % hop for w in wins), "the list has a ragged-end window"
    assert plan_spans([100, 50], [[], []], L, cfg) == []


def test_plan_spans_refusals():
    cfg, _ = W.net_config(SC.net_case(IDS[0]))
    for lengths, spans in (([100], [[(10, 30, 0), (29, 40, 1)]]),     # overlapping
                           ([100], [[(10, 10, 0)]]), ([100], [[(12, 10, 0)]]),      # start >= end
                           ([100], [[(-1, 10, 0)]]), ([100], [[(90, 101, 0)]]),     # outside the clip
                           ([100, 100], [[(0, 10, 0)]]), ([0], [[]])):
        with pytest.raises(ValueError):
            plan_spans(lengths, spans, 4000, cfg)
    with pytest.raises(ValueError):
        plan_spans([100], [[(0, 10, 0)]], 4000, cfg, pad_limit=0.99)
    with pytest.raises(ValueError):
        plan_spans([100], [[(0, 10, 0)]], 4000, cfg, max_windows=0)
    assert len(plan_spans([100], [[(10, 30, 0), (30, 40, 1)]], 4000, cfg)) >= 1      # abutting is allowed
    for bad in (-1, 2.5):
        with pytest.raises(ValueError):
            window.span_ramp(bad)
    # span_generator refuses before anything touches a device: a net that has none
    import torch
    net = SimpleNamespace(cfg=cfg, device="no-such-device")
    x, msgs = [torch.zeros(100)], torch.zeros(2, 16)
    for kw in (dict(spans=[[(0, 10, 0)]], fade_samples=-1), dict(spans=[[(0, 10, 0), (5, 20, 1)]]), dict(spans=[[(0, 10, 2)]]),
               dict(spans=[[(0, 10, 0)]], pad_limit=0.5), dict(spans=[[(0, 10, 0)]], gain=float("nan")), dict(spans=[[(0, 101, 0)]])):
        with pytest.raises(ValueError):
            window.span_generator(net, x, msgs, **kw)


def test_ramp_is_rounded_once_from_float64():
    for F in (1, 5, 7, 160):
        r = window.span_ramp(F)
        want = [np.float32(0.5 - 0.5 * np.cos(np.pi * (j + 0.5) / F)) for j in range(F)]
        assert r.dtype == np.float32 and np.array_equal(r, np.array(want, np.float32)) and 0 < r[0] <= r[-1] < 1
        assert (np.diff(r) > 0).all()
    assert window.span_ramp(0) is None


# ---- the twins ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lmax", SC.KERNEL_L)
def test_gather_twin(Lmax):
    n_src, rows, bad = SC.gather_case(Lmax)
    assert {wl for _, wl in rows} >= {0, 1, Lmax - 1, Lmax} and {o % 4 for o, _ in rows if o >= 0} == {0, 1, 2, 3} and len(bad) == 5
    src = np.arange(1, n_src + 1, dtype=np.float32)
    dst = np.full((len(rows), 1, Lmax), -7.0, np.float32)
    window.numpy_span_gather(src, rows, len(rows), Lmax, dst)
    for r, (off, wl) in enumerate(rows):
        assert window.span_gather_row_ok((off, wl), n_src, Lmax) == (r not in bad)
        if r in bad:
            assert (dst[r] == -7.0).all()                          # skipped whole
        else:
            assert np.array_equal(dst[r, 0, :wl], src[off:off + wl]) and not dst[r, 0, wl:].any()


@pytest.mark.parametrize("F", SC.KERNEL_F)
@pytest.mark.parametrize("Lmax", SC.KERNEL_L)
def test_scatter_twin(Lmax, F):
    n_out, rows, bad = SC.scatter_case(Lmax, F)
    Fn = Lmax + 3 if F == "long" else F
    ramp = window.span_ramp(Fn)
    assert any(ss < 0 for _, _, _, ss, _ in rows) and any(se > Lmax for _, _, _, _, se in rows) and len(bad) >= 7
    rng = np.random.default_rng(W.seed_of("scatter twin", Lmax, F))
    y = rng.standard_normal((len(rows), 1, Lmax)).astype(np.float32)
    x = rng.standard_normal(n_out).astype(np.float32)
    for xin in ("null", "separate", "out"):
        out = x.copy() if xin == "out" else np.full(n_out, -7.0, np.float32)
        window.numpy_span_scatter_add(y, None if xin == "null" else (out if xin == "out" else x), rows, ramp, SC.GAIN, out)
        want = x.copy() if xin == "out" else np.full(n_out, -7.0, np.float32)
        for r, (o, lo, hi, ss, se) in enumerate(rows):
            assert window.span_row_ok((o, lo, hi, ss, se), n_out, Lmax) == (r not in bad)
            if r in bad:
                continue
            for j in range(lo, hi):                               # sample by sample, three roundings
                m = min(j - ss, se - 1 - j)
                w = np.float32(SC.GAIN) * ramp[m] if m < Fn else np.float32(SC.GAIN)
                v = np.float32(w * y[r, 0, j])
                want[o + j] = v if xin == "null" else np.float32(x[o + j] + v)
        assert np.array_equal(out.view(np.int32), want.view(np.int32)), xin
    if Lmax > 8 and Fn > 0:                                        # the two ramps meet in a span shorter than 2 F
        o, lo, hi, ss, se = next(r for i, r in enumerate(rows) if i not in bad and (r[3], r[4]) == (r[1], r[2]))
        w = SC.weights(lo, hi, ramp, 1.0, np.float32)
        assert np.array_equal(w, w[::-1]) and (F != "long" or (w < 1).all())


# ---- the float64 stitch --------------------------------------------------------------------------------------------------------------------
def _oracle_route(cfg, onet, xs, msgs, spans, L, pad, fade, gain, add_input=True):
    """plan_spans' launches through the float64 oracle and the two twins, on the packed clips."""
    lengths = [len(x) for x in xs]
    bases = [int(v) for v in np.cumsum([0] + lengths[:-1])]
    packed = np.concatenate(xs).astype(np.float64)
    out = packed.copy() if add_input else np.zeros_like(packed)
    ramp = window.span_ramp(fade)
    for wins in plan_spans(lengths, spans, L, cfg, pad, 64):
        A, Lmax = len(wins), wins[-1].length
        xw = window.numpy_span_gather(packed, window.span_gather_desc(wins, bases), A, Lmax)
        y = W.oracle_forward(cfg, onet, xw.astype(np.float32), msgs[[w.msg for w in wins]], add_input=False)
        window.numpy_span_scatter_add(y, out if add_input else None, window.span_scatter_desc(wins, bases), ramp, gain, out)
    return [out[b0:b0 + T] for b0, T in zip(bases, lengths)]


@pytest.mark.parametrize("cid", IDS)
def test_stitched_oracle_spans_equal_the_whole_clip(cid):
    cfg, onet, L, lengths, spans, kinds, xs, msgs, deltas = shared(cid)
    worst = 0.0
    for pad in SC.PAD_LIMITS:
        for fade, gain in ((0, 1.0), (7, SC.GAIN)):
            got = _oracle_route(cfg, onet, xs, msgs, spans, L, pad, fade, gain)
            ramp = window.span_ramp(fade)
            for b, (x, sp) in enumerate(zip(xs, spans)):
                ref = SC.reference(x, deltas[b], sp, ramp, gain)
                err = float(np.abs(got[b] - ref).max()) / float(np.abs(ref).max())
                worst = max(worst, err)
                assert err <= STITCH_BAR, (pad, fade, b, err)
                out = SC.outside(len(x), sp)
                assert np.array_equal(got[b][out], x.astype(np.float64)[out])          # never rewritten
    print(f"SPAN STITCH {cid}: {worst:.1e} of the output's magnitude")


@pytest.mark.parametrize("cid", IDS)
def test_every_span_carries_a_residual_the_gpu_bar_can_see(cid):
    cfg, onet, L, lengths, spans, kinds, xs, msgs, deltas = shared(cid)
    least = np.inf
    for b, (x, sp) in enumerate(zip(xs, spans)):
        for s, e, m in sp:
            mag = float(np.abs(SC.reference(x, deltas[b], sp)).max())
            d = float(np.abs(deltas[b][m][s:e]).max())
            least = min(least, d / (GPU_BAR * mag))
            assert d > 100 * GPU_BAR * mag, (b, s, e, d, mag)
        for (s0, e0, m0), (s1, e1, m1) in zip(sp, sp[1:]):
            if e0 == s1:                                           # abutting: the two ids' residuals differ where they meet
                d = float(np.abs(deltas[b][m0][s0:e1] - deltas[b][m1][s0:e1]).max())
                assert d > 100 * GPU_BAR * mag, (b, e0, d)
    print(f"SPAN INPUT {cid}: the weakest span's max|delta| is {least:.0f} x the GPU bar")


def test_the_f16_net_spans_carry_a_residual_its_bar_can_see():
    import torch
    from oracle import wv_oracle_h16 as O16
    from oracle import wv_oracle_torch as OT
    from waveverify_amd.init import random_state_dict
    cfg, seed = W.net_config(SC.net_case(SC.F16_ID))
    onet = OT.Net(cfg, random_state_dict(cfg, seed))
    L, lengths, spans, _ = SC.cases(SC.F16_ID)
    xs, msgs = SC.clip_data(SC.F16_ID, lengths), SC.messages(SC.F16_ID)
    for x, sp in zip(xs, spans):
        for s, e, m in sp:
            xt = torch.from_numpy(x[None, None]).double()
            d = O16.decoder_forward(onet, O16.encoder_latent(onet, xt, torch.from_numpy(msgs[m:m + 1])))[0, 0, :len(x)].numpy()
            assert float(np.abs(d[s:e]).max()) > 100 * F16_BAR, (s, e, float(np.abs(d[s:e]).max()))


# ---- pass-through in a bank ------------------------------------------------------------------------------------------------------------------
def test_plan_tick_without_passthrough_is_unchanged():
    cfg, _ = W.net_config(SC.net_case(IDS[0]))
    hop, H = cfg.hop_length, halo(cfg)
    tk = {}
    for kind, arg in BK.mixed_schedule(hop, H):
        if kind == "open":
            tk[arg] = _Ticker(hop, H)
        elif kind == "push":
            ticks = {ord(n): tk[n].push(c) for n, c in arg.items()}
            sizes = {ord(n): c for n, c in arg.items()}
            for pad in BK.PAD_LIMITS:
                a, b = plan_tick(ticks, sizes, pad), plan_tick(ticks, sizes, pad, passthrough=frozenset())
                assert np.array_equal(a.desc, b.desc) and a.launches == b.launches and not any(ln.passthrough for ln in a.launches)
                assert (a.slots, a.n_x, a.windows, a.out, a.n_out, a.padded) == (b.slots, b.n_x, b.windows, b.out, b.n_out, b.padded)
                # all in pass-through: the same rows, one launch, nothing padded
                c = plan_tick(ticks, sizes, pad, passthrough=frozenset(ticks))
                assert sorted(map(tuple, c.desc[:, [0, 1, 2, 3, 5, 6, 7]])) == sorted(map(tuple, a.desc[:, [0, 1, 2, 3, 5, 6, 7]]))
                assert sum(1 for ln in c.launches if ln.A) <= 1 and all(ln.passthrough for ln in c.launches if ln.A) and c.padded == 0
                assert {s: k for s, (_, k) in c.out.items()} == {s: k for s, (_, k) in a.out.items()}


@pytest.mark.parametrize("cid", IDS)
def test_oracle_bank_with_switches_is_span_embedding(cid):
    """Every stream switches id -> None -> id while the schedule runs (some open in pass-through, some switch on ticks that complete no
    frame): its concatenated output is the span embedding of everything it pushed, span edges at the returned indices, to 1e-12; over the None
    stretches it is the input bit for bit; a tick of pass-through slots only launches nothing."""
    case, cfg, onet = _oracle(cid)
    hop, H = cfg.hop_length, halo(cfg)
    msgs = SC.messages(cid)
    worst, quiet = 0.0, 0
    for name, steps in BK.schedules(cfg):
        data = BK.stream_data(case, steps)
        xs = {n: x for n, (x, _) in data.items()}
        plan = SC.switch_plan(steps)
        for pad in BK.PAD_LIMITS:
            cur = {}
            bank = StreamBank(BK.CAPACITY, hop, H, lambda win, slots: W.oracle_forward(cfg, onet, win, msgs[[cur[s] for s in slots]]),
                              pad_limit=pad)

            def set_state(slot, st):
                if st is not None:
                    cur[slot] = st
                return bank.set_passthrough(slot, st is None)

            def open_stream(st):
                slot = bank.open()
                assert set_state(slot, st) == 0
                return slot
            out, marks, launches, only = SC.run_switching(bank, steps, xs, plan, open_stream, set_state)
            assert all(n == 0 for n, o in zip(launches, only) if o)
            quiet += sum(only)
            for n, x in xs.items():
                parts = [np.asarray(r).reshape(-1) for r in out[n] if r is not None]
                got = np.concatenate(parts) if parts else np.zeros(0)
                assert got.shape == x.shape
                if not x.size:
                    continue
                assert all(t % hop == 0 for t, _ in marks[n])
                sp = SC.spans_of(marks[n], x.size)
                ref = SC.reference(x, _deltas(cfg, onet, x, msgs, {m for _, _, m in sp}), sp)
                err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
                worst = max(worst, err)
                assert err <= STITCH_BAR, (name, pad, n, err)
                off = SC.outside(x.size, sp)
                assert np.array_equal(got[off].astype(np.float32).view(np.int32), x[off].view(np.int32)), (name, pad, n)
        states = {st for n in plan for st in plan[n]}
        assert states == {0, 1, None} and any(plan[n][0] is None or m[0][1] is None for n, m in marks.items())
    assert quiet > 0, "some tick had pass-through slots only"
    print(f"SPAN BANK {cid}: {worst:.1e} of the output's magnitude")


def test_passthrough_misuse():
    bank = StreamBank(2, 8, 24, lambda win, slots: win * 2.0)
    a = bank.open()
    with pytest.raises(ValueError):
        bank.set_passthrough(1, True)                             # not open
    x = np.arange(1, 41, dtype=np.float32)
    assert np.array_equal(bank.push({a: x[:11]})[a][0], 2 * x[:8])
    assert bank.set_passthrough(a, True) == 8
    assert np.array_equal(bank.push({a: x[11:20]})[a][0], x[8:16]) and bank.stats["launches"] == 1
    assert bank.set_passthrough(a, False) == 16
    assert np.array_equal(bank.close(a)[0], 2 * x[16:20])
    assert bank.open() == a and np.array_equal(bank.push({a: x[:8]})[a][0], 2 * x[:8])      # a reopened slot starts under the net


# ---- the exports ---------------------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_listed_and_refuse_by_name():
    from waveverify_amd import _lib
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    lib = _lib.load()
    for name in ("wv_span_gather", "wv_span_scatter_add"):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert proto, f"{name} is not declared"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(proto.group(1).split(","))
        zero = {C.c_int: 0, C.c_int64: 0, C.c_float: 0.0}
        assert getattr(lib, name)(*[zero.get(t) for t in args]) == -1
        assert lib.wv_last_error().decode().startswith(name)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "wv_span_gather" in integration and "wv_span_scatter_add" in integration
