"""The session-bank case lists hit the edges they name, and the bank state machine (waveverify_amd/session.StreamBank) on the float64 oracle
gives every stream the whole-clip forward of what it pushed, whatever the launch grouping.  No GPU."""
import numpy as np
import pytest

import bank_cases as BK
import window_cases as W
from localized_cases import sigmoid64
from waveverify_amd.session import (StreamBank, Tick, _Ticker, bank_row_ok, numpy_advance, numpy_bank_advance, plan_tick)
from waveverify_amd.window import halo

EXACT, F16, F16_REFUSED = BK.net_cases()
STITCH_BAR = 1e-12                                                # tests/test_window_cases_cpu.py holds sessions to it; it measured 6e-16


def _ids(cases):
    return [c[0] for c in cases]


# ---- the lists -----------------------------------------------------------------------------------------------------------------------------
def test_net_cases_are_the_session_nets_of_the_window_fuzz():
    assert sorted({c[3][1] for c in EXACT}) == [0, 6, 9, 13, 14] and len(EXACT) == 15
    hops, halos = set(), set()
    for c in EXACT:
        cfg, _ = W.net_config(c)
        hops.add(cfg.hop_length)
        halos.add(halo(cfg))
    assert hops == {20, 16, 24, 12, 8} and min(halos) >= 176 and max(halos) <= 1032
    assert sorted(_ids(F16)) == sorted(BK.F16_BANKS) and len(F16_REFUSED) == 2


@pytest.mark.parametrize("case", EXACT[::3], ids=_ids(EXACT[::3]))
def test_schedules_hit_the_edges_by_name(case):
    cfg, _ = W.net_config(case)
    hop, H = cfg.hop_length, halo(cfg)
    (_, mixed), (_, equal) = BK.schedules(cfg)
    lengths = BK.stream_lengths(mixed)
    assert 4 <= len(lengths) - 1 <= BK.CAPACITY + 1 and max(lengths.values()) <= 3 * (H + hop)
    pushes = [arg for kind, arg in mixed if kind == "push"]
    assert any(sorted(p.values()) == sorted([0, 1, hop - 1, hop, hop + 1, 2 * hop + 3]) for p in pushes)        # one tick mixes them all
    assert any(n > H + hop for p in pushes for n in p.values())                                                 # a push beyond H + hop
    # the tickers say what each step does
    tk, events, first_tick, open_now, peak = {}, {}, {}, set(), 0
    tick_no = 0
    for kind, arg in mixed:
        if kind == "open":
            tk[arg], events[arg], first_tick[arg] = _Ticker(hop, H), [], tick_no
            open_now.add(arg)
            peak = max(peak, len(open_now))
        elif kind == "close":
            t = tk[arg].flush()
            events[arg].append(("close", t.wlen - t.keep if t.wlen else 0))
            open_now.discard(arg)
        else:
            for name in open_now:
                if name in arg:
                    t = tk[name].push(arg[name])
                    events[name].append(("push", t.wlen - t.keep if t.wlen else 0))
                else:
                    events[name].append(("absent", 0))
            tick_no += 1
    assert peak == BK.CAPACITY
    assert [e for e in events["B"][:4]] == [("push", 0)] * 4                       # a run that completes no frame
    assert events["B"][-1][0] == "close" and 0 < events["B"][-1][1] < hop           # closes mid-schedule with a partial frame
    assert events["C"][-1] == ("close", 0) and lengths["C"] % hop == 0              # closes on a hop multiple: nothing to emit
    assert ("absent", 0) in events["C"] and ("absent", 0) in events["A"]            # absent for some ticks
    assert first_tick["D"] == 3                                                     # opens at tick 3
    assert events["Z"] == [("close", 0)] and lengths["Z"] == 0                      # open then close with no push
    order = [(kind, arg) for kind, arg in mixed if kind != "push"]
    assert order.index(("close", "B")) < order.index(("open", "G"))                 # G reopens the lowest free slot: B's
    # the all-equal schedule: every push names every stream with one size
    assert all(len(set(arg.values())) == 1 and len(arg) == 4 for kind, arg in equal if kind == "push")


def test_advance_cases_hit_their_edges():
    assert tuple(c[1] for c in BK.advance_cases()) == (7, 255, 256, 257, 1025, 2051)
    for case in BK.advance_cases():
        capacity, hcap, A, Lmax, n_x, rows, kinds = case
        by = dict(zip(kinds, rows))
        assert all(bank_row_ok(r, capacity, hcap, n_x, A, Lmax) for r in rows)
        assert len({r[0] for r in rows}) == len(rows) < capacity and [r[0] for r in rows] != sorted(r[0] for r in rows)   # P < capacity, scattered
        windowed = [r for r in rows if r[5] > 0]
        assert len({r[4] for r in windowed}) == len(windowed) < A                   # distinct rows, one row of win unnamed
        slot, hv, x_off, n, row, wlen, drop, hv2 = by["still"]
        assert drop == 0 and n == 0 and hv2 == hv > 0
        slot, hv, x_off, n, row, wlen, drop, hv2 = by["overlap"]
        assert 0 < drop < hv and hv2 > drop
        slot, hv, x_off, n, row, wlen, drop, hv2 = by["from-x"]
        assert drop >= hv and hv2 == hcap and wlen == Lmax
        assert by["hv0"][1] == 0 and by["hv0"][5] > 0
        assert by["no-window"][5] == 0 and by["no-window"][3] > 0
        assert by["hop"][5] == 8 < Lmax
        for why, bad in BK.bad_rows(case):
            assert not bank_row_ok(bad, capacity, hcap, n_x, A, Lmax), why
        c2 = BK.second_tick(case)
        assert all(bank_row_ok(r, c2[0], c2[1], c2[4], c2[2], c2[3]) for r in c2[5])
        assert [r[1] for r in c2[5]] == [r[7] for r in rows]


# ---- the numpy restatement of wv_bank_advance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BK.advance_cases(), ids=[f"hcap{c[1]}" for c in BK.advance_cases()])
def test_numpy_bank_advance_is_numpy_advance_stream_by_stream(case):
    capacity, hcap, A, Lmax, n_x, rows, _ = case
    hist0, x = BK.advance_data(case, 0)
    hist = hist0.copy()
    win = numpy_bank_advance(hist, x, np.array(rows, np.int64), A, Lmax)
    named = set()
    for slot, hv, x_off, n, row, wlen, drop, hv2 in rows:
        rwin, rnext = numpy_advance(hist0[slot: slot + 1], x[None, x_off: x_off + n], Tick(hv, wlen, 0, drop, hv2))
        assert np.array_equal(hist[slot, :hv2].view(np.int32), rnext[0, :hv2].view(np.int32))
        assert np.array_equal(hist[slot, hv2:].view(np.int32), hist0[slot, hv2:].view(np.int32))       # beyond hv2: left as it was
        if wlen:
            assert np.array_equal(win[row, 0, :wlen].view(np.int32), rwin[0, 0].view(np.int32)) and not win[row, 0, wlen:].any()
        named.add(slot)
    for slot in set(range(capacity)) - named:
        assert np.array_equal(hist[slot].view(np.int32), hist0[slot].view(np.int32))
    # a bad row among them changes nothing of its own and nothing of the others
    for why, bad in BK.bad_rows(case):
        h2 = hist0.copy()
        w2 = numpy_bank_advance(h2, x, np.array([r for r in rows if r[0] != 2] + [bad], np.int64), A, Lmax)
        assert np.array_equal(h2[2].view(np.int32), hist0[2].view(np.int32)), why
        others = [s for s in range(capacity) if s != 2]
        assert np.array_equal(h2[others].view(np.int32), hist[others].view(np.int32)) and not w2[2].any(), why
        assert np.array_equal(w2[[0, 1, 3]].view(np.int32), win[[0, 1, 3]].view(np.int32)), why


def test_plan_tick_groups_by_pad_limit():
    ticks = {s: Tick(0, w, 0, 0, 0) for s, w in enumerate((40, 100, 40, 0, 59, 61, 0))}
    sizes = {s: (7 if s != 6 else 0) for s in ticks}
    for pad, want in ((1.0, [[0, 2], [4], [5], [1]]), (1.5, [[0, 2, 4], [5], [1]]), (float("inf"), [[0, 2, 4, 5, 1]])):
        plan = plan_tick(ticks, sizes, pad)
        got = [[s for s, _ in plan.windows[ln.a_lo: ln.a_lo + ln.A]] for ln in plan.launches]
        assert got == want, pad
        assert all(ln.Lmax <= pad * min(ticks[s].wlen for s in g) for ln, g in zip(plan.launches, got))
        assert [int(r[0]) for r in plan.desc[plan.launches[0].a_lo + plan.launches[0].A: plan.launches[0].p_hi]] == [3]   # idle rides in launch 0
        assert 6 not in plan.desc[:, 0] and plan.out[6] == (plan.n_out, 0)          # nothing pushed, nothing completed: no descriptor
        assert plan.padded == sum(ln.Lmax - ticks[s].wlen for ln, g in zip(plan.launches, got) for s in g)
    only_idle = plan_tick({3: Tick(2, 0, 0, 0, 5)}, {3: 3}, 1.5)
    assert [(ln.A, ln.Lmax, ln.p_hi - ln.p_lo) for ln in only_idle.launches] == [(0, 0, 1)]
    assert plan_tick({3: Tick(2, 0, 0, 0, 2)}, {3: 0}, 1.5).launches == []


# ---- the state machine on the float64 oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_oracle_banks_equal_the_whole_clip(case):
    """Every stream's concatenated outputs are the whole-clip oracle on what it pushed, to 1e-12 of its magnitude, at every pad_limit: right
    padding and grouping change nothing.  A detector's running mean probability after every push is that of its completed prefix (the
    whole-clip logits' first columns: the oracle is causal frame by frame, which tests/test_window_plan.py shows)."""
    cfg, sd, onet = W.oracle_net(case)
    hop, H, kind = cfg.hop_length, halo(cfg), cfg.kind
    worst = 0.0
    for name, steps in BK.schedules(cfg):
        data = BK.stream_data(case, steps)
        refs = {n: W.oracle_forward(cfg, onet, x[None, None], m[None])[0] for n, (x, m) in data.items() if x.size}
        for pad in BK.PAD_LIMITS:
            msgs = {}
            bank = StreamBank(BK.CAPACITY, hop, H, lambda win, slots: W.oracle_forward(cfg, onet, win, np.stack([msgs[s] for s in slots])),
                              pad_limit=pad)

            def open_args(n):
                msgs[min(set(range(BK.CAPACITY)) - set(bank.open_slots()))] = data[n][1]
                return ()
            out, _ = BK.run(bank, steps, {n: x for n, (x, _) in data.items()}, open_args)
            assert bank.open_slots() == []
            for n, (x, _) in data.items():
                parts = [r for _, _, r in out[n] if r is not None]
                seen = [(pos // hop * hop if k == "push" else pos) for k, pos, _ in out[n]]
                assert sum(p.shape[-1] for p in parts) == x.size and seen[-1] == x.size, (name, n)
                if not x.size:
                    continue
                got, ref = np.concatenate(parts, axis=-1), refs[n]
                mag = float(np.abs(ref).max())
                err = float(np.abs(got - ref).max()) / mag
                worst = max(worst, err)
                assert got.shape == ref.shape and err <= STITCH_BAR, (name, pad, n, err)
                if kind == "detector":
                    acc, done = np.zeros(ref.shape[0]), 0
                    for (_, _, r), upto in zip(out[n], seen):
                        if r is not None:
                            acc += sigmoid64(r).sum(axis=1)
                            done += r.shape[-1]
                        assert done == upto
                        if upto:
                            e = float(np.abs(acc / upto - sigmoid64(ref[:, :upto]).mean(axis=1)).max())
                            assert e <= STITCH_BAR, (name, pad, n, upto, e)
    print(f"BANK {case[0]}: {worst:.1e} of the output's magnitude")


def test_bank_misuse_changes_no_stream():
    bank = StreamBank(2, 8, 24, lambda win, slots: win * 2.0)
    a, b = bank.open(), bank.open()
    assert (a, b) == (0, 1) and bank.open_slots() == [0, 1]
    with pytest.raises(RuntimeError):
        bank.open()
    x = np.arange(1, 41, dtype=np.float32)
    assert np.array_equal(bank.push({a: x[:13], b: x[:3]})[a][0], 2 * x[:8])
    for bad in ({5: x[:8]}, {a: x[:8], -1: x[:8]}, {a: x[:8].reshape(2, 4)}, {a: x[:8], b: x[None, :8]}):
        with pytest.raises(ValueError):
            bank.push(bad)
    with pytest.raises(ValueError):
        bank.close(7)
    assert bank.samples_seen(a) == 8 and bank.samples_seen(b) == 0                   # the refused pushes advanced nothing
    assert np.array_equal(bank.close(b)[0], 2 * x[:3])
    with pytest.raises(ValueError):
        bank.push({b: x[:1]})
    with pytest.raises(ValueError):
        bank.samples_seen(b)
    assert np.array_equal(bank.push({a: x[13:40]})[a][0], 2 * x[8:40]) and bank.open() == b
    with pytest.raises(ValueError):
        StreamBank(0, 8, 24, None)
    with pytest.raises(ValueError):
        StreamBank(2, 8, 24, None, pad_limit=0.9)
