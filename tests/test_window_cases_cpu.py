"""The windowed / live-session fuzz on the CPU (tests/window_cases.py): the case lists hit every edge they are written for, by name; the
analytic receptive field (window.receptive_context / halo) bounds the float64 oracle's measured one at EVERY phase of the hop; plan() on the
case lists partitions every clip; windows and live sessions on the float64 oracle, stitched, are the whole clip to 1e-12 of its magnitude;
the ticker's history is the input's tail after every tick.  No GPU, no library."""
import numpy as np
import pytest

import window_cases as W
from test_window_plan import _check_partition
from waveverify_amd.session import StreamSession, _Ticker, numpy_advance
from waveverify_amd.window import halo, plan, receptive_context

NETS = W.net_cases()
EXACT = [c for c in NETS if c[1] == "f32"]
F16 = [c for c in NETS if c[1] == "f16"]
STITCH_BAR = 1e-12                                                # of the output's largest magnitude; measured 6e-16


def _ids(cases):
    return [c[0] for c in cases]


# ---- the lists hit their edges -------------------------------------------------------------------------------------------------------------
def test_net_cases_cover_the_configurations():
    assert len({c[3][1] for c in EXACT}) >= 8
    seen = {k: set() for k in ("hop", "dilation_base", "residual_kernel_size", "n_residual_enc", "n_residual_dec", "strides")}
    for cid, _, kind, (_, idx, kw) in EXACT:
        seen["hop"].add(int(np.prod(kw["strides"])))
        seen["strides"].add(len(kw["strides"]))
        for k in ("dilation_base", "residual_kernel_size", "n_residual_enc", "n_residual_dec"):
            seen[k].add(kw[k])
    assert {8, 12, 16, 20, 24, 32} <= seen["hop"], seen
    assert {1, 2} <= seen["dilation_base"] and {3, 5} <= seen["residual_kernel_size"], seen
    assert {0, 3} <= seen["n_residual_enc"] and {0, 3} <= seen["n_residual_dec"] and 4 in seen["strides"], seen
    for idx in W.EXACT:
        assert {c[2] for c in EXACT if c[3][1] == idx} == set(W.KINDS)
    ids = {c[3][1] for c in F16}
    assert {"generator", "detector", "locator", "nbits36.detector", "narrow16.detector", "narrow16.generator"} <= ids
    sweeps = {i.split(".")[0] for i in ids if i.startswith("sweep")}
    assert len(sweeps) >= 2 and all({f"{s}.{k}" for k in W.KINDS} <= ids for s in sweeps)


@pytest.mark.parametrize("case", NETS, ids=_ids(NETS))
def test_clip_cases_hit_the_planner_edges(case):
    cfg, _ = W.net_config(case)
    hop, H = cfg.hop_length, halo(cfg)
    kinds_seen, windows_seen, per_window = set(), set(), {}
    for wk, window, kinds, lengths in W.clip_cases(cfg):
        L = -(-window // hop) * hop
        windows_seen.add(wk)
        assert 3 <= len(lengths) <= 5 and max(lengths) <= 4 * L
        assert min(lengths) <= L < max(lengths), "a list mixes clips of one window with clips of several"
        want = W.lengths_of(L, H, hop, 2)
        counts = {}
        for name, T in zip(kinds, lengths):
            assert T == want[name]
            counts[name] = plan([T], window, cfg)
            kinds_seen.add(name)
        if wk == "min":
            assert window == H + hop == L
        if wk == "min+hop":
            assert window == H + 2 * hop == L
        if wk == "drawn":
            assert (window - H) % hop == 0 and 3 <= (window - H) // hop <= 8
        if wk == "unrounded":
            assert window % hop and L > window
        # the named edges are what their names say
        for name, launches in counts.items():
            wins = sorted((w for g in launches for w in g), key=lambda w: w.start)
            if name in ("one", "hop-1", "hop", "L-1", "L"):
                assert len(wins) == 1 and wins[0].length == want[name]
            if name == "L+1":
                assert len(wins) == 2 and wins[1].keep_hi - wins[1].keep_lo == 1
            if name == "edge-1":
                assert len(wins) == 2 and wins[1].length == L - 1
            if name == "edge":
                assert len(wins) == 2 and wins[1].length == L and wins[1].keep_hi == want[name]
            if name == "edge+1":
                assert len(wins) == 3 and wins[1].length == L and wins[2].keep_hi - wins[2].keep_lo == 1
            if name == "four-ragged":
                assert len(wins) >= 4 and wins[-1].length % hop and wins[-1].length < L
        per_window.setdefault(wk, set()).update(kinds)
    assert kinds_seen == set(W.LENGTH_KINDS) and windows_seen == set(W.WINDOW_KINDS)
    assert all(k == set(W.LENGTH_KINDS) for k in per_window.values()), "every length kind at every window"
    assert set(W.MAX_WINDOWS) == {1, 2, 64}


@pytest.mark.parametrize("case", NETS, ids=_ids(NETS))
def test_push_cases_hit_the_ticker_edges(case):
    cfg, _ = W.net_config(case)
    hop, H = cfg.hop_length, halo(cfg)
    scheds = W.push_cases(cfg)
    assert {S for _, S, _ in scheds} == {1, 3}
    sizes = [n for _, _, s in scheds for n in s]
    assert {1, hop - 1, hop, hop + 1} <= set(sizes)
    assert any(s and s[0] == 0 for _, _, s in scheds), "a first push of 0"
    assert any(n > H + hop for n in sizes), "a push beyond the history capacity"
    assert any(s and sum(s) % hop == 0 for _, _, s in scheds), "a hop-aligned total: flush() emits nothing"
    assert any(sum(s) % hop for _, _, s in scheds), "a ragged total"
    assert any(s == () for _, _, s in scheds), "flush() alone"
    run = 0
    for _, _, s in scheds:
        seen = cur = 0
        for n in s:
            cur = cur + 1 if (seen + n) // hop == seen // hop and n > 0 else 0
            run = max(run, cur)
            seen += n
    assert run >= 3, "a run of pushes none of which completes a frame"


def test_advance_cases_hit_their_edges():
    cases = W.advance_cases()
    for S, hcap, hv, n, wlen, drop, hv2 in cases:                   # the documented contract
        assert S >= 1 and hcap >= 1 and 0 <= hv <= hcap and n >= 0 and 0 <= wlen <= hv + n and drop >= 0 and 0 <= hv2 <= hcap and drop + hv2 == hv + n
    has = lambda f: any(f(*c) for c in cases)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: hv == 0 and n > 0)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: n == 0 and wlen == 0 and hv2 > 0)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: n == 0 and wlen > 0)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: hv2 == 0 and wlen > 0)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: wlen == 0 and hv2 == 0)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: wlen < 256 < hv2)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: hv2 < 256 < wlen)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: 256 < hv2 < wlen)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: 256 < wlen < hv2)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: wlen == hv2 == 256)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: hcap % 4 and n % 4 and wlen % 4)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: drop > hv > 0)
    assert has(lambda S, hcap, hv, n, wlen, drop, hv2: S > 64)


def test_data_movement_tables_hit_their_edges():
    tables = W.reduce_mean_cases()
    assert {nb for _, nb, *_ in tables} == {1, 16, 36}
    for nb in (16, 36):
        sizes = [(len(lengths)) * nb_ for _, nb_, _, _, lengths in tables if nb_ == nb]
        assert min(sizes) < 256 < max(sizes)
    for n_rows, nb, ptr, rows, lengths in tables:
        assert len(ptr) == len(lengths) + 1 and ptr[-1] == len(rows)
        real = [r for r in rows if 0 <= r < n_rows]
        assert real != sorted(real), "rows in permuted order"
        assert any(a == b for a, b in zip(ptr, ptr[1:])), "an empty row range"
        assert 0 in lengths and -1 in rows and n_rows in rows
    assert {L % 4 for L in W.GATHER_L} >= {0, 1, 3} and min(W.GATHER_L) == 1
    assert any(L < 1024 for L in W.GATHER_L) and 1024 in W.GATHER_L and any(1024 < L < 2048 for L in W.GATHER_L) and max(W.GATHER_L) > 2048
    for L in W.GATHER_L:                                            # every row class of dst meets every residue of the source offset
        offs = W.gather_offsets(L + 41, L)
        assert {(w % 4, o % 4) for w, o in enumerate(offs[:W.GATHER_INSIDE])} == {(r, q) for r in range(4) for q in range(4)}
        assert sum(0 <= o <= 41 for o in offs) == W.GATHER_INSIDE + 1 and sum(not 0 <= o <= 41 for o in offs) >= 3
        for e in (0, 1):                                            # so both paths' conditions occur wherever L % 4 allows
            paths = W.gather_paths(L, e, L + 41)
            assert {s_ for s_, _ in paths} == {True, False}
            assert {d for _, d in paths} == ({True} if L % 4 == 0 and e == 0 else {False} if L % 4 == 0 else {True, False})
            assert (True, True) in paths or (L % 4 == 0 and e == 1)
    sc = W.scatter_cases()
    assert {C for C, *_ in sc} == {1, 3, 17} and {L for _, L, *_ in sc} == set(W.GATHER_L)
    for L in W.GATHER_L:
        assert {u for _, L_, u, _ in sc if L_ == L} == {"sample", "frame"}
    for C, L, unit, keeps in sc:
        assert (0, L) in keeps and any(lo == hi for lo, hi in keeps) and any(hi == L and lo > 0 for lo, hi in keeps)
        if L > 8:
            assert {lo % 4 for lo, _ in keeps} == {0, 1, 2, 3} and {hi % 4 for _, hi in keeps} == {0, 1, 2, 3}
            assert {e for e in (0, 1) if W.scatter_paths((C, L, unit, keeps), e) == {True, False}}, "rows on the 16-byte path and rows on the scalar one"
        Ts, desc, n_out = W.scatter_layout((C, L, unit, keeps))
        assert [d[2:] for d in desc] == [list(k) for k in keeps] and n_out == C * sum(Ts)
        if L > 8:
            assert {(d[0] + c * d[1]) % 4 for d in desc for c in range(C)} == {0, 1, 2, 3}, "destination rows at every residue mod 4"


# ---- the receptive field, at every phase of the hop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_receptive_field_at_every_phase(case):
    """One input sample perturbed at p = 2 hop + phase, every phase of the hop (the phases run as one batch of the float64 oracle): no
    output changes at or beyond p + halo, none before p's frame, and the largest reach t - p over the phases is <= receptive_context."""
    cfg, sd, onet = W.oracle_net(case)
    hop, H, R = cfg.hop_length, halo(cfg), receptive_context(cfg)
    assert H % hop == 0 and H > R >= H - hop
    T = 3 * hop + H + hop + 3
    x, msg = W.clip_data(case, T, 0)
    reach, base = 0, {}
    for lo in range(0, hop, 8):                                     # a row is compared with the same row of an unperturbed batch of the same shape:
        ph = list(range(lo, min(hop, lo + 8)))                      # the same arithmetic, so any difference is the perturbation's
        n = len(ph)
        if n not in base:
            base[n] = W.oracle_forward(cfg, onet, np.repeat(x, n, axis=0), np.repeat(msg, n, axis=0))
        xb = np.repeat(x, n, axis=0)
        for i, f in enumerate(ph):
            xb[i, 0, 2 * hop + f] += 0.5
        yb = W.oracle_forward(cfg, onet, xb, np.repeat(msg, n, axis=0))
        for i, f in enumerate(ph):
            p = 2 * hop + f
            changed = np.nonzero(np.any(yb[i] != base[n][i], axis=0))[0]
            assert changed.size, f"phase {f}: the perturbation reached no output"
            assert changed.max() < p + H, (f, int(changed.max()) - p, H)
            assert changed.min() >= p // hop * hop, (f, int(changed.min()), p)
            reach = max(reach, int(changed.max()) - p)
    print(f"REACH {case[0]}: hop {hop} halo {H} receptive_context {R} measured {reach} ({'tight' if reach == R else f'{R - reach} short of the formula'})")
    assert reach <= R, (reach, R)


# ---- plan() on the case lists ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NETS, ids=_ids(NETS))
def test_plan_partitions_every_clip_list(case):
    cfg, _ = W.net_config(case)
    hop, H = cfg.hop_length, halo(cfg)
    for _, window, _, lengths in W.clip_cases(cfg):
        L = -(-window // hop) * hop
        for mw in W.MAX_WINDOWS:
            launches = plan(lengths, window, cfg, mw)
            _check_partition(launches, list(lengths), hop, mw)
            for w in (w for g in launches for w in g):
                assert w.length <= L
                if w.start == 0:
                    assert w.keep_lo == 0
                else:                                               # every non-first window keeps from exactly start + H
                    assert w.keep_lo == w.start + H
            firsts = [w for g in launches for w in g if w.start == 0]
            assert sorted(w.clip for w in firsts) == list(range(len(lengths)))


# ---- stitched oracle windows and oracle sessions ------------------------------------------------------------------------------------------------
def _stitch_lists(cfg, idx):
    """The minimum window's list and, under another rotation, the drawn window's: all ten length kinds on one or the other."""
    a = W.clip_cases(cfg, windows=("min", "drawn"), salt=idx, full=False)
    assert {k for _, _, kinds, _ in a for k in kinds} == set(W.LENGTH_KINDS)
    return a


@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_stitched_oracle_windows_equal_the_whole_clip(case):
    """What this pins is the alignment rules (hop phase, the clip's own start and end).  It does not pin the halo's last samples: the farthest
    taps carry so little weight that windows with a halo one hop short still stitch to about 1e-13; test_receptive_field_at_every_phase does."""
    cfg, sd, onet = W.oracle_net(case)
    worst = 0.0
    for wk, window, kinds, lengths in _stitch_lists(cfg, case[3][1]):
        data = [W.clip_data(case, T, b) for b, T in enumerate(lengths)]
        refs = [W.oracle_forward(cfg, onet, x, m)[0] for x, m in data]
        outs = [np.full_like(r, np.nan) for r in refs]
        for group in plan(lengths, window, cfg, 2):
            xw = np.concatenate([data[w.clip][0][:, :, w.start: w.start + w.length] for w in group])
            mw = np.concatenate([data[w.clip][1] for w in group])
            yw = W.oracle_forward(cfg, onet, xw, mw)
            for i, w in enumerate(group):
                outs[w.clip][:, w.keep_lo: w.keep_hi] = yw[i, :, w.keep_lo - w.start: w.keep_hi - w.start]
        for name, got, ref in zip(kinds, outs, refs):
            err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
            worst = max(worst, err)
            assert err <= STITCH_BAR, (wk, name, err)
    print(f"STITCH {case[0]}: {worst:.1e} of the output's magnitude")


@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_oracle_sessions_equal_the_whole_clip(case):
    cfg, sd, onet = W.oracle_net(case)
    hop, H = cfg.hop_length, halo(cfg)
    worst = 0.0
    for name, S, sizes in W.push_cases(cfg):
        T = sum(sizes)
        if T == 0:
            sess = StreamSession(S, hop, H, lambda win, keep: pytest.fail("a forward without samples"))
            assert sess.flush() is None and sess.samples_seen == 0
            continue
        x = np.concatenate([W.clip_data(case, T, s)[0] for s in range(S)])
        msg = np.concatenate([W.clip_data(case, T, s)[1] for s in range(S)])
        ref = W.oracle_forward(cfg, onet, x, msg)
        sess = StreamSession(S, hop, H, lambda win, keep: W.oracle_forward(cfg, onet, win, msg)[:, :, keep:], numpy_advance)
        outs, seen, emitted = [], 0, 0
        for n in sizes:
            y = sess.push(x[:, 0, seen: seen + n])
            seen += n
            got = 0 if y is None else y.shape[-1]
            assert got == seen // hop * hop - emitted
            emitted += got
            if y is not None:
                outs.append(y)
        y = sess.flush()
        assert (y is None) == (T % hop == 0)
        if y is not None:
            outs.append(y)
        got = np.concatenate(outs, axis=-1)
        assert got.shape == ref.shape
        err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
        worst = max(worst, err)
        assert err <= STITCH_BAR, (name, err)
    print(f"SESSION {case[0]}: {worst:.1e} of the output's magnitude")


# ---- the ticker ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NETS, ids=_ids(NETS))
def test_ticker_history_is_the_inputs_tail(case):
    cfg, _ = W.net_config(case)
    hop, H = cfg.hop_length, halo(cfg)
    for name, S, sizes in W.push_cases(cfg):
        T = sum(sizes)
        x = np.arange(1, S * T + 1, dtype=np.float32).reshape(S, T)
        tk = _Ticker(hop, H)
        hist = np.zeros((S, tk.cap), np.float32)
        seen = emitted = 0
        for n in list(sizes) + [None]:
            t_out0 = tk.t_out
            tick = tk.flush() if n is None else tk.push(n)
            new = x[:, seen: seen + (n or 0)]
            seen += n or 0
            assert 0 <= tick.hv <= tk.cap and 0 <= tick.hv2 <= tk.cap and tick.drop + tick.hv2 == tick.hv + new.shape[1], (name, tick)
            win, hist = numpy_advance(hist, new, tick)
            want = seen - emitted if n is None else seen // hop * hop - emitted
            assert tick.wlen - tick.keep == want if tick.wlen else want == 0, (name, tick)
            emitted += want
            if tick.wlen:                                           # the window ends at the last completed frame and starts at most H before the new ones
                end = emitted
                assert np.array_equal(win[:, 0], x[:, end - tick.wlen: end]) and tick.keep == t_out0 - (end - tick.wlen)
                assert tick.keep == min(t_out0, H) or end - tick.wlen == 0
            if n is None:
                assert tick.hv2 == 0 and emitted == T
            else:
                assert np.array_equal(hist[:, :tick.hv2], x[:, tk.h0: tk.t_in]) and tk.t_in == seen
