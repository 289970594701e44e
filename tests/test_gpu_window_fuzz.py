"""Windowed and live-session execution on small nets against float64 (waveverify_amd/window.py, session.py, csrc/wv_window.hip and the
windowed modes of the head kernels), on the cases of tests/window_cases.py.

a. The four data-movement entry points through the C ABI on guarded arenas (tests/guard.py), every pointer on a 256-byte boundary and one
   element past it: bit-equal to numpy restatements, nothing written outside what they promise, every documented refusal -1.
b. windowed_generator / _locator / _detector / _detector_mean_prob / _detector_frame_sums of nine drawn configurations (each as generator,
   detector and locator) against the FLOAT64 ORACLE ON THE WHOLE CLIP, at the bars of test_gpu_infer_fuzz.test_whole_nets_fuzz (5e-5
   generator, 1e-4 logits, of the reference's largest magnitude over the clip list) and test_gpu_window's 1e-6 on mean probabilities; the
   result of a clip bit-equal across max_windows 1 / 2 / 64 and whether it runs alone or in a mixed list.
c. EmbedSession / LocateSession / DetectSession over push schedules, against the same oracle and bars.
d. b and c with precision="f16" against oracle/wv_oracle_h16 on the whole clip at test_gpu_h16's WM_BAR / LOGIT_BAR / det_mean_bar(T).

Every figure is printed as a MEASURE line before it is asserted (pytest -s); the worst cases measured on the MI355X stand below the bars."""
import functools

import numpy as np
import pytest
import torch

import window_cases as W
from guard import Guards
from localized_cases import frame_sums_ref, sigmoid64
from waveverify_amd.session import Tick, numpy_advance

pytestmark = pytest.mark.gpu

GEN_BAR, LOGIT_BAR32 = 5e-5, 1e-4                                 # tests/test_gpu_infer_fuzz.py::test_whole_nets_fuzz
MEAN_BAR = 1e-6                                                   # tests/test_gpu_window.py (mean probabilities, windowed and sessions)

# MEASURED on the MI355X, the worst case per kind over the whole file (test_print_the_worst_cases prints them).  Relative figures are of the
# reference's largest magnitude over the clip list; no bar had to be widened, so no whole-clip comparison stands behind any of them.
#   exact, windowed   generator 6.4e-7 (residual alone 4.0e-6; bar 5e-5), detector logits 7.4e-6, locator logits 2.3e-6 (bar 1e-4),
#                     mean probability 1.9e-7 (bar 1e-6), frame sums per gated sample 1.5e-6 gated / 8.0e-7 without a gate
#   exact, sessions   EmbedSession 7.3e-7, LocateSession 2.3e-6, DetectSession mean probability 1.2e-7
#   f16, windowed     generator 5.8e-5 absolute (WM_BAR 1e-4), detector logits 2.8e-4 and locator logits 1.8e-4 of max(1, |logits|max)
#                     (LOGIT_BAR 1e-3), mean probability 0.26 of det_mean_bar(T) with the head16 tail, 0.06 with the f32 tail (36 bits)
#   f16, sessions     EmbedSession 4.6e-5 absolute, LocateSession 9.9e-5, DetectSession 0.17 of det_mean_bar(T)
# The data-movement tests and every grouping comparison are bit equality.

NETS = W.net_cases()
EXACT = [c for c in NETS if c[1] == "f32"]
F16 = [c for c in NETS if c[1] == "f16" and c[3][1] not in W.F16_REFUSED]
F16_REFUSED = [c for c in NETS if c[1] == "f16" and c[3][1] in W.F16_REFUSED]
FRAME_SUM_NETS = (0, 6, 14)                                       # hop 20, 16 and 8
SESSION_NETS = (0, 6, 9, 13, 14)                                  # hop 20, 16, 24, 12 and 8; #6 and #9 have four strides


def _ids(cases):
    return [c[0] for c in cases]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


@functools.lru_cache(maxsize=None)
def _net(cid):
    """-> (case, cfg, HipNet, float64 oracle net) of a case id, built once."""
    from waveverify_amd.nets import HipNet
    case = next(c for c in NETS if c[0] == cid)
    cfg, sd, onet = W.oracle_net(case)
    return case, cfg, HipNet(cfg, sd), onet


@functools.lru_cache(maxsize=None)
def _net16(cid):
    """-> (case, cfg, HipNet, torch oracle net of the f16 mode's arithmetic)."""
    from oracle import wv_oracle_torch as OT
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    case = next(c for c in NETS if c[0] == cid)
    cfg, seed = W.net_config(case)
    sd = random_state_dict(cfg, seed)
    return case, cfg, HipNet(cfg, sd), OT.Net(cfg, sd)


WORST = {}


def measure(what, err, bar):
    """Print, keep the worst per `what`, assert."""
    WORST[what] = max(WORST.get(what, 0.0), err)
    print(f"MEASURE {what}: {err:.2e} (bar {bar:.1e}; worst so far {WORST[what]:.2e})")
    assert np.isfinite(err) and err <= bar, (what, err, bar)


def rel_err(got, ref, mag):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max()) / mag if ref.size else 0.0


# =============================================================================================== a. data movement through the C ABI
def _abi():
    """-> (the library, torch's current stream as the ABI's `void* stream`)."""
    from waveverify_amd import _lib
    return _lib.load(), _lib.stream()


def _advance(lib, st, hist, hcap, hv, x, n, win, wlen, hout, drop, hv2, S):
    return lib.wv_session_advance(hist, hcap, hv, x, n, win, wlen, hout, drop, hv2, S, st)


ADVANCE = W.advance_cases()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", ADVANCE, ids=["-".join(map(str, c)) for c in ADVANCE])
def test_session_advance_vs_numpy(case, offset):
    """win and hist_out[:, :hv2] bit-equal to session.numpy_advance, hist_out[:, hv2:] unwritten; then that history, its tail still holding the
    guard pattern, goes back in as `hist` for a second tick, which matches the reference run on the zero-tailed history."""
    S, hcap, hv, n, wlen, drop, hv2 = case
    lib, st = _abi()
    rng = np.random.default_rng(W.seed_of("advance", case))
    hist_np = rng.standard_normal((S, hcap)).astype(np.float32)
    x_np = rng.standard_normal((S, n)).astype(np.float32)
    g = Guards(offset=offset)
    hist = g.input(hist_np, "hist")
    x = g.input(x_np, "x") if n else None
    win = g.output((S, 1, wlen), name="win") if wlen else None
    hout = g.output((S, hcap), name="hist_out")
    rc = _advance(lib, st, hist.t.data_ptr(), hcap, hv, x.t.data_ptr() if n else None, n, win.t.data_ptr() if wlen else None, wlen,
                  hout.t.data_ptr(), drop, hv2, S)
    assert rc == 0
    torch.cuda.synchronize()
    rwin, rnext = numpy_advance(hist_np, x_np, Tick(hv, wlen, 0, drop, hv2))
    tail = torch.zeros((S, hcap), dtype=torch.bool)
    tail[:, hv2:] = True
    hist.check()
    if n:
        x.check()
    hout.check(expect_unwritten=tail)
    assert np.array_equal(bits(hout.t[:, :hv2]), rnext[:, :hv2].view(np.int32))
    if wlen:
        win.check()
        assert np.array_equal(bits(win.t), rwin.view(np.int32))
    # the second tick: everything valid plus the same new samples; the window takes all of it, the history keeps what fits
    hv_b, n_b = hv2, n
    wlen_b, hv2_b = hv_b + n_b, min(hcap, hv_b + n_b)
    drop_b = hv_b + n_b - hv2_b
    g2 = Guards(offset=offset)
    win2 = g2.output((S, 1, wlen_b), name="win2") if wlen_b else None
    hout2 = g2.output((S, hcap), name="hist_out2")
    snap = bits(hout.t)
    rc = _advance(lib, st, hout.t.data_ptr(), hcap, hv_b, x.t.data_ptr() if n else None, n_b, win2.t.data_ptr() if wlen_b else None, wlen_b,
                  hout2.t.data_ptr(), drop_b, hv2_b, S)
    assert rc == 0
    torch.cuda.synchronize()
    rwin2, rnext2 = numpy_advance(rnext, x_np, Tick(hv_b, wlen_b, 0, drop_b, hv2_b))
    tail2 = torch.zeros((S, hcap), dtype=torch.bool)
    tail2[:, hv2_b:] = True
    hout2.check(expect_unwritten=tail2)
    assert np.array_equal(bits(hout.t), snap) and not hout.guard_report()
    assert np.array_equal(bits(hout2.t[:, :hv2_b]), rnext2[:, :hv2_b].view(np.int32))
    if wlen_b:
        win2.check()
        assert np.array_equal(bits(win2.t), rwin2.view(np.int32))


@pytest.mark.parametrize("offset", [0, 1])
def test_session_advance_refusals(offset):
    """Each documented refusal returns -1 (WV_EINVAL) and leaves the guarded outputs as they were."""
    lib, st = _abi()
    S, hcap, hv, n, wlen, drop, hv2 = 2, 37, 11, 9, 16, 4, 16
    rng = np.random.default_rng(3)
    g = Guards(offset=offset)
    hist = g.input(rng.standard_normal((S, hcap)).astype(np.float32), "hist")
    x = g.input(rng.standard_normal((S, hcap + 1)).astype(np.float32), "x")          # long enough for every n below
    win, hout = g.output((S, 1, 64), name="win"), g.output((S, hcap), name="hist_out")
    H, X, Wn, O_ = hist.t.data_ptr(), x.t.data_ptr(), win.t.data_ptr(), hout.t.data_ptr()
    ok = dict(hist=H, hcap=hcap, hv=hv, x=X, n=n, win=Wn, wlen=wlen, hout=O_, drop=drop, hv2=hv2, S=S)
    refusals = {                                                  # each changes the valid call so that one condition alone is at fault
        "hist == hist_out": dict(hout=H),
        "hv > hcap": dict(hv=hcap + 1, drop=drop + hcap + 1 - hv),
        "wlen > hv + n": dict(wlen=hv + n + 1),
        "drop + hv2 != hv + n (short)": dict(drop=drop - 1),
        "drop + hv2 != hv + n (long)": dict(hv2=hv2 + 1),
        "hv2 > hcap": dict(n=hcap + 1, drop=hv, hv2=hcap + 1),
        "n > 0 without x": dict(x=None),
        "wlen > 0 without win": dict(win=None),
        "S == 0": dict(S=0),
        "S == 65536": dict(S=65536),
        "null hist": dict(hist=None),
        "null hist_out": dict(hout=None),
    }
    everything = lambda o: torch.ones(o.t.shape, dtype=torch.bool)
    for why, change in refusals.items():
        a = dict(ok, **change)
        rc = _advance(lib, st, a["hist"], a["hcap"], a["hv"], a["x"], a["n"], a["win"], a["wlen"], a["hout"], a["drop"], a["hv2"], a["S"])
        assert rc == -1, (why, rc)
        assert lib.wv_last_error(), why
        torch.cuda.synchronize()
        win.check(expect_unwritten=everything(win))
        hout.check(expect_unwritten=everything(hout))
        hist.check(), x.check()
    rc = _advance(lib, st, ok["hist"], hcap, hv, X, n, Wn, wlen, O_, drop, hv2, S)      # and the call they were all derived from runs
    assert rc == 0


REDUCE = W.reduce_mean_cases()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", REDUCE, ids=[f"nb{c[1]}-B{len(c[4])}" for c in REDUCE])
def test_window_reduce_mean_vs_a_sequential_f64_loop(case, offset):
    n_rows, nb, ptr, rows, lengths = case
    lib, st = _abi()
    B = len(lengths)
    rng = np.random.default_rng(W.seed_of("reduce data", nb, B))
    psum_np = (rng.uniform(0, 1, (n_rows, nb)) * rng.integers(1, 5000, (n_rows, 1))).astype(np.float32)
    ref = np.zeros((B, nb), np.float32)
    for b in range(B):
        for k in range(nb):
            acc = 0.0
            for r in rows[ptr[b]: ptr[b + 1]]:                    # the table's order, one f64 add per row
                if 0 <= r < n_rows:
                    acc += float(psum_np[r, k])
            ref[b, k] = np.float32(acc / lengths[b]) if lengths[b] > 0 else np.float32(0)
    g = Guards(offset=offset)
    psum, ptr_g, rows_g = g.input(psum_np, "psum"), g.input(np.array(ptr, np.int32), "ptr"), g.input(np.array(rows, np.int32), "rows")
    len_g = g.input(np.array(lengths, np.int64), "lengths")
    mean = g.output((B, nb), name="mean")
    rc = lib.wv_window_reduce_mean(psum.t.data_ptr(), n_rows, ptr_g.t.data_ptr(), rows_g.t.data_ptr(), len_g.t.data_ptr(), mean.t.data_ptr(), B, nb, st)
    assert rc == 0
    g.check()                                                     # inputs unchanged, guards intact, every element of mean written
    assert np.array_equal(bits(mean.t), ref.view(np.int32))
    assert (mean.t[3] == 0).all() and (mean.t[1] == 0).all()      # len == 0; an empty row range


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("L", W.GATHER_L)
def test_window_gather_rows_choose_their_path(L, offset):
    """Every row class of dst (row w starts w * L floats in) meets every residue mod 4 of the source offset, so with L % 4 != 0 the 16-byte and
    the scalar path are chosen row by row (window_cases.gather_paths, asserted for both buffer alignments in test_window_cases_cpu.py);
    out-of-range offsets leave their rows unwritten."""
    lib, st = _abi()
    rng = np.random.default_rng(W.seed_of("gather", L))
    n_src = L + 41
    src_np = rng.standard_normal(n_src).astype(np.float32)
    offs_np = np.array(W.gather_offsets(n_src, L), np.int64)
    Wn = len(offs_np)
    g = Guards(offset=offset)
    src, offs = g.input(src_np, "src"), g.input(offs_np, "offs")
    dst = g.output((Wn, 1, L), name="dst")
    assert src.t.data_ptr() % 16 == dst.t.data_ptr() % 16 == 4 * offset           # the alignment gather_paths was evaluated for
    assert lib.wv_window_gather(src.t.data_ptr(), n_src, offs.t.data_ptr(), dst.t.data_ptr(), Wn, L, st) == 0
    torch.cuda.synchronize()
    inside = (offs_np >= 0) & (offs_np + L <= n_src)
    assert inside.sum() == W.GATHER_INSIDE + 1 and (~inside).sum() >= 3
    dst.check(expect_unwritten=torch.from_numpy(np.repeat(~inside, L).reshape(Wn, 1, L)))
    src.check(), offs.check()
    got = dst.t.cpu().numpy()
    for w in np.nonzero(inside)[0]:
        assert np.array_equal(got[w, 0].view(np.int32), src_np[offs_np[w]: offs_np[w] + L].view(np.int32)), (w, offs_np[w])


SCATTER = W.scatter_cases()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", SCATTER, ids=[f"C{c[0]}-L{c[1]}-{c[2]}" for c in SCATTER])
def test_window_scatter_writes_only_the_kept_ranges(case, offset):
    """One window per keep range, each into a clip of its own whose start puts the destination at another residue mod 4
    (window_cases.scatter_layout).  The descriptors are window.scatter's (sample units) or window.frame_scatter_desc's (frame units: L counts
    frames, the last kept frame of a clip partial)."""
    Cc, L, unit, keeps = case
    lib, st = _abi()
    rng = np.random.default_rng(W.seed_of("scatter", case))
    Wn = len(keeps)
    Ts, desc, n_out = W.scatter_layout(case)
    y_np = rng.standard_normal((Wn, Cc, L)).astype(np.float32)
    g = Guards(offset=offset)
    y, desc_g = g.input(y_np, "y"), g.input(np.array(desc, np.int64), "desc")
    out = g.output((n_out,), name="out")
    assert y.t.data_ptr() % 16 == out.t.data_ptr() % 16 == 4 * offset             # the alignment scatter_paths was evaluated for
    assert lib.wv_window_scatter(y.t.data_ptr(), desc_g.t.data_ptr(), out.t.data_ptr(), n_out, Wn, Cc, L, st) == 0
    torch.cuda.synchronize()
    want, written = np.zeros(n_out, np.float32), np.zeros(n_out, bool)
    for w, (o, rs, lo, hi) in enumerate(desc):
        for c in range(Cc):
            want[o + c * rs + lo: o + c * rs + hi] = y_np[w, c, lo:hi]
            written[o + c * rs + lo: o + c * rs + hi] = True
    assert written.sum() == Cc * sum(hi - lo for lo, hi in keeps)
    out.check(expect_unwritten=torch.from_numpy(~written))
    y.check(), desc_g.check()
    assert np.array_equal(out.t.cpu().numpy()[written].view(np.int32), want[written].view(np.int32))


# =============================================================================================== b. windowed forwards, exact path
def _clips(case, lengths):
    data = [W.clip_data(case, T, b) for b, T in enumerate(lengths)]
    return [x for x, _ in data], np.concatenate([m for _, m in data])


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and torch.equal(u, v), f"{what}: clip {i} differs"


def _grouping(run, n_clips, what, alone=True):
    """run(max_windows, clip indices or None) -> list of tensors.  Bit-equal across max_windows, and alone against in the list."""
    outs = {mw: run(mw, None) for mw in W.MAX_WINDOWS}
    for mw in W.MAX_WINDOWS[1:]:
        _same(outs[mw], outs[W.MAX_WINDOWS[0]], f"{what}: max_windows {mw} against {W.MAX_WINDOWS[0]}")
    for b in range(n_clips if alone else 0):
        _same(run(64, [b]), [outs[64][b]], f"{what}: clip {b} alone against in the list")
    return outs[64]


@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_windowed_forwards_vs_float64(case):
    from waveverify_amd import window
    case, cfg, net, onet = _net(case[0])
    kind, hop, nb, idx = cfg.kind, cfg.hop_length, cfg.head_bits, case[3][1]
    for wk, win, kinds, lengths in W.clip_cases(cfg, salt=idx, full=False):       # each length kind at two of the four windows
        xs, msg = _clips(case, lengths)
        xt, mt = [cu(x[0, 0]) for x in xs], cu(msg)
        what = f"{case[0]} window {wk}={win} lengths {lengths}"
        pick = lambda sel: (xt if sel is None else [xt[b] for b in sel])
        if kind == "generator":
            delta = [W.oracle_forward(cfg, onet, x, msg[b: b + 1], add_input=False)[0, 0] for b, x in enumerate(xs)]
            for add in (True, False):
                refs = [d + x[0, 0].astype(np.float64) for d, x in zip(delta, xs)] if add else delta
                run = lambda mw, sel: window.windowed_generator(net, pick(sel), mt if sel is None else mt[sel], window=win, max_windows=mw, add_input=add)
                got = _grouping(run, len(xs), what, alone=add)             # add_input changes no window, row or descriptor
                mag = max(float(np.abs(r).max()) for r in refs)
                for b, (y, r) in enumerate(zip(got, refs)):
                    assert y.shape == (lengths[b],)
                    measure(f"exact generator{'' if add else ' (residual alone)'}", rel_err(y, r, mag), GEN_BAR)
        else:
            refs = [W.oracle_forward(cfg, onet, x)[0] for x in xs]                     # [C, T] float64
            mag = max(float(np.abs(r).max()) for r in refs)
            fwd = window.windowed_locator if kind == "locator" else window.windowed_detector
            got = _grouping(lambda mw, sel: fwd(net, pick(sel), window=win, max_windows=mw), len(xs), what)
            for b, (y, r) in enumerate(zip(got, refs)):
                assert y.shape == ((lengths[b],) if kind == "locator" else (nb, lengths[b]))
                measure(f"exact {kind} logits", rel_err(y.view(r.shape), r, mag), LOGIT_BAR32)
            if kind == "detector":
                mref = np.stack([sigmoid64(r).mean(axis=1) for r in refs])
                mp = _grouping(lambda mw, sel: list(window.windowed_detector_mean_prob(net, pick(sel), window=win, max_windows=mw)), len(xs), what + " mean")
                assert torch.stack(mp).shape == (len(xs), nb)
                measure("exact detector mean probability", rel_err(torch.stack(mp), mref, 1.0), MEAN_BAR)
                if idx in FRAME_SUM_NETS:
                    _frame_sums(net, cfg, xt, refs, lengths, win, mag, what)
    # a [B,1,T] tensor returns [B,C,T], bit-equal to the list form
    T = lengths[-1]
    xb = np.concatenate([W.clip_data(case, T, b)[0] for b in range(2)])
    if kind == "generator":
        m2 = np.concatenate([W.clip_data(case, T, b)[1] for b in range(2)])
        yb = window.windowed_generator(net, cu(xb), cu(m2), window=win, max_windows=2)
        yl = window.windowed_generator(net, [cu(xb[0, 0]), cu(xb[1, 0])], cu(m2), window=win, max_windows=2)
        assert yb.shape == (2, 1, T)
    else:
        fwd = window.windowed_locator if kind == "locator" else window.windowed_detector
        yb, yl = fwd(net, cu(xb), window=win, max_windows=2), fwd(net, [cu(xb[0, 0]), cu(xb[1, 0])], window=win, max_windows=2)
        assert yb.shape == (2, nb, T)
    assert torch.equal(yb, torch.stack([y.view(yb.shape[1:]) for y in yl]))


def _frame_sums(net, cfg, xt, refs, lengths, win, mag, what):
    """windowed_detector_frame_sums with and without gates against localized_cases.frame_sums_ref of the float64 logits.  The gated-sample
    counts are exact.  A frame's sum owes what its samples' logits owe: sigmoid's slope is at most 1/4, so LOGIT_BAR32 * |logits|max / 4 per
    gated sample, plus the 1e-6 per sample that the mean probabilities are held to (f32 sigmoids summed in f32)."""
    from waveverify_amd import window
    hop, nb = cfg.hop_length, cfg.head_bits
    bar = LOGIT_BAR32 * mag / 4 + MEAN_BAR
    rng = np.random.default_rng(W.seed_of("gates", what))
    gates_np = [rng.uniform(0, 1, T).astype(np.float32) for T in lengths]
    gates_np[0][:] = 0.0                                          # one clip wholly ungated
    gates = [cu(gt) for gt in gates_np]
    for gated in (True, False):
        run = lambda mw, sel: window.windowed_detector_frame_sums(net, xt if sel is None else [xt[b] for b in sel],
                                                                  (gates if sel is None else [gates[b] for b in sel]) if gated else None,
                                                                  0.4 if gated else 0.0, window=win, max_windows=mw)
        got = _grouping(run, len(xt), what + " frame sums")
        for b, T in enumerate(lengths):
            ref = frame_sums_ref(refs[b][None], gates_np[b] if gated else None, 0.4, hop, T)[0]
            assert got[b].shape == ref.shape == (nb + 1, -(-T // hop))
            assert np.array_equal(got[b][nb].cpu().numpy().astype(np.float64), ref[nb])
            per = np.abs(got[b][:nb].cpu().numpy().astype(np.float64) - ref[:nb]) / np.maximum(ref[nb], 1.0)
            measure(f"exact detector frame sums, per gated sample ({'gated' if gated else 'no gate'})", float(per.max()), bar)


# =============================================================================================== c. sessions, exact path
SESSIONS = [c for c in EXACT if c[3][1] in SESSION_NETS]


def _open(net, kind, S, msg, precision="f32"):
    from waveverify_amd.session import DetectSession, EmbedSession, LocateSession
    if kind == "generator":
        return EmbedSession(net, cu(msg), precision)
    return (LocateSession if kind == "locator" else DetectSession)(net, S, precision)


def _session_data(case, S, T):
    x = np.concatenate([W.clip_data(case, max(T, 1), s)[0] for s in range(S)])[:, :, :T]
    msg = np.concatenate([W.clip_data(case, max(T, 1), s)[1] for s in range(S)])
    return x, msg


def _run_schedule(sess, kind, xt, sizes, hop):
    """-> per push (seen, result), then flush's; checks each push's column count."""
    steps, seen, emitted = [], 0, 0
    for n in sizes:
        r = sess.push(xt[:, 0, seen: seen + n])
        seen += n
        want = seen // hop * hop - emitted
        if kind == "detector":
            assert r.samples_seen == seen // hop * hop
        else:
            assert r.shape == (xt.shape[0], 1, want), (n, r.shape, want)
        emitted += want
        steps.append((seen, want, r))
    return steps, sess.flush()


@pytest.mark.parametrize("case", SESSIONS, ids=_ids(SESSIONS))
def test_sessions_vs_float64(case):
    case, cfg, net, onet = _net(case[0])
    kind, hop, nb = cfg.kind, cfg.hop_length, cfg.head_bits
    for name, S, sizes in W.push_cases(cfg):
        T = sum(sizes)
        x, msg = _session_data(case, S, T)
        xt = cu(x)
        sess = _open(net, kind, S, msg)
        steps, last = _run_schedule(sess, kind, xt, sizes, hop)
        what = f"{case[0]} schedule {name}"
        if kind == "detector":
            prev = None
            for seen, want, st in steps:
                mlen = seen // hop * hop
                if want == 0 and prev is not None:
                    assert torch.equal(st.mean_prob, prev.mean_prob), what
                elif mlen:
                    ref = sigmoid64(W.oracle_forward(cfg, onet, x[:, :, :mlen])).mean(axis=2)
                    measure("exact DetectSession mean probability", rel_err(st.mean_prob, ref, 1.0), MEAN_BAR)
                else:
                    assert (st.mean_prob == 0).all()
                assert torch.equal(st.bits, (st.mean_prob >= 0.5).to(torch.int32))
                prev = st
            assert last.samples_seen == T
            if T % hop == 0 and prev is not None:                 # nothing left for flush(): the state stays
                assert torch.equal(last.mean_prob, prev.mean_prob), what
            if T:
                ref = sigmoid64(W.oracle_forward(cfg, onet, x)).mean(axis=2)
                measure("exact DetectSession mean probability", rel_err(last.mean_prob, ref, 1.0), MEAN_BAR)
            else:
                assert (last.mean_prob == 0).all() and last.mean_prob.shape == (S, nb)
        else:
            assert last.shape == (S, 1, T % hop), (what, last.shape)
            got = torch.cat([r for _, _, r in steps] + [last], dim=-1)
            assert got.shape == (S, 1, T)
            if T:
                ref = W.oracle_forward(cfg, onet, x, msg)
                measure(f"exact {'EmbedSession' if kind == 'generator' else 'LocateSession'}", rel_err(got, ref, float(np.abs(ref).max())),
                        GEN_BAR if kind == "generator" else LOGIT_BAR32)
        with pytest.raises(RuntimeError):
            sess.push(xt[:, 0, :1])
        # reset(): the next outputs are a fresh session's, bit for bit
        if T:
            sess.reset()
            fresh = _open(net, kind, S, msg)
            cut = min(T, 3 * hop + 1)
            again, anew = ([s_.push(xt[:, 0, :cut]), s_.flush()] for s_ in (sess, fresh))
            for a, b in zip(again, anew):
                if kind == "detector":
                    assert a.samples_seen == b.samples_seen and torch.equal(a.mean_prob, b.mean_prob) and torch.equal(a.bits, b.bits), what
                else:
                    assert torch.equal(a, b), what


# =============================================================================================== d. the f16 mode
from test_gpu_h16 import LOGIT_BAR as LOGIT_BAR16, WM_BAR, det_mean_bar  # noqa: E402

F16_WINDOWS = (("min", ("L+1", "edge+1")), ("min+hop", ("four-ragged",)))            # 2 and 3 / 4 windows per clip; the oracle takes ~0.2 s a clip
F16_PARAMS = [(c, w) for c in F16 for w in F16_WINDOWS]


def _oracle16(cfg, net, x, msg):
    """-> (whole-clip reference [C, T] float64, mean probabilities [nb] or None)."""
    from oracle import wv_oracle_h16 as O16
    if cfg.kind == "generator":
        return O16.embed(net, x, msg).double().numpy()[0], None
    lg = O16.detect_logits(net, x).double().numpy()[0]
    return lg, (O16.detect_mean_prob(net, x).double().numpy()[0] if cfg.kind == "detector" else None)


@pytest.mark.parametrize("case,wcase", F16_PARAMS, ids=[f"{c[0]}-{w[0]}" for c, w in F16_PARAMS])
def test_windowed_f16_vs_its_oracle(case, wcase):
    from oracle import wv_oracle_h16 as O16
    from waveverify_amd import window
    from waveverify_amd.window import halo
    case, cfg, net, onet = _net16(case[0])
    kind, hop, nb, H = cfg.kind, cfg.hop_length, cfg.head_bits, halo(cfg)
    wk, kinds = wcase
    win = H + hop if wk == "min" else H + 2 * hop
    by_kind = W.lengths_of(win, H, hop, 2)
    lengths = [by_kind[k] for k in kinds]
    assert all(2 <= len([w for g in window.plan([T], win, cfg) for w in g]) <= 4 for T in lengths)
    xs, msg = _clips(case, lengths)
    xt, mt = [cu(x[0, 0]) for x in xs], cu(msg)
    what = f"{case[0]} f16 window {win} lengths {lengths}"
    pick = lambda sel: (xt if sel is None else [xt[b] for b in sel])
    refs = [_oracle16(cfg, onet, x, msg[b: b + 1]) for b, x in enumerate(xs)]
    if kind == "generator":
        got = _grouping(lambda mw, sel: window.windowed_generator(net, pick(sel), mt if sel is None else mt[sel], window=win, precision="f16",
                                                                  max_windows=mw), len(xs), what)
        for b, y in enumerate(got):
            assert y.shape == (lengths[b],)
            measure("f16 generator (absolute)", rel_err(y, refs[b][0][0], 1.0), WM_BAR)
        return
    fwd = window.windowed_locator if kind == "locator" else window.windowed_detector
    got = _grouping(lambda mw, sel: fwd(net, pick(sel), window=win, precision="f16", max_windows=mw), len(xs), what)
    for b, y in enumerate(got):
        r = refs[b][0]
        measure(f"f16 {kind} logits", rel_err(y.view(r.shape), r, max(1.0, float(np.abs(r).max()))), LOGIT_BAR16)
    if kind == "detector":
        mp = _grouping(lambda mw, sel: list(window.windowed_detector_mean_prob(net, pick(sel), window=win, precision="f16", max_windows=mw)),
                       len(xs), what + " mean")
        for b, T in enumerate(lengths):
            measure(f"f16 detector mean probability / det_mean_bar(T) ({'head16' if O16.head16_gate(cfg) else 'f32 tail'})",
                    rel_err(mp[b], refs[b][1], 1.0) / det_mean_bar(T), 1.0)


F16_SESSIONS = [("h.generator", "aligned"), ("h.locator", "aligned"), ("h.detector", "aligned"), ("h.nbits36.detector", "aligned")]


@pytest.mark.parametrize("cid,sched", F16_SESSIONS, ids=[c for c, _ in F16_SESSIONS])
def test_sessions_f16_vs_their_oracle(cid, sched):
    """One stream over the schedule with a push beyond the history capacity.  The DetectSessions are compared after the first push that
    completes a frame, after the long push and after flush() (an oracle run of the default detector takes seconds); the states between
    are held to the column counts and to `unchanged when nothing completed`."""
    from oracle import wv_oracle_h16 as O16
    case, cfg, net, onet = _net16(cid)
    kind, hop = cfg.kind, cfg.hop_length
    name, S, sizes = next(s for s in W.push_cases(cfg) if s[0] == sched)
    T = sum(sizes)
    x, msg = _session_data(case, S, T)
    xt = cu(x)
    sess = _open(net, kind, S, msg, "f16")
    steps, last = _run_schedule(sess, kind, xt, sizes, hop)
    if kind == "detector":
        first = next(i for i, (_, want, _) in enumerate(steps) if want)
        longest = max(range(len(steps)), key=lambda i: sizes[i])
        prev = None
        for i, (seen, want, st) in enumerate(steps):
            mlen = seen // hop * hop
            if want == 0 and prev is not None:
                assert torch.equal(st.mean_prob, prev.mean_prob)
            if i in (first, longest):
                ref = O16.detect_mean_prob(onet, x[:, :, :mlen]).double().numpy()
                measure("f16 DetectSession mean probability / det_mean_bar(T)", rel_err(st.mean_prob, ref, 1.0) / det_mean_bar(mlen), 1.0)
            prev = st
        assert last.samples_seen == T and T % hop == 0 and torch.equal(last.mean_prob, prev.mean_prob)
        ref = O16.detect_mean_prob(onet, x).double().numpy()
        measure("f16 DetectSession mean probability / det_mean_bar(T)", rel_err(last.mean_prob, ref, 1.0) / det_mean_bar(T), 1.0)
    else:
        assert last.shape == (S, 1, T % hop)
        got = torch.cat([r for _, _, r in steps] + [last], dim=-1)
        if kind == "generator":
            measure("f16 EmbedSession (absolute)", rel_err(got, O16.embed(onet, x, msg).double().numpy(), 1.0), WM_BAR)
        else:
            ref = O16.detect_logits(onet, x).double().numpy()
            measure("f16 LocateSession logits", rel_err(got, ref, max(1.0, float(np.abs(ref).max()))), LOGIT_BAR16)
    with pytest.raises(RuntimeError):
        sess.push(xt[:, 0, :1])


@pytest.mark.parametrize("case", F16_REFUSED, ids=_ids(F16_REFUSED))
def test_windowed_f16_refuses_nets_without_a_plan(case):
    """The 16-channel nets have no f16 plan: the windowed routes and the sessions say so, as the whole-clip entry points do; none falls back."""
    from waveverify_amd import window
    from waveverify_amd.window import halo
    case, cfg, net, _ = _net16(case[0])
    hop, win = cfg.hop_length, halo(cfg) + cfg.hop_length
    x, msg = W.clip_data(case, win + hop + 1, 0)
    xt, mt = [cu(x[0, 0])], cu(msg)
    calls = {"generator": [lambda: window.windowed_generator(net, xt, mt, window=win, precision="f16")],
             "detector": [lambda: window.windowed_detector(net, xt, window=win, precision="f16"),
                          lambda: window.windowed_detector_mean_prob(net, xt, window=win, precision="f16"),
                          lambda: window.windowed_detector_frame_sums(net, xt, window=win, precision="f16")]}[cfg.kind]
    calls.append(lambda: _open(net, cfg.kind, 1, msg, "f16").push(cu(x[:, 0, :2 * hop])))
    for call in calls:
        with pytest.raises(RuntimeError, match="f16"):
            call()
    exact = window.windowed_generator(net, xt, mt, window=win) if cfg.kind == "generator" else window.windowed_detector(net, xt, window=win)
    assert torch.isfinite(exact[0]).all()


def test_print_the_worst_cases():
    """The last test of the file: the worst figure per kind over what ran before it (pytest -s)."""
    for what, err in sorted(WORST.items()):
        print(f"WORST {what}: {err:.2e}")
