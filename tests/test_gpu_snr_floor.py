"""The SNR floor of embedding on the MI355X (csrc/wv_snr_floor.hip, waveverify_amd/snr_floor.py, WaveVerify.set_snr_floor, session.EmbedBank /
native_bank.NativeEmbedBank.set_snr_floor); cases in tests/snr_floor_cases.py.

1. The kernel through the C ABI on guarded arenas (tests/guard.py, offsets 0 and 1): out, gains and gstate bit-equal to the twin for add 0
   and 1, the bad rows' targets untouched beside the good rows, inputs and guards unchanged, every refusal -1 with nothing written, a
   poisoned state under the fresh flag never read.
2. Routes, bit for bit: embed_batch, embed_clips (window 2 H), embed_spans_clips, embed_native_batch and embed_spans_native_batch equal the
   twin (or native.upsample_add of the twin's v with gain 1) applied to the residual the same route returns with add_input=False and the
   floor off; exact and f16; alone or in the mixed list; set_precision reaches it.
3. Routes against float64: the 16 kHz and span routes on x1 / x6 / x13 against the twin's formula in float64 on the whole-clip oracle
   residual, at test_gpu_span's GEN_BAR (5e-5 of the reference's largest magnitude).
4. Live: an EmbedBank under a floor on bank_cases schedules with span_cases.switch_plan, (a) bit-equal to the twin applied stream by stream
   to what a floor-less add_input=False bank returns, (b) within GEN_BAR of the float64 reference, (c) pass-through bit for bit and as many
   launches as the floor-less bank, (d) a reused slot never sees its predecessor's state, (e) NativeEmbedBank (48 kHz stereo and 8 kHz mono
   in one bank) is upsample_add of the shaped residual with gain 1.
5. With the floor None the outputs are those of a WaveVerify whose switch was never touched.

MEASURED on the MI355X (the `SNR FLOOR ...` lines of the test output), of the reference's largest magnitude against
a bar of 5e-5: embed_clips 1.2e-7 (x1), 1.5e-7 (x6), 2.1e-7 (x13); embed_spans_clips 1.0e-7, 8.3e-8, 9.2e-8; the live bank 1.2e-7 on both
schedules; everything else is bit equality."""
import functools

import numpy as np
import pytest
import torch

import bank_cases as BK
import snr_floor_cases as FC
import span_cases as SC
import window_cases as W
from guard import Guards
from waveverify_amd import native, window
from waveverify_amd import snr_floor as SF
from waveverify_amd.window import halo

pytestmark = pytest.mark.gpu

GEN_BAR = 5e-5                                                    # tests/test_gpu_span.py: of the reference's largest magnitude
DB = FC.ROUTE_DB
IDS = (0xBEEF, 0x1234, 7)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().contiguous().numpy().reshape(-1)


def bits(t):
    return (host(t) if isinstance(t, torch.Tensor) else np.ascontiguousarray(t).reshape(-1)).view(np.int32)


def _abi():
    from waveverify_amd import _lib
    return _lib.load(), _lib.stream()


shape_level = FC.shape_level


def twin_rows(xs, rs, L, s=1.0, add=True, db=DB):
    """The twin on whole rows -> ([out], [gains])."""
    rho, ramp = SF.rho_of(db), SF.floor_ramp(L)
    res = [SF.floor_row(host(x), host(r), s, rho, ramp, None, add) for x, r in zip(xs, rs)]
    return [o for o, _ in res], [g for _, g in res]


# =============================================================================================== 1. the kernel through the C ABI
def _run_kernel(lib, st, case, L, rho, add, offset, gstate_np):
    g = Guards(offset=offset)
    x, r = g.input(case["x"], "x"), g.input(case["r"], "r")
    desc, ramp = g.input(case["rows"], "desc", offset=0), g.input(SF.floor_ramp(L), "ramp")
    out, gains = g.output((case["n_out"],), name="out"), g.output((case["n_gains"],), name="gains")
    gstate = g.output((FC.N_STATE,), name="gstate")
    gstate.tflat.copy_(cu(gstate_np))
    rc = lib.wv_snr_floor(x.t.data_ptr(), x.t.numel(), r.t.data_ptr(), r.t.numel(), out.t.data_ptr(), case["n_out"], desc.t.data_ptr(),
                          len(case["rows"]), case["n_max"], gstate.t.data_ptr(), FC.N_STATE, gains.t.data_ptr(), case["n_gains"], ramp.t.data_ptr(),
                          L, rho, add, st)
    assert rc == 0, lib.wv_last_error()
    torch.cuda.synchronize()
    for a in (x, r, desc, ramp):
        a.check()                                                      # inputs and their guards unchanged
    return out, gains, gstate


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("L", FC.FRAMES)
def test_kernel_vs_twin(L, offset):
    lib, st = _abi()
    case, rho = FC.kernel_case(L), SF.rho_of(DB)
    for add in (0, 1):
        out, gains, gstate = _run_kernel(lib, st, case, L, rho, add, offset, case["gstate"])
        want, want_state, want_gains, kept, gkept = FC.twin(case, L, rho, bool(add))
        out.check(expect_unwritten=torch.from_numpy(~kept))            # the bad rows' targets untouched, every served sample written
        gains.check(expect_unwritten=torch.from_numpy(~gkept))
        assert not gstate.guard_report()
        assert np.array_equal(bits(out.t)[kept], want.view(np.int32)[kept]), add
        assert np.array_equal(bits(gains.t)[gkept], want_gains.view(np.int32)[gkept]), add
        assert np.array_equal(bits(gstate.t), want_state.view(np.int32)), add
        # another value where the poison was: a state under the fresh flag is not read, the result is unchanged
        other = case["gstate"].copy()
        other[np.isnan(other)] = 0.5
        out2, gains2, gstate2 = _run_kernel(lib, st, case, L, rho, add, offset, other)
        assert np.array_equal(bits(out2.t), bits(out.t)) and np.array_equal(bits(gains2.t), bits(gains.t))
        assert np.array_equal(bits(gstate2.t), bits(gstate.t))


def test_kernel_refusals_write_nothing():
    lib, st = _abi()
    g = Guards()
    x, r = g.input(np.ones(64, np.float32), "x"), g.input(np.ones(64, np.float32), "r")
    desc = g.input(np.array([[0, 0, 0, 64, SF.strength_bits(1.0), 0, 1, 0]], np.int64), "desc", offset=0)
    ramp = g.input(SF.floor_ramp(4), "ramp")
    out, gains, gstate = g.output((64,), name="out"), g.output((16,), name="gains"), g.output((2,), name="gstate")
    ok = dict(x=x.t.data_ptr(), n_x=64, r=r.t.data_ptr(), n_r=64, out=out.t.data_ptr(), n_out=64, desc=desc.t.data_ptr(), A=1, n_max=64,
              gstate=gstate.t.data_ptr(), n_state=2, gains=gains.t.data_ptr(), n_gains=16, ramp=ramp.t.data_ptr(), L=4, rho=0.01, add=1)
    call = lambda a: lib.wv_snr_floor(a["x"], a["n_x"], a["r"], a["n_r"], a["out"], a["n_out"], a["desc"], a["A"], a["n_max"], a["gstate"],   # noqa: E731
                                      a["n_state"], a["gains"], a["n_gains"], a["ramp"], a["L"], a["rho"], a["add"], st)
    for why, kw in (("null x", dict(x=None)), ("null r", dict(r=None)), ("null out", dict(out=None)), ("null desc", dict(desc=None)),
                    ("null ramp", dict(ramp=None)), ("n_x < 0", dict(n_x=-1)), ("n_r < 0", dict(n_r=-1)), ("n_out < 0", dict(n_out=-1)),
                    ("n_state < 0", dict(n_state=-1)), ("states without gstate", dict(gstate=None)), ("n_gains < 0", dict(n_gains=-1)),
                    ("gains without their array", dict(gains=None)), ("L < 1", dict(L=0)), ("L beyond the limit", dict(L=SF.MAX_FRAME + 1)),
                    ("rho = 0", dict(rho=0.0)), ("rho < 0", dict(rho=-1.0)), ("rho = nan", dict(rho=float("nan"))),
                    ("rho = inf", dict(rho=float("inf"))), ("A < 0", dict(A=-1)), ("A > 65535", dict(A=65536)), ("n_max < 0", dict(n_max=-1)),
                    ("n_max beyond 2^31 - 1", dict(n_max=1 << 31)), ("add = 2", dict(add=2)), ("out is x", dict(out=x.t.data_ptr())),
                    ("out is r", dict(out=r.t.data_ptr())), ("out overlaps x", dict(out=x.t.data_ptr() + 128))):
        assert call({**ok, **kw}) == -1, why
        assert lib.wv_last_error().decode().startswith("wv_snr_floor"), why
    assert call({**ok, "A": 0}) == 0 and call({**ok, "n_max": 0}) == 0    # success without a launch
    torch.cuda.synchronize()
    for a in (x, r, desc, ramp):
        a.check()
    out.check(expect_unwritten=torch.ones(64, dtype=torch.bool))
    gains.check(expect_unwritten=torch.ones(16, dtype=torch.bool))
    gstate.check(expect_unwritten=torch.ones(2, dtype=torch.bool))


# =============================================================================================== 2. routes, bit for bit
def _new_wv(cid):
    """-> (WaveVerify whose generator is the small net `cid`, in that net's precision mode; cfg; the float64 oracle net or None)."""
    from waveverify_amd import WaveVerify
    from waveverify_amd.init import random_state_dict
    case = SC.net_case(cid)
    if case[1] == "f32":
        cfg, sd, onet = W.oracle_net(case)
    else:
        cfg, seed = W.net_config(case)
        sd, onet = random_state_dict(cfg, seed), None
    w = WaveVerify.__new__(WaveVerify)
    w.device = torch.device("cuda", torch.cuda.current_device())
    w._build({"generator": sd}, {"generator": cfg})
    w.sample_rate, w.watermark_bits = WaveVerify.DEFAULT_SAMPLE_RATE, cfg.msg_dimension
    w.set_precision(case[1])
    return w, cfg, onet


_wv = functools.lru_cache(maxsize=None)(_new_wv)


@functools.lru_cache(maxsize=None)
def _clips(cid):
    """-> (L, lengths, spans, the clips of span_cases under a block envelope)."""
    cfg = W.net_config(SC.net_case(cid))[0]
    L, lengths, spans, _ = SC.cases(cid)
    xs = [shape_level(x, 5 * cfg.hop_length, (cid, b)) for b, x in enumerate(SC.clip_data(cid, lengths))]
    return L, lengths, spans, xs


def _same(got, want, what):
    assert len(got) == len(want)
    for b, (a, w) in enumerate(zip(got, want)):
        assert np.array_equal(bits(a), w.view(np.int32)), (what, b)


@pytest.mark.parametrize("cid", FC.EXACT_IDS + (FC.F16_ID,))
def test_16k_routes_are_the_twin_on_the_routes_own_residual(cid):
    wv, cfg, _ = _wv(cid)
    gen, prec, hop = wv.model.generator, wv.generator_precision, cfg.hop_length
    L, lengths, spans, xs = _clips(cid)
    clips = [cu(x) for x in xs]
    ws = 2 * halo(cfg) / 16000
    Wn = wv._window_samples(ws)
    idlist = [IDS[b % 3] for b in range(len(xs))]
    xb = cu(FC.batch_clips(cid))[:, None]
    T = xb.shape[-1]
    msg2 = wv._messages([IDS[0], IDS[1]])
    sp = [[(s, e, IDS[m]) for s, e, m in c] for c in spans]
    msgs, rows, _ = wv._span_messages(sp)
    # the residuals with the floor off, as the routes themselves return them
    assert wv.snr_floor_db is None
    r_batch = gen.generator(xb, msg2, add_input=False, precision=prec)
    r_clips = window.windowed_generator(gen, clips, wv._messages(idlist), Wn, prec, add_input=False)
    r_spans = window.span_generator(gen, clips, msgs, rows, Wn, prec, fade_samples=7, gain=SC.GAIN, add_input=False)
    plain_batch, plain_clips = wv.embed_batch(xb, msg2), wv.embed_clips(clips, idlist, ws)
    wv.set_snr_floor(DB)
    try:
        got = wv.embed_batch(xb, msg2)
        assert got.shape == xb.shape
        want, g_want = twin_rows(xb[:, 0], r_batch[:, 0], hop)
        _same(got[:, 0], want, "embed_batch")
        _, gains = SF.apply(xb, r_batch, DB, frame=hop, return_gains=True)         # the QC trace is the twin's gains
        assert gains.shape == (2, -(-T // hop)) and np.array_equal(bits(gains), np.concatenate(g_want).view(np.int32))
        g_all = np.concatenate(g_want)
        assert (g_all < 1).any() and (g_all == 0).any(), "capped and silent frames"
        assert (g_all == 1).any() or prec == "f16", "uncapped frames (tests/test_snr_floor_cpu.py holds the exact nets' inputs to it)"

        mixed = wv.embed_clips(clips, idlist, ws)
        _same(mixed, twin_rows(clips, r_clips, hop)[0], "embed_clips")
        for b in (1, 3):
            assert torch.equal(wv.embed_clips([clips[b]], [idlist[b]], ws)[0], mixed[b]), b    # alone or in the mixed list, the same bits
        as_batch = wv.embed_clips(xb, [IDS[0], IDS[1]], ws)
        assert as_batch.shape == xb.shape                                              # [B,1,T] in, [B,1,T] out

        spanned = wv.embed_spans_clips(clips, sp, ws, fade_samples=7, strength=SC.GAIN)
        _same(spanned, twin_rows(clips, r_spans, hop)[0], "embed_spans_clips")
        for b, x in enumerate(xs):
            off = SC.outside(len(x), spans[b])
            assert np.array_equal(bits(spanned[b])[off], x.view(np.int32)[off]), b       # outside every span: the input's bits
        # alone or in the mixed list, the same bits (at pad_limit 1, where test_gpu_span holds the floor-less route to the same)
        one = dict(fade_samples=7, strength=SC.GAIN, pad_limit=1.0)
        assert torch.equal(wv.embed_spans_clips([clips[2]], [sp[2]], ws, **one)[0], wv.embed_spans_clips(clips, sp, ws, **one)[2])
        silent = [np.flatnonzero(~x.astype(bool)) for x in xs]
        assert sum(len(z) for z in silent) > 0
        for b, z in enumerate(silent):                                                 # silence stays silent through the real route
            assert np.array_equal(bits(mixed[b])[z], xs[b].view(np.int32)[z])
        if prec == "f16":                                                              # set_precision reaches the floored route
            wv.set_precision("f32")
            assert not torch.equal(wv.embed_batch(xb, msg2), got)
    finally:
        wv.set_snr_floor(None)
        wv.set_precision(prec)
    # 5. with the floor None again: the bits of a WaveVerify whose switch was never touched
    fresh, _, _ = _new_wv(cid)
    assert torch.equal(wv.embed_batch(xb, msg2), plain_batch) and torch.equal(fresh.embed_batch(xb, msg2), plain_batch)
    for a, b_, c in zip(wv.embed_clips(clips, idlist, ws), plain_clips, fresh.embed_clips(clips, idlist, ws)):
        assert torch.equal(a, b_) and torch.equal(c, b_)


NATIVE_SPANS = [(100, 900, 0xBEEF), (900, 1500, 0x1234), (3000, 4700, 0xBEEF)]


@pytest.mark.parametrize("sr,Cn", [(48000, 2), (44100, 1)])
@pytest.mark.parametrize("cid", ["x13.generator", FC.F16_ID])
def test_native_routes_are_upsample_add_of_the_twins_residual(cid, sr, Cn):
    import native_cases as NC
    wv, cfg, _ = _wv(cid)
    gen, prec, hop = wv.model.generator, wv.generator_precision, cfg.hop_length
    Tn = int(0.3 * sr) + 1
    audio = cu(shape_level((NC.inputs(sr, Cn, Tn)[0][:1] * np.float32(0.2)).astype(np.float32), sr // 100, (cid, sr)))      # [1, C, Tn]
    x16 = wv.to_model_rate(audio, sr)
    assert x16.shape[-1] >= 4700
    msg = wv._messages(IDS[0])
    ws = 2 * halo(cfg) / 16000
    Wn = wv._window_samples(ws)
    msgs, rows, _ = wv._span_messages([NATIVE_SPANS])
    d_whole = gen.generator(x16, msg, add_input=False, precision=prec)
    d_win = window.windowed_generator(gen, x16, msg, Wn, prec, add_input=False)
    d_span = window.span_generator(gen, x16, msgs, rows, wv._window_samples(30.0), prec, fade_samples=7, gain=0.5, add_input=False)
    plain = wv.embed_native_batch(audio, sr, msg, 0.5)
    wv.set_snr_floor(DB)
    try:
        for d, kw in ((d_whole, {}), (d_win, dict(window_seconds=ws))):
            v, g = twin_rows(x16[:, 0], d[:, 0], hop, s=0.5, add=False)                # the strength moves into the floor
            want = native.upsample_add(audio, cu(v[0])[None, None], sr, 1.0)
            got = wv.embed_native_batch(audio, sr, msg, 0.5, **kw)
            assert got.shape == audio.shape and torch.equal(got, want), kw
            assert (g[0] < 0.5).any()
        assert not torch.equal(got, plain)
        v, _ = twin_rows(x16[:, 0], d_span[:, 0], hop, s=1.0, add=False)               # the strength is inside the masked residual
        want = native.upsample_add(audio, cu(v[0])[None, None], sr, 1.0)
        assert torch.equal(wv.embed_spans_native_batch(audio, sr, [NATIVE_SPANS], 0.5, 7), want)
    finally:
        wv.set_snr_floor(None)
    assert torch.equal(wv.embed_native_batch(audio, sr, msg, 0.5), plain)


# =============================================================================================== 3. routes against float64
@pytest.mark.parametrize("cid", FC.EXACT_IDS)
def test_16k_routes_vs_float64_on_the_whole_clip(cid):
    wv, cfg, onet = _wv(cid)
    hop = cfg.hop_length
    L, lengths, spans, xs = _clips(cid)
    clips = [cu(x) for x in xs]
    ws = 2 * halo(cfg) / 16000
    idlist = [IDS[b % 3] for b in range(len(xs))]
    m_clips = host(wv._messages(idlist)).reshape(len(xs), -1)
    sp = [[(s, e, IDS[m]) for s, e, m in c] for c in spans]
    msgs, rows, _ = wv._span_messages(sp)
    m_span = host(msgs).reshape(msgs.shape[0], -1)
    rho, ramp7 = SF.rho_of(DB), window.span_ramp(7)
    oracle = lambda x, m: W.oracle_forward(cfg, onet, x[None, None], m[None], add_input=False)[0, 0]      # noqa: E731
    wv.set_snr_floor(DB)
    try:
        got_clips = wv.embed_clips(clips, idlist, ws)
        got_spans = wv.embed_spans_clips(clips, sp, ws, fade_samples=7, strength=SC.GAIN)
    finally:
        wv.set_snr_floor(None)
    worst = {"clips": 0.0, "spans": 0.0}
    for b, x in enumerate(xs):
        ref, _ = FC.reference64(x, oracle(x, m_clips[b]), rho, hop)
        deltas = {m: oracle(x, m_span[m]) for m in {m for _, _, m in rows[b]}}
        masked = SC.reference(x, deltas, rows[b], ramp7, SC.GAIN, add_input=False)
        ref_s, _ = FC.reference64(x, masked, rho, hop)
        for what, got, want in (("clips", got_clips[b], ref), ("spans", got_spans[b], ref_s)):
            err = float(np.abs(host(got) - want).max()) / float(np.abs(want).max())
            worst[what] = max(worst[what], err)
            assert err <= GEN_BAR, (what, cid, b, err)
    print(f"SNR FLOOR exact {cid}: worst error embed_clips {worst['clips']:.2e}, embed_spans_clips {worst['spans']:.2e} (bar {GEN_BAR:.1e})")


# =============================================================================================== 4. live
@functools.lru_cache(maxsize=None)
def _live(precision):
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    cid = "x13.generator" if precision == "f32" else FC.F16_ID
    case = SC.net_case(cid)
    if precision == "f32":
        cfg, sd, onet = W.oracle_net(case)
    else:
        cfg, seed = W.net_config(case)
        sd, onet = random_state_dict(cfg, seed), None
    return cid, case, cfg, HipNet(cfg, sd), onet


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("sched", ["mixed", "equal"])
def test_embed_bank_under_a_floor(sched, precision):
    from waveverify_amd.session import EmbedBank
    cid, case, cfg, net, onet = _live(precision)
    hop = cfg.hop_length
    msgs = SC.messages(cid)
    steps = dict(BK.schedules(cfg))[sched]
    xs = {n: shape_level(x, 3 * hop, (cid, n)) for n, (x, _) in BK.stream_data(case, steps).items()}
    plan = SC.switch_plan(steps)
    rho, ramp = SF.rho_of(DB), SF.floor_ramp(hop)
    state_msg = lambda st: None if st is None else msgs[st]             # noqa: E731

    def play(bank, through=True):
        """through=False: a bank that has no pass-through keeps its last id over the None stretches (its residual there is not used)."""
        def set_state(slot, st):
            if st is None and not through:
                return bank.samples_seen(slot)
            return bank.set_message(slot, state_msg(st))
        return SC.run_switching(bank, steps, xs, plan, lambda st: bank.open(state_msg(0 if st is None and not through else st)), set_state, take=cu)

    floored = EmbedBank(net, BK.CAPACITY, precision, 1.5)
    floored.set_snr_floor(DB)
    out, marks, launches, only = play(floored)

    class ResidualBank(EmbedBank):
        """No floor, the generator's residual alone (add_input=False), but with the pass-through of an add_input=True bank, so that every
        launch has the rows the floored bank's has: a row's bits depend on the batch it runs in (its padding), by a few ulp."""

        def _net(self, win, tabs, ln):
            return self.net.generator(win, tabs["msg"][ln.a_lo:ln.a_lo + ln.A], add_input=False, precision=self.precision)
    out_r, marks_r, _, _ = play(ResidualBank(net, BK.CAPACITY, precision, 1.5))
    plain = EmbedBank(net, BK.CAPACITY, precision, 1.5)
    _, _, launches_p, _ = play(plain)
    assert launches == launches_p and floored.stats["launches"] == plain.stats["launches"]      # (c) the floor adds no generator launch
    assert all(n == 0 for n, o in zip(launches, only) if o)
    worst, lowered = 0.0, 0
    for n, x in xs.items():
        assert len(out[n]) == len(out_r[n])
        if not x.size:
            continue
        sp = SC.spans_of(marks[n], x.size)
        inside = ~SC.outside(x.size, sp)
        pos, g_prev = 0, None
        for i, (pf, pr) in enumerate(zip(out[n], out_r[n])):
            pf, pr = host(pf), host(pr)
            assert pf.shape == pr.shape
            if not pf.size:
                continue
            a, b = pos, pos + pf.size
            pos = b
            assert a % hop == 0 and (inside[a:b].all() or not inside[a:b].any())
            if not inside[a]:
                assert np.array_equal(pf.view(np.int32), x[a:b].view(np.int32)), (n, i)           # (c) pass-through: the input's bits
                g_prev = None                                              # leaving pass-through, the state is fresh
                continue
            want, g = SF.floor_row(x[a:b], pr, 1.0, rho, ramp, g_prev)
            assert np.array_equal(pf.view(np.int32), want.view(np.int32)), (sched, precision, n, i)     # (a)
            g_prev = g[-1]
            lowered += int((g < 1).sum())
        assert pos == x.size
        if onet is not None:                                               # (b) the float64 reference of the file route
            got = np.concatenate([host(p) for p in out[n]])
            deltas = {m: W.oracle_forward(cfg, onet, x[None, None], msgs[m:m + 1], add_input=False)[0, 0] for m in {m for _, _, m in sp}}
            ref, _ = FC.reference64(x, SC.reference(x, deltas, sp, add_input=False), rho, hop)
            err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
            worst = max(worst, err)
            assert err <= GEN_BAR, (sched, n, err)
    assert lowered > 0, "the floor turned some frame down"
    if onet is not None:
        print(f"SNR FLOOR live {sched}: worst error {worst:.2e} (bar {GEN_BAR:.1e})")


def test_a_reused_slot_never_sees_its_predecessors_state_and_the_public_route():
    from waveverify_amd import native_bank as NB
    from waveverify_amd.session import EmbedBank
    wv, cfg, _ = _wv("x13.generator")
    hop = cfg.hop_length
    rho, ramp = SF.rho_of(DB), SF.floor_ramp(hop)
    wv.set_snr_floor(DB)
    try:
        bank = wv.open_embed_bank(capacity=2)
        native_b = wv.open_embed_bank(capacity=2, rates=(48000, 8000))
        with pytest.raises(ValueError, match="open_embed_bank"):
            wv.open_embed_session([1])
    finally:
        wv.set_snr_floor(None)
    assert type(bank) is EmbedBank and bank.snr_floor_db == DB and isinstance(native_b, NB.NativeEmbedBank) and native_b.inner.snr_floor_db == DB
    assert wv.open_embed_bank(capacity=2).snr_floor_db is None
    with pytest.raises(ValueError):
        native_b.open(IDS[0], sample_rate=8000, strength=float("nan"))
    x = shape_level(SC.clip_data("x13.generator", (20 * hop + 5,))[0], 3 * hop, "reuse")
    resid = EmbedBank(wv.model.generator, 2, "f32", 1.5, bank._messages, add_input=False)

    def whole(b):
        s = b.open(IDS[0])
        return s, np.concatenate([host(b.push({s: cu(x[:7 * hop + 3])})[s]), host(b.push({s: cu(x[7 * hop + 3:])})[s]), host(b.close(s))])
    s0, first = whole(bank)
    _, r = whole(resid)
    want, g = SF.floor_row(x, r, 1.0, rho, ramp)
    assert np.array_equal(first.view(np.int32), want.view(np.int32)) and (g < 1).any()
    bank._gstate.fill_(float("nan"))                                       # whatever the slot's last stream left
    s1, second = whole(bank)
    assert s1 == s0 and np.array_equal(second.view(np.int32), first.view(np.int32))
    with pytest.raises(RuntimeError, match="first open"):
        bank.set_snr_floor(None)


def test_native_embed_bank_is_up_add_of_the_shaped_residual():
    """48 kHz stereo and 8 kHz mono in one bank under a floor, each with its own strength: the inner bank's residual is the twin's v on what
    a floor-less add_input=False bank returns for the same 16 kHz pieces, and every stream's output is native.upsample_add of it with gain 1."""
    import test_gpu_native_bank as TNB
    from waveverify_amd import native_bank as NB
    from waveverify_amd.session import EmbedBank
    wv, cfg, _ = _wv("x6.generator")
    gen, hop = wv.model.generator, cfg.hop_length
    rho, ramp = SF.rho_of(DB), SF.floor_ramp(hop)
    who = {"A": (48000, 2), "B": (8000, 1)}
    gains = {"A": 0.75, "B": 1.0}
    steps = [("open", "A"), ("open", "B")]
    for k in range(14):                                                    # 10 ms packets; B sits every third tick out
        steps.append(("push", {"A": 480, "B": 80} if k % 3 else {"A": 480}))
    steps += [("close", "A"), ("close", "B")]
    T = BK.stream_lengths(steps)
    xs = {n: cu(shape_level(np.random.default_rng(W.seed_of("snr floor native bank", n)).standard_normal((who[n][1], T[n])).astype(np.float32) * 0.1,
                            who[n][0] // 100, n)) for n in who}

    class Bank(TNB.RecordingEmbedBank):
        def open(self, name, **kw):
            return super().open(TNB.message(gen, name), strength=gains[name], **kw)
    bank = Bank(gen, (48000, 8000), 2, 2, "f32")
    bank.set_snr_floor(DB)
    out, slot = TNB.NBC.run(bank, steps, xs, who, open_args=lambda n: (n,))
    ref = TNB.play_16k(EmbedBank(gen, 2, "f32", 1.5, None, add_input=False), steps, xs, who, lambda n: (TNB.message(gen, n),),
                       lambda a, b: torch.cat([a, b]))
    lowered = 0
    for n, x in xs.items():
        x16 = host(native.downmix_resample(x[None], who[n][0])[0, 0])
        shaped = bank.residuals[slot[n]]
        assert len(shaped) == len(ref[n])
        pos, g_prev = 0, None
        for i, (a, b) in enumerate(zip(shaped, ref[n])):
            a, b = host(a), host(b) if b is not None else np.zeros(0, np.float32)
            assert a.shape == b.shape
            if not a.size:
                continue
            want, g = SF.floor_row(x16[pos:pos + a.size], b, gains[n], rho, ramp, g_prev, add=False)
            assert pos % hop == 0 and np.array_equal(a.view(np.int32), want.view(np.int32)), (n, i)
            pos, g_prev = pos + a.size, g[-1]
            lowered += int((g < gains[n]).sum())
        assert pos == x16.size
        y = torch.cat([r for _, _, r in out[n]], dim=1)
        assert y.shape == x.shape
        assert torch.equal(y, native.upsample_add(x[None], torch.cat(shaped)[None], who[n][0], 1.0)[0]), n
    assert lowered > 0
