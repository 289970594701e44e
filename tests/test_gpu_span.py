"""Span embedding on the MI355X (waveverify_amd/window.py plan_spans / span_generator, csrc/wv_window.hip wv_span_gather / wv_span_scatter_add,
WaveVerify.embed_spans*, session.EmbedBank.set_message); cases in tests/span_cases.py.

1. The two kernels through the C ABI on guarded arenas (tests/guard.py), every buffer on a 256-byte boundary and one element past it:
   bit-equal to their numpy twins, good rows beside every kind of bad row with the bad rows' targets untouched, every refusal -1 and nothing
   written.
2. The 16 kHz route on three exact small nets and, in the f16 mode, on one sweep configuration: inside the spans against x + w * delta of
   the FLOAT64 ORACLE (oracle/wv_oracle_h16 for f16) ON THE WHOLE CLIP at the window fuzz's bars (5e-5 of the reference's largest magnitude;
   test_gpu_h16's WM_BAR absolute), outside them bit-equal to the input; alone or in the mixed list, the same bits.
3. The native-rate route and the file API: bit-equal to native.upsample_add of the masked 16 kHz residual.
4. Live: EmbedBank with set_message switches against the float64 oracle's span embedding of each stream.

MEASURED on the MI355X (the `SPAN ...` lines of the test output): exact route 1.6e-7 of the reference's largest
magnitude (bar 5e-5), f16 route 4.7e-5 absolute (bar 1e-4), live route 2.6e-7 (bar 5e-5); everything else is bit equality."""
import functools

import numpy as np
import pytest
import torch

import bank_cases as BK
import span_cases as SC
import window_cases as W
from guard import Guards
from waveverify_amd import window

pytestmark = pytest.mark.gpu

GEN_BAR = 5e-5                                                    # tests/test_gpu_window_fuzz.py: of the reference's largest magnitude
from test_gpu_h16 import WM_BAR  # noqa: E402


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _abi():
    from waveverify_amd import _lib
    return _lib.load(), _lib.stream()


# =============================================================================================== 1. the kernels through the C ABI
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("Lmax", SC.KERNEL_L)
def test_span_gather_vs_twin(Lmax, offset):
    lib, st = _abi()
    n_src, rows, bad = SC.gather_case(Lmax)
    A = len(rows)
    src_np = np.random.default_rng(W.seed_of("span gather", Lmax)).standard_normal(n_src).astype(np.float32)
    g = Guards(offset=offset)
    src, desc = g.input(src_np, "src"), g.input(np.array(rows, np.int64), "desc", offset=0)
    dst = g.output((A, 1, Lmax), name="dst")
    assert lib.wv_span_gather(src.t.data_ptr(), n_src, desc.t.data_ptr(), dst.t.data_ptr(), A, Lmax, st) == 0
    torch.cuda.synchronize()
    skipped = torch.zeros((A, 1, Lmax), dtype=torch.bool)
    skipped[bad] = True
    for a in (src, desc):
        a.check()
    dst.check(expect_unwritten=skipped)                                # the bad rows' targets untouched, every other element written
    want = window.numpy_span_gather(src_np, rows, A, Lmax)
    good = [r for r in range(A) if r not in bad]
    assert np.array_equal(bits(dst.t)[good], want.view(np.int32)[good])


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("F", SC.KERNEL_F)
@pytest.mark.parametrize("Lmax", SC.KERNEL_L)
def test_span_scatter_add_vs_twin(Lmax, F, offset):
    lib, st = _abi()
    n_out, rows, bad = SC.scatter_case(Lmax, F)
    A = len(rows)
    Fn = Lmax + 3 if F == "long" else F
    ramp_np = window.span_ramp(Fn)
    rng = np.random.default_rng(W.seed_of("span scatter", Lmax, F))
    y_np = rng.standard_normal((A, 1, Lmax)).astype(np.float32)
    x_np = rng.standard_normal(n_out).astype(np.float32)
    for xin in ("null", "separate", "out"):
        g = Guards(offset=offset)
        y, desc = g.input(y_np, "y"), g.input(np.array(rows, np.int64), "desc", offset=0)
        ramp = g.input(ramp_np, "ramp") if Fn else None
        x = g.input(x_np, "x") if xin == "separate" else None
        out = g.output((n_out,), name="out")
        if xin == "out":
            out.tflat.copy_(cu(x_np))
        xp = {"null": None, "separate": x.t.data_ptr() if x else None, "out": out.t.data_ptr()}[xin]
        rc = lib.wv_span_scatter_add(y.t.data_ptr(), xp, desc.t.data_ptr(), ramp.t.data_ptr() if ramp else None, Fn, SC.GAIN, out.t.data_ptr(),
                                     n_out, A, Lmax, st)
        assert rc == 0
        torch.cuda.synchronize()
        for a in g.arenas[:-1]:
            a.check()                                                  # inputs and their guards unchanged
        want = x_np.copy() if xin == "out" else np.zeros(n_out, np.float32)
        window.numpy_span_scatter_add(y_np, None if xin == "null" else x_np, rows, ramp_np, SC.GAIN, want)
        kept = np.zeros(n_out, bool)
        for r, (o, lo, hi, _, _) in enumerate(rows):
            if r not in bad:
                kept[o + lo:o + hi] = True
        if xin == "out":
            assert not out.guard_report()
            assert np.array_equal(bits(out.t), want.view(np.int32)), xin        # outside the keep ranges still x, bit for bit
        else:
            out.check(expect_unwritten=torch.from_numpy(~kept))        # nothing outside the served rows' keep ranges is written
            assert np.array_equal(bits(out.t)[kept], want.view(np.int32)[kept]), xin


def test_span_kernel_refusals_write_nothing():
    lib, st = _abi()
    g = Guards()
    src, y = g.input(np.ones(64, np.float32), "src"), g.input(np.ones((2, 1, 16), np.float32), "y")
    gd, sd = g.input(np.array([[0, 16], [16, 16]], np.int64), "gdesc"), g.input(np.array([[0, 0, 16, 0, 16], [16, 0, 16, 0, 16]], np.int64), "sdesc")
    ramp = g.input(window.span_ramp(4), "ramp")
    dst, out = g.output((2, 1, 16), name="dst"), g.output((64,), name="out")
    ga = dict(src=src.t.data_ptr(), n_src=64, desc=gd.t.data_ptr(), dst=dst.t.data_ptr(), A=2, Lmax=16)
    call = lambda a: lib.wv_span_gather(a["src"], a["n_src"], a["desc"], a["dst"], a["A"], a["Lmax"], st)
    for why, kw in (("null desc", dict(desc=None)), ("null dst", dict(dst=None)), ("samples without src", dict(src=None)), ("n_src < 0", dict(n_src=-1)),
                    ("A < 0", dict(A=-1)), ("A > 65535", dict(A=65536)), ("Lmax < 1", dict(Lmax=0))):
        assert call({**ga, **kw}) == -1, why
        assert lib.wv_last_error().decode().startswith("wv_span_gather"), why
    sa = dict(y=y.t.data_ptr(), x=None, desc=sd.t.data_ptr(), ramp=ramp.t.data_ptr(), F=4, gain=1.0, out=out.t.data_ptr(), n_out=64, A=2, Lmax=16)
    call = lambda a: lib.wv_span_scatter_add(a["y"], a["x"], a["desc"], a["ramp"], a["F"], a["gain"], a["out"], a["n_out"], a["A"], a["Lmax"], st)
    for why, kw in (("null y", dict(y=None)), ("null desc", dict(desc=None)), ("null out", dict(out=None)), ("n_out < 1", dict(n_out=0)),
                    ("F < 0", dict(F=-1)), ("a fade without ramp", dict(ramp=None)), ("gain not a number", dict(gain=float("nan"))),
                    ("A < 0", dict(A=-1)), ("A > 65535", dict(A=65536)), ("Lmax < 1", dict(Lmax=0))):
        assert call({**sa, **kw}) == -1, why
        assert lib.wv_last_error().decode().startswith("wv_span_scatter_add"), why
    assert lib.wv_span_gather(ga["src"], 64, ga["desc"], ga["dst"], 0, 16, st) == 0          # A == 0: success, no launch
    assert call({**sa, "A": 0}) == 0
    torch.cuda.synchronize()
    everything = torch.ones(64, dtype=torch.bool)
    for a in (src, y, gd, sd, ramp):
        a.check()
    dst.check(expect_unwritten=everything[:32].view(2, 1, 16))
    out.check(expect_unwritten=everything)


# =============================================================================================== 2. the 16 kHz route
@functools.lru_cache(maxsize=None)
def _exact(cid):
    """-> (cfg, HipNet, L, lengths, spans, xs, msgs, per clip {message row: the float64 oracle's whole-clip residual}), built once."""
    from waveverify_amd.nets import HipNet
    cfg, sd, onet = W.oracle_net(SC.net_case(cid))
    L, lengths, spans, _ = SC.cases(cid)
    xs, msgs = SC.clip_data(cid, lengths), SC.messages(cid)
    deltas = [{m: W.oracle_forward(cfg, onet, x[None, None], msgs[m:m + 1], add_input=False)[0, 0] for m in {m for _, _, m in sp}}
              for x, sp in zip(xs, spans)]
    return cfg, HipNet(cfg, sd), L, lengths, spans, xs, msgs, deltas


def _check_route(got, xs, spans, deltas, fade, gain, bar, mag_of, what):
    ramp, worst = window.span_ramp(fade), 0.0
    for b, (y, x, sp) in enumerate(zip(got, xs, spans)):
        y = y.cpu().numpy().reshape(-1)
        assert y.shape == x.shape and np.isfinite(y).all()
        off = SC.outside(len(x), sp)
        assert np.array_equal(y[off].view(np.int32), x[off].view(np.int32)), (what, b)          # outside the spans: the input's bits
        ref = SC.reference(x, deltas[b], sp, ramp, gain)
        err = float(np.abs(y - ref).max()) / mag_of(ref)
        worst = max(worst, err)
        assert err <= bar, (what, b, err, bar)
        for s, e, _ in sp:
            assert not np.array_equal(y[s:e], x[s:e])                                         # and a span was written
    print(f"SPAN {what}: worst error {worst:.2e} (bar {bar:.1e})")


@pytest.mark.parametrize("fade", SC.FADES)
@pytest.mark.parametrize("pad", SC.PAD_LIMITS)
@pytest.mark.parametrize("cid", SC.EXACT_IDS)
def test_span_route_vs_float64_whole_clip(cid, pad, fade):
    cfg, net, L, lengths, spans, xs, msgs, deltas = _exact(cid)
    gain = SC.GAIN if fade else 1.0
    got = window.span_generator(net, [cu(x) for x in xs], cu(msgs), spans, L, "f32", pad, fade_samples=fade, gain=gain)
    assert bits(got[3]).tobytes() == xs[3].view(np.int32).tobytes()                          # the span-less clip
    _check_route(got, xs, spans, deltas, fade, gain, GEN_BAR, lambda ref: float(np.abs(ref).max()), f"exact {cid} pad {pad} fade {fade}")
    # the residual alone: zeros outside the spans, and the watermarked clip is the input plus it, rounded once
    d = window.span_generator(net, [cu(x) for x in xs], cu(msgs), spans, L, "f32", pad, fade_samples=fade, gain=gain, add_input=False)
    for b, x in enumerate(xs):
        assert not d[b].cpu().numpy()[SC.outside(len(x), spans[b])].any()
        assert torch.equal(cu(x) + d[b], got[b])


@pytest.mark.parametrize("cid", SC.EXACT_IDS)
def test_span_route_alone_or_in_the_mixed_list(cid):
    cfg, net, L, lengths, spans, xs, msgs, _ = _exact(cid)
    mixed = window.span_generator(net, [cu(x) for x in xs], cu(msgs), spans, L, "f32", 1.0, fade_samples=7, gain=SC.GAIN)
    for b, x in enumerate(xs):
        alone = window.span_generator(net, [cu(x)], cu(msgs), [spans[b]], L, "f32", 1.0, fade_samples=7, gain=SC.GAIN)
        assert torch.equal(alone[0], mixed[b]), b
    batch = window.span_generator(net, cu(np.stack([xs[2], xs[2][::-1].copy()]))[:, None], cu(msgs), [spans[2], spans[2]], L)
    assert batch.shape == (2, 1, lengths[2])                                                  # [B,1,T] in, [B,1,T] out
    assert torch.equal(batch[0, 0], window.span_generator(net, [cu(xs[2])], cu(msgs), [spans[2]], L)[0])


def test_span_route_f16_vs_its_oracle():
    from oracle import wv_oracle_h16 as O16
    from oracle import wv_oracle_torch as OT
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    cid = SC.F16_ID
    cfg, seed = W.net_config(SC.net_case(cid))
    sd = random_state_dict(cfg, seed)
    net, onet = HipNet(cfg, sd), OT.Net(cfg, sd)
    L, lengths, spans, _ = SC.cases(cid)
    xs, msgs = SC.clip_data(cid, lengths), SC.messages(cid)

    def delta(x, m):
        xt = torch.from_numpy(x[None, None]).double()
        return O16.decoder_forward(onet, O16.encoder_latent(onet, xt, torch.from_numpy(msgs[m:m + 1])))[0, 0, :len(x)].numpy()
    deltas = [{m: delta(x, m) for m in {m for _, _, m in sp}} for x, sp in zip(xs, spans)]
    for pad in SC.PAD_LIMITS:
        for fade, gain in ((0, 1.0), (7, SC.GAIN)):
            got = window.span_generator(net, [cu(x) for x in xs], cu(msgs), spans, L, "f16", pad, fade_samples=fade, gain=gain)
            _check_route(got, xs, spans, deltas, fade, gain, WM_BAR, lambda ref: 1.0, f"f16 {cid} pad {pad} fade {fade} (absolute)")


# =============================================================================================== 3. the native-rate route and the file API
@functools.lru_cache(maxsize=None)
def _wv():
    """A WaveVerify whose generator is the small net x13 (hop 12, halo 408): the public calls need nothing of its size."""
    from waveverify_amd import WaveVerify
    cfg, seed = W.net_config(SC.net_case("x13.generator"))
    return WaveVerify.random_init(seed=seed, configs={"generator": cfg})


NATIVE_SPANS = [(100, 900, 0xBEEF), (900, 1500, 0x1234), (3000, 4700, 0xBEEF)]


@pytest.mark.parametrize("sr,Cn", [(48000, 2), (44100, 1)])
def test_native_route_is_upsample_add_of_the_masked_residual(sr, Cn):
    import native_cases as NC
    from waveverify_amd import native
    wv = _wv()
    Tn = int(0.3 * sr) + 1
    audio = cu((NC.inputs(sr, Cn, Tn)[0][:1] * np.float32(0.2)).astype(np.float32))      # [1, C, Tn]
    x16 = wv.to_model_rate(audio, sr)
    assert x16.shape[-1] >= 4700
    msgs, rows, ids = wv._span_messages([NATIVE_SPANS])
    assert msgs.shape == (2, 16) and [r[2] for r in rows[0]] == [0, 1, 0] and [i.to_int() for i in ids] == [0xBEEF, 0x1234, 0xBEEF]
    W16 = wv._window_samples(30.0)
    for fade, strength in ((0, 1.0), (7, 0.5)):
        d16 = window.span_generator(wv.model.generator, x16, msgs, rows, W16, fade_samples=fade, add_input=False)
        clips = wv.embed_spans_clips(x16, [NATIVE_SPANS], fade_samples=fade)
        assert torch.equal(clips, x16 + d16)                                               # d16 is embed_spans_clips minus the input, restated
        off = torch.from_numpy(SC.outside(x16.shape[-1], NATIVE_SPANS)).cuda()
        assert not d16[0, 0][off].any() and d16[0, 0][~off].abs().max() > 1e-3
        got = wv.embed_spans_native_batch(audio, sr, [NATIVE_SPANS], strength, fade)
        assert got.shape == audio.shape and torch.equal(got, native.upsample_add(audio, d16, sr, strength))
    # strength is the gain of the 16 kHz route: the twin's arithmetic with gain = strength
    half = wv.embed_spans_clips(x16, [NATIVE_SPANS], fade_samples=7, strength=0.5)
    want = window.span_generator(wv.model.generator, x16, msgs, rows, W16, fade_samples=7, gain=0.5)
    assert torch.equal(half, want) and not torch.equal(half, clips)


def test_embed_spans_file_api(tmp_path):
    import native_cases as NC
    from waveverify_amd.utils import load_audio, load_audio_native, save_audio
    from waveverify_amd.watermark_id import WatermarkID
    wv = _wv()
    sr, Cn, Tn = 44100, 2, 13231                                                           # 0.3 s
    x = (NC.inputs(sr, Cn, Tn)[0] * np.float32(0.2)).astype(np.float32)
    src, out = tmp_path / "stereo.wav", tmp_path / "out" / "wm.wav"
    save_audio(torch.from_numpy(x[0]), src, sr)
    spans_s = [(0.01, 0.05, 0xBEEF), (0.05, 0.09, "0001001000110100"), (0.2, 9.0, WatermarkID.custom(7))]      # the last end is clamped
    audio16, _ = load_audio(src, 16000)
    T16 = int(audio16.shape[-1])
    spans = [(160, 800, 0xBEEF), (800, 1440, 0x1234), (3200, T16, 7)]
    a, asr, ids = wv.embed_spans(src, spans_s, fade_ms=1.0)
    assert asr == 16000 and a.shape == (T16,) and [i.to_int() for i in ids] == [0xBEEF, 0x1234, 7]
    want = wv.embed_spans_clips(audio16.unsqueeze(0), [spans], fade_samples=16).squeeze(0).cpu().numpy().squeeze()
    assert np.array_equal(a.view(np.int32), want.view(np.int32))
    off = SC.outside(T16, spans)
    assert np.array_equal(a[off].view(np.int32), audio16.numpy()[0][off].view(np.int32)) and not np.array_equal(a[~off], audio16.numpy()[0][~off])
    arr, rsr, ids = wv.embed_spans(src, spans_s, out, native=True, strength=0.5, fade_ms=1.0)
    assert rsr == sr and arr.shape == (Cn, Tn) and len(ids) == 3
    file_audio, _ = load_audio_native(src)
    direct = wv.embed_spans_native_batch(file_audio.unsqueeze(0), sr, [spans], 0.5, 16)
    assert np.array_equal(bits(direct[0]), arr.view(np.int32))
    saved, ssr = load_audio_native(out)
    assert ssr == sr and tuple(saved.shape) == (Cn, Tn)
    with pytest.raises(ValueError, match="native"):
        wv.embed_spans(src, spans_s, strength=0.5)
    with pytest.raises(RuntimeError, match="Failed to embed watermark spans"):
        wv.embed_spans(src, [(0.01, 0.05, 1), (0.04, 0.06, 2)])
    with pytest.raises(RuntimeError, match="Failed to embed watermark spans"):
        wv.embed_spans(src, [(0.01, 0.05, "not an id")])


def test_set_precision_reaches_the_span_route():
    from waveverify_amd import WaveVerify
    cid = SC.F16_ID
    cfg, seed = W.net_config(SC.net_case(cid))
    wv = WaveVerify.random_init(seed=seed, configs={"generator": cfg})
    L, lengths, spans, _ = SC.cases(cid)
    x = cu(SC.clip_data(cid, lengths)[1])
    ids = (0xBEEF, 0x1234, 7)
    sp = [(s, e, ids[m]) for s, e, m in spans[1]]
    exact = wv.embed_spans_clips([x], [sp], window_seconds=L / 16000)[0]
    wv.set_precision("f16")
    half = wv.embed_spans_clips([x], [sp], window_seconds=L / 16000)[0]
    msgs, rows, _ = wv._span_messages([sp])
    want = window.span_generator(wv.model.generator, [x], msgs, rows, wv._window_samples(L / 16000), "f16")[0]
    assert torch.equal(half, want) and not torch.equal(half, exact)


# =============================================================================================== 4. live: EmbedBank.set_message
@functools.lru_cache(maxsize=None)
def _live():
    from waveverify_amd.nets import HipNet
    case = SC.net_case("x13.generator")
    cfg, sd, onet = W.oracle_net(case)
    return case, cfg, HipNet(cfg, sd), onet


@pytest.mark.parametrize("sched", ["mixed", "equal"])
def test_embed_bank_with_switches_vs_float64_span_embedding(sched):
    from waveverify_amd.session import EmbedBank
    case, cfg, net, onet = _live()
    hop = cfg.hop_length
    msgs = SC.messages("x13.generator")
    steps = dict(BK.schedules(cfg))[sched]
    data = BK.stream_data(case, steps)
    xs = {n: x for n, (x, _) in data.items()}
    plan = SC.switch_plan(steps)
    bank = EmbedBank(net, BK.CAPACITY, "f32", 1.5)
    state_msg = lambda st: None if st is None else msgs[st]
    out, marks, launches, only = SC.run_switching(bank, steps, xs, plan, lambda st: bank.open(state_msg(st)),
                                                  lambda slot, st: bank.set_message(slot, state_msg(st)), take=cu)
    assert all(n == 0 for n, o in zip(launches, only) if o)                                   # pass-through ticks launch nothing ...
    assert sum(only) > 0 or sched == "equal"                    # ... and the mixed schedule has some (equal: the streams' phases differ)
    assert any(m[0][1] is None for m in marks.values()), "a stream opened in pass-through"
    assert any(len({t for t, _ in m}) < len(m) for m in marks.values()) or sched == "equal", "a switch on a tick that completed no frame"
    worst = 0.0
    for n, x in xs.items():
        got = torch.cat([r.reshape(-1) for r in out[n]]).cpu().numpy() if out[n] else np.zeros(0, np.float32)
        assert got.shape == x.shape
        if not x.size:
            continue
        assert all(t % hop == 0 for t, _ in marks[n])
        sp = SC.spans_of(marks[n], x.size)
        deltas = {m: W.oracle_forward(cfg, onet, x[None, None], msgs[m:m + 1], add_input=False)[0, 0] for m in {m for _, _, m in sp}}
        ref = SC.reference(x, deltas, sp)
        err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
        worst = max(worst, err)
        assert err <= GEN_BAR, (sched, n, err)
        off = SC.outside(x.size, sp)
        assert np.array_equal(got[off].view(np.int32), x[off].view(np.int32)), (sched, n)    # the None stretches: the input's bits
    print(f"SPAN live {sched}: worst error {worst:.2e} (bar {GEN_BAR:.1e})")


def test_a_slot_that_never_switches_is_the_lockstep_session():
    """Three streams never call set_message while a fourth beside them goes id -> None -> id: the three are bit-equal to the lockstep
    EmbedSession with equal pushes, whose code the feature does not touch."""
    from waveverify_amd.session import EmbedBank, EmbedSession
    case, cfg, net, onet = _live()
    hop = cfg.hop_length
    steps, sizes = BK.equal_schedule(cfg, S=4)
    data = BK.stream_data(case, steps)
    names = list(data)
    msg3 = np.stack([data[n][1] for n in names[:3]])
    sess = EmbedSession(net, cu(msg3))
    bank = EmbedBank(net, 4, "f32", float("inf"))
    slots = [bank.open(data[n][1]) for n in names]
    pos, launches0 = 0, None
    for k, c in enumerate(sizes):
        if k % 3 == 1:
            assert bank.set_message(slots[3], None) == bank.samples_seen(slots[3])
        if k % 3 == 2:
            bank.set_message(slots[3], data[names[0]][1])
        want = sess.push(cu(np.stack([data[n][0][pos:pos + c] for n in names[:3]])))
        res = bank.push({s: cu(data[n][0][pos:pos + c]) for s, n in zip(slots, names)})
        pos += c
        for i in range(3):
            assert torch.equal(res[slots[i]], want[i, 0]), (k, i)
    want = sess.flush()
    for i in range(3):
        assert torch.equal(bank.close(slots[i]), want[i, 0])
    with pytest.raises(ValueError):
        bank.set_message(slots[0], None)                                                      # closed
    with pytest.raises(ValueError):
        bank.set_message(slots[3], np.zeros(5, np.float32))                                   # not a message
    with pytest.raises(ValueError):
        EmbedBank(net, 2, add_input=False).open(None)                                         # the residual alone has no pass-through
