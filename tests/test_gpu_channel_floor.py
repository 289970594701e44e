"""The per-channel SNR floor at a file's own rate on the MI355X (csrc/wv_channel_floor.hip, waveverify_amd/channel_floor.py,
native.upsample_add_floor, WaveVerify.set_channel_snr_floor); cases in tests/channel_floor_cases.py.

1. The kernel through the C ABI on guarded arenas (tests/guard.py, offsets 0 and 1) and a poisoned workspace: out, the add=False form and the
   gains bit-equal to the twin on every case, u for the twin formed by the existing kernel (native.upsample_add on zeros); in place
   (out = x) the same bits; a row with a strength outside the rule skipped whole; refusals write nothing.
2. With the cap never reached (min_snr_db = -200) the fused call is native.upsample_add bit for bit: the new kernel's u is the old one.
3. The defect, end to end on a small exact net: a stereo 48 kHz batch whose right channel is silent gets non-zero samples in that channel
   under set_snr_floor(20) alone (today's behaviour), and gets it back bit for bit under set_channel_snr_floor(20), while every native frame
   of the loud channel meets the bar derived in channel_floor_cases.py.
4. embed_native_batch and embed_spans_native_batch under the channel floor against a float64 restatement of the whole route (float64
   downmix, the float64 oracle generator, float64 upsample, the twin's formula in float64), allowed twice the error of the same route with
   the floor off against its own restatement on the same inputs.
5. Both floors set: the documented composition, computed with the two twins.  The file API (embed and embed_spans with native=True) on a
   stereo file with a silent channel.  The f16 generator once: the guarantee and the silent channel.

MEASURED on the MI355X (the `CHANNEL FLOOR ...` lines of the test output), of the reference's largest magnitude,
floor off / floor on: embed_native_batch 6.1e-7 / 2.4e-7 (x13, 48 kHz stereo), 7.9e-7 / 3.9e-7 (x13, 44.1 kHz x3), 7.4e-7 / 4.0e-7 and
1.0e-6 / 3.1e-7 (x6); embed_spans_native_batch 4.4e-7 / 1.8e-7, 3.7e-7 / 1.4e-7, 1.0e-6 / 5.6e-7, 4.0e-7 / 1.4e-7.  The worst loud-channel
frame lies 5.5e-7 dB under the floor (bar 2.07e-6), 4.5e-7 dB with the f16 generator.  Everything else is bit equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import channel_floor_cases as CC
import native_cases as NC
import snr_floor_cases as FC
import span_cases as SC
import window_cases as W
from guard import Guards
from waveverify_amd import channel_floor as CF
from waveverify_amd import native, window
from waveverify_amd import snr_floor as SF

pytestmark = pytest.mark.gpu

DB = CC.MIN_SNR_DB
IDS = (0xBEEF, 0x1234, 7)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().contiguous().numpy()


def bits(t):
    return (host(t) if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).reshape(-1).view(np.int32)


def _abi():
    from waveverify_amd import _lib
    return _lib.load(), _lib.stream()


def u_of(delta, sr, Tn):
    """[B, T16] -> [B, Tn]: the residual at the native rate as the EXISTING kernel forms it (0 + 1 * u keeps u's bits; the chain never gives -0)."""
    d = cu(delta)
    return host(native.upsample_add(torch.zeros((d.shape[0], 1, Tn), device="cuda"), d, sr, 1.0))[:, 0]


def twin(x, u, s, sr, hop, db, add=True):
    """The twin row by row -> (out [B, C, Tn], gains [B, C, F])."""
    orig, nw, _, _ = CC.geometry(sr)
    res = [CF.numpy_channel_floor(x[b], u[b], orig, nw, hop, s[b], SF.rho_of(db), add) for b in range(len(x))]
    return np.stack([o for o, _ in res]), np.stack([g for _, g in res])


def fused(lib, st, g, x_t, delta, s, sr, hop, db, add, out_t=None, want_gains=True):
    """One wv_native_floor_up_add through the C ABI inside the Guards `g` -> (out arena or None when out_t is given, gains arena, workspace)."""
    B, Cn, Tn = x_t.shape
    kt, orig, nw, L, width = native.tables(sr, "cuda")[1]
    d = g.input(delta, "delta")
    sg = g.input(s, "strengths")
    F = native.floor_frames(Tn, sr, hop)
    out = g.output((B, Cn, Tn), name="out") if out_t is None else None
    gains = g.output((B, Cn, F), name="gains") if want_gains else None
    need = C.c_size_t(0)
    assert lib.wv_native_floor_up_add_bytes(B, Cn, delta.shape[1], Tn, orig, nw, L, width, hop, C.byref(need)) == 0, lib.wv_last_error()
    ws = g.workspace(need.value)
    rc = lib.wv_native_floor_up_add(x_t.data_ptr(), d.t.data_ptr(), kt.data_ptr(), (out.t if out_t is None else out_t).data_ptr(), B, Cn,
                                    delta.shape[1], Tn, orig, nw, L, width, hop, SF.rho_of(db), sg.t.data_ptr(), add,
                                    None if gains is None else gains.t.data_ptr(), ws.t.data_ptr(), need.value, st)
    assert rc == 0, lib.wv_last_error()
    return out, gains, ws


# =============================================================================================== 1. the kernel through the C ABI
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", CC.IDS)
def test_kernel_vs_twin(name, offset):
    lib, st = _abi()
    c = CC.case(name)
    _, sr, hop, Cn, B, Tn, _, _ = c
    x, delta, s = CC.inputs(c)
    u = u_of(delta, sr, Tn)
    for add in (1, 0):
        g = Guards(offset=offset)
        xin = g.input(x, "x")
        out, gains, _ = fused(lib, st, g, xin.t, delta, s, sr, hop, DB, add)
        g.check()                                                          # inputs unchanged, every out and gains element written, no guard touched
        want, want_g = twin(x, u, s, sr, hop, DB, bool(add))
        assert np.array_equal(bits(out.t), want.reshape(-1).view(np.int32)), (name, add)
        assert np.array_equal(bits(gains.t), want_g.reshape(-1).view(np.int32)), (name, add)
    # in place: out = x gives the same bits (add = 1, the last `want` is add = 0's)
    want, _ = twin(x, u, s, sr, hop, DB, True)
    g = Guards(offset=offset)
    xio = g.output((B, Cn, Tn), name="x = out")
    xio.tflat.copy_(cu(x).reshape(-1))
    fused(lib, st, g, xio.t, delta, s, sr, hop, DB, 1, out_t=xio.t, want_gains=False)
    torch.cuda.synchronize()
    assert not xio.guard_report()
    assert np.array_equal(bits(xio.t), want.reshape(-1).view(np.int32)), name


def test_a_row_with_a_strength_outside_the_rule_is_skipped_whole_and_refusals_write_nothing():
    lib, st = _abi()
    c = CC.case("8k.hop3.rows")
    _, sr, hop, Cn, B, Tn, _, _ = c
    x, delta, s = CC.inputs(c)
    bad = s.copy()
    bad[1], bad[3], bad[4] = -0.5, np.nan, np.inf
    g = Guards()
    xin = g.input(x, "x")
    out, gains, _ = fused(lib, st, g, xin.t, delta, bad, sr, hop, DB, 1)
    torch.cuda.synchronize()
    skipped = torch.zeros((B, Cn, Tn), dtype=torch.bool)
    skipped[[1, 3, 4]] = True
    out.check(expect_unwritten=skipped)
    gains.check(expect_unwritten=torch.zeros(gains.shape, dtype=torch.bool).index_fill_(0, torch.tensor([1, 3, 4]), True))
    want, want_g = twin(x, u_of(delta, sr, Tn), s, sr, hop, DB)
    for b in (0, 2):
        assert np.array_equal(bits(out.t[b]), want[b].reshape(-1).view(np.int32)) and np.array_equal(bits(gains.t[b]), want_g[b].reshape(-1).view(np.int32))
    # refusals: nothing launched, nothing written
    kt, orig, nw, L, width = native.tables(sr, "cuda")[1]
    g2 = Guards()
    xin, d, sg = g2.input(x, "x"), g2.input(delta, "delta"), g2.input(s, "strengths")
    out, gains, ws = g2.output((B, Cn, Tn), name="out"), g2.output(tuple(want_g.shape), name="gains"), g2.workspace(1 << 16)
    ok = dict(x=xin.t.data_ptr(), d=d.t.data_ptr(), kt=kt.data_ptr(), out=out.t.data_ptr(), B=B, C=Cn, T16=delta.shape[1], Tn=Tn, orig=orig, nw=nw,
              L=L, width=width, hop=hop, rho=0.01, s=sg.t.data_ptr(), add=1, gains=gains.t.data_ptr(), ws=ws.t.data_ptr(), wb=1 << 16)
    call = lambda a: lib.wv_native_floor_up_add(a["x"], a["d"], a["kt"], a["out"], a["B"], a["C"], a["T16"], a["Tn"], a["orig"], a["nw"], a["L"],   # noqa: E731
                                                a["width"], a["hop"], a["rho"], a["s"], a["add"], a["gains"], a["ws"], a["wb"], st)
    for why, kw in (("null x", dict(x=None)), ("null delta", dict(d=None)), ("null kernels_t", dict(kt=None)), ("null out", dict(out=None)),
                    ("null strengths", dict(s=None)), ("null workspace", dict(ws=None)), ("B = 0", dict(B=0)), ("C = 65", dict(C=65)),
                    ("Tn = 0", dict(Tn=0)), ("T16 too short for Tn", dict(T16=3)), ("hop = 0", dict(hop=0)), ("rho = 0", dict(rho=0.0)),
                    ("rho = nan", dict(rho=float("nan"))), ("rho = inf", dict(rho=float("inf"))), ("add = 2", dict(add=2)),
                    ("a frame beyond the limit", dict(hop=2 * CF.MAX_FRAME + 2)), ("a misaligned workspace", dict(ws=ws.t.data_ptr() + 4)),
                    ("a workspace too small", dict(wb=16))):
        assert call({**ok, **kw}) == -1, why
        assert lib.wv_last_error().decode().startswith("wv_native_floor_up_add:"), why
    torch.cuda.synchronize()
    for a in (xin, d, sg):
        a.check()
    out.check(expect_unwritten=torch.ones((B, Cn, Tn), dtype=torch.bool))
    gains.check(expect_unwritten=torch.ones(tuple(want_g.shape), dtype=torch.bool))
    assert not ws.guard_report() and bool((ws.t == 0xFF).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.upsample_add_floor(torch.zeros(1, 2, 96), torch.zeros(1, 1, 32), 48000, DB)


# =============================================================================================== 2. the cap inactive: the old kernel's bits
@pytest.mark.parametrize("name", ["48k.hop320.tiles", "44k.hop320", "11k.hop5", "8k.hop1", "16k.hop320", "48k.one"])
def test_with_the_cap_never_reached_the_fused_call_is_upsample_add(name):
    c = CC.case(name)
    _, sr, hop, Cn, B, Tn, _, _ = c
    x, delta, _ = CC.inputs(c)
    rng = np.random.default_rng(W.seed_of("channel floor inactive", name))
    x = np.where(x == 0, rng.uniform(0.1, 0.5, x.shape).astype(np.float32), x)          # no silent channel: q >= s in every frame
    for s in (1.0, 0.75):
        got, g = native.upsample_add_floor(cu(x), cu(delta), sr, -200.0, s, hop=hop, return_gains=True)
        assert bool((g == s).all())
        assert torch.equal(got, native.upsample_add(cu(x), cu(delta), sr, s)), (name, s)


# =============================================================================================== 3. the defect, end to end
def _wv(cid):
    import test_gpu_snr_floor as TSF
    return TSF._wv(cid)


def _route_audio(cid, sr, Cn, B, silent):
    """[B, Cn, Tn] float32, 0.3 s at `sr` under a block envelope of 10 ms blocks (loud and quiet passages, digital silence), channel `silent` all zero."""
    Tn = int(0.3 * sr) + 1
    x = FC.shape_level((NC.inputs(sr, Cn, Tn)[0][:B] * np.float32(0.2)).astype(np.float32), sr // 100, ("channel floor", cid, sr))
    if silent is not None:
        x[:, silent] = 0.0
    return x


def _assert_bound(x, v, sr, hop, db, what):
    orig, nw, _, _ = CC.geometry(sr)
    worst = np.inf
    for b in range(x.shape[0]):
        for ch in range(x.shape[1]):
            snr = CF.native_frame_snr_db(x[b, ch], v[b, ch], orig, nw, hop)
            worst = min(worst, float((snr - db).min()))
            assert (snr >= db - CC.BOUND_DB).all(), (what, b, ch, float((snr - db).min()))
    return worst


@pytest.mark.parametrize("cid", ["x13.generator", "x1.generator"])
def test_a_silent_channel_gets_the_watermark_under_the_16k_floor_and_stays_silent_under_the_channel_floor(cid):
    wv, cfg, _ = _wv(cid)
    sr, hop = 48000, cfg.hop_length
    x = _route_audio(cid, sr, 2, 2, silent=1)
    audio = cu(x)
    msg = wv._messages([IDS[0], IDS[1]])
    assert wv.snr_floor_db is None and wv.channel_snr_floor_db is None
    plain = wv.embed_native_batch(audio, sr, msg, 0.75)
    delta = wv.model.generator.generator(wv.to_model_rate(audio, sr), msg, add_input=False, precision=wv.generator_precision)
    wv.set_snr_floor(DB)
    try:
        old = wv.embed_native_batch(audio, sr, msg, 0.75)
    finally:
        wv.set_snr_floor(None)
    assert int((old[:, 1] != 0).sum()) > x.shape[-1] // 2, "the 16 kHz floor leaves the residual in the silent channel: the defect"
    wv.set_channel_snr_floor(DB)
    try:
        got = wv.embed_native_batch(audio, sr, msg, 0.75)
    finally:
        wv.set_channel_snr_floor(None)
    assert got.shape == audio.shape
    assert np.array_equal(bits(got[:, 1]), x[:, 1].reshape(-1).view(np.int32)), "the silent channel comes back bit for bit"
    want, gains = native.upsample_add_floor(audio, delta, sr, DB, 0.75, hop=hop, return_gains=True)
    assert torch.equal(got, want)
    v = host(native.upsample_add_floor(audio, delta, sr, DB, 0.75, hop=hop, add=False))
    assert not v[:, 1].any() and v[:, 0].any()
    worst = _assert_bound(x, v, sr, hop, DB, cid)
    g = host(gains)
    assert (g[:, 1] == 0).all() and (g[:, 0] < 0.75).any() and (g[:, 0] > 0).any()
    assert torch.equal(wv.embed_native_batch(audio, sr, msg, 0.75), plain)              # the switch off again: the bits of before
    print(f"CHANNEL FLOOR defect {cid}: worst loud-channel frame {worst:.2e} dB against the floor (bar -{CC.BOUND_DB:.2e})")


# =============================================================================================== 4. against the float64 restatement
NATIVE_SPANS = [(100, 900, 0), (900, 1500, 1), (3000, 4700, 0)]


def _rel(got, ref):
    return float(np.abs(host(got).astype(np.float64) - ref).max()) / float(np.abs(ref).max())


@pytest.mark.parametrize("sr,Cn", [(48000, 2), (44100, 3)])
@pytest.mark.parametrize("cid", ["x13.generator", "x6.generator"])
def test_routes_vs_float64(cid, sr, Cn):
    """The tolerance is measured: the error of the same route with the floor off against its float64 restatement on the same inputs; under the
    floor twice it is allowed (the floor multiplies the residual by a gain <= strength and adds one rounding)."""
    wv, cfg, onet = _wv(cid)
    hop, s = cfg.hop_length, 0.75
    x = _route_audio(cid, sr, Cn, 2, silent=Cn - 1)
    B, _, Tn = x.shape
    audio = cu(x)
    ids = [IDS[0], IDS[1]]
    msg = wv._messages(ids)
    m = host(msg).reshape(B, -1)
    sp = [[(a, e, IDS[i]) for a, e, i in NATIVE_SPANS]] * B
    msgs, rows, _ = wv._span_messages(sp)
    ms = host(msgs).reshape(msgs.shape[0], -1)
    rho, ramp7 = SF.rho_of(DB), window.span_ramp(7)
    oracle = lambda x16, mm: W.oracle_forward(cfg, onet, x16[None, None], mm[None], add_input=False)[0, 0]      # noqa: E731
    off = wv.embed_native_batch(audio, sr, msg, s), wv.embed_spans_native_batch(audio, sr, sp, s, 7)
    wv.set_channel_snr_floor(DB)
    try:
        on = wv.embed_native_batch(audio, sr, msg, s), wv.embed_spans_native_batch(audio, sr, sp, s, 7)
    finally:
        wv.set_channel_snr_floor(None)
    e_off, e_on = [0.0, 0.0], [0.0, 0.0]
    lowered = 0
    for b in range(B):
        x16 = CC.down64(x[b], sr)
        d_whole = oracle(x16, m[b])
        deltas = {r: oracle(x16, ms[r]) for r in {r for _, _, r in rows[b]}}
        d_span = SC.reference(x16, deltas, rows[b], ramp7, 1.0, add_input=False)
        for i, d in enumerate((d_whole, d_span)):
            u = CC.up64(d, sr, Tn)
            ref_on, g = CC.floor64(x[b], u, sr, hop, s, rho)
            e_off[i] = max(e_off[i], _rel(off[i][b], x[b].astype(np.float64) + s * u[None]))
            e_on[i] = max(e_on[i], _rel(on[i][b], ref_on))
            lowered += int((g < s).sum())
    assert lowered > 0
    print(f"CHANNEL FLOOR float64 {cid} {sr} Hz x{Cn}: embed_native_batch off {e_off[0]:.2e} on {e_on[0]:.2e}; "
          f"embed_spans_native_batch off {e_off[1]:.2e} on {e_on[1]:.2e} (bar: twice the floor-less error)")
    for i, what in enumerate(("embed_native_batch", "embed_spans_native_batch")):
        assert e_off[i] <= NC.BAR, (what, e_off[i])                                     # the floor-less route holds the README's 2e-5
        assert e_on[i] <= 2 * e_off[i], (what, e_on[i], e_off[i])


# =============================================================================================== 5. both floors; f16
@pytest.mark.parametrize("sr,Cn", [(48000, 2), (11025, 1)])
def test_both_floors_compose_in_the_documented_order(sr, Cn):
    wv, cfg, _ = _wv("x6.generator")
    gen, hop, s = wv.model.generator, cfg.hop_length, 0.75
    x = _route_audio("x6.generator", sr, Cn, 2, silent=1 if Cn > 1 else None)
    audio = cu(x)
    msg = wv._messages([IDS[0], IDS[1]])
    x16 = wv.to_model_rate(audio, sr)
    d = gen.generator(x16, msg, add_input=False, precision=wv.generator_precision)
    wv.set_snr_floor(10.0)
    wv.set_channel_snr_floor(DB)
    try:
        got = wv.embed_native_batch(audio, sr, msg, s)
    finally:
        wv.set_snr_floor(None)
        wv.set_channel_snr_floor(None)
    # the 16 kHz floor shapes the residual, the strength inside it ...
    ramp = SF.floor_ramp(hop)
    v16 = np.stack([SF.floor_row(host(x16[b, 0]), host(d[b, 0]), s, SF.rho_of(10.0), ramp, None, False)[0] for b in range(2)])
    # ... and the channel floor runs on that residual with cap 1.0
    u = u_of(v16, sr, x.shape[-1])
    want, g = twin(x, u, np.ones(2, np.float32), sr, hop, DB)
    assert np.array_equal(bits(got), want.reshape(-1).view(np.int32))
    assert (g < 1).any() and (g == 1).any()


def test_the_file_routes_keep_a_silent_channel_of_the_file(tmp_path):
    from waveverify_amd.utils import load_audio_native, save_audio
    wv, cfg, _ = _wv("x6.generator")
    sr = 44100
    x = _route_audio("x6.generator", sr, 2, 1, silent=1)[0]                               # [2, Tn], |x| <= 0.1: save_audio's clamp stays idle
    src, out = tmp_path / "stereo.wav", tmp_path / "wm.wav"
    save_audio(torch.from_numpy(x), src, sr)
    spans = [(0.02, 0.1, IDS[0]), (0.15, 0.25, IDS[1])]
    wv.set_channel_snr_floor(DB)
    try:
        arr, rsr, _ = wv.embed(src, IDS[0], out, native=True, strength=0.75)
        want = wv.embed_native_batch(cu(x)[None], sr, wv._messages(IDS[0]), 0.75)[0]
        sarr, _, _ = wv.embed_spans(src, spans, native=True, fade_ms=1.0)
    finally:
        wv.set_channel_snr_floor(None)
    plain, _, _ = wv.embed(src, IDS[0], native=True, strength=0.75)
    assert rsr == sr and arr.shape == x.shape and np.array_equal(bits(want), arr.reshape(-1).view(np.int32))
    saved, _ = load_audio_native(out)
    assert np.array_equal(bits(saved), arr.reshape(-1).view(np.int32))
    for a in (arr, sarr):
        assert not a[1].any() and not np.array_equal(a[0], x[0])                          # the silent channel of the file stays silent
    assert plain[1].any()                                                                 # ... and without the switch it does not


def test_the_f16_generator_once():
    wv, cfg, _ = _wv(FC.F16_ID)
    assert wv.generator_precision == "f16"
    sr, hop = 44100, cfg.hop_length
    x = _route_audio(FC.F16_ID, sr, 2, 2, silent=0)
    audio = cu(x)
    msg = wv._messages([IDS[0], IDS[1]])
    delta = wv.model.generator.generator(wv.to_model_rate(audio, sr), msg, add_input=False, precision="f16")
    wv.set_channel_snr_floor(DB)
    try:
        got = wv.embed_native_batch(audio, sr, msg)
    finally:
        wv.set_channel_snr_floor(None)
    assert np.array_equal(bits(got[:, 0]), x[:, 0].reshape(-1).view(np.int32))
    assert torch.equal(got, native.upsample_add_floor(audio, delta, sr, DB, 1.0, hop=hop))
    v = host(native.upsample_add_floor(audio, delta, sr, DB, 1.0, hop=hop, add=False))
    assert v[:, 1].any() and not v[:, 0].any()
    worst = _assert_bound(x, v, sr, hop, DB, "f16")
    print(f"CHANNEL FLOOR f16: worst frame {worst:.2e} dB against the floor (bar -{CC.BOUND_DB:.2e})")
