"""The native-rate embed route on the GPU (csrc/wv_native.hip, waveverify_amd/native.py, WaveVerify.embed(native=True)): the two fused
kernels through the C ABI in guard-band arenas, bit for bit against the calls they fuse (effects.resample_waveform around an f32 channel
mean and a broadcast add) and within the project's filter bar of a float64 restatement of the whole route; their refusals; the batch route
against its own parts; and the file API.  Cases: tests/native_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import native_cases as NC
from guard import Arena, Guards
from waveverify_amd import WatermarkID, _lib, native
from waveverify_amd import effects as E
from waveverify_amd.utils import load_audio, load_audio_native, save_audio

pytestmark = pytest.mark.gpu
BAR = NC.BAR
B = NC.BATCH
M = NC.MODEL_RATE


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def rel(got, ref) -> float:
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert np.isfinite(g).all()
    return float(np.abs(g - ref).max() / max(1e-300, np.abs(ref).max()))


def untouched(out) -> None:
    torch.cuda.synchronize()
    out.check(expect_unwritten=torch.ones(out.t.shape, dtype=torch.bool))


def front_call(xg, kg, yg, b, c, tn, geom, tout) -> int:
    orig, nw, L, width = geom
    return _lib.load().wv_native_downmix_resample(xg.t.data_ptr(), kg.t.data_ptr(), yg.t.data_ptr(), b, c, tn, orig, nw, L, width, tout, stream())


def back_call(xg, dg, kg, og, b, c, t16, tn, geom, gain) -> int:
    orig, nw, L, width = geom
    return _lib.load().wv_native_upsample_add(xg.t.data_ptr(), dg.t.data_ptr(), kg.t.data_ptr(), og.t.data_ptr(), b, c, t16, tn, orig, nw, L, width,
                                              float(gain), stream())


def table_t(of, nf):
    kt, orig, nw, L, width = native.transposed_table(of, nf)
    return kt, (orig, nw, L, width)


# ================================================================== 1. the front end
@pytest.mark.parametrize("sr,Tn", NC.cases())
def test_front_end(sr, Tn, tmp_path):
    kt, geom = table_t(sr, M)
    T16 = NC.t16(Tn, sr)
    for Cn in NC.CHANNELS:
        x, _ = NC.inputs(sr, Cn, Tn)
        g = Guards(offset=1)
        xg, kg = g.input(x, "x"), g.input(kt, "kernels_t")
        yg = g.output((B, T16), name="y")
        assert front_call(xg, kg, yg, B, Cn, Tn, geom, T16) == 0
        g.check()                                                       # guards intact, inputs unchanged, every output written
        first = bits(yg.t)
        mono = NC.mono_f32(x)
        parts = E.resample_waveform(cu(mono), sr, M)                    # the calls this kernel fuses
        assert np.array_equal(first, bits(parts)), f"C={Cn}: not the bits of resample_waveform(mean)"
        if Cn <= 2:                                                     # the file loader's own tensor for the same audio
            for b in range(B):
                path = tmp_path / f"c{Cn}_{b}.wav"
                save_audio(torch.from_numpy(x[b]), path, sr)
                loaded, lsr = load_audio(path)
                assert lsr == M and np.array_equal(bits(loaded[0]), first[b]), f"C={Cn} clip {b}: not load_audio's bits"
        e = rel(yg.t, NC.front64(x, sr))
        print(f"RECORD front end {sr} C={Cn} Tn={Tn} T16={T16}: {e:.3e}")
        assert e <= BAR
        yg.refill_pattern()
        assert front_call(xg, kg, yg, B, Cn, Tn, geom, T16) == 0
        g.check()
        assert np.array_equal(bits(yg.t), first)
        y = native.downmix_resample(xg.t, sr)                           # the host layer makes exactly this call
        assert tuple(y.shape) == (B, 1, T16) and np.array_equal(bits(y[:, 0]), first)


# ================================================================== 2. the back end
@pytest.mark.parametrize("sr,Tn", NC.cases())
def test_back_end(sr, Tn):
    kt, geom = table_t(M, sr)
    T16 = NC.t16(Tn, sr)
    for Cn in NC.CHANNELS:
        x, delta = NC.inputs(sr, Cn, Tn)
        up = E.resample_waveform(cu(delta), M, sr)[..., :Tn].cpu().numpy()                  # [B, Tn] f32
        u64 = NC.up64(delta, sr, Tn)
        for gain in NC.GAINS:
            g = Guards(offset=1)
            xg, dg, kg = g.input(x, "x"), g.input(delta, "delta"), g.input(kt, "kernels_t")
            og = g.output((B, Cn, Tn), name="out")
            assert back_call(xg, dg, kg, og, B, Cn, T16, Tn, geom, gain) == 0
            g.check()
            got = og.t.cpu().numpy()
            want = x + (np.float32(gain) * up).astype(np.float32)[:, None, :]              # two roundings, broadcast over the channels
            assert want.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), f"C={Cn} gain={gain}"
            e = rel(og.t, NC.back64(x, delta, sr, gain))
            gu = gain * u64
            e_res = float(np.abs((got.astype(np.float64) - x.astype(np.float64)).mean(axis=1) - gu).max() / max(1e-300, np.abs(gu).max()))
            print(f"RECORD back end {sr} C={Cn} Tn={Tn} gain={gain}: {e:.3e}, recovered residual {e_res:.3e}")
            assert e <= BAR and e_res <= BAR
            # in place: out == x
            ag = Arena((B, Cn, Tn), name="x in place", offset=1)
            ag.t.copy_(cu(x))
            assert back_call(ag, dg, kg, ag, B, Cn, T16, Tn, geom, gain) == 0
            torch.cuda.synchronize()
            assert not ag.guard_report()
            dg.check(); kg.check()
            assert np.array_equal(bits(ag.t), got.view(np.int32))
            if gain == NC.GAINS[-1]:                                    # the host layer: fresh output, a given output, in place
                xt, dt = xg.t, dg.t
                assert np.array_equal(bits(native.upsample_add(xt, dt.unsqueeze(1), sr, gain)), got.view(np.int32))
                buf = torch.empty_like(xt)
                assert native.upsample_add(xt, dt, sr, gain, out=buf) is buf and np.array_equal(bits(buf), got.view(np.int32))
                xc = xt.clone()
                assert native.upsample_add(xc, dt, sr, gain, out=xc) is xc and np.array_equal(bits(xc), got.view(np.int32))
                xg.check()


# ================================================================== 3. refusals
def test_refusals_write_nothing_and_the_same_buffers_are_then_served():
    sr, Cn, Tn = 44100, 2, 1001
    x, delta = NC.inputs(sr, Cn, Tn)
    T16 = NC.t16(Tn, sr)
    ktf, gf = table_t(sr, M)
    ktb, gb = table_t(M, sr)
    g = Guards(offset=1)
    xg, dg, kfg, kbg = g.input(x, "x"), g.input(delta, "delta"), g.input(ktf, "front table"), g.input(ktb, "back table")
    yg, og = g.output((B, T16), name="y"), g.output((B, Cn, Tn), name="out")
    lib = _lib.load()
    P = lambda a: a.t.data_ptr()                                                            # noqa: E731

    def front(x_=None, k_=None, y_=None, b=B, c=Cn, tn=Tn, orig=gf[0], nw=gf[1], L=gf[2], width=gf[3], tout=T16):
        ptr = [P(xg) if x_ is None else x_, P(kfg) if k_ is None else k_, P(yg) if y_ is None else y_]
        return lib.wv_native_downmix_resample(*ptr, b, c, tn, orig, nw, L, width, tout, stream())

    def back(x_=None, d_=None, k_=None, o_=None, b=B, c=Cn, t16=T16, tn=Tn, orig=gb[0], nw=gb[1], L=gb[2], width=gb[3]):
        ptr = [P(xg) if x_ is None else x_, P(dg) if d_ is None else d_, P(kbg) if k_ is None else k_, P(og) if o_ is None else o_]
        return lib.wv_native_upsample_add(*ptr, b, c, t16, tn, orig, nw, L, width, 1.0, stream())

    null = C.c_void_p(None)
    t_max_f = NC.resample_t_max(Tn, gf[0], gf[1])
    t_max_b = NC.resample_t_max(T16, gb[0], gb[1])
    refused = [("x null", front(x_=null)), ("kernels_t null", front(k_=null)), ("y null", front(y_=null)),
               ("B = 0", front(b=0)), ("B = 65536", front(b=65536)), ("C = 0", front(c=0)), ("C = 65", front(c=65)),
               ("Tn = 0", front(tn=0)), ("orig = 0", front(orig=0)), ("nw = 0", front(nw=0)), ("L = 0", front(L=0)), ("Tout = 0", front(tout=0)),
               ("width = -1", front(width=-1)), ("Tout past the maximum", front(tout=t_max_f + 1)),
               ("LDS window past 64 KB", front(orig=64, nw=1, L=2 * 390 + 64, width=390, tout=1)),
               ("x null", back(x_=null)), ("delta null", back(d_=null)), ("kernels_t null", back(k_=null)), ("out null", back(o_=null)),
               ("B = 0", back(b=0)), ("B = 65536", back(b=65536)), ("C = 0", back(c=0)), ("C = 65", back(c=65)),
               ("T16 = 0", back(t16=0)), ("Tn = 0", back(tn=0)), ("orig = 0", back(orig=0)), ("nw = 0", back(nw=0)), ("L = 0", back(L=0)),
               ("width = -1", back(width=-1)), ("Tn past the maximum", back(t16=1)),
               ("LDS window past 64 KB", back(orig=64, nw=1, L=2 * 390 + 64, width=390, tn=1))]
    assert Tn > NC.resample_t_max(1, gb[0], gb[1]) and T16 <= t_max_f and Tn <= t_max_b
    for what, rc in refused:
        assert rc == -1, what
        assert b"wv_native_" in lib.wv_last_error(), what
    untouched(yg)
    untouched(og)
    # B = 65536 on buffers that do hold 65536 clips
    xb = g.input(np.zeros((65536, 1, 1), np.float32), "x 65536 clips")
    yb = g.output((65536, 1), name="y 65536 clips")
    assert lib.wv_native_downmix_resample(P(xb), P(kfg), P(yb), 65536, 1, 1, 1, 1, 1, 0, 1, stream()) == -1
    assert lib.wv_native_upsample_add(P(xb), P(xb), P(kfg), P(yb), 65536, 1, 1, 1, 1, 1, 1, 0, 1.0, stream()) == -1
    untouched(yb)
    # the same buffers inside the contract: served
    assert front() == 0 and back() == 0
    g.arenas.remove(yb)
    g.check()
    assert np.array_equal(bits(yg.t), bits(E.resample_waveform(cu(NC.mono_f32(x)), sr, M)))
    assert rel(og.t, NC.back64(x, delta, sr, 1.0)) <= BAR


def test_one_workgroup_per_tile_far_past_one_tile():
    """A clip of many tiles with B = 3 and 5 channels at the rate with the largest table: every tile's window starts where it should."""
    sr, Cn, Tn, Bn = 44100, 5, 70001, 3
    rng = np.random.default_rng(7)
    x = rng.uniform(-NC.PEAK, NC.PEAK, (Bn, Cn, Tn)).astype(np.float32)
    T16 = NC.t16(Tn, sr)
    delta = rng.uniform(-NC.PEAK, NC.PEAK, (Bn, 1, T16)).astype(np.float32)
    y = native.downmix_resample(cu(x), sr)
    assert np.array_equal(bits(y[:, 0]), bits(E.resample_waveform(cu(NC.mono_f32(x)), sr, M)))
    out = native.upsample_add(cu(x), cu(delta), sr, 0.37)
    up = E.resample_waveform(cu(delta[:, 0]), M, sr)[..., :Tn].cpu().numpy()
    want = x + (np.float32(0.37) * up).astype(np.float32)[:, None, :]
    assert np.array_equal(bits(out), want.view(np.int32))


# ================================================================== 4. the route
@pytest.fixture(scope="module")
def wv():
    from waveverify_amd import WaveVerify
    return WaveVerify.random_init(seed=0)


def _msg(wid: int) -> torch.Tensor:
    return torch.tensor([[int(c) for c in WatermarkID.custom(wid).bits]], dtype=torch.float32).cuda()


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("sr", [48000, 44100])
def test_route_is_its_parts(wv, sr, precision):
    Cn, Tn = 2, 4801
    x, _ = NC.inputs(sr, Cn, Tn)
    xt, msg = cu(x), _msg(0xBEEF)
    wv.set_precision(precision)
    try:
        for strength in (1.0, 0.5):
            got = wv.embed_native_batch(xt, sr, msg, strength)
            assert tuple(got.shape) == (B, Cn, Tn) and got.dtype == torch.float32
            x16 = wv.to_model_rate(xt, sr)
            assert tuple(x16.shape) == (B, 1, NC.t16(Tn, sr))
            delta = wv.model.generator.generator(x16, msg, add_input=False, precision=precision)
            want = native.upsample_add(xt, delta, sr, strength)
            assert np.array_equal(bits(got), bits(want)), (sr, precision, strength)
            assert float((got - xt).abs().max()) > 0                    # a residual did arrive
            # windowed: 2e-5, what windowed against whole is allowed elsewhere in the suite
            win = wv.embed_native_batch(xt, sr, msg, strength, window_seconds=0.4)
            e = float((win.double() - got.double()).abs().max())
            print(f"RECORD route {sr} {precision} strength={strength}: windowed against whole {e:.3e}")
            assert e <= 2e-5
        assert np.array_equal(bits(xt), x.view(np.int32))               # the caller's audio is not written
    finally:
        wv.set_precision("f32")


def test_route_windowed_over_several_windows(wv):
    """A clip whose 16 kHz copy is longer than the window, so that the residual really is assembled from windows."""
    sr, Cn, Tn = 48000, 2, 24001
    x = np.random.default_rng(11).uniform(-NC.PEAK, NC.PEAK, (1, Cn, Tn)).astype(np.float32)
    xt, msg = cu(x), _msg(77)
    W = wv._window_samples(0.4)
    assert NC.t16(Tn, sr) > W
    whole = wv.embed_native_batch(xt, sr, msg)
    win = wv.embed_native_batch(xt, sr, msg, window_seconds=0.4)
    e = float((win.double() - whole.double()).abs().max())
    print(f"RECORD route windowed, T16={NC.t16(Tn, sr)} W={W}: {e:.3e}")
    assert e <= 2e-5


# ================================================================== 5. the file API
def test_file_api(wv, tmp_path):
    sr, Cn, Tn = 44100, 2, 4801
    x = (NC.inputs(sr, Cn, Tn)[0] * np.float32(0.2)).astype(np.float32)                    # |x| <= 0.1, the level of the suite's synthetic clips
    src, out = tmp_path / "stereo.wav", tmp_path / "out" / "wm.wav"
    save_audio(torch.from_numpy(x[0]), src, sr)
    arr, rsr, wid = wv.embed(src, 0xBEEF, out, native=True)
    assert rsr == sr and isinstance(wid, WatermarkID) and wid.to_int() == 0xBEEF
    assert arr.shape == (Cn, Tn) and arr.dtype == np.float32
    saved, ssr = load_audio_native(out)
    assert ssr == sr and tuple(saved.shape) == (Cn, Tn)
    print(f"RECORD file API: peak of the watermarked audio {np.abs(arr).max():.3f}")
    assert np.abs(arr).max() <= 1.0                                     # save_audio's clamp was idle ...
    assert np.array_equal(saved.numpy().view(np.int32), arr.view(np.int32))                # ... so the file holds the returned bits
    want = wv.embed_native_batch(cu(x[:1]), sr, _msg(0xBEEF))
    assert np.array_equal(bits(want[0]), arr.view(np.int32))
    half, _, _ = wv.embed(src, 0xBEEF, native=True, strength=0.5, window_seconds=0.4)
    assert half.shape == (Cn, Tn)
    # the detector side is unchanged: it sees the loader's down-mix and resample of the saved file, which are to_model_rate's bits
    det, conf = wv.detect(out)
    _, mp = wv.detect_batch(wv.to_model_rate(saved.cuda(), sr))
    assert conf == mp.mean().item()
    assert det.bits == "".join(str(int(v)) for v in (mp[0] >= 0.5).int().tolist())
    # a mono file comes back as [Tn]
    mono = tmp_path / "mono.wav"
    save_audio(torch.from_numpy(x[0, :1]), mono, sr)
    arr1, rsr1, _ = wv.embed(mono, 5, native=True)
    assert arr1.shape == (Tn,) and rsr1 == sr
    # without native: the route of before, 16 kHz mono
    a, asr, _ = wv.embed(src, 0xBEEF)
    audio, _ = load_audio(src)
    ref = wv.embed_batch(audio.unsqueeze(0), _msg(0xBEEF).cpu()).squeeze(0).cpu().numpy().squeeze()
    assert asr == M and a.shape == (NC.t16(Tn, sr),) and np.array_equal(a.view(np.int32), ref.view(np.int32))
    with pytest.raises(ValueError, match="native"):
        wv.embed(src, 0xBEEF, strength=0.5)
