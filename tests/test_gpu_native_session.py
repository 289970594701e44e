"""Native-rate live sessions on the GPU (csrc/wv_native.hip's session entry points, waveverify_amd/native_session.py).

1. The two stages alone through the C ABI: every buffer in a guard-band arena one element off alignment, histories NaN-poisoned beyond their
   valid length, the push schedules of tests/test_native_session_cpu.py plus a push that crosses a 256-output tile; the concatenated outputs
   are native.downmix_resample / native.upsample_add of the whole signal BIT FOR BIT, two runs are equal, and refusals write nothing.
2. The embed route is its parts, bit for bit, and within 2e-5 of embed_native_batch on the whole input (the suite's bar for windowed
   against whole, the measure of tests/test_gpu_native.py: the largest absolute difference).
3. Detect and locate sessions against the 16 kHz sessions given to_model_rate of the same audio.

Measured on the MI355X (RECORD lines, pytest -s), the session against embed_native_batch on the whole input by largest absolute difference:
    exact f32, bar 2e-5: small generator (hop 16) 5.6e-8 at 48 kHz stereo and 3.0e-8 at 44.1 kHz mono (strength 0.5); full-size generator 3.7e-8 and 3.0e-8.
    f16 session against the f16 route on the whole input, bar 2e-5: 0 at both rates.  Against the EXACT route the f16 session stands
    3.1e-5 (48 kHz) and 3.3e-5 (44.1 kHz) off: that is the f16 mode's own distance from the exact path, which the suite bars at 1e-4
    (test_gpu_h16's WM_BAR), not a distance between windowed and whole; it is asserted at that bar."""
import ctypes as C

import numpy as np
import pytest
import torch

import native_cases as NC
import window_cases as W
from guard import Guards
from waveverify_amd import _lib, native
from waveverify_amd import native_session as NS
from waveverify_amd.session import DetectSession, EmbedSession, LocateSession

pytestmark = pytest.mark.gpu
M = NC.MODEL_RATE
RATES = [48000, 44100, 22050, 8000, 16000]
HOP = 16
WM_BAR = 1e-4                                                               # the f16 mode's watermarked samples against the exact path's (test_gpu_h16)
NAN = np.float32(np.nan)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t) -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.int32)


def P(arena):
    return arena.t.data_ptr()


def schedules(sr: int):
    """test_native_session_cpu.schedules, and one push of 257 * orig / nw inputs: more than 256 outputs, so the push crosses a tile."""
    orig, nw, L, width = native.table_geometry(sr, M)
    lat = NS.EmbedPlan(sr, HOP).latency_samples
    a, b = orig * HOP // 3, orig * HOP // 2
    return [("flush only", ()), ("one sample", (1,)), ("pushes of 0", (0, 5, 0, 0, orig + 3, 0)),
            ("fewer than width in total", (width // 2, max(0, width - 1 - width // 2))), ("exactly orig", (orig,)),
            ("one push longer than ten histories", (3, 10 * max(L, lat) + 7, 2)),
            ("ends on a hop multiple", (a, b, orig * HOP - a - b)),
            ("a push across a tile", (7, -(-257 * orig // nw), 5))]


def poisoned(valid: np.ndarray, cap: int) -> np.ndarray:
    """[..., v] -> [..., cap] with NaN beyond the valid part."""
    out = np.full(valid.shape[:-1] + (cap,), NAN, np.float32)
    out[..., :valid.shape[-1]] = valid
    return out


def unwritten_beyond(shape, v: int) -> torch.Tensor:
    m = torch.ones(shape, dtype=torch.bool)
    m[..., :v] = False
    return m


def down_call(lib, hist, x, kt, y, hout, t, S, Cn, geom, cap=None):
    orig, nw, L, width = geom
    return lib.wv_native_session_down(P(hist), hist.t.shape[1] if cap is None else cap, t.hv, P(x) if t.n else None, t.n, P(kt), P(y) if t.n_out else None,
                                      t.n_out, t.pad, P(hout), t.drop, t.hv2, S, Cn, orig, nw, L, width, stream())


def up_call(lib, rhist, r, kt, pend, x, out, pout, rout, t, S, Cn, geom, gain):
    orig, nw, L, width = geom
    b = t.back
    return lib.wv_native_session_up_add(P(rhist), rhist.t.shape[1], b.hv, P(r) if b.n else None, b.n, P(kt), P(pend), pend.t.shape[2], t.pv,
                                        P(x) if x.t.shape[2] else None, x.t.shape[2], P(out) if b.n_out else None, b.n_out, b.pad, float(gain),
                                        P(pout), P(rout), b.drop, b.hv2, S, Cn, orig, nw, L, width, stream())


# ================================================================== 1. the stages alone
@pytest.mark.parametrize("sr", RATES)
def test_front_stage_is_downmix_resample_bit_for_bit(sr):
    lib = _lib.load()
    kt, orig, nw, L, width = native.transposed_table(sr, M)
    geom = (orig, nw, L, width)
    for i, (name, sizes) in enumerate(schedules(sr)):
        S, Cn, T = (1, 3)[i % 2], 1 + i % 3, sum(sizes)
        x = np.random.default_rng([sr, i]).uniform(-NC.PEAK, NC.PEAK, (S, Cn, T)).astype(np.float32)
        plan = NS.StagePlan(*geom)
        hist = np.zeros((S, 0), np.float32)
        ys, at = [], 0
        for n in list(sizes) + [None]:
            t = plan.flush() if n is None else plan.push(n)
            assert hist.shape[1] == t.hv
            g = Guards(offset=1)
            hg, kg = g.input(poisoned(hist, L), "history"), g.input(kt, "kernels_t")
            xg = g.input(x[:, :, at:at + t.n] if t.n else np.zeros((1,), np.float32), "x")
            yg, og = g.output((S, max(t.n_out, 1)), name="y"), g.output((S, L), name="next history")
            assert down_call(lib, hg, xg, kg, yg, og, t, S, Cn, geom) == 0, (name, lib.wv_last_error())
            torch.cuda.synchronize()
            hg.check(); kg.check(); xg.check()
            yg.check(expect_unwritten=None if t.n_out else torch.ones(yg.t.shape, dtype=torch.bool))
            og.check(expect_unwritten=unwritten_beyond((S, L), t.hv2))
            y1, h1 = bits(yg.t[:, :t.n_out]), bits(og.t[:, :t.hv2])
            yg.refill_pattern(); og.refill_pattern()                         # a second run gives the same bits
            assert down_call(lib, hg, xg, kg, yg, og, t, S, Cn, geom) == 0
            torch.cuda.synchronize()
            assert np.array_equal(bits(yg.t[:, :t.n_out]), y1) and np.array_equal(bits(og.t[:, :t.hv2]), h1), name
            ys.append(yg.t[:, :t.n_out].cpu().numpy())
            hist = og.t[:, :t.hv2].cpu().numpy()
            at += t.n
            assert t.hv2 < L
        got = np.concatenate(ys, axis=1)
        assert got.shape == (S, NC.t16(T, sr) if T else 0), name
        if T:
            want = native.downmix_resample(cu(x), sr)[:, 0]
            assert np.array_equal(got.view(np.int32), bits(want)), f"{sr} {name}: not downmix_resample's bits"


@pytest.mark.parametrize("sr", RATES)
def test_back_stage_is_upsample_add_bit_for_bit(sr):
    lib = _lib.load()
    kt, orig, nw, L, width = native.transposed_table(M, sr)
    geom = (orig, nw, L, width)
    for i, (name, sizes) in enumerate(schedules(sr)):
        S, Cn, T = (3, 1)[i % 2], 1 + (i + 1) % 3, sum(sizes)
        gain = (1.0, 0.37)[i % 2] if name != "a push across a tile" else 1.0
        rng = np.random.default_rng([sr, i, 7])
        x = rng.uniform(-NC.PEAK, NC.PEAK, (S, Cn, T)).astype(np.float32)
        res = rng.uniform(-NC.PEAK, NC.PEAK, (S, NC.t16(T, sr) if T else 0)).astype(np.float32)
        plan = NS.EmbedPlan(sr, HOP)                                          # the residual arrives in hop multiples, the rest at flush
        pcap = plan.pcap
        rhist, pend = np.zeros((S, 0), np.float32), np.zeros((S, Cn, 0), np.float32)
        outs, at, rat = [], 0, 0
        for n in list(sizes) + [None]:
            t = plan.flush() if n is None else plan.push(n)
            b = t.back
            assert b.n == t.n_res and (t.final or t.n_res % HOP == 0) and rhist.shape[1] == b.hv and pend.shape[2] == t.pv
            nx = 0 if n is None else n
            g = Guards(offset=1)
            rg, pg, kg = g.input(poisoned(rhist, L), "residual history"), g.input(poisoned(pend, pcap), "pending"), g.input(kt, "kernels_t")
            dg = g.input(res[:, rat:rat + b.n] if b.n else np.zeros((1,), np.float32), "residual")
            xg = g.input(x[:, :, at:at + nx], "x") if nx else g.input(np.zeros((S, Cn, 0), np.float32), "x")
            og = g.output((S, Cn, max(b.n_out, 1)), name="out")
            po, ro = g.output((S, Cn, pcap), name="next pending"), g.output((S, L), name="next residual history")

            def run():
                assert up_call(lib, rg, dg, kg, pg, xg, og, po, ro, t, S, Cn, geom, gain) == 0, (name, lib.wv_last_error())
                torch.cuda.synchronize()
            run()
            for a in (rg, pg, kg, dg, xg):
                a.check()
            og.check(expect_unwritten=None if b.n_out else torch.ones(og.t.shape, dtype=torch.bool))
            po.check(expect_unwritten=unwritten_beyond((S, Cn, pcap), t.pv2))
            ro.check(expect_unwritten=unwritten_beyond((S, L), b.hv2))
            first = [bits(og.t[:, :, :b.n_out]), bits(po.t[:, :, :t.pv2]), bits(ro.t[:, :b.hv2])]
            og.refill_pattern(); po.refill_pattern(); ro.refill_pattern()
            run()
            again = [bits(og.t[:, :, :b.n_out]), bits(po.t[:, :, :t.pv2]), bits(ro.t[:, :b.hv2])]
            assert all(np.array_equal(u, v) for u, v in zip(first, again)), name
            outs.append(og.t[:, :, :b.n_out].cpu().numpy())
            pend, rhist = po.t[:, :, :t.pv2].cpu().numpy(), ro.t[:, :b.hv2].cpu().numpy()
            at, rat = at + nx, rat + b.n
            assert t.pv2 < plan.latency_samples and b.hv2 < L
        got = np.concatenate(outs, axis=2)
        assert got.shape == (S, Cn, T) and rat == res.shape[1], name
        if T:
            want = native.upsample_add(cu(x), cu(res), sr, gain)
            assert np.array_equal(got.view(np.int32), bits(want)), f"{sr} {name} gain={gain}: not upsample_add's bits"


def test_refusals_write_nothing_and_the_same_buffers_are_then_served():
    sr, S, Cn, n = 44100, 3, 2, 1001
    lib = _lib.load()
    ktf, *gf = native.transposed_table(sr, M)
    ktb, *gb = native.transposed_table(M, sr)
    rng = np.random.default_rng(3)
    x = rng.uniform(-NC.PEAK, NC.PEAK, (S, Cn, n)).astype(np.float32)
    res = rng.uniform(-NC.PEAK, NC.PEAK, (S, NC.t16(n, sr))).astype(np.float32)
    plan = NS.EmbedPlan(sr, HOP)
    t = plan.push(n)
    f, b = t.front, t.back
    assert f.n_out > 256 and b.n_out > 256 and t.pv2 > 0 and f.hv2 > 0 and b.hv2 > 0
    Lf, Lb, pcap = gf[2], gb[2], plan.pcap
    g = Guards(offset=1)
    hg, kfg, kbg, xg = g.input(poisoned(np.zeros((S, 0), np.float32), Lf), "history"), g.input(ktf, "front table"), g.input(ktb, "back table"), g.input(x, "x")
    rg, pg = g.input(poisoned(np.zeros((S, 0), np.float32), Lb), "residual history"), g.input(poisoned(np.zeros((S, Cn, 0), np.float32), pcap), "pending")
    dg = g.input(res[:, :b.n], "residual")
    yg, ho = g.output((S, f.n_out), name="y"), g.output((S, Lf), name="next history")
    og, po, ro = g.output((S, Cn, b.n_out), name="out"), g.output((S, Cn, pcap), name="next pending"), g.output((S, Lb), name="next residual history")
    null = None

    def down(hist=P(hg), hcap=Lf, hv=f.hv, x_=P(xg), n_=f.n, k_=P(kfg), y_=P(yg), n_out=f.n_out, pad=f.pad, hout=P(ho), drop=f.drop, hv2=f.hv2, s=S, c=Cn,
             orig=gf[0], nw=gf[1], L=gf[2], width=gf[3]):
        return lib.wv_native_session_down(hist, hcap, hv, x_, n_, k_, y_, n_out, pad, hout, drop, hv2, s, c, orig, nw, L, width, stream())

    def up(rhist=P(rg), rcap=Lb, rv=b.hv, r_=P(dg), nr=b.n, k_=P(kbg), pend=P(pg), pcap_=pcap, pv=t.pv, x_=P(xg), n_=n, out=P(og), k=b.n_out, pad=b.pad,
           pout=P(po), rout=P(ro), rdrop=b.drop, rv2=b.hv2, s=S, c=Cn, orig=gb[0], nw=gb[1], L=gb[2], width=gb[3]):
        return lib.wv_native_session_up_add(rhist, rcap, rv, r_, nr, k_, pend, pcap_, pv, x_, n_, out, k, pad, 1.0, pout, rout, rdrop, rv2, s, c, orig, nw,
                                            L, width, stream())

    refused = [("hist null", down(hist=null)), ("x null", down(x_=null)), ("kernels_t null", down(k_=null)), ("y null", down(y_=null)),
               ("hist_out null", down(hout=null)), ("hist_out == hist", down(hout=P(hg))),
               ("S = 0", down(s=0)), ("S = 65536", down(s=65536)), ("C = 0", down(c=0)), ("C = 65", down(c=65)),
               ("L = 0", down(L=0)), ("orig = 0", down(orig=0)), ("nw = 0", down(nw=0)), ("width = -1", down(width=-1)),
               ("pad = -1", down(pad=-1)), ("pad > width", down(pad=gf[3] + 1)), ("n = -1", down(n_=-1)), ("n_out = -1", down(n_out=-1)),
               ("hv beyond the capacity", down(hv=Lf + 1, drop=f.drop + Lf + 1)), ("hv2 beyond the capacity", down(hv2=Lf + 1, drop=n - Lf - 1)),
               ("not a suffix", down(drop=f.drop - 1)), ("hcap = 0", down(hcap=0)), ("more outputs than the inputs give", down(n_out=f.n_out + 3 * gf[1])),
               ("LDS window past 64 KB", down(orig=64, nw=1, L=2 * 8200 + 64, width=8200, n_out=1)),
               ("rhist null", up(rhist=null)), ("r null", up(r_=null)), ("kernels_t null", up(k_=null)), ("pend null", up(pend=null)), ("x null", up(x_=null)),
               ("out null", up(out=null)), ("pend_out null", up(pout=null)), ("rhist_out null", up(rout=null)), ("pend_out == pend", up(pout=P(pg))),
               ("rhist_out == rhist", up(rout=P(rg))),
               ("S = 0", up(s=0)), ("S = 65536", up(s=65536)), ("C = 0", up(c=0)), ("C = 65", up(c=65)),
               ("L = 0", up(L=0)), ("orig = 0", up(orig=0)), ("nw = 0", up(nw=0)), ("width = -1", up(width=-1)), ("pad > width", up(pad=gb[3] + 1)),
               ("rv beyond the capacity", up(rv=Lb + 1, rdrop=b.drop + Lb + 1)), ("rv2 beyond the capacity", up(rv2=Lb + 1, rdrop=b.n - Lb - 1)),
               ("pv beyond the capacity", up(pv=pcap + 1)), ("pending beyond the capacity", up(k=0)), ("k > pv + n", up(k=n + 1)),
               ("not a suffix", up(rdrop=b.drop + 1)), ("k = -1", up(k=-1)), ("nr = -1", up(nr=-1)), ("n = -1", up(n_=-1)),
               ("LDS window past 64 KB", up(orig=64, nw=1, L=2 * 8200 + 64, width=8200))]
    assert n > pcap                                                          # k = 0 would leave more pending than the delay line holds
    for what, rc in refused:
        assert rc == -1, what
        assert b"wv_native_session_" in lib.wv_last_error(), what
    torch.cuda.synchronize()
    for out in (yg, ho, og, po, ro):
        out.check(expect_unwritten=torch.ones(out.t.shape, dtype=torch.bool))
    # the same buffers inside the contract: served.  What a push emits is final: the first samples of the whole-signal result
    assert down() == 0 and up() == 0
    torch.cuda.synchronize()
    for a in (hg, kfg, kbg, xg, rg, pg, dg):
        a.check()
    yg.check(); og.check()
    ho.check(expect_unwritten=unwritten_beyond((S, Lf), f.hv2)); po.check(expect_unwritten=unwritten_beyond((S, Cn, pcap), t.pv2))
    ro.check(expect_unwritten=unwritten_beyond((S, Lb), b.hv2))
    assert np.array_equal(bits(yg.t), bits(native.downmix_resample(cu(x), sr)[:, 0, :f.n_out]))
    assert np.array_equal(bits(og.t), bits(native.upsample_add(cu(x), cu(res), sr, 1.0)[:, :, :b.n_out]))
    assert np.array_equal(bits(po.t[:, :, :t.pv2]), x[:, :, b.n_out:].view(np.int32))
    # nothing to do at all: served without a launch
    empty = NS.StageTick(0, 0, gf[3], 0, 0, 0)
    assert down(hv=0, n_=0, x_=null, y_=null, n_out=0, pad=gf[3], drop=0, hv2=0) == 0
    assert empty.n_out == 0


# ================================================================== 2. the route
PUSHES = (960, 0, 1, 3000, 959, 4000)                                        # then the rest in one push, then flush()


def pieces(T: int):
    out = [n for n in PUSHES]
    assert sum(out) < T
    return out + [T - sum(out)]


def run_session(sess, x: torch.Tensor):
    parts, at = [], 0
    for n in pieces(x.shape[2]):
        parts.append(sess.push(x[:, :, at:at + n]))
        at += n
        assert sess.samples_in - sess.samples_out < sess.latency_samples
    parts.append(sess.flush())
    assert sess.samples_out == sess.samples_in == x.shape[2]
    return torch.cat(parts, dim=2)


def residual_by_parts(net, msg, precision, x: torch.Tensor, sr: int) -> torch.Tensor:
    """The residual of a plain 16 kHz residual session fed downmix_resample of the whole input, in the pieces the native session's front stage
    hands on (the inner session's windows, and so its bits, follow the pieces)."""
    x16 = native.downmix_resample(x, sr)[:, 0]
    plain = EmbedSession(net, msg, precision, add_input=False)
    plan = NS.StagePlan(*native.table_geometry(sr, M))
    parts, at = [], 0
    for n in pieces(x.shape[2]) + [None]:
        k = (plan.flush() if n is None else plan.push(n)).n_out
        if k or n is None:
            parts.append(plain.push(x16[:, at:at + k]))
        at += k
    assert at == x16.shape[1]
    parts.append(plain.flush())
    return torch.cat(parts, dim=2)


@pytest.fixture(scope="module")
def wv():
    from waveverify_amd import WaveVerify
    return WaveVerify.random_init(seed=0)


@pytest.fixture(scope="module")
def small():
    """A WaveVerify around a small generator of window_cases.net_cases() with hop <= 32."""
    from waveverify_amd import WaveVerify
    case = next(c for c in W.net_cases() if c[1] == "f32" and c[2] == "generator" and W.net_config(c)[0].hop_length <= 32)
    cfg, sd, _ = W.oracle_net(case)
    w = WaveVerify.__new__(WaveVerify)
    w.device = torch.device("cuda", torch.cuda.current_device())
    w._build({"generator": sd}, {"generator": cfg})
    w.sample_rate, w.watermark_bits = WaveVerify.DEFAULT_SAMPLE_RATE, cfg.msg_dimension
    return w


def clip(sr: int, S: int, Cn: int, T: int) -> torch.Tensor:
    """The suite's synthetic level (0.1 N(0, 1)) on every channel."""
    r = np.random.default_rng([sr, S, Cn, T, 5])
    return cu(np.clip(0.1 * r.standard_normal((S, Cn, T)), -1.0, 1.0).astype(np.float32))


def check_route(w, sr, Cn, T, precision, strength, label):
    S = 2
    gen = w.model.generator
    msg = cu(np.random.default_rng(9).integers(0, 2, (S, gen.cfg.msg_dimension)).astype(np.float32))
    x = clip(sr, S, Cn, T)
    keep = x.clone()
    w.set_precision(precision)
    try:
        sess = NS.NativeEmbedSession(gen, msg, sr, Cn, strength, precision)
        got = run_session(sess, x)
        assert tuple(got.shape) == (S, Cn, T) and got.dtype == torch.float32
        want = native.upsample_add(x, residual_by_parts(gen, msg, precision, x, sr), sr, strength)
        assert np.array_equal(bits(got), bits(want)), f"{label}: the route is not its parts"
        assert float((got - x).abs().max()) > 0                            # a residual did arrive
        # windowed against whole, 2e-5: for the exact path that is embed_native_batch in exact f32; the f16 session is held to the f16 route on
        # the whole input at the same bar (as test_gpu_native holds its windowed route), and to the exact route at the f16 mode's own bar
        whole = w.embed_native_batch(x, sr, msg, strength)
        e = float((got.double() - whole.double()).abs().max())
        print(f"RECORD native session {label} {sr} C={Cn} {precision} strength={strength}: against the whole input {e:.3e}")
        assert e <= 2e-5
        if precision != "f32":
            w.set_precision("f32")
            e32 = float((got.double() - w.embed_native_batch(x, sr, msg, strength).double()).abs().max())
            print(f"RECORD native session {label} {sr} C={Cn} {precision}: against the EXACT whole input {e32:.3e}")
            assert e32 <= WM_BAR
        assert np.array_equal(bits(x), bits(keep))                          # the caller's audio is not written
        sess.reset()                                                        # a second run after reset(): the same bits
        assert np.array_equal(bits(run_session(sess, x)), bits(got))
        with pytest.raises(RuntimeError, match="flushed"):
            sess.push(x[:, :, :1])
        with pytest.raises(ValueError, match="expected new samples"):
            NS.NativeEmbedSession(gen, msg, sr, Cn, strength, precision).push(x[:, 0])
    finally:
        w.set_precision("f32")


@pytest.mark.parametrize("sr,Cn", [(48000, 2), (44100, 1)])
def test_route_is_its_parts_small_generator(small, sr, Cn):
    assert small.model.generator.cfg.hop_length <= 32
    check_route(small, sr, Cn, 9601, "f32", 1.0 if Cn == 2 else 0.5, "small generator")


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("sr,Cn", [(48000, 2), (44100, 1)])
def test_route_is_its_parts_full_size(wv, sr, Cn, precision):
    check_route(wv, sr, Cn, int(0.3 * sr), precision, 1.0, "full size")


def test_open_embed_session_api(wv):
    sess = wv.open_embed_session([1, 2], sample_rate=48000, channels=2, strength=0.5)
    assert isinstance(sess, NS.NativeEmbedSession) and sess.S == 2 and sess.latency_samples == 41 + 3 * (320 + 15)
    assert type(wv.open_embed_session([1, 2])) is EmbedSession and type(wv.open_detect_session(2)) is DetectSession
    assert type(wv.open_locate_session(2)) is LocateSession
    x = clip(48000, 2, 2, 2000)
    out = torch.cat([sess.push(x), sess.flush()], dim=2)
    assert tuple(out.shape) == (2, 2, 2000)
    with pytest.raises(ValueError, match="44101"):
        wv.open_embed_session(1, sample_rate=44101)


# ================================================================== 3. detect and locate
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_detect_and_locate_sessions_are_the_16k_sessions_behind_the_front_stage(wv, precision):
    sr, S, Cn, T = 44100, 2, 2, 13230
    x = clip(sr, S, Cn, T)
    x16 = wv.to_model_rate(x, sr)[:, 0]
    wv.set_precision(precision)
    try:
        for kind in ("detect", "locate"):
            nat = (wv.open_detect_session if kind == "detect" else wv.open_locate_session)(S, sample_rate=sr, channels=Cn)
            ref = (wv.open_detect_session if kind == "detect" else wv.open_locate_session)(S)
            assert isinstance(nat, NS.NativeDetectSession if kind == "detect" else NS.NativeLocateSession)
            plan = NS.StagePlan(*native.table_geometry(sr, M))
            a, r, at, at16 = [], [], 0, 0
            for n in pieces(T):
                a.append(nat.push(x[:, :, at:at + n]))
                k = plan.push(n).n_out
                r.append(ref.push(x16[:, at16:at16 + k]))
                at, at16 = at + n, at16 + k
            k = plan.flush().n_out
            last = ref.push(x16[:, at16:at16 + k])
            assert at16 + k == x16.shape[1]
            fa, fr = nat.flush(), ref.flush()
            if kind == "detect":
                assert fa.samples_seen == fr.samples_seen == x16.shape[1]
                assert np.array_equal(bits(fa.mean_prob), bits(fr.mean_prob)) and torch.equal(fa.bits, fr.bits)
                for u, v in zip(a, r):                                      # and every state on the way
                    assert u.samples_seen == v.samples_seen and np.array_equal(bits(u.mean_prob), bits(v.mean_prob))
            else:
                got, want = torch.cat(a + [fa], dim=2), torch.cat(r + [last, fr], dim=2)
                assert tuple(got.shape) == (S, 1, x16.shape[1]) and np.array_equal(bits(got), bits(want))
    finally:
        wv.set_precision("f32")
