"""Native-rate live sessions without a GPU (waveverify_amd/native_session.py): the integer plan and the session state
machine on the numpy stages in float64, chunked pushes plus flush EXACTLY equal to a plain whole-signal routine; the plan alone driven to 2^40
samples; the two exports; the defaults of open_*_session; the table-size refusal."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import native_cases as NC
from waveverify_amd import _lib, native
from waveverify_amd import native_session as NS
from waveverify_amd.session import NumpyArrays, StreamSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("wv_native_session_down", "wv_native_session_up_add")
RATES = [48000, 44100, 22050, 8000, 16000]
M = NC.MODEL_RATE
HOP, HALO = 16, 40
GAIN = 0.37


# ---- the whole-signal routine: per output, one multiply and one add per tap in ascending j, float64 ------------------------------------------
def whole_resample(sig: np.ndarray, of: int, nf: int, T_out: int) -> np.ndarray:
    k, orig, nw, L, width = NC.table(of, nf)
    m = np.arange(T_out)
    n, f = m // nw, m % nw
    z = np.zeros((sig.shape[0], width + max(sig.shape[1], (int(n[-1]) + 1) * orig + L if T_out else 0)), np.float64)
    z[:, width:width + sig.shape[1]] = sig
    acc = np.zeros((sig.shape[0], T_out), np.float64)
    k64 = k.astype(np.float64)
    for j in range(L):
        acc += k64[f, j] * z[:, n * orig + j]
    return acc


def whole_front(x: np.ndarray, sr: int) -> np.ndarray:
    mono = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        mono = mono + x[:, c]
    mono = mono / np.float64(x.shape[1])
    return whole_resample(mono, sr, M, NC.t16(x.shape[2], sr) if x.shape[2] else 0)


def model(win: np.ndarray) -> np.ndarray:
    """A pointwise 'generator residual': the same for a sample whatever window holds it, so chunking cannot show in it."""
    return 0.25 * win * win - 0.1 * win


def whole_embed(x: np.ndarray, sr: int) -> np.ndarray:
    u = whole_resample(model(whole_front(x, sr)), M, sr, x.shape[2])
    return x + np.float64(GAIN) * u[:, None, :]


def inner_session(S: int, forward):
    return StreamSession(S, HOP, HALO, forward, arrays=NumpyArrays(np.float64))


def schedules(sr: int):
    """The fixed list of push schedules (flush() follows each)."""
    orig, nw, L, width = native.table_geometry(sr, M)
    lat = NS.EmbedPlan(sr, HOP, HALO).latency_samples
    a, b = orig * HOP // 3, orig * HOP // 2
    return [("flush only", ()), ("one sample", (1,)), ("pushes of 0", (0, 5, 0, 0, orig + 3, 0)),
            ("fewer than width in total", (width // 2, max(0, width - 1 - width // 2))), ("exactly orig", (orig,)),
            ("one push longer than ten histories", (3, 10 * max(L, lat) + 7, 2)),
            ("ends on a hop multiple", (a, b, orig * HOP - a - b))]          # orig * HOP native samples are nw * HOP model samples


def signal(sr: int, S: int, Cn: int, T: int) -> np.ndarray:
    return np.random.default_rng([sr, S, Cn, T]).uniform(-NC.PEAK, NC.PEAK, (S, Cn, T))


@pytest.mark.parametrize("sr", RATES)
def test_embed_session_chunked_is_the_whole_signal_exactly(sr):
    for i, (name, sizes) in enumerate(schedules(sr)):
        S, Cn, T = 1 + i % 2, 1 + i % 3, sum(sizes)
        x = signal(sr, S, Cn, T)
        sess = NS.HostEmbedSession(inner_session(S, lambda win, keep: model(win[:, :, keep:])), sr, Cn, GAIN, dtype=np.float64)
        plan = sess._plan
        Lf, Lb = plan.front.L, plan.back.L
        outs, at = [], 0
        for n in sizes:
            outs.append(sess.push(x[:, :, at:at + n]))
            at += n
            assert outs[-1].shape[:2] == (S, Cn)
            assert plan.front.t_in - plan.front.h0 < Lf and plan.back.t_in - plan.back.h0 < Lb, name     # histories < L
            assert sess.samples_out <= sess.samples_in == at, name                                       # emitted <= received
            assert sess.samples_in - sess.samples_out < sess.latency_samples, name                       # the lag within the bound
            assert sess.samples_in - sess.samples_out <= plan.pcap, name
        outs.append(sess.flush())
        if name == "ends on a hop multiple":
            assert T and NC.t16(T, sr) % HOP == 0 and plan.ticker.t_in == NC.t16(T, sr)
        got = np.concatenate(outs, axis=2)
        assert got.shape == (S, Cn, T) and sess.samples_out == T, name
        if T:
            assert np.array_equal(got, whole_embed(x, sr)), f"{sr} {name}"
        with pytest.raises(RuntimeError, match="flushed"):
            sess.push(x[:, :, :0])
        with pytest.raises(RuntimeError, match="flushed"):
            sess.flush()
        sess.reset()                                                                                     # a reset session starts over
        if T:
            again = np.concatenate([sess.push(x), sess.flush()], axis=2)
            assert np.array_equal(again, got), name


class RecordingFront(NS.HostFrontSession):
    """Keeps what the front stage hands to the inner session."""

    def _down(self, x, t):
        y = super()._down(x, t)
        self.__dict__.setdefault("ys", []).append(y)
        return y


@pytest.mark.parametrize("sr", RATES)
def test_front_session_chunked_is_the_whole_front_exactly(sr):
    """Detect / locate sessions are the front stage before a 16 kHz session: what reaches the inner session, concatenated, is the whole
    recording at 16 kHz, and the inner session has seen all of it after flush()."""
    for i, (name, sizes) in enumerate(schedules(sr)):
        S, Cn, T = 1 + (i + 1) % 2, 1 + (i + 1) % 3, sum(sizes)
        x = signal(sr, S, Cn, T)
        sess = RecordingFront(inner_session(S, lambda win, keep: win[:, :, keep:]), sr, Cn, dtype=np.float64)
        at = 0
        for n in sizes:
            sess.push(x[:, :, at:at + n])
            at += n
            assert sess._plan.t_in - sess._plan.h0 < sess._plan.L and sess._plan.t_out <= sess._plan.total(), name
        flushed = sess.flush()
        n16 = NC.t16(T, sr) if T else 0
        assert sess._plan.t_out == n16 and sess.inner.samples_seen == n16, name
        if name == "ends on a hop multiple":
            assert flushed is None                                          # the inner flush had nothing left
        got = np.concatenate(sess.ys, axis=1)
        assert got.shape == (S, n16)
        if T:
            assert np.array_equal(got, whole_front(x, sr)), f"{sr} {name}"


def test_shape_errors():
    sess = NS.HostEmbedSession(inner_session(2, lambda win, keep: model(win[:, :, keep:])), 48000, 2, dtype=np.float64)
    for bad in (np.zeros((2, 5)), np.zeros((1, 2, 5)), np.zeros((2, 3, 5))):
        with pytest.raises(ValueError, match="expected new samples"):
            sess.push(bad)
    with pytest.raises(ValueError, match="channels"):
        NS.HostEmbedSession(inner_session(1, None), 48000, 65)


# ---- the plan alone, far past 2^31 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [48000, 44100, 8000])
def test_plan_to_2_pow_40_hands_kernels_small_numbers(sr):
    plan = NS.EmbedPlan(sr, 320, 4096)
    sizes = (1 << 26, 0, 1, (1 << 24) + 12345, 7, 959)
    lim, worst, i = 1 << 31, 0, 0
    while plan.t_in < 1 << 40:
        t = plan.push(sizes[i % len(sizes)])
        i += 1
        handed = [t.pv, t.pv2, t.n_res]
        for st in (t.front, t.back):
            handed += [st.hv, st.n, st.pad, st.n_out, st.drop, st.hv2]
        for tk in t.inner:
            handed += [tk.hv, tk.wlen, tk.keep, tk.drop, tk.hv2]
        assert min(handed) >= 0 and max(handed) < lim, (plan.t_in, t)
        worst = max(worst, max(handed))
        assert t.front.hv2 < plan.front.L and t.back.hv2 < plan.back.L and t.pv2 < plan.latency_samples
    assert plan.t_in >= 1 << 40 and plan.front.n_done * plan.front.orig > lim            # the positions themselves did pass 2^31
    t = plan.flush()
    assert plan.t_out == plan.t_in and t.pv2 == 0 and t.back.hv2 == 0 and t.front.hv2 == 0
    assert worst < lim


def test_latency_bound_is_the_issue_formula():
    for sr in RATES:
        plan = NS.EmbedPlan(sr, HOP)
        assert plan.latency_samples == plan.front.L + -(-(HOP + plan.back.L) * sr // M)
    assert NS.EmbedPlan(16000, HOP).latency_samples == HOP + 2


# ---- exports, defaults, refusals ---------------------------------------------------------------------------------------------------------
def test_exports_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    declared = set(re.findall(r"\b(wv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in EXPORTS:
        assert name in declared and name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is _lib.SIGNATURES[name][0] and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES[EXPORTS[0]][1]) == 19 and len(_lib.SIGNATURES[EXPORTS[1]][1]) == 26
    zero = {C.c_int: 0, C.c_float: 0.0}
    for name in EXPORTS:                                                    # all-null, all-zero calls never reach a launch
        assert getattr(lib, name)(*[zero.get(t) for t in _lib.SIGNATURES[name][1]]) == -1
        assert name in lib.wv_last_error().decode()


def test_open_session_defaults_return_the_present_classes():
    from waveverify_amd import WaveVerify, session

    class Net:
        device = "cpu"

    made = []
    wv = WaveVerify.__new__(WaveVerify)
    wv.sample_rate, wv.watermark_bits = 16000, 16
    wv.generator_precision = wv.detector_precision = wv.locator_precision = "f32"
    wv._need = lambda name: Net()
    wv._messages = lambda ids: "msg"
    orig = {}
    for cls in ("EmbedSession", "DetectSession", "LocateSession"):
        orig[cls] = getattr(session, cls)
    try:
        for cls in orig:
            setattr(session, cls, type(cls, (), {"__init__": lambda self, *a, _c=cls, **k: made.append((_c, a[1:], k))}))
        assert type(wv.open_embed_session(5)).__name__ == "EmbedSession"
        assert type(wv.open_detect_session()).__name__ == "DetectSession" and type(wv.open_detect_session(3)).__name__ == "DetectSession"
        assert type(wv.open_locate_session(2)).__name__ == "LocateSession"
        assert made == [("EmbedSession", ("msg", "f32"), {}), ("DetectSession", (1, "f32"), {}), ("DetectSession", (3, "f32"), {}),
                        ("LocateSession", (2, "f32"), {})]
    finally:
        for cls, c in orig.items():
            setattr(session, cls, c)
    for fn, names in ((WaveVerify.open_embed_session, ["watermark_ids", "sample_rate", "channels", "strength"]),
                      (WaveVerify.open_detect_session, ["n", "sample_rate", "channels"]), (WaveVerify.open_locate_session, ["n", "sample_rate", "channels"])):
        p = inspect.signature(fn).parameters
        assert list(p)[1:] == names
        assert p["sample_rate"].default == 16000 and p["channels"].default == 1
    assert inspect.signature(WaveVerify.open_embed_session).parameters["strength"].default == 1.0
    for name in ("NativeEmbedSession", "NativeDetectSession", "NativeLocateSession"):
        assert inspect.isclass(getattr(NS, name))


def test_rates_whose_table_passes_16_mb_are_refused_as_for_files():
    wv_cls = __import__("waveverify_amd").WaveVerify
    wv = wv_cls.__new__(wv_cls)
    wv.sample_rate = 16000
    wv.generator_precision = wv.detector_precision = wv.locator_precision = "f32"

    class Net:
        device = "cpu"
    wv._need = lambda name: Net()
    wv._messages = lambda ids: np.zeros((1, 16), np.float32)
    with pytest.raises(ValueError, match="44101") as e_file:
        native.check_rate(44101)
    for open_ in (lambda: wv.open_embed_session(5, sample_rate=44101, channels=2), lambda: wv.open_detect_session(1, sample_rate=44101),
                  lambda: wv.open_locate_session(1, 44101, 2), lambda: NS.EmbedPlan(44101, HOP),
                  lambda: NS.HostEmbedSession(inner_session(1, None), 44101, 2)):
        with pytest.raises(ValueError, match="44101") as e:
            open_()
        assert str(e.value) == str(e_file.value)
