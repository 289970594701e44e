"""The per-channel SNR floor on the CPU (tests/channel_floor_cases.py; waveverify_amd/channel_floor.py): the frame
map; the twin on one channel at 16 kHz is snr_floor.floor_row bit for bit; the generalised energy is snr_floor.frame_energy on equal frames;
the per-channel, per-native-frame bound in float64 on every case, no weight above its frame's gain; a silent channel and a frame of u == 0
come back bit for bit; the export is declared, listed, bound, documented and refuses by name; the switch validates like check_db, refuses
the live native openers, and leaves the pinned signatures alone.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import channel_floor_cases as CC
import window_cases as W
from waveverify_amd import channel_floor as CF
from waveverify_amd import snr_floor as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u_of(c, delta):
    """A residual at the native rate for the twin: the float64 restatement of the back end, rounded to f32 (the guarantee holds whatever u is)."""
    return CC.up64(delta, c[1], c[5]).astype(np.float32)


# ---- the frame map ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [48000, 44100, 11025, 8000, 16000, 22050, 96000])
@pytest.mark.parametrize("hop", [1, 3, 4, 7, 12, 320])
def test_frame_map_is_monotone_covers_the_row_and_lengths_differ_by_at_most_one(sr, hop):
    orig, nw, _, _ = CC.geometry(sr)
    for Tn in (1, 2, 37, 1000, 4 * 960 + 7):
        m = np.arange(Tn)
        f = CF.frame_of(m, orig, nw, hop)
        st = CF.frame_starts(Tn, orig, nw, hop)
        F = len(st) - 1
        assert f[0] == 0 and f[-1] == F - 1 and (np.diff(f) >= 0).all()
        assert st[0] == 0 and st[F - 1] <= Tn - 1 < st[F]                   # every sample has a frame and the last frame holds one
        assert np.array_equal(f, np.searchsorted(st, m, side="right") - 1)  # frame f is exactly [start(f), start(f + 1))
        lens = np.diff(st)
        assert lens.max() - lens.min() <= 1 and lens.max() == -(-(nw * hop) // orig)
        if (hop * nw) % orig == 0:
            assert np.array_equal(f, m // (hop * nw // orig)) and lens.min() == lens.max()
    shapes = {48000: {960}, 44100: {882}, 11025: {220, 221}, 8000: {160}, 16000: {320}}
    if hop == 320 and sr in shapes:
        assert set(np.diff(CF.frame_starts(100000, orig, nw, hop))) == shapes[sr]
    if sr == 8000 and hop in (1, 3, 4, 7):
        assert set(np.diff(CF.frame_starts(1000, orig, nw, hop))) == {1: {0, 1}, 3: {1, 2}, 4: {2}, 7: {3, 4}}[hop]


# ---- one definition, one fixed point ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 3, 12, 63, 64, 65, 320])
def test_the_twin_at_16k_on_one_channel_is_the_16k_floor_and_the_energy_is_frame_energy(L):
    rng = np.random.default_rng(W.seed_of("channel floor fixed point", L))
    for n in (1, L, 3 * L + L // 2, 9 * L + 1):
        f = np.arange(n) // L
        F = f[-1] + 1
        x = (rng.standard_normal(n) * np.exp(rng.uniform(np.log(1e-3), 0, F))[f]).astype(np.float32)
        r = (rng.standard_normal(n) * np.exp(rng.uniform(np.log(1e-2), np.log(0.3), F))[f]).astype(np.float32)
        if F >= 4:
            x[L:2 * L] = 0.0
            r[2 * L:3 * L] = 0.0
        st = CF.frame_starts(n, 1, 1, L)
        assert np.array_equal(st, np.arange(F + 1) * L)
        assert np.array_equal(CF.frame_energy_var(x, st), SF.frame_energy(x, L))
        for s in (1.0, 0.75, 0.0):
            for add in (True, False):
                for db in CC.FLOORS:
                    want, g = SF.floor_row(x, r, s, SF.rho_of(db), SF.floor_ramp(L), None, add)
                    got, gg = CF.numpy_channel_floor(x[None], r, 1, 1, L, s, SF.rho_of(db), add)
                    assert np.array_equal(got[0].view(np.int32), want.view(np.int32)) and np.array_equal(gg[0].view(np.int32), g.view(np.int32))


def test_the_generalised_energy_keeps_the_order_written_down_on_unequal_frames():
    rng = np.random.default_rng(W.seed_of("channel floor order"))
    a = (rng.standard_normal(2000) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
    st = CF.frame_starts(2000, 640, 441, 320)                              # 220 / 221
    got = CF.frame_energy_var(a, st)
    for f in range(len(got)):
        p = [0.0] * 16
        for k, v in enumerate(a[st[f]:min(st[f + 1], 2000)]):
            p[(k >> 2) & 15] += float(v) * float(v)
        for h in (8, 4, 2, 1):
            p = [p[j] + p[j + h] for j in range(h)]
        assert got[f] == p[0], f
    e = lambda v: SF.frame_energy(v, 8)[0]                                     # noqa: E731
    assert np.array_equal(CF.frame_energy_var(a[:5], np.array([0, 0, 3, 3, 9])), [0.0, e(a[:3]), 0.0, e(a[3:5])])      # empty frames give 0


# ---- the guarantee ----------------------------------------------------------------------------------------------------------------------------
def test_per_channel_per_native_frame_bound_and_weight_never_above_the_gain():
    """In float64, per channel and native frame, 10 log10(Ex / sum v^2) >= min_snr_db - BOUND_DB (derived in channel_floor_cases.py: one f32
    rounding of the gain and one of each product, counted at a whole unit in the last place)."""
    worst, kinds = np.inf, set()
    for c in CC.CASES:
        name, sr, hop, Cn, B, Tn, silent, _ = c
        orig, nw, _, _ = CC.geometry(sr)
        x, delta, s = CC.inputs(c)
        st = CF.frame_starts(Tn, orig, nw, hop)
        f = CF.frame_of(np.arange(Tn), orig, nw, hop)
        for db in CC.FLOORS:
            rho = SF.rho_of(db)
            for b in range(B):
                u = u_of(c, delta[b])
                v, g = CF.numpy_channel_floor(x[b], u, orig, nw, hop, s[b], rho, add=False)
                assert g.shape == (Cn, len(st) - 1) and (g <= s[b]).all() and (g >= 0).all()
                assert (np.abs(v) <= np.abs(g[:, f] * u[None])).all(), name         # w <= g[f]: the product is monotone in w
                for ch in range(Cn):
                    snr = CF.native_frame_snr_db(x[b, ch], v[ch], orig, nw, hop)
                    worst = min(worst, float((snr - db).min()))
                    assert (snr >= db - CC.BOUND_DB).all(), (name, db, b, ch, float((snr - db).min()))
                if db == CC.MIN_SNR_DB:
                    kinds |= CC.kinds_of(g, CF.frame_energy_var(u, st), s[b])
    assert kinds == {"capped", "uncapped", "rising", "falling", "u=0"}, kinds
    print(f"CHANNEL FLOOR bound: worst frame {worst:.2e} dB against the floor (bar -{CC.BOUND_DB:.2e})")


def test_a_silent_channel_and_a_frame_without_residual_come_back_bit_for_bit():
    rho = SF.rho_of(CC.MIN_SNR_DB)
    seen = set()
    for c in CC.CASES:
        name, sr, hop, Cn, B, Tn, silent, sign = c
        orig, nw, _, _ = CC.geometry(sr)
        x, delta, s = CC.inputs(c)
        st = np.minimum(CF.frame_starts(Tn, orig, nw, hop), Tn)
        for b in range(B):
            u = u_of(c, delta[b])
            out, g = CF.numpy_channel_floor(x[b], u, orig, nw, hop, s[b], rho)
            if silent is not None:
                assert np.array_equal(out[silent].view(np.int32), x[b, silent].view(np.int32)), name
                assert np.signbit(out[silent]).all() == bool(sign)
                seen.add("-0" if sign else "+0")
                if s[b] > 0 and Tn > 1:                                        # ... while a channel with a programme carries the watermark
                    loud = (silent + 1) % Cn
                    assert not np.array_equal(out[loud], x[b, loud]), name
            for fi, (a, e) in enumerate(zip(st[:-1], st[1:])):
                if e > a and not u[a:e].any():
                    seen.add("u=0")
                    assert (g[:, fi] == s[b]).all() and np.array_equal(out[:, a:e].view(np.int32), x[b][:, a:e].view(np.int32)), (name, fi)
    assert seen == {"+0", "-0", "u=0"}, seen


def test_the_case_list_is_the_issues():
    rates = {c[1] for c in CC.CASES}
    assert rates == {48000, 44100, 11025, 8000, 16000}
    assert {c[2] for c in CC.CASES if c[1] == 8000} >= {1, 3, 4, 7} and all(any(c[1] == r and c[2] == 320 for c in CC.CASES) for r in rates)
    assert {c[3] for c in CC.CASES} == {1, 2, 3, 64} and {c[4] for c in CC.CASES} == {1, 5}
    ends = set()
    for name, sr, hop, Cn, B, Tn, _, _ in CC.CASES:
        orig, nw, _, _ = CC.geometry(sr)
        st = CF.frame_starts(Tn, orig, nw, hop)
        ends.add("one" if Tn == 1 else "short" if len(st) == 2 and Tn < st[1] else "whole" if st[-1] == Tn else "inside")
    assert ends == {"one", "short", "whole", "inside"}, ends
    assert any(s == 0 for s in CC.STRENGTHS5)
    for c in CC.CASES:
        x, delta, s = CC.inputs(c)
        for a in (x, delta):
            nz = np.abs(a[a != 0])
            assert nz.size == 0 or nz.min() > 1e-12                           # far above the f32 denormal range (1.2e-38), squares included


# ---- the export -------------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_listed_bound_and_refuses_by_name():
    from waveverify_amd import _lib
    from waveverify_amd.build import SOURCES
    assert "wv_channel_floor.hip" in SOURCES
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("wv_native_floor_up_add", "wv_native_floor_up_add_bytes"):
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert proto, f"{name} is not declared"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(proto.group(1).split(","))
        assert name in doc
    lim = re.search(r"#define\s+WV_CHANNEL_FLOOR_MAX_FRAME\s+(\d+)", header)
    lds = re.search(r"#define\s+WV_CHANNEL_FLOOR_LDS_FLOATS\s+(\d+)", header)
    assert lim and int(lim.group(1)) == CF.MAX_FRAME and lds and int(lds.group(1)) == CF.LDS_FLOATS
    lib = _lib.load()
    # addresses that a refusal never follows: every call below is refused before anything is launched
    buf = (C.c_float * 1024)()
    at = lambda k: C.addressof(buf) + 4 * k                                    # noqa: E731
    base = (C.addressof(buf) + 255) // 256 * 256                              # a 256-byte boundary inside buf for the workspace
    ok = dict(x=at(0), delta=at(64), kt=at(96), out=at(128), B=1, C=2, T16=11, Tn=32, orig=1, nw=3, L=15, width=7, hop=4, rho=0.01, s=at(200),
              add=1, gains=None, ws=base + 1024, ws_bytes=2048)
    call = lambda a: lib.wv_native_floor_up_add(a["x"], a["delta"], a["kt"], a["out"], a["B"], a["C"], a["T16"], a["Tn"], a["orig"], a["nw"],   # noqa: E731
                                                a["L"], a["width"], a["hop"], a["rho"], a["s"], a["add"], a["gains"], a["ws"], a["ws_bytes"], None)
    need = C.c_size_t(0)
    size = lambda a, p=None: lib.wv_native_floor_up_add_bytes(a["B"], a["C"], a["T16"], a["Tn"], a["orig"], a["nw"], a["L"], a["width"],       # noqa: E731
                                                              a["hop"], C.byref(need) if p is None else p)
    assert size(ok) == 0 and need.value == 256 + 256                           # u [1][32] and g [1][2][3], each rounded up to 256 bytes
    assert ok["ws_bytes"] >= need.value
    shared = (("B < 1", dict(B=0)), ("B > 65535", dict(B=65536)), ("C < 1", dict(C=0)), ("C > 64", dict(C=65)), ("T16 < 1", dict(T16=0)),
              ("Tn < 1", dict(Tn=0)), ("orig < 1", dict(orig=0)), ("nw < 1", dict(nw=0)), ("L < 1", dict(L=0)), ("width < 0", dict(width=-1)),
              ("output longer than the resampler gives", dict(Tn=37)), ("a window beyond 64 KB", dict(orig=20000, L=20014, Tn=1)),
              ("hop < 1", dict(hop=0)), ("hop < 0", dict(hop=-3)), ("nw * hop beyond 2^31 - 1", dict(hop=1 << 30)),
              ("a frame beyond the limit", dict(hop=(CF.MAX_FRAME + 1) // 3 + 1)),
              ("a frame that with its window passes the LDS budget", dict(orig=6000, nw=6001, L=6014, hop=4000, T16=6000, Tn=6001)))
    only_call = (("null x", dict(x=None)), ("null delta", dict(delta=None)), ("null kernels_t", dict(kt=None)), ("null out", dict(out=None)),
                 ("null strengths", dict(s=None)), ("null workspace", dict(ws=None)), ("rho = 0", dict(rho=0.0)), ("rho < 0", dict(rho=-1.0)),
                 ("rho = nan", dict(rho=float("nan"))), ("rho = inf", dict(rho=float("inf"))), ("add = 2", dict(add=2)), ("add = -1", dict(add=-1)),
                 ("a misaligned workspace", dict(ws=base + 1028)), ("a workspace too small", dict(ws_bytes=511)))
    for why, kw in shared + only_call:
        assert call({**ok, **kw}) == -1, why
        assert lib.wv_last_error().decode().startswith("wv_native_floor_up_add:"), why
    for why, kw in shared:
        need.value = 12345
        assert size({**ok, **kw}) == -1 and need.value == 12345, why
        assert lib.wv_last_error().decode().startswith("wv_native_floor_up_add_bytes:"), why
    assert size(ok, C.POINTER(C.c_size_t)()) == -1
    assert not any(buf)


# ---- the switch -------------------------------------------------------------------------------------------------------------------------------
def _bare():
    from waveverify_amd import WaveVerify
    wv = WaveVerify.__new__(WaveVerify)
    wv.sample_rate = WaveVerify.DEFAULT_SAMPLE_RATE
    return wv


def test_set_channel_snr_floor_validates_like_check_db():
    wv = _bare()
    assert wv.channel_snr_floor_db is None and wv.snr_floor_db is None
    wv.set_channel_snr_floor(20)
    assert wv.channel_snr_floor_db == 20.0 and isinstance(wv.channel_snr_floor_db, float) and wv.snr_floor_db is None
    for bad in (float("nan"), float("inf"), -float("inf"), "loud", True, [20.0]):
        with pytest.raises(ValueError):
            wv.set_channel_snr_floor(bad)
        assert wv.channel_snr_floor_db == 20.0                                 # a refusal changes nothing
    wv.set_channel_snr_floor(np.float32(-3.0))
    assert wv.channel_snr_floor_db == -3.0
    wv.set_channel_snr_floor(None)
    assert wv.channel_snr_floor_db is None


def test_the_live_native_openers_are_refused_under_a_channel_floor():
    wv = _bare()
    wv.set_channel_snr_floor(30.0)
    for kw in (dict(sample_rate=48000, channels=2), dict(sample_rate=44100), dict(channels=2), dict(strength=0.5)):
        with pytest.raises(ValueError, match=r"set_channel_snr_floor\(None\)"):
            wv.open_embed_session([1, 2], **kw)
    with pytest.raises(ValueError, match=r"set_channel_snr_floor\(None\)"):
        wv.open_embed_bank(rates=(48000, 8000))
    with pytest.raises(ValueError, match=r"set_channel_snr_floor\(None\)"):
        wv.open_embed_bank(capacity=4, rates=(44100,), max_channels=6)


def test_upsample_add_floor_refuses_before_anything_runs():
    import torch
    from waveverify_amd import native
    x, d = torch.zeros(1, 2, 96), torch.zeros(1, 1, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.upsample_add_floor(x, d, 48000, 20.0)                           # a CPU tensor
    for bad in (dict(strength=-1.0), dict(strength=float("nan")), dict(strength=[1.0, 1.0]), dict(hop=0), dict(min_snr_db=None),
                dict(min_snr_db=float("inf"))):
        with pytest.raises(ValueError):
            native.upsample_add_floor(x, d, 48000, **{"min_snr_db": 20.0, **bad})


def test_pinned_signatures_are_unchanged():
    from waveverify_amd import WaveVerify, native
    from waveverify_amd.native_bank import NativeEmbedBank
    from waveverify_amd.session import EmbedBank
    sig = lambda fn: list(inspect.signature(fn).parameters)                    # noqa: E731
    assert sig(WaveVerify.set_channel_snr_floor) == ["self", "min_snr_db"] and sig(WaveVerify.set_snr_floor) == ["self", "min_snr_db"]
    assert sig(WaveVerify.embed_native_batch) == ["self", "audio", "sample_rate", "message", "strength", "window_seconds"]
    assert sig(WaveVerify.embed_spans_native_batch) == ["self", "audio", "sample_rate", "spans", "strength", "fade_samples", "window_seconds"]
    assert sig(WaveVerify.open_embed_bank) == ["self", "capacity", "pad_limit", "rates", "max_channels"]
    assert sig(WaveVerify.open_embed_session) == ["self", "watermark_ids", "sample_rate", "channels", "strength"]
    assert sig(WaveVerify.embed) == ["self", "audio_path", "watermark_id", "output_path", "native", "strength", "window_seconds"]
    assert sig(WaveVerify.embed_spans) == ["self", "audio_path", "spans", "output_path", "native", "strength", "fade_ms", "window_seconds"]
    assert sig(EmbedBank.set_snr_floor) == ["self", "min_snr_db"] and sig(NativeEmbedBank.set_snr_floor) == ["self", "min_snr_db"]
    assert sig(native.upsample_add) == ["audio", "delta", "sample_rate", "gain", "out"]
    p = inspect.signature(native.upsample_add_floor).parameters
    assert list(p) == ["audio", "delta", "sample_rate", "min_snr_db", "strength", "hop", "add", "return_gains", "out"]
    assert (p["strength"].default, p["hop"].default, p["add"].default, p["return_gains"].default, p["out"].default) == (1.0, 320, True, False, None)
    assert list(inspect.signature(SF.apply).parameters) == ["x", "residual", "min_snr_db", "strength", "frame", "add", "return_gains"]
