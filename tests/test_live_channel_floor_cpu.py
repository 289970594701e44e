"""The live per-channel SNR floor without a GPU (waveverify_amd/native_bank.py, native_session.EmbedPlan): the plan's
emission rule on integers alone to 2^40 samples; HostEmbedBank on float32 arrays with a toy causal inner bank under the floor, every stream's
concatenated output and gains ARRAY-EQUAL to channel_floor.numpy_channel_floor on its whole input and the whole residual through
numpy_resample; a silent channel back bit for bit and the loud one inside the bound; slot reuse over poisoned state; the half bits; the floor off
is today's bank; both floors; the row rule clause by clause; the export; the opener."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import channel_floor_cases as CFC
import live_channel_floor_cases as LC
import native_bank_cases as NBC
from waveverify_amd import _lib, native
from waveverify_amd import channel_floor as CF
from waveverify_amd import native_bank as NB
from waveverify_amd import native_session as NS
from waveverify_amd.session import NumpyArrays, StreamBank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORT = "wv_native_bank_floor_up_add"
F32 = np.float32


def model(win: np.ndarray) -> np.ndarray:
    """A pointwise 'generator residual' (tests/test_native_bank_cpu.py's), in the window's own dtype."""
    return (0.25 * win * win - 0.1 * win).astype(win.dtype)


class ToyBank(StreamBank):
    """A causal 16 kHz inner bank on float32 arrays that keeps every slot's residual as it returned it."""

    def __init__(self, capacity, hop, scaled=False):
        super().__init__(capacity, hop, LC.HALO, self._fwd, arrays=NumpyArrays(F32))
        self.res = {}
        if scaled:                                                            # what native_bank looks for in a bank under the 16 kHz floor
            self.snr_floor_db, self._strength = 30.0, np.ones(capacity, F32)

    def _fwd(self, win, slots):
        y = model(win)
        return y * self._strength[slots][:, None, None] if hasattr(self, "_strength") else y

    def _on_open(self, slot, *message):
        self.res[slot] = []

    def _log(self, slot, v):
        if v is not None:
            self.res[slot].append(np.asarray(v, F32).reshape(-1))
        return v

    def push(self, items):
        out = super().push(items)
        for s in items:
            self._log(s, out[s])
        return out

    def close(self, slot):
        return self._log(slot, super().close(slot))

    def residual(self, slot):
        return np.concatenate(self.res[slot] + [np.zeros(0, F32)])


def embed_bank(rates, hop, capacity, floor=LC.MIN_SNR_DB, scaled=False):
    bank = NB.HostEmbedBank(ToyBank(capacity, hop, scaled), rates, LC.MAX_CHANNELS, dtype=F32)
    if floor is not None:
        bank.set_channel_snr_floor(floor)
    return bank


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def play(bank, streams, after=None):
    """streams {name: (sr, C, strength, sizes, x)}: all open, tick j pushes every stream's j-th size, a stream closes on the tick after its last
    push -> {name: (out [C, T], gains [C, F], residual, [emitted per tick])}."""
    slot = {n: bank.open(None, sample_rate=v[0], channels=v[1], strength=v[2]) for n, v in streams.items()}
    at = {n: 0 for n in streams}
    outs, gains, counts, res = ({n: [] for n in streams} for _ in range(4))
    j, live = 0, set(streams)
    while live:
        push = {n: streams[n][3][j] for n in live if j < len(streams[n][3])}
        if push:
            got = bank.push({slot[n]: streams[n][4][:, at[n]:at[n] + k] for n, k in push.items()})
            for n, k in push.items():
                at[n] += k
                outs[n].append(got[slot[n]])
                gains[n].append(bank.gains(slot[n]))
                counts[n].append(got[slot[n]].shape[1])
                assert bank.samples_in(slot[n]) - bank.samples_out(slot[n]) < bank.latency_samples(slot[n]), n
                assert got[slot[n]].dtype == F32 and bank.gains(slot[n]).shape[0] == streams[n][1]
            if after:
                after([slot[n] for n in push])
        for n in sorted(live - set(push)):
            last = bank.close(slot[n])
            outs[n].append(last)
            gains[n].append(bank.gains(slot[n]))
            counts[n].append(last.shape[1])
            res[n] = bank.inner.residual(slot[n])
            live.discard(n)
            if after:
                after([slot[n]])
        j += 1
    return {n: (np.concatenate(outs[n], axis=1), np.concatenate(gains[n], axis=1), res[n], counts[n]) for n in streams}


def geometry_streams(sr, hop, seed=0):
    streams = {}
    for i, (name, sizes) in enumerate(LC.schedules(sr, hop)):
        Cn = 1 + i % 3
        streams[name] = (sr, Cn, (1.0, 0.75)[i % 2], sizes, LC.stream_x(sr, hop, Cn, sum(sizes), [seed, i], silent=1 if Cn == 2 else None))
    return streams


def check_streams(got, streams, hop, cap=None):
    kinds = set()
    for n, (sr, Cn, s, sizes, x) in streams.items():
        out, g, r, counts = got[n]
        assert out.shape == x.shape, n
        u = LC.whole_u(r, sr, x.shape[1])
        want, wg = LC.twin(x, u, sr, hop, s if cap is None else cap)
        assert same(out, want), (n, "not the twin's output")
        assert same(g, wg), (n, "not the twin's gains")
        if x.shape[1]:
            orig, nw = LC.back(sr)[:2]
            st = CF.frame_starts(x.shape[1], orig, nw, hop)
            kinds |= CFC.kinds_of(wg, CF.frame_energy_var(u, st), F32(s))
            v = CF.numpy_channel_floor(x, u, orig, nw, hop, s if cap is None else cap, LC.RHO, add=False)[0]
            assert same(out, np.where(v == 0, x, x + v))                      # v is the watermark this output carries
            for c in range(Cn):
                if not x[c].any():
                    assert np.array_equal(bits(out[c]), bits(x[c])), (n, "a silent channel changed")      # +0 and -0 alike
                else:
                    snr = CF.native_frame_snr_db(x[c], v[c], orig, nw, hop)
                    assert (snr >= LC.MIN_SNR_DB - CFC.BOUND_DB).all(), (n, c, snr.min())
    return kinds


# ---- the plan: integers only ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,hop", LC.GEOMETRIES + ((8000, 3), (192000, 320)), ids=LC.GEO_IDS + ["8000.hop3", "192000.hop320"])
def test_the_plan_holds_whole_frames_and_stays_inside_its_lag_to_2_40_samples(sr, hop):
    rng = np.random.default_rng([sr, hop])
    p, q = NS.EmbedPlan(sr, hop, LC.HALO, True), NS.EmbedPlan(sr, hop, LC.HALO)
    orig, nw = p.back.orig, p.back.nw
    Lf = -(-nw * hop // orig)
    assert p.latency_samples == q.latency_samples + Lf and p.pcap == p.latency_samples and p.ucap == Lf
    start = lambda f: -(-f * nw * hop // orig)                                # noqa: E731
    small = [0, 1, 2, Lf - 1, Lf, Lf + 1, 3 * Lf + 1, 1000]
    empties = 0
    for i in range(6000):
        n = int(rng.choice(small)) if i % 50 else int(rng.integers(1, 2 ** 35))
        if p.t_in + n > 2 ** 40:
            break
        t, t0 = p.push(n), q.push(n)
        fl = t.floor
        assert t.back == t0.back and t.front == t0.front                      # the back StagePlan stays as it is
        assert p.t_out <= p.back.t_out <= p.t_in                              # emitted <= u available <= received
        assert 0 <= fl.uv2 == p.back.t_out - p.t_out < Lf and fl.uv + t.back.n_out == fl.k + fl.uv2
        assert p.t_in - p.t_out < p.latency_samples and t.pv2 == p.t_in - p.t_out <= p.pcap and t.pv + n - fl.k == t.pv2
        assert fl.nf >= 0 and fl.k == start(fl.f0 + fl.nf) - start(fl.f0) and p.t_out == start(p.frames) and fl.f0 + fl.nf == p.frames
        # the emission rule: start(Fd) samples have left, Fd the largest f with start(f) <= t_u
        Fd = p.back.t_out * orig // (nw * hop)
        assert start(Fd) == p.t_out and start(Fd + 1) > p.back.t_out and p.frames <= Fd
        empties += Fd - p.frames
        assert p.frames == (0 if p.t_out == 0 else ((p.t_out - 1) * orig) // (nw * hop) + 1)
    assert p.t_in > 2 ** 39 and (empties > 0) == (nw * hop < orig)
    t = p.flush()
    q.flush()
    assert p.t_out == p.t_in == q.t_out and t.floor.uv2 == 0 and t.pv2 == 0 and t.floor.uv + t.back.n_out == t.floor.k
    assert t.floor.f0 + t.floor.nf == ((p.t_in - 1) * orig) // (nw * hop) + 1 and t.final
    empty = NS.EmbedPlan(sr, hop, LC.HALO, True).flush()
    assert (empty.floor.f0, empty.floor.nf, empty.floor.k, empty.floor.uv, empty.floor.uv2) == (0, 0, 0, 0, 0)


# ---- the state machine ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,hop", LC.GEOMETRIES, ids=LC.GEO_IDS)
def test_every_stream_is_the_twin_on_its_whole_recording(sr, hop):
    streams = geometry_streams(sr, hop)
    bank = embed_bank((sr,), hop, len(streams))
    got = play(bank, streams)
    kinds = check_streams(got, streams, hop)
    assert {"capped", "uncapped", "rising", "falling"} <= kinds, kinds
    assert got["close only"][0].shape == (1, 0) and got["close only"][1].shape == (1, 0)
    assert (0 in got["dribble"][3][1:-1] or hop == 1) and max(got["dribble"][3][1:-1]) > 0      # some ticks emit nothing, some a frame
    assert bank.open_slots() == [] and bank.stats["front_launches"] == bank.stats["back_launches"] == bank.stats["uploads"] == bank.stats["ticks"]
    if (sr, hop) == (8000, 1):
        assert (got["long"][1][:, 1::2] == F32(streams["long"][2])).all()     # the empty frames: the cap


def mixed_streams(seed=0):
    steps, who = LC.mixed()
    T = NBC.BC.stream_lengths(steps)
    xs = {n: LC.stream_x(who[n][0], LC.MIX_HOP, who[n][1], T[n], [seed, i], silent=1 if who[n][1] == 2 and i % 2 == 0 else None)
          for i, n in enumerate(T)}
    return steps, who, xs


def run_mixed(bank, steps, who, xs, strengths, after=None):
    """-> {stream: (out, gains, residual)}; slots are reused, so a stream's residual is read as it closes."""
    slot, pos, outs, gains, res = {}, {}, {}, {}, {}
    for kind, arg in steps:
        if kind == "open":
            slot[arg], pos[arg], outs[arg], gains[arg] = bank.open(None, sample_rate=who[arg][0], channels=who[arg][1], strength=strengths[arg]), 0, [], []
        elif kind == "close":
            outs[arg].append(bank.close(slot[arg]))
            gains[arg].append(bank.gains(slot[arg]))
            res[arg] = bank.inner.residual(slot[arg])
            if after:
                after([slot[arg]])
        else:
            got = bank.push({slot[n]: xs[n][:, pos[n]:pos[n] + k] for n, k in arg.items()})
            for n, k in arg.items():
                pos[n] += k
                outs[n].append(got[slot[n]])
                gains[n].append(bank.gains(slot[n]))
            if after:
                after([slot[n] for n in arg])
    return {n: (np.concatenate(outs[n], axis=1), np.concatenate(gains[n], axis=1), res[n], None) for n in outs}


def test_the_mixed_schedule_over_five_rates_and_the_half_bits():
    steps, who, xs = mixed_streams()
    strengths = {n: (1.0, 0.37)[i % 2] for i, n in enumerate(who)}
    bank = embed_bank(LC.MIX_RATES, LC.MIX_HOP, NBC.BC.CAPACITY)
    prev, ticks = [list(bank._half)], [0]

    def after(slots):
        assert bank._half == [h ^ (s in slots) for s, h in enumerate(prev[0])], slots
        prev[0] = list(bank._half)
        ticks[0] += 1
    got = run_mixed(bank, steps, who, xs, strengths, after)
    check_streams(got, {n: (who[n][0], who[n][1], strengths[n], None, xs[n]) for n in xs}, LC.MIX_HOP)
    assert ticks[0] == bank.stats["ticks"] > 10 and 0 < sum(prev[0]) < 6


def test_a_reopened_slot_reads_nothing_its_last_stream_left():
    a, b = LC.stream_x(48000, 16, 2, 3000, 5), LC.stream_x(8000, 16, 3, 700, 6)

    def second(bank):
        s = bank.open(None, sample_rate=8000, channels=3, strength=0.37)
        parts = [bank.push({s: b[:, :300]})[s], bank.push({s: b[:, 300:]})[s]]
        g = [bank.gains(s)]
        parts.append(bank.close(s))
        return s, np.concatenate(parts, axis=1), np.concatenate(g + [bank.gains(s)], axis=1)
    used = embed_bank((48000, 8000), 16, 2)
    s = used.open(None, sample_rate=48000, channels=2)
    used.push({s: a[:, :1700]})
    used.push({s: a[:, 1700:2990]})
    for state in (used._rhist, used._pend, used._uhold, used._gprev):
        assert np.abs(state[s]).max() > 0                                     # the first stream did leave state in the slot, in all four
    used.close(s)
    for state in (used._hist, used._rhist, used._pend, used._uhold, used._gprev):
        state[:] = np.nan                                                     # both halves, every slot
    s2, got, g2 = second(used)
    s3, want, g3 = second(embed_bank((48000, 8000), 16, 2))
    assert s2 == s3 == s and got.shape == b.shape and not np.isnan(got).any() and same(got, want) and same(g2, g3) and g2.shape[1] > 10


def test_the_floor_off_is_todays_bank_and_the_setter_is_legal_only_before_the_first_open():
    steps, who, xs = mixed_streams(seed=3)
    plain = embed_bank(LC.MIX_RATES, LC.MIX_HOP, NBC.BC.CAPACITY, floor=None)
    offed = embed_bank(LC.MIX_RATES, LC.MIX_HOP, NBC.BC.CAPACITY)             # set, then switched off again
    offed.set_channel_snr_floor(None)
    assert offed.channel_snr_floor_db is None and offed._pend.shape == plain._pend.shape and not hasattr(plain, "_uhold")
    with pytest.raises(RuntimeError, match="set_channel_snr_floor"):
        plain.gains(0)
    logs = []
    for bank in (plain, offed):
        out, _ = NBC.run(bank, steps, xs, who, open_args=lambda n: (None,))
        logs.append(out)
        assert bank.latency_samples(bank.open(None, sample_rate=48000)) == NS.EmbedPlan(48000, LC.MIX_HOP, LC.HALO).latency_samples
    for n in logs[0]:
        for (_, _, g), (_, _, w) in zip(logs[0][n], logs[1][n]):
            assert same(g, w), n
    assert plain.stats == offed.stats and plain.stats["ticks"] > 10
    with pytest.raises(RuntimeError, match="before the bank's first open"):
        plain.set_channel_snr_floor(20.0)
    fresh = embed_bank((48000,), 16, 2, floor=None)
    for bad in (float("nan"), float("inf"), "20"):
        with pytest.raises((ValueError, TypeError)):
            fresh.set_channel_snr_floor(bad)
    fresh.set_channel_snr_floor(20.0)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="strength"):
            fresh.open(None, sample_rate=48000, strength=bad)
    assert fresh.open_slots() == [] and fresh.latency_samples(fresh.open(None, sample_rate=48000)) == NS.EmbedPlan(48000, 16, LC.HALO).latency_samples + 48
    with pytest.raises(ValueError, match="LDS"):
        embed_bank((192000,), 4096, 1)                                        # a frame of 49152 native samples


def test_both_floors_the_inner_bank_carries_the_strength_and_the_cap_is_one():
    sr, hop = 44100, 16
    streams = {n: v for n, v in geometry_streams(sr, hop, seed=7).items() if n in ("edges", "long", "dribble")}
    bank = embed_bank((sr,), hop, len(streams), scaled=True)
    got = play(bank, streams)
    check_streams(got, streams, hop, cap=1.0)                                 # on the residual as the inner bank shaped it, strength inside
    plain = play(embed_bank((sr,), hop, len(streams)), streams)
    for n, v in streams.items():
        if v[2] != 1.0:
            assert not same(got[n][2], plain[n][2]) and np.allclose(got[n][2], F32(v[2]) * plain[n][2], rtol=1e-6, atol=0)


# ---- the row rule --------------------------------------------------------------------------------------------------------------------------
def stage_args(p):
    rcap, pcap, ucap = LC.state_caps()
    geo = [LC.back(sr) for sr in LC.STAGE_RATES]
    return (LC.STAGE_CAPACITY, rcap, pcap, ucap, LC.MAX_CHANNELS, p["n_r"], p["n_x"], p["n_out"], p["n_gains"], geo, LC.STAGE_HOP)


def test_the_row_rule_accepts_every_good_row_and_rejects_every_bad_one():
    ticks, totals = LC.floor_ticks()
    half = {s: 0 for s in range(LC.STAGE_CAPACITY)}
    clauses, good, spans, finals, idle = set(), 0, 0, 0, 0
    for tick in ticks:
        p = LC.pack_floor_tick(tick, half)
        args = stage_args(p)
        for row, cap in zip(p["back"], p["cap"]):
            assert NB.native_bank_floor_up_row_ok(row, cap, *args), row
            for bad_cap in (-1.0, np.inf, np.nan):
                assert not NB.native_bank_floor_up_row_ok(row, bad_cap, *args)
            for why, bad in LC.bad_floor_rows(row, *args):
                assert not NB.native_bank_floor_up_row_ok(bad, cap, *args), (why, bad)
                clauses.add(why)
            geo = args[9][int(row[1])]
            spans += int(row[16]) > NB.floor_tile_frames(*geo[:3], LC.STAGE_HOP)
            finals += int(row[20])
            idle += int(row[16]) == 0
            good += 1
        assert NB.floor_up_blocks(p["back"], args[9], LC.STAGE_HOP) >= 1
        for s in (LC.STAGE_SLOTS[i] for i in tick):
            half[s] ^= 1
    assert good > 30 and len(clauses) == 47 and spans >= 5 and finals == 5 and idle > 5


def test_the_numpy_stage_skips_bad_rows_whole_and_serves_their_neighbours():
    ticks, _ = LC.floor_ticks()
    rcap, pcap, ucap = LC.state_caps()
    tabs = [native.transposed_table(LC.M, sr) for sr in LC.STAGE_RATES]
    half = {s: 0 for s in range(LC.STAGE_CAPACITY)}
    rng = np.random.default_rng(2)
    state = [np.zeros((LC.STAGE_CAPACITY, 2, rcap), F32), np.zeros((LC.STAGE_CAPACITY, 2, LC.MAX_CHANNELS, pcap), F32),
             np.zeros((LC.STAGE_CAPACITY, 2, ucap), F32), np.zeros((LC.STAGE_CAPACITY, 2, LC.MAX_CHANNELS), F32)]
    served = 0
    for tick in ticks[:8]:
        p = LC.pack_floor_tick(tick, half)
        x, r = rng.uniform(-0.5, 0.5, p["n_x"]).astype(F32), rng.uniform(-0.05, 0.05, p["n_r"]).astype(F32)
        ref = [a.copy() for a in state]
        want = NB.numpy_bank_floor_up_add(*ref, r, x, p["back"], p["cap"], tabs, LC.STAGE_HOP, LC.RHO, p["n_out"], p["n_gains"])
        k = int(np.argmax(p["back"][:, 9]))
        bad = [b for _, b in LC.bad_floor_rows(p["back"][k], *stage_args(p))]
        bad = [(2,) + b[1:] if 0 <= b[0] < LC.STAGE_CAPACITY else b for b in bad]     # the bad rows name a slot nobody else does
        for a in state:
            a[2] = np.nan
        desc = np.array(bad[::2] + [tuple(v) for v in p["back"]] + bad[1::2], np.int64)
        cap = np.concatenate([np.ones(len(bad[::2]), F32), p["cap"], np.ones(len(bad[1::2]), F32)])
        got = NB.numpy_bank_floor_up_add(*state, r, x, desc, cap, tabs, LC.STAGE_HOP, LC.RHO, p["n_out"], p["n_gains"])
        assert same(got[0], want[0]) and same(got[1], want[1])
        for a, b in zip(state, ref):
            assert np.isnan(a[2]).all()
            a[2] = 0
            assert np.array_equal(a, b)
        served += len(bad)
        for s in (LC.STAGE_SLOTS[i] for i in tick):
            half[s] ^= 1
    assert served > 300 and np.abs(want[0]).max() > 0


# ---- the export and the opener -------------------------------------------------------------------------------------------------------------
def test_the_export_is_declared_listed_bound_and_refuses_by_name():
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    lib = _lib.load()
    decl = re.search(r"\bint " + EXPORT + r"\(([^;]*)\);", header)
    assert decl and EXPORT in _lib.SIGNATURES
    fn = getattr(lib, EXPORT)
    assert fn.restype is _lib.SIGNATURES[EXPORT][0] and list(fn.argtypes) == _lib.SIGNATURES[EXPORT][1]
    assert len(fn.argtypes) == decl.group(1).count(",") + 1 == 26
    assert "{slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half, f0, nf, uv, uv2, g_off, final}" in header
    assert NB.FLOOR_DESC == 21 and len(LC.FIELDS) == 21
    from waveverify_amd import build
    assert "wv_live_floor.hip" in build.SOURCES and any(h.endswith("wv_native_bank.h") for h in build.HEADERS)
    zero = {C.c_int: 0, C.c_int64: 0, C.c_double: 0.0}
    assert fn(*[zero.get(t) for t in _lib.SIGNATURES[EXPORT][1]]) == -1 and EXPORT in lib.wv_last_error().decode()
    # the tile rule is the kernel's: 48 kHz under hop 320 holds 7 frames of 960 beside the frame before them
    assert NB.floor_tile_frames(*LC.back(48000)[:3], 320) == 7 and NB.floor_tile_frames(*LC.back(48000)[:3], 16) == 16
    assert NB.floor_tile_frames(*LC.back(8000)[:3], 1) == 16 and NB.floor_tile_frames(*LC.back(192000)[:3], 4096) == 0


def test_the_new_opener_and_the_old_refusals():
    from waveverify_amd import WaveVerify
    p = inspect.signature(WaveVerify.open_native_embed_bank).parameters
    assert list(p)[1:] == ["rates", "capacity", "pad_limit", "max_channels", "channel_snr_floor_db"]
    assert (p["capacity"].default, p["pad_limit"].default, p["max_channels"].default, p["channel_snr_floor_db"].default) == (64, 1.5, 2, "instance")
    assert p["rates"].default is inspect.Parameter.empty

    class Net:
        device = "cpu"
    made, needed = [], []
    wv = WaveVerify.__new__(WaveVerify)
    wv.sample_rate, wv.watermark_bits = 16000, 16
    wv.generator_precision = "f32"
    wv._need = lambda name: needed.append(name) or Net()

    class Bank:
        def __init__(self, *a, **k):
            made.append(["made", a[1:5]])

        def set_snr_floor(self, db):
            made[-1].append(("snr", db))

        def set_channel_snr_floor(self, db):
            made[-1].append(("channel", db))
    keep = NB.NativeEmbedBank
    try:
        NB.NativeEmbedBank = Bank
        wv.open_native_embed_bank((48000, 8000), 3, max_channels=3)
        wv.set_snr_floor(30)
        wv.set_channel_snr_floor(20)
        wv.open_native_embed_bank((48000,))
        wv.open_native_embed_bank((48000,), channel_snr_floor_db=12.5)
        wv.open_native_embed_bank((48000,), channel_snr_floor_db=None)
    finally:
        NB.NativeEmbedBank = keep
    assert made == [["made", ((48000, 8000), 3, 3, "f32")], ["made", ((48000,), 64, 2, "f32"), ("snr", 30.0), ("channel", 20.0)],
                    ["made", ((48000,), 64, 2, "f32"), ("snr", 30.0), ("channel", 12.5)], ["made", ((48000,), 64, 2, "f32"), ("snr", 30.0)]]
    needed.clear()
    with pytest.raises(ValueError, match="44101"):
        wv.open_native_embed_bank((48000, 44101))
    with pytest.raises((ValueError, TypeError)):
        wv.open_native_embed_bank((48000,), channel_snr_floor_db=float("nan"))
    # the old openers still refuse while the instance's channel floor is set, and now name the way out
    with pytest.raises(ValueError, match=r"set_channel_snr_floor\(None\)") as e:
        wv.open_embed_bank(rates=(48000,))
    assert "open_native_embed_bank" in str(e.value)
    wv.set_snr_floor(None)
    with pytest.raises(ValueError, match=r"set_channel_snr_floor\(None\)") as e:
        wv.open_embed_session([1], 48000, 2)
    assert "lockstep" in str(e.value) and needed == []
