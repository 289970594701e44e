"""Native-rate session banks without a GPU (waveverify_amd/native_bank.py): the bank state machine on the numpy stages
in float64 with a toy causal inner bank, every stream's concatenated output EXACTLY that of a lockstep host session of one stream given the
same pushes; slot reuse over poisoned state; the half bits; open()'s refusals; the two exports; the row rule in Python."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import native_bank_cases as NBC
from waveverify_amd import _lib, native
from waveverify_amd import native_bank as NB
from waveverify_amd import native_session as NS
from waveverify_amd.session import NumpyArrays, StreamBank, StreamSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("wv_native_bank_down", "wv_native_bank_up_add")
HOP, HALO, M = NBC.HOP, NBC.HALO, NBC.M
GAINS = {"A": 1.0, "B": 0.37, "C": 1.0, "D": 0.37, "E": 0.5, "F": 1.0, "G": 0.37, "Z": 1.0}


def model(win: np.ndarray) -> np.ndarray:
    """A pointwise 'generator residual' (tests/test_native_session_cpu.py's): the same for a sample whatever window holds it."""
    return 0.25 * win * win - 0.1 * win


class ToyBank(StreamBank):
    def _on_open(self, slot, *message):                                      # an embed bank's open() takes a message
        pass


def inner_bank(capacity: int, forward):
    return ToyBank(capacity, HOP, HALO, lambda win, slots: forward(win), arrays=NumpyArrays(np.float64))


def inner_session(forward):
    return StreamSession(1, HOP, HALO, lambda win, keep: forward(win[:, :, keep:]), arrays=NumpyArrays(np.float64))


def embed_bank(capacity: int = 6):
    return NB.HostEmbedBank(inner_bank(capacity, model), NBC.RATES, NBC.MAX_CHANNELS, dtype=np.float64)


def cat(parts, C_):
    parts = [np.asarray(p).reshape(C_, -1) for p in parts if p is not None]
    return np.concatenate(parts, axis=1) if parts else np.zeros((C_, 0))


def lockstep(sess, x, sizes):
    """The session's outputs for stream x [C, T] pushed in `sizes`, then flushed: [per push result], flush result."""
    outs, at = [], 0
    for n in sizes:
        outs.append(sess.push(x[None, :, at:at + n]))
        at += n
    return outs, sess.flush()


def sizes_of(log):
    at, out = 0, []
    for kind, pos, _ in log:
        if kind == "push":
            out.append(pos - at)
            at = pos
    return out


@pytest.mark.parametrize("name,steps,who", NBC.schedules(HOP, HALO) + [("equal 44100",) + NBC.equal(44100, HOP, HALO)[:2]])
def test_embed_bank_is_a_lockstep_session_per_stream_exactly(name, steps, who):
    xs = NBC.stream_data(steps, who, dtype=np.float64)
    bank = embed_bank()
    out, _ = NBC.run(bank, steps, xs, who, open_args=lambda n: (None,), take=lambda x: x)
    for n, log in out.items():
        sr, Cn = who[n]
        sess = NS.HostEmbedSession(inner_session(model), sr, Cn, 1.0, dtype=np.float64)
        want, last = lockstep(sess, xs[n], sizes_of(log))
        got = [r for _, _, r in log]
        assert len(got) == len(want) + 1
        for g, w in zip(got, want + [last]):
            assert g.shape == w.shape[1:] and np.array_equal(g, w[0]), (name, n)
        assert cat(got, Cn).shape == xs[n].shape                              # as many samples came out as went in
    assert bank.open_slots() == [] and bank.stats["front_launches"] == bank.stats["back_launches"] == bank.stats["uploads"] == bank.stats["ticks"]


def test_embed_bank_strengths_and_latency():
    steps, who = NBC.mixed(HOP, HALO)
    xs = NBC.stream_data(steps, who, dtype=np.float64)

    class Bank(NB.HostEmbedBank):
        def open(self, name, **kw):
            return super().open(None, strength=GAINS[name], **kw)
    bank = Bank(inner_bank(6, model), NBC.RATES, NBC.MAX_CHANNELS, dtype=np.float64)
    seen = {}

    def after(kind, slots):
        if kind == "push":
            for s in slots:
                assert bank.samples_in(s) - bank.samples_out(s) < bank.latency_samples(s)
                seen[s] = bank.latency_samples(s)
    out, slot = NBC.run(bank, steps, xs, who, open_args=lambda n: (n,), after=after)
    for n, log in out.items():
        sr, Cn = who[n]
        sess = NS.HostEmbedSession(inner_session(model), sr, Cn, GAINS[n], dtype=np.float64)
        want, last = lockstep(sess, xs[n], sizes_of(log))
        assert np.array_equal(cat([r for _, _, r in log], Cn), cat([w[0] for w in want + [last]], Cn)), n
    assert seen[slot["A"]] == NS.EmbedPlan(48000, HOP, HALO).latency_samples


@pytest.mark.parametrize("name,steps,who", NBC.schedules(HOP, HALO))
def test_front_bank_is_a_lockstep_front_session_per_stream_exactly(name, steps, who):
    xs = NBC.stream_data(steps, who, seed=1, dtype=np.float64)
    ident = lambda win: win                                                   # noqa: E731
    bank = NB.HostFrontBank(inner_bank(6, ident), NBC.RATES, NBC.MAX_CHANNELS, dtype=np.float64)
    out, _ = NBC.run(bank, steps, xs, who)
    for n, log in out.items():
        sr, Cn = who[n]
        sess = NS.HostFrontSession(inner_session(ident), sr, Cn, dtype=np.float64)
        want, last = lockstep(sess, xs[n], sizes_of(log))
        # the lockstep flush() hands on what its inner flush returns; the bank's close likewise (its inner push's result is dropped by both)
        got = [r for _, _, r in log]
        for g, w in zip(got, want + [last]):
            assert (g is None) == (w is None), (name, n)
            if g is not None:
                assert np.array_equal(np.asarray(g).reshape(-1), w.reshape(-1)), (name, n)
        assert sess.inner.samples_seen == native.resampled_length(xs[n].shape[1], sr, M) if xs[n].shape[1] else True


def test_a_reopened_slot_reads_nothing_its_last_stream_left():
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-0.5, 0.5, (2, 3000)), rng.uniform(-0.5, 0.5, (3, 700))

    def second(bank):
        s = bank.open(None, sample_rate=8000, channels=3, strength=0.37)
        return s, np.concatenate([bank.push({s: b[:, :300]})[s], bank.push({s: b[:, 300:]})[s], bank.close(s)], axis=1)
    used = embed_bank(2)
    s = used.open(None, sample_rate=48000, channels=2)
    used.push({s: a[:, :1700]})
    used.push({s: a[:, 1700:]})
    used.close(s)
    for state in (used._hist, used._rhist, used._pend):
        assert np.abs(state[s]).max() > 0                                     # the first stream did leave state in the slot
        state[:] = np.nan                                                     # both halves, every slot
    s2, got = second(used)
    s3, want = second(embed_bank(2))
    assert s2 == s3 == s and got.shape == b.shape and not np.isnan(got).any() and np.array_equal(got, want)


def test_the_half_bit_flips_only_for_the_slots_a_tick_named():
    steps, who = NBC.mixed(HOP, HALO)
    xs = NBC.stream_data(steps, who, dtype=np.float64)
    bank = embed_bank()
    prev, ticks = [list(bank._half)], [0]

    def after(kind, slots):
        want = [h ^ (s in slots) for s, h in enumerate(prev[0])]
        assert bank._half == want, (kind, slots)
        prev[0] = list(bank._half)
        ticks[0] += 1
    NBC.run(bank, steps, xs, who, open_args=lambda n: (None,), after=after)
    assert ticks[0] == bank.stats["ticks"] > 10 and 0 < sum(prev[0]) < 6       # the slots did go different ways


def test_open_refusals_change_no_state():
    bank = embed_bank(2)

    def state():
        return (list(bank.inner._is_open), [id(p) for p in bank._plans], list(bank._half), list(bank._rate), list(bank._chan),
                list(bank._strength), bank._hist.copy(), dict(bank.stats))

    def same(a, b):
        return all(np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v for u, v in zip(a, b))
    s0 = bank.open(None, sample_rate=8000, channels=3)
    before = state()
    with pytest.raises(ValueError, match="32000"):
        bank.open(None, sample_rate=32000)
    with pytest.raises(ValueError, match="channels"):
        bank.open(None, sample_rate=48000, channels=NBC.MAX_CHANNELS + 1)
    with pytest.raises(ValueError, match="channels"):
        bank.open(None, sample_rate=48000, channels=0)
    assert same(before, state())
    s1 = bank.open(None, sample_rate=48000, channels=1)
    assert (s0, s1) == (0, 1)
    before = state()
    with pytest.raises(RuntimeError, match="slots"):
        bank.open(None, sample_rate=48000)
    assert same(before, state())
    with pytest.raises(ValueError, match="expected new samples"):
        bank.push({s0: np.zeros((2, 5))})
    with pytest.raises(ValueError, match="not open"):
        bank.push({5: np.zeros((1, 5))})
    assert same(before, state())
    # the bank's own refusals
    with pytest.raises(ValueError, match="distinct"):
        NB.check_rates((48000, 48000))
    with pytest.raises(ValueError, match="1 to 8"):
        NB.check_rates(tuple(range(8000, 8009)))
    with pytest.raises(ValueError, match="1 to 8"):
        NB.check_rates(())
    with pytest.raises(ValueError, match="44101"):
        NB.check_rates((48000, 44101))
    with pytest.raises(ValueError, match="max_channels"):
        NB.HostFrontBank(inner_bank(1, model), (48000,), 65)
    assert NB.check_rates([16000, 8000]) == (16000, 8000)                     # 16000 is a legal entry: the one-tap table


def test_core_openers_keep_todays_objects_and_refuse_rates_before_the_device():
    import inspect
    from waveverify_amd import WaveVerify, session
    for fn in (WaveVerify.open_embed_bank, WaveVerify.open_detect_bank, WaveVerify.open_locate_bank):
        p = inspect.signature(fn).parameters
        assert list(p)[1:] == ["capacity", "pad_limit", "rates", "max_channels"] and p["rates"].default is None and p["max_channels"].default == 2
    p = inspect.signature(WaveVerify.open_native_segment_bank).parameters
    assert list(p)[1:3] == ["rates", "max_channels"] and p["gated"].default is False

    class Net:
        device = "cpu"
    made, needed = [], []
    wv = WaveVerify.__new__(WaveVerify)
    wv.sample_rate, wv.watermark_bits = 16000, 16
    wv.generator_precision = wv.detector_precision = wv.locator_precision = "f32"
    wv._need = lambda name: needed.append(name) or Net()
    keep = {c: getattr(session, c) for c in ("EmbedBank", "DetectBank", "LocateBank")}
    try:
        for c in keep:
            setattr(session, c, type(c, (), {"__init__": lambda self, *a, _c=c, **k: made.append(_c)}))
        assert type(wv.open_embed_bank(3)).__name__ == "EmbedBank" and type(wv.open_detect_bank()).__name__ == "DetectBank"
        assert type(wv.open_locate_bank(pad_limit=1.0)).__name__ == "LocateBank" and made == ["EmbedBank", "DetectBank", "LocateBank"]
    finally:
        for c, v in keep.items():
            setattr(session, c, v)
    needed.clear()
    for open_ in (wv.open_embed_bank, wv.open_detect_bank, wv.open_locate_bank, lambda **k: wv.open_native_segment_bank(**k)):
        with pytest.raises(ValueError, match="44101"):
            open_(rates=(48000, 44101))
        with pytest.raises(ValueError, match="1 to 8"):
            open_(rates=tuple(8000 * i for i in range(1, 10)))
    with pytest.raises(ValueError, match="gate"):
        wv.open_native_segment_bank((48000,), gated=True)
    assert needed == []                                                       # refused before a net was asked for


# ---- exports -----------------------------------------------------------------------------------------------------------------------------
def test_exports_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    lib = _lib.load()
    for name in EXPORTS:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl and name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is _lib.SIGNATURES[name][0] and list(fn.argtypes) == _lib.SIGNATURES[name][1]
        assert len(fn.argtypes) == decl.group(1).count(",") + 1                # the header's arity
    assert len(_lib.SIGNATURES[EXPORTS[0]][1]) == 13 and len(_lib.SIGNATURES[EXPORTS[1]][1]) == 19
    assert "{slot, rate, C, hv, x_off, n, y_off, n_out, pad, drop, hv2, half}" in header
    assert "{slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half}" in header
    assert C.sizeof(_lib.WvNativeRate) == 24 and NB.MAX_RATES == int(re.search(r"#define WV_NATIVE_BANK_MAX_RATES (\d+)", header).group(1))
    zero = {C.c_int: 0, C.c_int64: 0}
    for name in EXPORTS:                                                      # all-null, all-zero calls never reach a launch
        assert getattr(lib, name)(*[zero.get(t) for t in _lib.SIGNATURES[name][1]]) == -1
        assert name in lib.wv_last_error().decode()


# ---- the row rule ------------------------------------------------------------------------------------------------------------------------
def test_the_row_rule_accepts_every_good_row_and_rejects_every_bad_one():
    hcap, rcap, pcap = NBC.state_caps()
    fgeo = [native.table_geometry(sr, M) for sr in NBC.RATES]
    bgeo = [native.table_geometry(M, sr) for sr in NBC.RATES]
    ticks, _ = NBC.stage_ticks()
    half = {s: 0 for s in range(NBC.STAGE_CAPACITY)}
    clauses_d, clauses_u, good = set(), set(), 0
    for tick in ticks:
        p = NBC.pack_tick(tick, half)
        for row in p["front"]:
            assert NB.native_bank_down_row_ok(row, NBC.STAGE_CAPACITY, hcap, p["n_x"], p["n_y"], fgeo), row
            for why, bad in NBC.bad_down_rows(row, NBC.STAGE_CAPACITY, hcap, p["n_x"], p["n_y"], fgeo):
                assert not NB.native_bank_down_row_ok(bad, NBC.STAGE_CAPACITY, hcap, p["n_x"], p["n_y"], fgeo), (why, bad)
                clauses_d.add(why)
        for row in p["back"]:
            args = (NBC.STAGE_CAPACITY, rcap, pcap, NBC.MAX_CHANNELS, p["n_r"], p["n_x"], p["n_out"], bgeo)
            assert NB.native_bank_up_row_ok(row, *args), row
            for why, bad in NBC.bad_up_rows(row, *args):
                assert not NB.native_bank_up_row_ok(bad, *args), (why, bad)
                clauses_u.add(why)
            good += 1
        assert NB.down_blocks(p["front"]) >= 0 and NB.up_blocks(p["back"]) >= 0      # a tick of pushes of 0 needs no block at all
        for s in (NBC.STAGE_SLOTS[i] for i in tick):
            half[s] ^= 1
    assert good > 30 and len(clauses_d) == 23 and len(clauses_u) == 30


def test_numpy_stages_skip_bad_rows_whole_and_serve_their_neighbours():
    hcap, rcap, pcap = NBC.state_caps()
    ftabs = [native.transposed_table(sr, M) for sr in NBC.RATES]
    fgeo = [t[1:] for t in ftabs]
    ticks, _ = NBC.stage_ticks()
    tick = ticks[6]                                                           # the tile-crossing pushes
    half = {s: 0 for s in range(NBC.STAGE_CAPACITY)}
    p = NBC.pack_tick(tick, half)
    rng = np.random.default_rng(2)
    x = rng.uniform(-0.5, 0.5, p["n_x"])
    hist = np.zeros((NBC.STAGE_CAPACITY, 2, hcap))
    want = NB.numpy_bank_down(hist.copy(), x, p["front"], ftabs, p["n_y"])
    bad = [b for _, b in NBC.bad_down_rows(p["front"][0], NBC.STAGE_CAPACITY, hcap, p["n_x"], p["n_y"], fgeo)]
    bad = [(2,) + b[1:] if 0 <= b[0] < NBC.STAGE_CAPACITY else b for b in bad]      # the bad rows name a slot nobody else does
    h2 = hist.copy()
    h2[2] = np.nan
    got = NB.numpy_bank_down(h2, x, np.array(list(p["front"]) + bad, np.int64), ftabs, p["n_y"])
    assert np.array_equal(got, want) and np.isnan(h2[2]).all() and np.abs(want).max() > 0
