"""The SNR floor on the CPU (tests/snr_floor_cases.py; waveverify_amd/snr_floor.py): on the twin the per-frame
bound holds at -1e-5 dB on every case; silent frames, r = 0 frames and -0.0 come back bit for bit; no weight exceeds its frame's gain; a row
cut at frame boundaries with carried state gives the bits of the whole row; the case list contains capped, uncapped, rising and falling
frames; the summation order is the one written down; the twin's formula on the float64 oracle's residual, fed by a StreamBank on the oracle
with id switches, reproduces the file-route reference; the switch's refusals; the pinned signatures; the export.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import bank_cases as BK
import snr_floor_cases as FC
import span_cases as SC
import window_cases as W
from waveverify_amd import snr_floor as SF
from waveverify_amd.session import StreamBank
from waveverify_amd.window import halo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_window_cases_cpu.py holds float64 stitching to 1e-12 of the output's magnitude (it measured 6e-16); the shaping can amplify a
# residual error by at most 1 + sqrt(L) <= 6.7 for the hops here
BANK_BAR = 1e-11


def good_rows(case):
    for i, row in enumerate(case["rows"]):
        if i not in case["bad"]:
            xo, ro, oo, n, sb, si, fresh, go = (int(v) for v in row)
            yield i, case["x"][xo:xo + n], case["r"][ro:ro + n], np.array(sb, np.uint32).view(np.float32), si, fresh


def all_rows(L):
    """Every (x, r, s) the bound is held on: the kernel case's good rows and the random rows under both strengths."""
    case = FC.kernel_case(L)
    rows = [(x, r, s) for _, x, r, s, _, _ in good_rows(case)]
    for i, (x, r) in enumerate(FC.random_rows(L)):
        rows.append((x, r, np.float32(FC.STRENGTHS[i % 2])))
    return rows


# ---- the guarantee ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", FC.FRAMES)
def test_per_frame_bound_and_weight_never_above_the_gain(L):
    ramp = SF.floor_ramp(L)
    worst, kinds = np.inf, set()
    for db in FC.FLOORS:
        rho = SF.rho_of(db)
        for x, r, s in all_rows(L):
            for g_prev in (None, np.float32(0.0), np.float32(0.3)):
                v, g = SF.floor_row(x, r, s, rho, ramp, g_prev, add=False)
                if not len(x):
                    assert not len(v) and not len(g)
                    continue
                snr = SF.frame_snr_db(x, v, L)
                worst = min(worst, float((snr - db).min()))
                assert (snr >= db - FC.BOUND_DB).all(), (L, db, float((snr - db).min()))
                f = np.arange(len(x)) // L
                assert (np.abs(v) <= np.abs(g[f] * r)).all()                   # w <= g[f]: the product is monotone in w
                assert (g <= s).all() and (g >= 0).all()
                Er = SF.frame_energy(r, L)
                kinds |= {"capped"} if (g[Er > 0] < s).any() else set()
                kinds |= {"uncapped"} if (g[Er > 0] == s).any() else set()
                kinds |= {"rising"} if (np.diff(g) > 0).any() else set()
                kinds |= {"falling"} if (np.diff(g) < 0).any() else set()
    assert kinds == {"capped", "uncapped", "rising", "falling"}, kinds
    print(f"SNR FLOOR bound L={L}: worst frame {worst:.2e} dB against the floor (bar -{FC.BOUND_DB:.0e})")


@pytest.mark.parametrize("L", FC.FRAMES)
def test_silence_and_empty_residual_come_back_bit_for_bit(L):
    ramp, rho = SF.floor_ramp(L), SF.rho_of(FC.MIN_SNR_DB)
    seen = set()
    for x, r, s in all_rows(L):
        if not len(x):
            continue
        out, g = SF.floor_row(x, r, s, rho, ramp)
        F = len(g)
        pad = F * L - len(x)
        xs, rs = np.pad(x, (0, pad)).reshape(F, L), np.pad(r, (0, pad)).reshape(F, L)
        for f in range(F):
            a, b = f * L, min((f + 1) * L, len(x))
            if not xs[f].any() and s > 0:
                seen.add("x=0")
                assert g[f] == (s if not rs[f].any() else 0) and np.array_equal(out[a:b].view(np.int32), x[a:b].view(np.int32))
            if not rs[f].any():
                seen.add("r=0")
                assert g[f] == s and np.array_equal(out[a:b].view(np.int32), x[a:b].view(np.int32))
        zero_v = (SF.floor_row(x, r, s, rho, ramp, add=False)[0] == 0)
        assert np.array_equal(out[zero_v].view(np.int32), x[zero_v].view(np.int32))
        if (np.signbit(x) & (x == 0) & zero_v).any():
            seen.add("-0.0")
    assert seen == {"x=0", "r=0", "-0.0"}, seen


@pytest.mark.parametrize("L", FC.FRAMES)
def test_pieces_with_carried_state_are_the_whole_row(L):
    ramp, rho = SF.floor_ramp(L), SF.rho_of(FC.MIN_SNR_DB)
    rng = np.random.default_rng(W.seed_of("snr floor pieces", L))
    for x, r, s in all_rows(L):
        F = -(-len(x) // L)
        if F < 2:
            continue
        for add in (True, False):
            whole, g = SF.floor_row(x, r, s, rho, ramp, None, add)
            cuts = sorted({int(c) for c in rng.integers(1, F, 3)})
            parts, gains, g_prev = [], [], None
            for a, b in zip([0] + cuts, cuts + [F]):
                o, gg = SF.floor_row(x[a * L:b * L], r[a * L:b * L], s, rho, ramp, g_prev, add)
                parts.append(o)
                gains.append(gg)
                g_prev = gg[-1]
            assert np.array_equal(np.concatenate(parts).view(np.int32), whole.view(np.int32))
            assert np.array_equal(np.concatenate(gains).view(np.int32), g.view(np.int32))


def test_the_summation_order_is_the_one_written_down():
    """frame_energy against a sample-by-sample restatement: partial (k >> 2) & 15, ascending k, then the four folds."""
    rng = np.random.default_rng(W.seed_of("snr floor order"))
    for L in (1, 3, 12, 63, 64, 65, 320):
        a = (rng.standard_normal(3 * L + L // 2) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
        got = SF.frame_energy(a, L)
        for f in range(len(got)):
            p = [0.0] * 16
            for k, v in enumerate(a[f * L:(f + 1) * L]):
                p[(k >> 2) & 15] += float(v) * float(v)
            for h in (8, 4, 2, 1):
                p = [p[j] + p[j + h] for j in range(h)]
            assert got[f] == p[0], (L, f)
    assert SF.frame_energy(np.zeros(0, np.float32), 8).shape == (0,)


def test_ramp_rho_and_check_db():
    for L in FC.FRAMES:
        r = SF.floor_ramp(L)
        assert r.dtype == np.float32 and r[-1] == 1.0 and np.array_equal(r, np.array([np.float32((k + 1) / L) for k in range(L)]))
    assert SF.rho_of(20.0) == 10.0 ** -2.0 and SF.rho_of(0) == 1.0
    assert SF.check_db(None) is None and SF.check_db(20) == 20.0 and SF.check_db(np.float32(-3.0)) == -3.0
    for bad in (float("nan"), float("inf"), -float("inf"), "20", True, [20.0]):
        with pytest.raises(ValueError):
            SF.check_db(bad)
    for bad in (0, -1, 2.5, SF.MAX_FRAME + 1):
        with pytest.raises(ValueError):
            SF.floor_ramp(bad)
    with pytest.raises(ValueError):
        SF.rho_of(None)
    with pytest.raises(ValueError):
        SF.rho_of(1e6)                                                         # underflows to 0 as a power ratio


# ---- the twin's table form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", FC.FRAMES)
def test_table_twin_skips_bad_rows_and_keeps_the_state_rules(L):
    case = FC.kernel_case(L)
    names = set(case["kinds"].values())
    assert {"n=0", "n<L", "n=L", "n=9L+1", "long", "carried", "fresh-poisoned"} <= names and len(case["bad"]) == 18
    rows = case["rows"]
    good = [i for i in range(len(rows)) if i not in case["bad"]]
    assert {int(rows[i][0]) % 4 for i in good} == {0, 1, 2, 3} and {int(rows[i][2]) % 4 for i in good} == {0, 1, 2, 3}
    assert any(rows[i][3] > (FC.TILE_FRAMES + 1) * L for i in good)
    n_x, n_r = len(case["x"]), len(case["r"])
    for i, row in enumerate(rows):
        assert SF.row_ok(row, n_x, n_r, case["n_out"], case["n_max"], FC.N_STATE, case["n_gains"], L) == (i not in case["bad"]), case["kinds"][i]
    rho, ramp = SF.rho_of(FC.MIN_SNR_DB), SF.floor_ramp(L)
    for add in (True, False):
        out, gstate, gains, kept, gkept = FC.twin(case, L, rho, add)
        assert np.isnan(out[~kept]).all() and not np.isnan(out[kept]).any()    # the poison was never read, the bad rows wrote nothing
        assert np.isnan(gains[~gkept]).all() and not np.isnan(gains[gkept]).any()
        for i, x, r, s, si, fresh in good_rows(case):
            oo, go = int(rows[i][2]), int(rows[i][7])
            g_prev = None if si < 0 or fresh else case["gstate"][si]
            o, g = SF.floor_row(x, r, s, rho, ramp, g_prev, add)
            assert np.array_equal(out[oo:oo + len(x)].view(np.int32), o.view(np.int32)), case["kinds"][i]
            if go >= 0:
                assert np.array_equal(gains[go:go + len(g)], g)
            if si >= 0:
                assert gstate[si] == (g[-1] if len(g) else case["gstate"][si])  # n = 0 leaves the state alone
        assert gstate[6] == case["gstate"][6]                                  # named by a bad row only


# ---- a bank on the float64 oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", FC.EXACT_IDS)
def test_oracle_bank_with_switches_then_the_floor_is_the_file_route(cid):
    """A StreamBank on the float64 oracle returns each stream's residual push by push while the streams switch id -> None -> id.  The floor's
    formula in float64, applied piece by piece with the bank's state rules (the gain carried from piece to piece, fresh at open and on
    leaving pass-through), is the file route's reference: span embedding with hard cuts of the whole stream, then the floor on the whole
    stream."""
    case = SC.net_case(cid)
    cfg, sd, onet = W.oracle_net(case)
    hop, H = cfg.hop_length, halo(cfg)
    msgs = SC.messages(cid)
    rho = SF.rho_of(FC.MIN_SNR_DB)
    name, steps = BK.schedules(cfg)[0]
    data = BK.stream_data(case, steps)
    xs = {n: x for n, (x, _) in data.items()}
    plan = SC.switch_plan(steps)
    cur = {}
    bank = StreamBank(BK.CAPACITY, hop, H, lambda win, slots: W.oracle_forward(cfg, onet, win, msgs[[cur[s] for s in slots]], add_input=False),
                      pad_limit=1.5)

    def set_state(slot, st):
        if st is not None:
            cur[slot] = st
        return bank.set_passthrough(slot, st is None)

    def open_stream(st):
        slot = bank.open()
        set_state(slot, st)
        return slot
    out, marks, _, _ = SC.run_switching(bank, steps, xs, plan, open_stream, set_state)
    worst, lowered = 0.0, 0
    for n, x in xs.items():
        if not x.size:
            continue
        sp = SC.spans_of(marks[n], x.size)
        inside = ~SC.outside(x.size, sp)
        got, pos, g_prev = [], 0, None
        for piece in out[n]:
            if piece is None or not np.asarray(piece).size:
                continue
            piece = np.asarray(piece, np.float64).reshape(-1)
            a, b = pos, pos + len(piece)
            pos = b
            assert a % hop == 0 and (inside[a:b].all() or not inside[a:b].any())   # a switch falls on a piece boundary
            if not inside[a]:
                got.append(x[a:b].astype(np.float64))                          # pass-through: the input, no floor, and the state goes stale
                g_prev = None
                continue
            o, g = FC.reference64(x[a:b], piece, rho, hop, 1.0, g_prev)
            got.append(o)
            g_prev = g[-1]
        got = np.concatenate(got)
        deltas = {m: W.oracle_forward(cfg, onet, x[None, None], msgs[m:m + 1], add_input=False)[0, 0] for m in {m for _, _, m in sp}}
        masked = SC.reference(x, deltas, sp, add_input=False)
        ref, g = FC.reference64(x, masked, rho, hop)
        lowered += int((g < 1).sum())
        err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
        worst = max(worst, err)
        assert err <= BANK_BAR, (n, err)
        assert np.array_equal(got[~inside], x[~inside].astype(np.float64))
    assert lowered > 0, "the floor turned some frame down"
    print(f"SNR FLOOR oracle bank {cid}: {worst:.1e} of the output's magnitude (bar {BANK_BAR:.0e})")


@pytest.mark.parametrize("cid", FC.EXACT_IDS)
def test_the_route_inputs_make_the_floor_cap_some_frames_and_spare_others(cid):
    """The input condition of tests/test_gpu_snr_floor.py's route tests, on the float64 oracle's residual."""
    cfg, sd, onet = W.oracle_net(SC.net_case(cid))
    x = FC.batch_clips(cid)
    msgs = SC.messages(cid)
    d = W.oracle_forward(cfg, onet, x[:, None], msgs[:2], add_input=False)[:, 0]
    g = np.concatenate([FC.reference64(x[b], d[b], SF.rho_of(FC.ROUTE_DB), cfg.hop_length)[1] for b in range(2)])
    assert (g == 1).sum() >= 5 and ((g < 1) & (g > 0)).sum() >= 5 and (g == 0).sum() >= 5, ((g == 1).sum(), (g < 1).sum(), (g == 0).sum())


# ---- the switch -----------------------------------------------------------------------------------------------------------------------------
def _bare():
    from waveverify_amd import WaveVerify
    wv = WaveVerify.__new__(WaveVerify)
    wv.snr_floor_db = None
    return wv


def test_set_snr_floor_and_its_refusals():
    wv = _bare()
    wv.set_snr_floor(20)
    assert wv.snr_floor_db == 20.0 and isinstance(wv.snr_floor_db, float)
    for bad in (float("nan"), float("inf"), "loud", True):
        with pytest.raises(ValueError):
            wv.set_snr_floor(bad)
        assert wv.snr_floor_db == 20.0                                         # a refusal changes nothing
    wv.set_snr_floor(None)
    assert wv.snr_floor_db is None


def test_open_embed_session_refuses_under_a_floor_and_names_the_bank():
    wv = _bare()
    wv.set_snr_floor(30.0)
    for kw in ({}, dict(sample_rate=48000, channels=2)):
        with pytest.raises(ValueError, match="open_embed_bank"):
            wv.open_embed_session([1, 2], **kw)


def test_pinned_signatures_are_unchanged():
    from waveverify_amd import WaveVerify
    from waveverify_amd.native_bank import NativeEmbedBank
    from waveverify_amd.session import EmbedBank
    sig = lambda fn: list(inspect.signature(fn).parameters)                    # noqa: E731
    assert sig(WaveVerify.embed_native_batch) == ["self", "audio", "sample_rate", "message", "strength", "window_seconds"]
    assert sig(WaveVerify.open_embed_bank) == ["self", "capacity", "pad_limit", "rates", "max_channels"]
    assert sig(WaveVerify.open_embed_session) == ["self", "watermark_ids", "sample_rate", "channels", "strength"]
    assert sig(WaveVerify.embed_batch) == ["self", "audio", "message"]
    assert sig(WaveVerify.embed_clips) == ["self", "clips", "watermark_ids", "window_seconds"]
    assert sig(WaveVerify.embed_spans_clips) == ["self", "clips", "spans", "window_seconds", "fade_samples", "strength", "pad_limit"]
    assert sig(WaveVerify.embed_spans_native_batch) == ["self", "audio", "sample_rate", "spans", "strength", "fade_samples", "window_seconds"]
    assert sig(WaveVerify.set_snr_floor) == ["self", "min_snr_db"]
    assert sig(EmbedBank.__init__) == ["self", "net", "capacity", "precision", "pad_limit", "messages", "add_input"]
    assert sig(EmbedBank.set_snr_floor) == ["self", "min_snr_db"] and sig(NativeEmbedBank.set_snr_floor) == ["self", "min_snr_db"]
    p = inspect.signature(SF.apply).parameters
    assert list(p) == ["x", "residual", "min_snr_db", "strength", "frame", "add", "return_gains"]
    assert p["strength"].default == 1.0 and p["add"].default is True and p["return_gains"].default is False


# ---- the export -----------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_listed_bound_and_refuses_by_name():
    from waveverify_amd import _lib
    from waveverify_amd.build import SOURCES
    assert "wv_snr_floor.hip" in SOURCES
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    proto = re.search(r"\bint\s+wv_snr_floor\s*\(([^;]*?)\)\s*;", header, re.S)
    assert proto, "wv_snr_floor is not declared"
    res, args = _lib.SIGNATURES["wv_snr_floor"]
    assert res is C.c_int and len(args) == len(proto.group(1).split(","))
    assert "wv_snr_floor" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    # addresses that a refusal never follows: every call below is refused (or has no row) before anything is launched
    buf = (C.c_float * 64)()
    at = lambda k: C.addressof(buf) + 4 * k                                    # noqa: E731
    ok = dict(x=at(0), n_x=16, r=at(16), n_r=16, out=at(32), n_out=16, desc=at(48), A=1, n_max=16, gstate=None, n_state=0, gains=None, n_gains=0,
              ramp=at(56), L=4, rho=0.01, add=1)
    call = lambda a: lib.wv_snr_floor(a["x"], a["n_x"], a["r"], a["n_r"], a["out"], a["n_out"], a["desc"], a["A"], a["n_max"], a["gstate"],   # noqa: E731
                                      a["n_state"], a["gains"], a["n_gains"], a["ramp"], a["L"], a["rho"], a["add"], None)
    refusals = (("null x", dict(x=None)), ("null r", dict(r=None)), ("null out", dict(out=None)), ("null desc", dict(desc=None)),
                ("null ramp", dict(ramp=None)), ("n_x < 0", dict(n_x=-1)), ("n_r < 0", dict(n_r=-1)), ("n_out < 0", dict(n_out=-1)),
                ("n_state < 0", dict(n_state=-1)), ("states without gstate", dict(n_state=2)), ("n_gains < 0", dict(n_gains=-1)),
                ("gains without their array", dict(n_gains=4)), ("L < 1", dict(L=0)), ("L beyond the limit", dict(L=SF.MAX_FRAME + 1)),
                ("rho = 0", dict(rho=0.0)), ("rho < 0", dict(rho=-1.0)), ("rho = nan", dict(rho=float("nan"))), ("rho = inf", dict(rho=float("inf"))),
                ("A < 0", dict(A=-1)), ("A > 65535", dict(A=65536)), ("n_max < 0", dict(n_max=-1)), ("n_max beyond 2^31 - 1", dict(n_max=1 << 31)),
                ("add = 2", dict(add=2)), ("out is x", dict(out=at(0))), ("out overlaps x", dict(out=at(8))), ("out overlaps r", dict(out=at(24))))
    for why, kw in refusals:
        assert call({**ok, **kw}) == -1, why
        assert lib.wv_last_error().decode().startswith("wv_snr_floor"), why
    assert call({**ok, "A": 0}) == 0 and call({**ok, "n_max": 0}) == 0         # success without a launch
    assert not any(buf)
