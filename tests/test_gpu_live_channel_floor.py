"""The live per-channel SNR floor on the GPU (csrc/wv_live_floor.hip, waveverify_amd/native_bank.py).

1. wv_native_bank_floor_up_add alone through the C ABI, every arena between guard bands at offsets 0 and 1, the four states NaN-patterned wherever
   they are not valid, five rates in one call: per slot the concatenated out and gains are channel_floor.numpy_channel_floor on the whole stream
   BIT FOR BIT, u from the existing kernel (native.upsample_add on zeros), and after every tick the slot's next half holds the twin's held u, the
   delayed originals and the last frame's gains; a second run with bad rows around the good ones gives the same bits; unnamed slots keep their
   pattern; refusals write nothing.
2. With the cap never reached (-200 dB) the bank's concatenated output is the floor-less bank's, bit for bit, only later.
3. NativeEmbedBank under the floor, f32 and f16: per stream the output and gains are the twin on (its whole input, u of the residuals the inner
   bank actually returned), bit for bit; the emission counts are HostEmbedBank's tick by tick; one upload, one front and one back launch a tick.
4. The defect end to end: a 48 kHz stereo stream with a silent right channel gets non-zero samples there under set_snr_floor alone, and its own
   bits under the channel floor, the left channel inside the bound in every native frame.
5. Against embed_native_batch under set_channel_snr_floor on the whole recording, by largest absolute difference.

Measured on the MI355X (RECORD lines, pytest -s; small generators of window_cases, 180 ms per stream in 10, 20 and 60 ms packets, floor 20 dB), a
stream's concatenated output against embed_native_batch under set_channel_snr_floor on its whole recording by largest absolute difference:
    exact f32, bar 2e-5: 3.0e-8 at 48 kHz stereo, 3.0e-8 at 44.1 kHz mono (strength 0.5), 2.4e-7 at 8 kHz with three channels.
    f16 bank against the f16 route on the whole input, bar 2e-5: 0 at all three rates.  Against the EXACT route the f16 bank stands 3.0e-5
    (48 kHz), 1.8e-5 (44.1 kHz) and 1.7e-5 (8 kHz) off: the f16 mode's own distance from the exact path, asserted at WM_BAR = 1e-4.  No frame's
    cap or ramp branch flipped between the routes far enough to show against either bar."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import channel_floor_cases as CFC
import live_channel_floor_cases as LC
import native_bank_cases as NBC
import window_cases as W
from guard import Guards
from waveverify_amd import _lib, native
from waveverify_amd import channel_floor as CF
from waveverify_amd import native_bank as NB
from waveverify_amd.session import NumpyArrays, StreamBank

pytestmark = pytest.mark.gpu
M = LC.M
WM_BAR = 1e-4                                                               # the f16 mode's watermarked samples against the exact path's (test_gpu_h16)
NAN = np.float32(np.nan)
NETS = {c[0]: c for c in W.net_cases()}


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t) -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t, np.float32)
    return a.view(np.int32)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def P(arena):
    return arena.t.data_ptr()


def kernel_u(res, sr, Tn):
    """u [Tn] as the existing kernel forms it: native.upsample_add on zeros with gain 1."""
    if Tn == 0:
        return np.zeros(0, np.float32)
    return native.upsample_add(torch.zeros(1, 1, Tn, device="cuda"), res.reshape(1, -1), sr, 1.0)[0, 0].cpu().numpy()


# ================================================================== 1. the entry point alone
def _fill(n, rows):
    a = np.full(n, NAN, np.float32)
    for off, v in rows:
        a[off:off + v.size] = v.reshape(-1)
    return a


def _mask(n, ranges):
    m = torch.ones(n, dtype=torch.bool)
    for off, k in ranges:
        m[off:off + k] = False
    return m


def back_table():
    pairs = [native.tables(sr, torch.device("cuda", torch.cuda.current_device())) for sr in LC.STAGE_RATES]
    ts = [p[1] for p in pairs]
    return (_lib.WvNativeRate * len(ts))(*[_lib.WvNativeRate(t[0].data_ptr(), *t[1:]) for t in ts]), pairs


class Stage:
    """The four states of LC.STAGE_CAPACITY slots between guard bands, all of it the guard's NaN pattern wherever no stream's state is valid."""

    def __init__(self, offset):
        self.rcap, self.pcap, self.ucap = LC.state_caps()
        cap, self.Cmax = LC.STAGE_CAPACITY, LC.MAX_CHANNELS
        self.g = Guards(offset=offset)
        self.rhist, self.pend = self.g.output((cap, 2, self.rcap), name="rhist"), self.g.output((cap, 2, self.Cmax, self.pcap), name="pend")
        self.uhold, self.gprev = self.g.output((cap, 2, self.ucap), name="uhold"), self.g.output((cap, 2, self.Cmax), name="gprev")
        self.states = (self.rhist, self.pend, self.uhold, self.gprev)
        self.half = {s: 0 for s in range(cap)}
        self.valid = {}                                                       # slot -> (rv, C, pv, uv, frames > 0) of its current half
        self.btab, self._keep = back_table()

    def check(self):
        torch.cuda.synchronize()
        masks = [torch.ones(a.t.shape, dtype=torch.bool) for a in self.states]
        for s, (rv, Cn, pv, uv, framed) in self.valid.items():
            h = self.half[s]
            masks[0][s, h, :rv] = False
            masks[1][s, h, :Cn, :pv] = False
            masks[2][s, h, :uv] = False
            if framed:
                masks[3][s, h, :Cn] = False
        for a, m in zip(self.states, masks):
            a.check(expect_unwritten=m)

    def call(self, lib, p, rg, xg, og, gg, dg, cg, rows=None, blocks=None, **kw):
        a = dict(rhist=P(self.rhist), rcap=self.rcap, pend=P(self.pend), pcap=self.pcap, uhold=P(self.uhold), ucap=self.ucap, gprev=P(self.gprev),
                 Cmax=self.Cmax, capacity=LC.STAGE_CAPACITY, r=P(rg), n_r=p["n_r"], x=P(xg), n_x=p["n_x"], rates=self.btab, n_rates=len(LC.STAGE_RATES),
                 desc=P(dg), cap=P(cg), P=len(p["back"]) if rows is None else rows,
                 blocks=NB.floor_up_blocks(p["back"], [LC.back(sr) for sr in LC.STAGE_RATES], LC.STAGE_HOP) if blocks is None else blocks,
                 hop=LC.STAGE_HOP, rho=LC.RHO, out=P(og), n_out=og.t.numel(), gains=P(gg), n_gains=gg.t.numel())
        a.update(kw)
        return lib.wv_native_bank_floor_up_add(a["rhist"], a["rcap"], a["pend"], a["pcap"], a["uhold"], a["ucap"], a["gprev"], a["Cmax"], a["capacity"],
                                               a["r"], a["n_r"], a["x"], a["n_x"], a["rates"], a["n_rates"], a["desc"], a["cap"], a["P"], a["blocks"],
                                               a["hop"], a["rho"], a["out"], a["n_out"], a["gains"], a["n_gains"], stream())


def stage_data():
    ticks, totals = LC.floor_ticks()
    xs = [LC.stream_x(sr, LC.STAGE_HOP, Cn, totals[i], [i, 11], silent=1 if Cn == 2 else None) for i, (sr, Cn) in enumerate(LC.STAGE_STREAMS)]
    res = []
    for i, (sr, _) in enumerate(LC.STAGE_STREAMS):
        n = native.resampled_length(totals[i], sr, M)
        rng = np.random.default_rng([i, 12])
        env = np.exp(rng.uniform(np.log(1e-3), np.log(0.2), n // LC.STAGE_HOP + 1))[np.arange(n) // LC.STAGE_HOP]
        res.append((rng.standard_normal(n) * env).astype(np.float32))
    return ticks, totals, xs, res


def run_stage(offset: int, with_bad: bool):
    """Plays LC.floor_ticks through the entry point -> per stream (out, gains), and the per-tick state checks are made on the way."""
    lib = _lib.load()
    ticks, totals, xs, res = stage_data()
    twins = []
    for i, (sr, Cn) in enumerate(LC.STAGE_STREAMS):
        u = kernel_u(cu(res[i]), sr, totals[i])
        twins.append((u,) + LC.twin(xs[i], u, sr, LC.STAGE_HOP, LC.STAGE_CAPS[i]))
    st = Stage(offset)
    geo = [LC.back(sr) for sr in LC.STAGE_RATES]
    at, rat, t_out, frames = ([0] * len(xs) for _ in range(4))
    outs, gains = {i: [] for i in range(len(xs))}, {i: [] for i in range(len(xs))}
    served_bad = 0
    for j, tick in enumerate(ticks):
        p = LC.pack_floor_tick(tick, st.half)
        good, cap = p["back"], p["cap"]
        desc, n_out, n_gains = good, p["n_out"], p["n_gains"]
        if with_bad and j in (5, 6, 7):                                       # the pushes that fill the stages and the longest ones
            k = int(np.argmax(good[:, 9]))
            gb = good[k].copy()
            spare_o, spare_g = n_out, n_gains
            n_out, n_gains = n_out + int(gb[2] * gb[9]) + 1, n_gains + int(gb[2] * gb[16]) + 1
            gb[[0, 8, 19]] = (2, spare_o, spare_g)                            # the bad rows name slot 2 and outputs of their own
            args = (LC.STAGE_CAPACITY, st.rcap, st.pcap, st.ucap, st.Cmax, p["n_r"], p["n_x"], n_out, n_gains, geo, LC.STAGE_HOP)
            bad = [b for _, b in LC.bad_floor_rows(gb, *args)]
            assert not any(NB.native_bank_floor_up_row_ok(b, 1.0, *args) for b in bad)
            desc = np.concatenate([np.array(bad[::2], np.int64), good, np.array(bad[1::2], np.int64), gb[None]])
            cap = np.concatenate([np.ones(len(bad[::2]), np.float32), cap, np.ones(len(bad[1::2]), np.float32), [np.float32(np.inf)]])
            served_bad += len(bad) + 1                                        # and one good row whose cap is not finite
        g = Guards(offset=offset)
        xg = g.input(_fill(p["n_x"], [(int(r[6]), xs[i][:, at[i]:at[i] + int(r[7])]) for i, r in zip(p["order"], good)]), "x")
        rg = g.input(_fill(p["n_r"], [(int(r[4]), res[i][rat[i]:rat[i] + int(r[5])]) for i, r in zip(p["order"], good)]), "r")
        dg, cg = g.input(desc, "desc"), g.input(cap, "cap")
        og, gg = g.output((n_out,), name="out"), g.output((n_gains,), name="gains")
        snap = [a.t.clone() for a in st.states]
        assert st.call(lib, p, rg, xg, og, gg, dg, cg, rows=len(desc)) == 0, lib.wv_last_error()
        torch.cuda.synchronize()
        for a in (xg, rg, dg, cg):
            a.check()
        og.check(expect_unwritten=_mask(n_out, [(int(r[8]), int(r[2] * r[9])) for r in good]))
        gg.check(expect_unwritten=_mask(n_gains, [(int(r[19]), int(r[2] * r[16])) for r in good]))
        for i, r in zip(p["order"], good):
            Cn, k, nf, s, h = LC.STAGE_STREAMS[i][1], int(r[9]), int(r[16]), LC.STAGE_SLOTS[i], st.half[LC.STAGE_SLOTS[i]]
            outs[i].append(og.t[int(r[8]):int(r[8]) + Cn * k].view(Cn, k).cpu().numpy())
            gains[i].append(gg.t[int(r[19]):int(r[19]) + Cn * nf].view(Cn, nf).cpu().numpy())
            at[i], rat[i], t_out[i], frames[i] = at[i] + int(r[7]), rat[i] + int(r[5]), t_out[i] + k, frames[i] + nf
            for a, b in zip(st.states, snap):                                 # the half a row reads is unchanged; then it is stale
                assert torch.equal(a.t[s, h].view(torch.int32), b[s, h].view(torch.int32)), ("a launch wrote the half it reads", i)
                a.t[s, h].view(torch.int32).fill_(a.pattern)
            st.half[s] ^= 1
            uv2, pv2 = int(r[18]), int(r[13] + r[7] - r[9])
            st.valid[s] = (int(r[12]), Cn, pv2, uv2, frames[i] > 0)
            u, _, wg = twins[i]
            assert same(st.uhold.t[s, 1 - h, :uv2], u[t_out[i]:t_out[i] + uv2]), ("the held u", i, j)
            assert same(st.pend.t[s, 1 - h, :Cn, :pv2], xs[i][:, t_out[i]:t_out[i] + pv2]), ("the delay line", i, j)
            if frames[i]:
                assert same(st.gprev.t[s, 1 - h, :Cn], wg[:, frames[i] - 1]), ("the last frame's gains", i, j)
        st.check()                                                            # slots 2 and 4 and every stale half: still the pattern
    assert not with_bad or served_bad > 100
    assert at == totals and rat == [r.size for r in res] and t_out == totals
    return {i: (np.concatenate(outs[i], axis=1), np.concatenate(gains[i], axis=1)) for i in outs}, xs, twins


@functools.lru_cache(maxsize=None)
def _stage_once(offset):
    return run_stage(offset, False)


@pytest.mark.parametrize("offset", [0, 1])
def test_the_entry_point_is_the_twin_bit_for_bit_for_five_rates_in_one_call(offset):
    got, xs, twins = _stage_once(offset)
    kinds = set()
    for i, (sr, Cn) in enumerate(LC.STAGE_STREAMS):
        u, want, wg = twins[i]
        assert same(got[i][0], want), f"{sr}: not the twin's output"
        assert same(got[i][1], wg), f"{sr}: not the twin's gains"
        orig, nw = LC.back(sr)[:2]
        kinds |= CFC.kinds_of(wg, CF.frame_energy_var(u, CF.frame_starts(len(u), orig, nw, LC.STAGE_HOP)), np.float32(LC.STAGE_CAPS[i]))
        if Cn == 2:
            assert same(got[i][0][1], xs[i][1]) and np.abs(got[i][0][0] - xs[i][0]).max() > 0      # the silent channel: its own bits, +0 and -0
    assert {"capped", "uncapped", "rising", "falling"} <= kinds, kinds


def test_a_second_run_gives_the_same_bits_and_bad_rows_are_skipped_whole():
    got, _, _ = _stage_once(1)
    again, _, _ = run_stage(1, True)                                          # bad rows before and after the good ones on three ticks
    for i in got:
        assert same(got[i][0], again[i][0]) and same(got[i][1], again[i][1]), i


def test_refusals_write_nothing():
    lib = _lib.load()
    ticks, _, _, _ = stage_data()
    st = Stage(1)
    p = LC.pack_floor_tick(ticks[6], st.half)
    g = Guards(offset=1)
    xg, rg = g.input(np.zeros(p["n_x"], np.float32), "x"), g.input(np.zeros(p["n_r"], np.float32), "r")
    dg, cg = g.input(p["back"], "desc"), g.input(p["cap"], "cap")
    og, gg = g.output((p["n_out"],), name="out"), g.output((p["n_gains"],), name="gains")
    nr = len(LC.STAGE_RATES)

    def call(**kw):
        return st.call(lib, p, rg, xg, og, gg, dg, cg, **kw)

    def broken(**kw):
        t = (_lib.WvNativeRate * nr)(*[_lib.WvNativeRate(st.btab[i].kernels_t, st.btab[i].orig, st.btab[i].nw, st.btab[i].L, st.btab[i].width)
                                       for i in range(nr)])
        for k, v in kw.items():
            setattr(t[1], k, v)
        return t
    refused = [("rhist null", call(rhist=None)), ("pend null", call(pend=None)), ("uhold null", call(uhold=None)), ("gprev null", call(gprev=None)),
               ("r null", call(r=None)), ("x null", call(x=None)), ("out null", call(out=None)), ("gains null", call(gains=None)),
               ("desc null", call(desc=None)), ("cap null", call(cap=None)), ("rates null", call(rates=None)), ("capacity 0", call(capacity=0)),
               ("P = 65536", call(rows=65536)), ("P < 0", call(rows=-1)), ("blocks < 0", call(blocks=-1)), ("n_rates 9", call(n_rates=9)),
               ("orig 0", call(rates=broken(orig=0))), ("null table", call(rates=broken(kernels_t=None))), ("rcap 0", call(rcap=0)),
               ("pcap 0", call(pcap=0)), ("ucap 0", call(ucap=0)), ("Cmax 0", call(Cmax=0)), ("Cmax 65", call(Cmax=65)), ("n_r < 0", call(n_r=-1)),
               ("n_x < 0", call(n_x=-1)), ("n_out < 0", call(n_out=-1)), ("n_gains < 0", call(n_gains=-1)), ("hop 0", call(hop=0)),
               ("rho 0", call(rho=0.0)), ("rho nan", call(rho=float("nan"))), ("rho inf", call(rho=float("inf"))),
               ("a frame past the limit", call(hop=4097 * 441)), ("nw * hop past 2^31", call(hop=2 ** 31 - 1)),
               ("out overlaps x", call(out=P(xg))), ("out overlaps r", call(out=P(rg))), ("out overlaps pend", call(out=P(st.pend))),
               ("out overlaps uhold", call(out=P(st.uhold))), ("out overlaps gprev", call(out=P(st.gprev))), ("gains overlaps out", call(gains=P(og))),
               ("gains overlaps rhist", call(gains=P(st.rhist))), ("x overlaps pend", call(x=P(st.pend))), ("r overlaps uhold", call(r=P(st.uhold))),
               ("uhold overlaps rhist", call(uhold=P(st.rhist))), ("gprev overlaps pend", call(gprev=P(st.pend)))]
    for what, rc in refused:
        assert rc == -1, what
    assert call(hop=0) == -1 and b"wv_native_bank_floor_up_add" in lib.wv_last_error()
    assert call(rows=0) == 0 and call(blocks=0) == 0                          # nothing to do: success without a launch
    torch.cuda.synchronize()
    for a in (og, gg):
        a.check(expect_unwritten=torch.ones(a.t.shape, dtype=torch.bool))
    st.check()                                                                # every byte of the four states still the pattern
    for a in (xg, rg, dg, cg):
        a.check()


# ================================================================== the small nets
@functools.lru_cache(maxsize=None)
def _hip(cid):
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.nets import HipNet
    cfg, seed = W.net_config(NETS[cid])
    if NETS[cid][1] == "f32":
        cfg, sd, _ = W.oracle_net(NETS[cid])
    else:
        sd = random_state_dict(cfg, seed)
    return cfg, sd, HipNet(cfg, sd)


def generator(precision):
    return _hip("x6.generator" if precision == "f32" else "h.generator")[2]


def message(net, name) -> np.ndarray:
    return np.random.default_rng([ord(name), 3]).integers(0, 2, net.cfg.msg_dimension).astype(np.float32)


class RecordingEmbedBank(NB.NativeEmbedBank):
    """Keeps every slot's residual as the inner bank returned it."""

    def _residuals(self, ys, ticks, r_off, final):
        r = super()._residuals(ys, ticks, r_off, final)
        for s, t in ticks.items():
            self.__dict__.setdefault("residuals", {}).setdefault(s, []).append(r[r_off[s]:r_off[s] + t.n_res].clone())
        return r


class NullBank(StreamBank):
    """A 16 kHz inner bank of a generator's hop and halo that returns zeros: HostEmbedBank's state machine with nothing to compute."""

    def __init__(self, capacity, hop, H):
        super().__init__(capacity, hop, H, lambda win, slots: np.zeros_like(win), arrays=NumpyArrays(np.float32))

    def _on_open(self, slot, *message):
        pass


def mixed_on(gen, seed, silent=True):
    from waveverify_amd.window import halo
    steps, who = LC.mixed(gen.cfg.hop_length, halo(gen.cfg))
    T = NBC.BC.stream_lengths(steps)
    xs = {n: LC.stream_x(who[n][0], gen.cfg.hop_length, who[n][1], T[n], [seed, i], silent=1 if silent and who[n][1] == 2 and i % 2 == 0 else None)
          for i, n in enumerate(T)}
    return steps, who, xs


# ================================================================== 2. the cap never reached
def test_with_the_cap_never_reached_the_stream_is_the_floorless_banks_only_later():
    gen = generator("f32")
    steps, who, xs = mixed_on(gen, 1, silent=False)                           # a silent channel has Ex = 0: its gain is 0 at any floor
    dev = {n: cu(x) for n, x in xs.items()}
    strengths = {n: (1.0, 0.37)[i % 2] for i, n in enumerate(who)}

    class Bank(NB.NativeEmbedBank):
        def open(self, name, **kw):
            return super().open(message(gen, name), strength=strengths[name], **kw)
    plain, floored = Bank(gen, LC.MIX_RATES, NBC.BC.CAPACITY, LC.MAX_CHANNELS), Bank(gen, LC.MIX_RATES, NBC.BC.CAPACITY, LC.MAX_CHANNELS)
    floored.set_channel_snr_floor(-200.0)
    a, _ = NBC.run(plain, steps, dev, who, open_args=lambda n: (n,))
    b, _ = NBC.run(floored, steps, dev, who, open_args=lambda n: (n,))
    later = 0
    for n in a:
        ya, yb = torch.cat([r for _, _, r in a[n]], dim=1), torch.cat([r for _, _, r in b[n]], dim=1)
        assert ya.shape == yb.shape == dev[n].shape and same(ya, yb), n
        for (_, _, ra), (_, _, rb) in zip(a[n][:-1], b[n][:-1]):
            assert rb.shape[1] <= ra.shape[1] + LC.start(1, who[n][0], gen.cfg.hop_length)
            later += rb.shape[1] < ra.shape[1]
    assert later > 0 and plain.stats == floored.stats                         # the same stream and the same launches, only later


# ================================================================== 3. the bank under the floor
@pytest.mark.parametrize("both", [False, True], ids=["channel floor", "both floors"])
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_the_bank_is_the_twin_on_the_residuals_its_inner_bank_returned(precision, both):
    from waveverify_amd.window import halo
    gen = generator(precision)
    hop = gen.cfg.hop_length
    steps, who, xs = mixed_on(gen, 2)
    dev = {n: cu(x) for n, x in xs.items()}
    strengths = {n: (1.0, 0.37)[i % 2] for i, n in enumerate(who)}

    class Bank(RecordingEmbedBank):
        def open(self, name, **kw):
            return super().open(message(gen, name), strength=strengths[name], **kw)
    bank = Bank(gen, LC.MIX_RATES, NBC.BC.CAPACITY, LC.MAX_CHANNELS, precision)
    host = NB.HostEmbedBank(NullBank(NBC.BC.CAPACITY, hop, halo(gen.cfg)), LC.MIX_RATES, LC.MAX_CHANNELS, dtype=np.float32)
    for b in (bank, host):
        b.set_channel_snr_floor(LC.MIN_SNR_DB)
    if both:
        bank.set_snr_floor(30.0)
    gains, lag = {}, []

    def after(kind, slots):
        for s in slots:
            gains.setdefault(s, []).append(bank.gains(s))
            if kind == "push":
                lag.append(bank.latency_samples(s) - (bank.samples_in(s) - bank.samples_out(s)))
    out, slot = NBC.run(bank, steps, dev, who, open_args=lambda n: (n,), after=after)
    ref, _ = NBC.run(host, steps, xs, who, open_args=lambda n: (None,))
    taken = {s: list(v) for s, v in bank.residuals.items()}
    kinds = set()
    for n in out:
        assert [r.shape for _, _, r in out[n]] == [r.shape for _, _, r in ref[n]], (n, "not the host state machine's emission counts")
        res = torch.cat([taken[slot[n]].pop(0) for _ in out[n]])
        g = torch.cat([gains[slot[n]].pop(0) for _ in out[n]], dim=1)
        y = torch.cat([r for _, _, r in out[n]], dim=1)
        sr, Cn = who[n]
        assert y.shape == dev[n].shape
        u = kernel_u(res, sr, xs[n].shape[1])
        want, wg = LC.twin(xs[n], u, sr, hop, 1.0 if both else strengths[n])
        assert same(y, want), f"{precision} stream {n}: not the twin on its residual"
        assert same(g, wg), f"{precision} stream {n}: not the twin's gains"
        if xs[n].shape[1]:
            orig, nw = LC.back(sr)[:2]
            kinds |= CFC.kinds_of(wg, CF.frame_energy_var(u, CF.frame_starts(len(u), orig, nw, hop)), np.float32(1.0 if both else strengths[n]))
    assert all(not v for v in taken.values()) and min(lag) > 0 and {"capped", "rising", "falling"} <= kinds, kinds
    t = bank.stats["ticks"]
    assert t > 10 and bank.stats["uploads"] == bank.stats["front_launches"] == bank.stats["back_launches"] == t


# ================================================================== 4. the defect, end to end
def small_wv(precision):
    from waveverify_amd import WaveVerify
    cfg, sd, _ = _hip("x6.generator" if precision == "f32" else "h.generator")
    w = WaveVerify.__new__(WaveVerify)
    w.device = torch.device("cuda", torch.cuda.current_device())
    w._build({"generator": sd}, {"generator": cfg})
    w.sample_rate, w.watermark_bits = WaveVerify.DEFAULT_SAMPLE_RATE, cfg.msg_dimension
    w.set_precision(precision)
    return w


def test_a_silent_channel_of_a_live_stereo_feed_stays_silent_only_under_the_channel_floor():
    from waveverify_amd import WatermarkID
    w = small_wv("f32")
    hop = w.model.generator.cfg.hop_length
    sr, T = 48000, 180 * 48
    x = LC.stream_x(sr, hop, 2, T, [9], silent=1)
    x[0] = (0.1 * np.random.default_rng(9).standard_normal(T)).astype(np.float32)
    sizes = [480] * 4 + [960] * 2 + [2880] + [960] + [480] * 2                # 10, 20 and 60 ms packets, 180 ms
    assert sum(sizes) == T

    def run(bank):
        s = bank.open(WatermarkID.custom(0x1234), sample_rate=sr, channels=2)
        parts, at = [], 0
        for k in sizes:
            parts.append(bank.push({s: cu(x[:, at:at + k])})[s])
            at += k
        return torch.cat(parts + [bank.close(s)], dim=1).cpu().numpy()
    w.set_snr_floor(20.0)
    today = run(w.open_embed_bank(capacity=1, rates=(sr,)))
    assert today.shape == x.shape and np.count_nonzero(today[1]) > T // 2     # the 16 kHz floor alone: the residual lands on the silent channel
    w.set_snr_floor(None)
    w.set_channel_snr_floor(LC.MIN_SNR_DB)
    with pytest.raises(ValueError, match="open_native_embed_bank"):
        w.open_embed_bank(capacity=1, rates=(sr,))
    bank = w.open_native_embed_bank((sr,), capacity=1)
    assert type(bank) is NB.NativeEmbedBank and bank.channel_snr_floor_db == LC.MIN_SNR_DB
    bank.__class__ = RecordingEmbedBank                                       # the same bank, its residuals kept
    got = run(bank)
    assert same(got[1], x[1]), "the silent channel changed"
    orig, nw = LC.back(sr)[:2]
    u = kernel_u(torch.cat(bank.residuals[0]), sr, T)
    v = CF.numpy_channel_floor(x, u, orig, nw, hop, 1.0, LC.RHO, add=False)[0]
    assert same(got, np.where(v == 0, x, x + v)) and np.abs(v[0]).max() > 0 and not v[1].any()      # v is the watermark this output carries
    snr = CF.native_frame_snr_db(x[0], v[0], orig, nw, hop)
    assert (snr >= LC.MIN_SNR_DB - CFC.BOUND_DB).all(), snr.min()


# ================================================================== 5. against the whole recording
PACKETS = {"A": (48000, 2, 480), "B": (44100, 1, 882), "C": (8000, 3, 480)}    # 10, 20 and 60 ms packets


def packet_schedule(total_ms=180):
    steps = [("open", n) for n in PACKETS]
    at = {n: 0 for n in PACKETS}
    for ms in range(10, total_ms + 1, 10):
        push = {}
        for n, (sr, _, k) in PACKETS.items():
            if sr * ms // 1000 - at[n] >= k:
                push[n], at[n] = k, at[n] + k
        steps.append(("push", push))
    return steps + [("close", n) for n in PACKETS], {n: v[:2] for n, v in PACKETS.items()}


def worst_frame(got, whole, sr, hop):
    """The native frame that holds the largest difference -> (frame, its start, its end)."""
    m = int((got.double() - whole.double()).abs().max(dim=0).values.argmax())
    orig, nw = LC.back(sr)[:2]
    f = (m * orig) // (nw * hop)
    return f, LC.start(f, sr, hop), LC.start(f + 1, sr, hop)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_the_bank_against_embed_native_batch_under_the_channel_floor_on_the_whole_recording(precision):
    """RECORD (MI355X): exact f32 3.0e-8 / 3.0e-8 / 2.4e-7 (bar 2e-5); f16 against the f16 route 0 (bar 2e-5), against the exact route 3.0e-5 /
    1.8e-5 / 1.7e-5 (bar 1e-4); at 48 kHz stereo / 44.1 kHz mono / 8 kHz three channels."""
    w = small_wv(precision)
    gen = w.model.generator
    hop = gen.cfg.hop_length
    steps, who = packet_schedule()
    T = NBC.BC.stream_lengths(steps)
    xs = {n: cu(np.clip(0.1 * np.random.default_rng([4, i, T[n]]).standard_normal((who[n][1], T[n])), -1, 1).astype(np.float32))
          for i, n in enumerate(T)}
    strengths = {"A": 1.0, "B": 0.5, "C": 1.0}
    w.set_channel_snr_floor(LC.MIN_SNR_DB)
    try:
        class Bank(NB.NativeEmbedBank):
            def open(self, name, **kw):
                return super().open(message(gen, name), strength=strengths[name], **kw)
        bank = Bank(gen, (48000, 44100, 8000), 3, 3, precision)
        bank.set_channel_snr_floor(LC.MIN_SNR_DB)
        out, _ = NBC.run(bank, steps, xs, who, open_args=lambda n: (n,))
        for n, x in xs.items():
            sr = who[n][0]
            got = torch.cat([r for _, _, r in out[n]], dim=1)
            assert got.shape == x.shape and x.shape[1] > 1000 and float((got - x).abs().max()) > 0
            msg = cu(message(gen, n)[None])
            whole = w.embed_native_batch(x[None], sr, msg, strengths[n])[0]
            e = float((got.double() - whole.double()).abs().max())
            print(f"RECORD live channel floor {sr} C={who[n][1]} {precision} strength={strengths[n]}: against the whole input {e:.3e}"
                  f" (worst frame {worst_frame(got, whole, sr, hop)})")
            assert e <= 2e-5, worst_frame(got, whole, sr, hop)
            if precision != "f32":
                w.set_precision("f32")
                whole32 = w.embed_native_batch(x[None], sr, msg, strengths[n])[0]
                w.set_precision(precision)
                e32 = float((got.double() - whole32.double()).abs().max())
                print(f"RECORD live channel floor {sr} C={who[n][1]} {precision}: against the EXACT whole input {e32:.3e}"
                      f" (worst frame {worst_frame(got, whole32, sr, hop)})")
                assert e32 <= WM_BAR, worst_frame(got, whole32, sr, hop)
    finally:
        w.set_precision("f32")
        w.set_channel_snr_floor(None)
