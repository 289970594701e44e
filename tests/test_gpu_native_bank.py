"""Native-rate session banks on the GPU (csrc/wv_native.hip's bank entry points, waveverify_amd/native_bank.py).

1. The two stages alone through the C ABI, every arena between guard bands one element off alignment, the state NaN-poisoned wherever it is not
   valid: one call serves all five rates; per slot the concatenated outputs are native.downmix_resample / native.upsample_add of the whole
   recording BIT FOR BIT; a second run gives the same bits; unnamed slots keep their poison; bad rows are skipped whole; refusals write nothing.
2. Equal pushes at one rate: every bank output is the lockstep Native*Session's, bit for bit, f32 and f16.
3. The mixed schedule: each stream's result is the 16 kHz bank's on the same pieces of downmix_resample of its recording, bit for bit (for embed
   the residuals), and the embed output is upsample_add of that residual: the new code is exactly the two stages.
4. Each stream's embed output against embed_native_batch on its whole recording, by largest absolute difference.
5. The public route, and a slot re-opened at another rate and channel count.

Measured on the MI355X (RECORD lines, pytest -s; small generators of window_cases, 180 ms per stream in 10, 20 and 60 ms packets), a stream's
concatenated embed output against embed_native_batch on its whole recording by largest absolute difference:
    exact f32, bar 2e-5: 4.5e-8 at 48 kHz stereo, 3.0e-8 at 44.1 kHz mono (strength 0.5), 3.6e-7 at 8 kHz with three channels.
    f16 bank against the f16 route on the whole input, bar 2e-5: 0 at all three rates.  Against the EXACT route the f16 bank stands 2.7e-5
    (48 kHz), 1.5e-5 (44.1 kHz) and 2.1e-5 (8 kHz) off: the f16 mode's own distance from the exact path, asserted at WM_BAR = 1e-4."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import native_bank_cases as NBC
import window_cases as W
from guard import Guards
from waveverify_amd import _lib, native
from waveverify_amd import native_bank as NB
from waveverify_amd import native_session as NS

pytestmark = pytest.mark.gpu
M = NBC.M
WM_BAR = 1e-4                                                               # the f16 mode's watermarked samples against the exact path's (test_gpu_h16)
NAN = np.float32(np.nan)
NETS = {c[0]: c for c in W.net_cases()}


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t) -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.int32)


def P(arena):
    return arena.t.data_ptr()


def rate_tables():
    """-> (front table, back table, the device tensors they point to) over NBC.RATES."""
    pairs = [native.tables(sr, torch.device("cuda", torch.cuda.current_device())) for sr in NBC.RATES]
    mk = lambda ts: (_lib.WvNativeRate * len(ts))(*[_lib.WvNativeRate(t[0].data_ptr(), *t[1:]) for t in ts])      # noqa: E731
    return mk([p[0] for p in pairs]), mk([p[1] for p in pairs]), pairs


# ================================================================== 1. the stages alone
def _fill(n, rows):
    """A packed input arena: NaN in the gaps nobody may read."""
    a = np.full(n, NAN, np.float32)
    for off, v in rows:
        a[off:off + v.size] = v.reshape(-1)
    return a


def _mask(n, ranges):
    m = torch.ones(n, dtype=torch.bool)
    for off, k in ranges:
        m[off:off + k] = False
    return m


class Stages:
    """The state of a bank of NBC.STAGE_CAPACITY slots between guard bands, all of it the guard's NaN pattern wherever no stream's state is valid."""

    def __init__(self):
        self.hcap, self.rcap, self.pcap = NBC.state_caps()
        cap, self.Cmax = NBC.STAGE_CAPACITY, NBC.MAX_CHANNELS
        self.g = Guards(offset=1)
        self.hist, self.rhist = self.g.output((cap, 2, self.hcap), name="hist"), self.g.output((cap, 2, self.rcap), name="rhist")
        self.pend = self.g.output((cap, 2, self.Cmax, self.pcap), name="pend")
        self.half = {s: 0 for s in range(cap)}
        self.valid = {}                                                       # slot -> (hv, rv, C, pv) of its current half
        self.ftab, self.btab, self._keep = rate_tables()

    def expect(self):
        """The masks of the state elements that must still hold the poison pattern."""
        mh, mr, mp = (torch.ones(a.t.shape, dtype=torch.bool) for a in (self.hist, self.rhist, self.pend))
        for s, (hv, rv, Cn, pv) in self.valid.items():
            h = self.half[s]
            mh[s, h, :hv] = False
            mr[s, h, :rv] = False
            mp[s, h, :Cn, :pv] = False
        return mh, mr, mp

    def check(self):
        torch.cuda.synchronize()
        for a, m in zip((self.hist, self.rhist, self.pend), self.expect()):
            a.check(expect_unwritten=m)

    def down(self, lib, p, x, y, desc, n_rows=None, blocks=None):
        return lib.wv_native_bank_down(P(self.hist), NBC.STAGE_CAPACITY, self.hcap, P(x), p["n_x"], self.ftab, len(NBC.RATES), P(desc),
                                       len(p["front"]) if n_rows is None else n_rows, NB.down_blocks(p["front"]) if blocks is None else blocks, P(y),
                                       y.t.numel(), stream())

    def up(self, lib, p, r, x, out, desc, gain, n_rows=None, blocks=None):
        return lib.wv_native_bank_up_add(P(self.rhist), self.rcap, P(self.pend), self.pcap, self.Cmax, NBC.STAGE_CAPACITY, P(r), p["n_r"], P(x), p["n_x"],
                                         self.btab, len(NBC.RATES), P(desc), P(gain), len(p["back"]) if n_rows is None else n_rows,
                                         NB.up_blocks(p["back"]) if blocks is None else blocks, P(out), out.t.numel(), stream())

    def roll(self, tick, snap):
        """After a tick: the half a named slot's row read is unchanged (then re-poisoned here), its bit flips, its valid lengths move on."""
        for i, t in tick.items():
            s, h = NBC.STAGE_SLOTS[i], self.half[NBC.STAGE_SLOTS[i]]
            for a, b in zip((self.hist, self.rhist, self.pend), snap):
                assert torch.equal(a.t[s, h].view(torch.int32), b[s, h].view(torch.int32)), ("a launch wrote the half it reads", i)
                a.t[s, h].view(torch.int32).fill_(a.pattern)
            self.half[s] ^= 1
            self.valid[s] = (t.front.hv2, t.back.hv2, NBC.STREAMS[i][1], t.pv2)


def run_stages(with_bad: bool):
    """Plays NBC.stage_ticks through the two entry points -> ({stream: y bits}, {stream: out bits})."""
    lib = _lib.load()
    ticks, totals = NBC.stage_ticks()
    st = Stages()
    fgeo = [native.table_geometry(sr, M) for sr in NBC.RATES]
    bgeo = [native.table_geometry(M, sr) for sr in NBC.RATES]
    xs = [np.random.default_rng([i, 11]).uniform(-NBC.PEAK, NBC.PEAK, (Cn, totals[i])).astype(np.float32) for i, (_, Cn) in enumerate(NBC.STREAMS)]
    res = [np.random.default_rng([i, 12]).uniform(-NBC.PEAK, NBC.PEAK, native.resampled_length(totals[i], sr, M)).astype(np.float32)
           for i, (sr, _) in enumerate(NBC.STREAMS)]
    at, rat = [0] * len(xs), [0] * len(xs)
    ys, outs = {i: [] for i in range(len(xs))}, {i: [] for i in range(len(xs))}
    served_bad = 0
    for j, tick in enumerate(ticks):
        p = NBC.pack_tick(tick, st.half)
        front, back, gain = p["front"], p["back"], p["gain"]
        spare_y, spare_o = p["n_y"], p["n_out"]
        n_y, n_out = p["n_y"], p["n_out"]
        if with_bad and j in (6, 7):                                          # the tile-crossing tick and the longest pushes
            k = int(np.argmax(front[:, 7]))
            gf, gb = front[k].copy(), back[k].copy()
            n_y, n_out = n_y + int(gf[7]) + 1, n_out + int(gb[2] * gb[9]) + 1
            gf[[0, 6]], gb[[0, 8]] = (2, spare_y), (2, spare_o)               # the bad rows name slot 2 and outputs of their own
            bad_f = [b for _, b in NBC.bad_down_rows(gf, NBC.STAGE_CAPACITY, st.hcap, p["n_x"], n_y, fgeo)]
            bad_b = [b for _, b in NBC.bad_up_rows(gb, NBC.STAGE_CAPACITY, st.rcap, st.pcap, st.Cmax, p["n_r"], p["n_x"], n_out, bgeo)]
            assert not any(NB.native_bank_down_row_ok(b, NBC.STAGE_CAPACITY, st.hcap, p["n_x"], n_y, fgeo) for b in bad_f)
            assert not any(NB.native_bank_up_row_ok(b, NBC.STAGE_CAPACITY, st.rcap, st.pcap, st.Cmax, p["n_r"], p["n_x"], n_out, bgeo) for b in bad_b)
            front = np.concatenate([np.array(bad_f[::2], np.int64), front, np.array(bad_f[1::2], np.int64)])
            back = np.concatenate([np.array(bad_b[::2], np.int64), back, np.array(bad_b[1::2], np.int64)])
            gain = np.concatenate([np.ones(len(bad_b[::2]), np.float32), gain, np.ones(len(bad_b[1::2]), np.float32)])
            served_bad += len(bad_f) + len(bad_b)
        good_f, good_b = p["front"], p["back"]
        g = Guards(offset=1)
        xg = g.input(_fill(p["n_x"], [(int(r[4]), xs[i][:, at[i]:at[i] + int(r[5])]) for i, r in zip(p["order"], good_f)]), "x")
        rg = g.input(_fill(p["n_r"], [(int(r[4]), res[i][rat[i]:rat[i] + int(r[5])]) for i, r in zip(p["order"], good_b)]), "r")
        fd, bd, gg = g.input(front, "front desc"), g.input(back, "back desc"), g.input(gain, "gain")
        yg, og = g.output((n_y,), name="y"), g.output((n_out,), name="out")
        snap = [a.t.clone() for a in (st.hist, st.rhist, st.pend)]
        q = dict(p, front=front, back=back)
        assert st.down(lib, q, xg, yg, fd, blocks=NB.down_blocks(good_f)) == 0, lib.wv_last_error()
        assert st.up(lib, q, rg, xg, og, bd, gg, blocks=NB.up_blocks(good_b)) == 0, lib.wv_last_error()
        torch.cuda.synchronize()
        for a in (xg, rg, fd, bd, gg):
            a.check()
        yg.check(expect_unwritten=_mask(n_y, [(int(r[6]), int(r[7])) for r in good_f]))
        og.check(expect_unwritten=_mask(n_out, [(int(r[8]), int(r[2] * r[9])) for r in good_b]))
        for i, rf, rb in zip(p["order"], good_f, good_b):
            Cn = NBC.STREAMS[i][1]
            ys[i].append(yg.t[int(rf[6]):int(rf[6] + rf[7])].cpu().numpy())
            outs[i].append(og.t[int(rb[8]):int(rb[8] + Cn * rb[9])].view(Cn, int(rb[9])).cpu().numpy())
            at[i], rat[i] = at[i] + int(rf[5]), rat[i] + int(rb[5])
        st.roll(tick, snap)
        st.check()                                                            # slots 2 and 4 and every stale half: still poison
    assert not with_bad or served_bad > 50
    assert at == totals and rat == [r.size for r in res]
    return ({i: np.concatenate(v) for i, v in ys.items()}, {i: np.concatenate(v, axis=1) for i, v in outs.items()}), xs, res


@functools.lru_cache(maxsize=None)
def _stages_once():
    return run_stages(False)


def test_stages_are_the_file_kernels_bit_for_bit_for_five_rates_in_one_call():
    (ys, outs), xs, res = _stages_once()
    for i, (sr, Cn) in enumerate(NBC.STREAMS):
        want_y = native.downmix_resample(cu(xs[i][None]), sr)[0, 0]
        assert ys[i].shape == tuple(want_y.shape) and np.array_equal(bits(ys[i]), bits(want_y)), f"{sr}: not downmix_resample's bits"
        want = native.upsample_add(cu(xs[i][None]), cu(res[i][None]), sr, NBC.STAGE_GAINS[i])[0]
        assert outs[i].shape == tuple(want.shape) and np.array_equal(bits(outs[i]), bits(want)), f"{sr}: not upsample_add's bits"


def test_a_second_run_gives_the_same_bits_and_bad_rows_are_skipped_whole():
    (ys, outs), _, _ = _stages_once()
    (ys2, outs2), _, _ = run_stages(True)                                     # with bad rows before and after the good ones on two ticks
    for i in ys:
        assert np.array_equal(bits(ys[i]), bits(ys2[i])) and np.array_equal(bits(outs[i]), bits(outs2[i])), i


def test_refusals_write_nothing():
    lib = _lib.load()
    ticks, totals = NBC.stage_ticks()
    st = Stages()
    p = NBC.pack_tick(ticks[6], st.half)                                      # the tile-crossing pushes
    g = Guards(offset=1)
    xg, rg = g.input(np.zeros(p["n_x"], np.float32), "x"), g.input(np.zeros(p["n_r"], np.float32), "r")
    fd, bd, gg = g.input(p["front"], "front desc"), g.input(p["back"], "back desc"), g.input(p["gain"], "gain")
    yg, og = g.output((p["n_y"],), name="y"), g.output((p["n_out"],), name="out")
    Pn, cap = len(p["front"]), NBC.STAGE_CAPACITY
    nr = len(NBC.RATES)
    bad_rate = (_lib.WvNativeRate * nr)(*[_lib.WvNativeRate(st.ftab[i].kernels_t, st.ftab[i].orig, st.ftab[i].nw, st.ftab[i].L, st.ftab[i].width)
                                          for i in range(nr)])

    def down(hist=P(st.hist), capacity=cap, hcap=st.hcap, x=P(xg), n_x=p["n_x"], rates=st.ftab, n_rates=nr, desc=P(fd), rows=Pn, blocks=4, y=P(yg),
             n_y=p["n_y"]):
        return lib.wv_native_bank_down(hist, capacity, hcap, x, n_x, rates, n_rates, desc, rows, blocks, y, n_y, stream())

    def up(rhist=P(st.rhist), rcap=st.rcap, pend=P(st.pend), pcap=st.pcap, Cmax=st.Cmax, capacity=cap, r=P(rg), n_r=p["n_r"], x=P(xg), n_x=p["n_x"],
           rates=st.btab, n_rates=nr, desc=P(bd), gain=P(gg), rows=Pn, blocks=4, out=P(og), n_out=p["n_out"]):
        return lib.wv_native_bank_up_add(rhist, rcap, pend, pcap, Cmax, capacity, r, n_r, x, n_x, rates, n_rates, desc, gain, rows, blocks, out, n_out,
                                         stream())

    def broken(**kw):
        t = (_lib.WvNativeRate * nr)(*[_lib.WvNativeRate(bad_rate[i].kernels_t, bad_rate[i].orig, bad_rate[i].nw, bad_rate[i].L, bad_rate[i].width)
                                       for i in range(nr)])
        for k, v in kw.items():
            setattr(t[1], k, v)
        return t
    refused = [("hist null", down(hist=None)), ("x null", down(x=None)), ("y null", down(y=None)), ("desc null", down(desc=None)),
               ("rates null", down(rates=None)), ("capacity 0", down(capacity=0)), ("capacity past the limit", down(capacity=1048577)),
               ("P < 0", down(rows=-1)), ("P = 65536", down(rows=65536)), ("n_rates 0", down(n_rates=0)), ("n_rates 9", down(n_rates=9)),
               ("orig 0", down(rates=broken(orig=0))), ("nw 0", down(rates=broken(nw=0))), ("L 0", down(rates=broken(L=0))),
               ("width -1", down(rates=broken(width=-1))), ("null table", down(rates=broken(kernels_t=None))),
               ("LDS window past 64 KB", down(rates=broken(orig=64, nw=1, L=2 * 8200 + 64, width=8200))), ("hcap 0", down(hcap=0)),
               ("n_x < 0", down(n_x=-1)), ("n_y < 0", down(n_y=-1)), ("blocks < 0", down(blocks=-1)),
               ("x overlaps y", down(x=P(yg))), ("y overlaps hist", down(y=P(st.hist))), ("x overlaps hist", down(x=P(st.hist))),
               ("rhist null", up(rhist=None)), ("pend null", up(pend=None)), ("r null", up(r=None)), ("x null", up(x=None)), ("out null", up(out=None)),
               ("desc null", up(desc=None)), ("gain null", up(gain=None)), ("rates null", up(rates=None)), ("capacity 0", up(capacity=0)),
               ("P = 65536", up(rows=65536)), ("n_rates 9", up(n_rates=9)), ("orig 0", up(rates=broken(orig=0))), ("rcap 0", up(rcap=0)),
               ("pcap 0", up(pcap=0)), ("Cmax 0", up(Cmax=0)), ("Cmax 65", up(Cmax=65)), ("n_r < 0", up(n_r=-1)), ("n_out < 0", up(n_out=-1)),
               ("out overlaps x", up(out=P(xg))), ("out overlaps r", up(out=P(rg))), ("out overlaps pend", up(out=P(st.pend))),
               ("out overlaps rhist", up(out=P(st.rhist))), ("x overlaps pend", up(x=P(st.pend))), ("r overlaps rhist", up(r=P(st.rhist))),
               ("pend overlaps rhist", up(pend=P(st.rhist)))]
    for what, rc in refused:
        assert rc == -1, what
        assert b"wv_native_bank_" in lib.wv_last_error(), what
    assert down(rows=0) == 0 and up(rows=0) == 0 and down(blocks=0) == 0      # nothing to do: success without a launch
    torch.cuda.synchronize()
    for a in (yg, og):
        a.check(expect_unwritten=torch.ones(a.t.shape, dtype=torch.bool))
    st.check()                                                                # every byte of the state still poison
    for a in (xg, rg, fd, bd, gg):
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


def nets(precision):
    ids = ("x6.generator", "x6.detector", "x14.locator") if precision == "f32" else ("h.generator", "h.detector", "h.locator")
    return [_hip(i)[2] for i in ids]


def message(net, name) -> np.ndarray:
    return np.random.default_rng([ord(name), 3]).integers(0, 2, net.cfg.msg_dimension).astype(np.float32)


def clip_data(steps, who, seed=0):
    """The suite's synthetic level (0.1 N(0, 1)) on every channel -> {stream: [C, T] device tensor}."""
    out = {}
    for i, (name, T) in enumerate(NBC.BC.stream_lengths(steps).items()):
        r = np.random.default_rng([seed, i, T, 5])
        out[name] = cu(np.clip(0.1 * r.standard_normal((who[name][1], T)), -1.0, 1.0).astype(np.float32))
    return out


def same_state(a, b, what):
    assert a.samples_seen == b.samples_seen and torch.equal(a.mean_prob, b.mean_prob) and torch.equal(a.bits, b.bits), what


def seg_key(s):
    return (s.frames, s.start_s, s.end_s, s.coverage, s.confidence, str(s.watermark), None if s.prob is None else s.prob.tobytes())


def counters_say_one_launch_per_stage_and_tick(bank, embed):
    n = bank.stats["ticks"]
    assert n > 0 and bank.stats["front_launches"] == n and bank.stats["uploads"] == n and bank.stats["back_launches"] == (n if embed else 0)


# ================================================================== 2. equal pushes are the lockstep native session
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("kind", ["embed", "detect", "locate", "segment"])
def test_equal_pushes_are_the_lockstep_native_session_bit_for_bit(kind, precision):
    gen, det, loc = nets(precision)
    sr, S = 44100, 3
    net = {"embed": gen, "detect": det, "locate": loc, "segment": det}[kind]
    steps, who, sizes = NBC.equal(sr, net.cfg.hop_length)
    xs = clip_data(steps, who)
    names = list(xs)
    x = torch.stack([xs[n] for n in names])
    if kind == "embed":
        bank = NB.NativeEmbedBank(gen, (sr,), S, 2, precision)
        sess = NS.NativeEmbedSession(gen, np.stack([message(gen, n) for n in names]), sr, 2, 1.0, precision)
        open_args = lambda n: (message(gen, n),)                              # noqa: E731
    elif kind == "segment":
        kw = dict(min_gap_frames=1, min_len_frames=1, precision=precision)
        bank, sess, open_args = NB.NativeSegmentBank(det, loc, (sr,), S, 2, **kw), NS.NativeSegmentSession(det, loc, S, sr, 2, **kw), lambda n: ()
    else:
        cls_b, cls_s = (NB.NativeDetectBank, NS.NativeDetectSession) if kind == "detect" else (NB.NativeLocateBank, NS.NativeLocateSession)
        bank, sess, open_args = cls_b(net, (sr,), S, 2, precision), cls_s(net, S, sr, 2, precision), lambda n: ()
    out, slot = NBC.run(bank, steps, xs, who, open_args=open_args)
    want, at = [], 0
    for n in sizes:
        want.append(sess.push(x[:, :, at:at + n]))
        at += n
    if kind == "segment":
        polled = sess.poll()
        last = sess.flush()
        for s, n in enumerate(names):
            assert [seg_key(v) for v in out[n][-1][2]] == [seg_key(v) for v in list(polled[s]) + list(last[s])], (kind, precision, n)
        counters_say_one_launch_per_stage_and_tick(bank, False)
        return
    want.append(sess.flush())
    for s, n in enumerate(names):
        assert len(out[n]) == len(want)
        for i, ((_, _, got), w) in enumerate(zip(out[n], want)):
            what = f"{kind} {precision} stream {n} step {i}"
            if kind == "detect":
                from waveverify_amd.session import DetectState
                same_state(got, DetectState(w.mean_prob[s], w.bits[s], w.samples_seen), what)
            elif kind == "locate":
                assert got.shape == w[s, 0].shape and torch.equal(got, w[s, 0]), what
            else:
                assert got.shape == w[s].shape and torch.equal(got, w[s]), what
    counters_say_one_launch_per_stage_and_tick(bank, kind == "embed")


# ================================================================== 3. the mixed schedule is the 16 kHz bank behind the front stage
class RecordingEmbedBank(NB.NativeEmbedBank):
    """Keeps every slot's residual as the inner bank returned it."""

    def _residuals(self, ys, ticks, r_off, final):
        r = super()._residuals(ys, ticks, r_off, final)
        for s, t in ticks.items():
            self.__dict__.setdefault("residuals", {}).setdefault(s, []).append(r[r_off[s]:r_off[s] + t.n_res].clone())
        return r


def play_16k(ref, steps, xs, who, open_args, join):
    """The same schedule on a 16 kHz bank, each piece what the front stage makes final of downmix_resample of the whole recording."""
    x16 = {n: native.downmix_resample(x[None], who[n][0])[0, 0] if x.shape[1] else x.new_zeros(0) for n, x in xs.items()}
    plans = {n: NS.StagePlan(*native.table_geometry(who[n][0], M)) for n in xs}
    slot, at, out = {}, {}, {}
    for kind, arg in steps:
        if kind == "open":
            slot[arg], at[arg], out[arg] = ref.open(*open_args(arg)), 0, []
        elif kind == "close":
            k = plans[arg].flush().n_out
            first = ref.push({slot[arg]: x16[arg][at[arg]:at[arg] + k]})
            assert at[arg] + k == x16[arg].shape[0]
            out[arg].append(join(None if first is None else first[slot[arg]], ref.close(slot[arg])))
        else:
            ks = {n: plans[n].push(m).n_out for n, m in arg.items()}
            res = ref.push({slot[n]: x16[n][at[n]:at[n] + k] for n, k in ks.items()})
            for n, k in ks.items():
                at[n] += k
                out[n].append(None if res is None else res[slot[n]])
    return out


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("kind", ["embed", "detect", "locate", "segment"])
def test_mixed_rates_are_the_16k_bank_behind_the_front_stage_bit_for_bit(kind, precision):
    from waveverify_amd.session import DetectBank, EmbedBank, LocateBank, SegmentBank
    gen, det, loc = nets(precision)
    net = {"embed": gen, "detect": det, "locate": loc, "segment": det}[kind]
    from waveverify_amd.window import halo
    from waveverify_amd.session import segment_halo
    H = segment_halo(det.cfg, loc.cfg) if kind == "segment" else halo(net.cfg)
    steps, who = NBC.mixed(net.cfg.hop_length, H)
    xs = clip_data(steps, who, seed=2)
    cap, Cm = NBC.BC.CAPACITY, NBC.MAX_CHANNELS
    cat = lambda a, b: torch.cat([a, b])                                      # noqa: E731
    if kind == "embed":
        gains = {n: (1.0, 0.37)[i % 2] for i, n in enumerate(who)}

        class Bank(RecordingEmbedBank):
            def open(self, name, **kw):
                return super().open(message(gen, name), strength=gains[name], **kw)
        bank = Bank(gen, NBC.RATES, cap, Cm, precision)
        out, slot = NBC.run(bank, steps, xs, who, open_args=lambda n: (n,))
        ref = play_16k(EmbedBank(gen, cap, precision, 1.5, None, add_input=False), steps, xs, who, lambda n: (message(gen, n),), cat)
        # slots are reused (G takes B's, Z takes C's): walk the recorded residuals per slot in stream order
        taken = {s: list(v) for s, v in bank.residuals.items()}
        for n in out:
            got_r = [taken[slot[n]].pop(0) for _ in out[n]]
            assert len(got_r) == len(ref[n])
            for i, (a, b) in enumerate(zip(got_r, ref[n])):
                assert a.shape == b.shape and torch.equal(a, b), f"embed {precision} stream {n} step {i}: not the 16 kHz bank's residual"
            y = torch.cat([r for _, _, r in out[n]], dim=1)
            assert y.shape == xs[n].shape
            if xs[n].shape[1]:
                want = native.upsample_add(xs[n][None], torch.cat(got_r)[None], who[n][0], gains[n])[0]
                assert torch.equal(y, want), f"embed {precision} stream {n}: not upsample_add of its residual"
        assert all(not v for v in taken.values())
        counters_say_one_launch_per_stage_and_tick(bank, True)
        return
    if kind == "segment":
        kw = dict(min_gap_frames=1, min_len_frames=1, precision=precision)
        bank, ref_bank = NB.NativeSegmentBank(det, loc, NBC.RATES, cap, Cm, **kw), SegmentBank(det, loc, cap, **kw)
        join = lambda a, b: b                                                 # noqa: E731
    else:
        cls_b, cls_r = (NB.NativeDetectBank, DetectBank) if kind == "detect" else (NB.NativeLocateBank, LocateBank)
        bank, ref_bank = cls_b(net, NBC.RATES, cap, Cm, precision), cls_r(net, cap, precision)
        join = (lambda a, b: b) if kind == "detect" else cat
    out, _ = NBC.run(bank, steps, xs, who)
    ref = play_16k(ref_bank, steps, xs, who, lambda n: (), join)
    for n in out:
        assert len(out[n]) == len(ref[n])
        for i, ((_, _, got), want) in enumerate(zip(out[n], ref[n])):
            what = f"{kind} {precision} stream {n} step {i}"
            if kind == "detect":
                same_state(got, want, what)
            elif kind == "locate":
                assert got.shape == want.shape and torch.equal(got, want), what
            elif got is not None or want is not None:
                assert [seg_key(v) for v in got] == [seg_key(v) for v in want], what
    counters_say_one_launch_per_stage_and_tick(bank, False)


# ================================================================== 4. against the whole recording
def small_wv(cid):
    from waveverify_amd import WaveVerify
    cfg, sd, _ = _hip(cid)
    w = WaveVerify.__new__(WaveVerify)
    w.device = torch.device("cuda", torch.cuda.current_device())
    w._build({"generator": sd}, {"generator": cfg})
    w.sample_rate, w.watermark_bits = WaveVerify.DEFAULT_SAMPLE_RATE, cfg.msg_dimension
    return w


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


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_embed_bank_against_embed_native_batch_on_the_whole_recording(precision):
    """RECORD (MI355X): exact f32 4.5e-8 / 3.0e-8 / 3.6e-7 (bar 2e-5); f16 against the f16 route 0 (bar 2e-5), against the exact route 2.7e-5 /
    1.5e-5 / 2.1e-5 (bar 1e-4); at 48 kHz stereo / 44.1 kHz mono / 8 kHz three channels."""
    w = small_wv("x6.generator" if precision == "f32" else "h.generator")
    gen = w.model.generator
    steps, who = packet_schedule()
    xs = clip_data(steps, who, seed=4)
    gains = {"A": 1.0, "B": 0.5, "C": 1.0}
    w.set_precision(precision)
    try:
        class Bank(NB.NativeEmbedBank):
            def open(self, name, **kw):
                return super().open(message(gen, name), strength=gains[name], **kw)
        bank = Bank(gen, (48000, 44100, 8000), 3, 3, precision)
        out, _ = NBC.run(bank, steps, xs, who, open_args=lambda n: (n,))
        for n, x in xs.items():
            got = torch.cat([r for _, _, r in out[n]], dim=1)
            assert got.shape == x.shape and x.shape[1] > 1000 and float((got - x).abs().max()) > 0
            msg = cu(message(gen, n)[None])
            whole = w.embed_native_batch(x[None], who[n][0], msg, gains[n])[0]
            e = float((got.double() - whole.double()).abs().max())
            print(f"RECORD native bank {who[n][0]} C={who[n][1]} {precision} strength={gains[n]}: against the whole input {e:.3e}")
            assert e <= 2e-5
            if precision != "f32":
                w.set_precision("f32")
                e32 = float((got.double() - w.embed_native_batch(x[None], who[n][0], msg, gains[n])[0].double()).abs().max())
                w.set_precision(precision)
                print(f"RECORD native bank {who[n][0]} C={who[n][1]} {precision}: against the EXACT whole input {e32:.3e}")
                assert e32 <= WM_BAR
    finally:
        w.set_precision("f32")


# ================================================================== 5. the public route
def test_public_route_and_a_slot_reopened_at_another_rate():
    from waveverify_amd import WatermarkID
    from waveverify_amd.session import EmbedBank
    w = small_wv("x6.generator")
    w.set_precision("f32")
    ids = [WatermarkID.custom(0x1234), WatermarkID.custom(0xBEEF)]
    assert type(w.open_embed_bank(capacity=2)) is EmbedBank                  # today's object with today's arguments
    rng = np.random.default_rng(8)
    a, b = cu(0.1 * rng.standard_normal((2, 3000)).astype(np.float32)), cu(0.1 * rng.standard_normal((3, 900)).astype(np.float32))

    def second(bank):
        s = bank.open(ids[1], sample_rate=8000, channels=3, strength=0.5)
        return s, torch.cat([bank.push({s: b[:, :400]})[s], bank.push({s: b[:, 400:]})[s], bank.close(s)], dim=1)
    used = w.open_embed_bank(capacity=2, rates=(48000, 8000), max_channels=3)
    assert isinstance(used, NB.NativeEmbedBank) and used.rates == (48000, 8000) and used.max_channels == 3
    s = used.open(ids[0], sample_rate=48000, channels=2)
    first = torch.cat([used.push({s: a[:, :1700]})[s], used.push({s: a[:, 1700:]})[s], used.close(s)], dim=1)
    assert first.shape == a.shape and used.latency_samples is not None
    s2, got = second(used)
    s3, want = second(w.open_embed_bank(capacity=2, rates=(48000, 8000), max_channels=3))
    assert s2 == s3 == s == 0 and got.shape == b.shape and torch.equal(got, want)
    other = second(w.open_embed_bank(capacity=2, rates=(8000,), max_channels=3))[1]
    assert torch.equal(got, other)                                            # and the rate table's other entries do not show
    with pytest.raises(ValueError, match="22050"):
        used.open(ids[0], sample_rate=22050)
    with pytest.raises(ValueError, match="44101"):
        w.open_embed_bank(rates=(44101,))
