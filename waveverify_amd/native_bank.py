"""Session banks at the streams' own sample rates and channel counts.

`session.py`'s banks let 16 kHz mono streams open, push and close on their own; `native_session.py` lets streams in lockstep keep their rate and
channels.  Here every slot of a bank has its OWN rate (one of the bank's `rates`), channel count, packet length and resampler state:

    front stage   every pushed slot's new samples -> f32 channel mean -> 16 kHz, ONE launch per tick (wv_native_bank_down)
    inner bank    the 16 kHz bank of session.py (the generator returning its residual alone)
    back stage    every slot's residual -> its own rate, strength times it added to its delayed originals, ONE launch (wv_native_bank_up_add)

whatever the mix of rates on the tick.  Under set_channel_snr_floor the back stage is wv_native_bank_floor_up_add instead: whole native frames
leave per tick, with the held residual and the last frame's gains as two more ping-pong states.  The integer plans are native_session's StagePlan / EmbedPlan, one per slot; a tick turns them into
descriptor rows.  The stages' state is ping-pong per slot: a row's `half` names the half holding the slot's state, the launch writes the next
state into the other, and the bank flips the bit of every slot the tick named.  The Host* classes run the state machine on numpy arrays (any
float dtype) through numpy_bank_down / numpy_bank_up_add, which restate the kernels row rule included; the Native* classes bind it to the HIP
entry points and the HipNet banks, where there is no CPU fallback.  A bank's arrays come from its inner bank's backend (session.NumpyArrays /
TorchArrays), and its slot table is the inner bank's."""
from __future__ import annotations

import numpy as np

from . import _lib, channel_floor, native, snr_floor
from .native import MODEL_RATE
from .native_session import EmbedPlan, EmbedTick, StagePlan, StageTick, numpy_down, numpy_resample, numpy_up_add
from .session import DetectBank, EmbedBank, LocateBank, NumpyArrays, SegmentBank, plan_tick

MAX_RATES = 8                                        # WV_NATIVE_BANK_MAX_RATES
MAX_COUNT = 2 ** 31 - 257                            # the largest sample count of a descriptor row
TILE = 256
FLOOR_DESC = 21                                      # fields of a wv_native_bank_floor_up_add descriptor row
FLOOR_MAX_NF, FLOOR_U_FLOATS, FLOOR_G_FLOATS = 16, 8192, 17 * 64      # csrc/wv_live_floor.hip's LF_MAX_NF, LF_U_FLOATS, LF_G_FLOATS


def _tiles(v: int) -> int:
    return -(-int(v) // TILE)


def check_rates(rates) -> tuple:
    """-> the bank's rates as a tuple of distinct ints; ValueError for none, more than 8, a repeat or a rate native.check_rate refuses."""
    rates = tuple(int(r) for r in rates)
    if not 1 <= len(rates) <= MAX_RATES:
        raise ValueError(f"a native-rate bank serves 1 to {MAX_RATES} distinct sample rates, got {len(rates)}")
    if len(set(rates)) != len(rates):
        raise ValueError(f"the rates of a bank must be distinct, got {rates}")
    for r in rates:
        native.check_rate(r)
    return rates


# ---------------------------------------------------------------------------------------------------------------- the row rule
def _roll_ok(cap: int, valid: int, fresh: int, drop: int, nxt: int) -> bool:
    return 0 <= valid <= cap and 0 <= fresh <= MAX_COUNT and drop >= 0 and 0 <= nxt <= cap and drop + nxt == valid + fresh


def _count_ok(cnt: int, seq: int, pad: int, orig: int, nw: int) -> bool:
    return 0 <= cnt <= MAX_COUNT and cnt <= (-(-(seq + pad) // orig) + 1) * nw


def _range_ok(off: int, rows: int, length: int, total: int) -> bool:
    return 0 <= off and off + rows * length <= total


def native_bank_down_row_ok(row, capacity: int, hcap: int, n_x: int, n_y: int, rates) -> bool:
    """Whether wv_native_bank_down serves a descriptor row (it skips any other whole).  rates: [(orig, nw, L, width)] of the call's table."""
    slot, rate, C, hv, x_off, n, y_off, n_out, pad, drop, hv2, half = (int(v) for v in row)
    if not (0 <= slot < capacity and 0 <= rate < len(rates) and 1 <= C <= 64 and half in (0, 1)):
        return False
    orig, nw, _, width = rates[rate]
    return (_roll_ok(hcap, hv, n, drop, hv2) and 0 <= pad <= width and _count_ok(n_out, hv + n, pad, orig, nw) and _range_ok(x_off, C, n, n_x)
            and _range_ok(y_off, 1, n_out, n_y))


def native_bank_up_row_ok(row, capacity: int, rcap: int, pcap: int, Cmax: int, n_r: int, n_x: int, n_out: int, rates) -> bool:
    """Whether wv_native_bank_up_add serves a descriptor row (it skips any other whole)."""
    slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half = (int(v) for v in row)
    if not (0 <= slot < capacity and 0 <= rate < len(rates) and 1 <= C <= min(64, Cmax) and half in (0, 1)):
        return False
    orig, nw, _, width = rates[rate]
    return (_roll_ok(rcap, rv, nr, rdrop, rv2) and 0 <= pv <= pcap and 0 <= n <= MAX_COUNT and k >= 0 and 0 <= pv + n - k <= pcap
            and 0 <= pad <= width and _count_ok(k, rv + nr, pad, orig, nw) and _range_ok(r_off, 1, nr, n_r) and _range_ok(x_off, C, n, n_x)
            and _range_ok(out_off, C, k, n_out))


def floor_tile_frames(orig: int, nw: int, L: int, hop: int) -> int:
    """The frames one workgroup of wv_native_bank_floor_up_add serves at a rate (lf_geom of csrc/wv_live_floor.hip); 0: the entry point refuses the
    rate, because a frame passes channel_floor.MAX_FRAME or two frames, the input window and the gains pass channel_floor.LDS_FLOATS."""
    maxlen = -(-nw * hop // orig)
    room = min(channel_floor.LDS_FLOATS - FLOOR_G_FLOATS - (((nw + TILE - 2) // nw) * orig + L), FLOOR_U_FLOATS)
    if maxlen > channel_floor.MAX_FRAME or room < 2 * maxlen:
        return 0
    return min(room // maxlen - 1, FLOOR_MAX_NF)


def _start(f: int, M: int, orig: int) -> int:
    return -(-f * M // orig)


def native_bank_floor_up_row_ok(row, cap, capacity: int, rcap: int, pcap: int, ucap: int, Cmax: int, n_r: int, n_x: int, n_out: int, n_gains: int,
                                rates, hop: int) -> bool:
    """Whether wv_native_bank_floor_up_add serves a descriptor row with the cap `cap` (it skips any other whole)."""
    slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half, f0, nf, uv, uv2, g_off, final = (int(v) for v in row)
    cap = np.float32(cap)
    if not (np.isfinite(cap) and cap >= 0):
        return False
    if not (0 <= slot < capacity and 0 <= rate < len(rates) and 1 <= C <= min(64, Cmax) and half in (0, 1) and final in (0, 1)):
        return False
    orig, nw, _, width = rates[rate]
    M, nu = nw * hop, k + uv2 - uv
    if not (_roll_ok(rcap, rv, nr, rdrop, rv2) and 0 <= pv <= pcap and 0 <= n <= MAX_COUNT and k >= 0 and 0 <= pv + n - k <= pcap
            and 0 <= uv <= ucap and 0 <= uv2 <= ucap and not (final and uv2) and 0 <= pad <= width and _count_ok(nu, rv + nr, pad, orig, nw)
            and f0 >= 0 and 0 <= nf <= MAX_COUNT and f0 + nf <= 2 ** 62 // M):
        return False
    whole = _start(f0 + nf, M, orig) - _start(f0, M, orig)
    if final:
        frames = k == 0 if nf == 0 else _start(f0 + nf - 1, M, orig) - _start(f0, M, orig) < k <= whole
    else:
        frames = k == whole
    return (frames and _range_ok(r_off, 1, nr, n_r) and _range_ok(x_off, C, n, n_x) and _range_ok(out_off, C, k, n_out)
            and (g_off == -1 or _range_ok(g_off, C, nf, n_gains)))


def down_row(slot: int, rate: int, C: int, t: StageTick, x_off: int, y_off: int, half: int) -> list:
    return [slot, rate, C, t.hv, x_off, t.n, y_off, t.n_out, t.pad, t.drop, t.hv2, half]


def up_row(slot: int, rate: int, C: int, t: EmbedTick, r_off: int, x_off: int, n: int, out_off: int, half: int) -> list:
    b = t.back
    return [slot, rate, C, b.hv, r_off, b.n, x_off, n, out_off, b.n_out, b.pad, b.drop, b.hv2, t.pv, half]


def floor_up_row(slot: int, rate: int, C: int, t: EmbedTick, r_off: int, x_off: int, n: int, out_off: int, half: int, g_off: int = -1) -> list:
    b, fl = t.back, t.floor
    return [slot, rate, C, b.hv, r_off, b.n, x_off, n, out_off, fl.k, b.pad, b.drop, b.hv2, t.pv, half, fl.f0, fl.nf, fl.uv, fl.uv2, g_off, int(t.final)]


def down_blocks(desc) -> int:
    """The x-extent wv_native_bank_down needs for these rows: the largest tile-plus-history-block count."""
    return max((_tiles(r[7]) + _tiles(r[10]) for r in np.asarray(desc).reshape(-1, 12)), default=0)


def up_blocks(desc) -> int:
    return max((_tiles(r[9]) + _tiles(r[12]) + _tiles(r[13] + r[7] - r[9]) for r in np.asarray(desc).reshape(-1, 15)), default=0)


def floor_up_blocks(desc, rates, hop: int) -> int:
    """The x-extent wv_native_bank_floor_up_add needs for these rows; rates: [(orig, nw, L, width)] of the call's table."""
    need = 0
    for r in np.asarray(desc).reshape(-1, FLOOR_DESC):
        nf = int(r[16])
        tiles = -(-nf // max(floor_tile_frames(*rates[int(r[1])][:3], hop), 1))
        need = max(need, tiles + _tiles(r[12]) + _tiles(r[13] + r[7] - r[9]) + _tiles(r[18]) + (nf == 0))
    return need


def _geometry(tables) -> list:
    return [tuple(int(v) for v in t[1:]) for t in tables]


# ---------------------------------------------------------------------------------------------------------------- the stages on host arrays
def numpy_bank_down(hist: np.ndarray, x: np.ndarray, desc: np.ndarray, tables, n_y: int) -> np.ndarray:
    """Reference of wv_native_bank_down: hist [capacity, 2, hcap] (the half a row does not name is written, only [0, hv2)), x the packed new
    samples, tables [native.transposed_table(...)] -> y [n_y] (zeros where no served row writes; the kernel leaves those alone)."""
    capacity, _, hcap = hist.shape
    y = np.zeros(n_y, hist.dtype)
    geo = _geometry(tables)
    for row in np.asarray(desc).reshape(-1, 12):
        if not native_bank_down_row_ok(row, capacity, hcap, int(x.shape[0]), n_y, geo):
            continue
        slot, rate, C, hv, x_off, n, y_off, n_out, pad, drop, hv2, half = (int(v) for v in row)
        xs = np.asarray(x[x_off:x_off + C * n], hist.dtype).reshape(1, C, n)
        out, nxt = numpy_down(hist[slot, half][None], xs, StageTick(hv, n, pad, n_out, drop, hv2), tables[rate])
        y[y_off:y_off + n_out] = out[0]
        hist[slot, 1 - half, :hv2] = nxt[0, :hv2]
    return y


def numpy_bank_up_add(rhist: np.ndarray, pend: np.ndarray, r: np.ndarray, x: np.ndarray, desc: np.ndarray, gain: np.ndarray, tables,
                      n_out: int) -> np.ndarray:
    """Reference of wv_native_bank_up_add: rhist [capacity, 2, rcap], pend [capacity, 2, Cmax, pcap], r and x the packed residuals and new
    originals, gain [P] -> out [n_out]."""
    capacity, _, rcap = rhist.shape
    Cmax, pcap = pend.shape[2:]
    out = np.zeros(n_out, pend.dtype)
    geo = _geometry(tables)
    for p, row in enumerate(np.asarray(desc).reshape(-1, 15)):
        if not native_bank_up_row_ok(row, capacity, rcap, pcap, Cmax, int(r.shape[0]), int(x.shape[0]), n_out, geo):
            continue
        slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half = (int(v) for v in row)
        pv2 = pv + n - k
        t = EmbedTick(None, (), nr, StageTick(rv, nr, pad, k, rdrop, rv2), pv, pv2)
        xs = np.asarray(x[x_off:x_off + C * n], pend.dtype).reshape(1, C, n)
        o, pnxt, rnxt = numpy_up_add(rhist[slot, half][None], np.asarray(r[r_off:r_off + nr])[None], pend[slot, half, :C][None], xs, t, tables[rate],
                                     gain[p])
        out[out_off:out_off + C * k] = o.reshape(-1)
        pend[slot, 1 - half, :C, :pv2] = pnxt[0, :, :pv2]
        rhist[slot, 1 - half, :rv2] = rnxt[0, :rv2]
    return out


def numpy_bank_floor_up_add(rhist: np.ndarray, pend: np.ndarray, uhold: np.ndarray, gprev: np.ndarray, r: np.ndarray, x: np.ndarray,
                            desc: np.ndarray, cap: np.ndarray, tables, hop: int, rho: float, n_out: int, n_gains: int = 0):
    """Reference of wv_native_bank_floor_up_add: rhist [capacity, 2, rcap], pend [capacity, 2, Cmax, pcap], uhold
    [capacity, 2, ucap], gprev [capacity, 2, Cmax], r and x the packed residuals and new originals, desc [P, 21], cap [P] -> (out [n_out] float32,
    gains [n_gains] float32).  The resampler runs in the states' dtype, the floor in float32 (channel_floor.numpy_floor_frames)."""
    capacity, _, rcap = rhist.shape
    Cmax, pcap = pend.shape[2:]
    ucap = uhold.shape[2]
    out, gains = np.zeros(n_out, np.float32), np.zeros(n_gains, np.float32)
    geo = _geometry(tables)
    for p, row in enumerate(np.asarray(desc).reshape(-1, FLOOR_DESC)):
        if not native_bank_floor_up_row_ok(row, cap[p], capacity, rcap, pcap, ucap, Cmax, int(r.shape[0]), int(x.shape[0]), n_out, n_gains, geo, hop):
            continue
        slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half, f0, nf, uv, uv2, g_off, final = (int(v) for v in row)
        orig, nw = geo[rate][:2]
        seq = np.concatenate([rhist[slot, half, :rv], np.asarray(r[r_off:r_off + nr], rhist.dtype)])
        seq_u = np.concatenate([uhold[slot, half, :uv], numpy_resample(seq[None], pad, k + uv2 - uv, tables[rate])[0].astype(uhold.dtype)])
        seq_x = np.concatenate([pend[slot, half, :C, :pv], np.asarray(x[x_off:x_off + C * n], pend.dtype).reshape(C, n)], axis=1)
        starts = np.array([_start(f0 + i, nw * hop, orig) - _start(f0, nw * hop, orig) for i in range(nf + 1)], np.int64)
        o, g = channel_floor.numpy_floor_frames(seq_x[:, :k], seq_u[:k], starts, cap[p], rho, None if f0 == 0 else gprev[slot, half, :C])
        out[out_off:out_off + C * k] = o.reshape(-1)
        if g_off >= 0:
            gains[g_off:g_off + C * nf] = g.reshape(-1)
        rhist[slot, 1 - half, :rv2] = seq[rdrop:rdrop + rv2]
        pend[slot, 1 - half, :C, :pv + n - k] = seq_x[:, k:]
        uhold[slot, 1 - half, :uv2] = seq_u[k:k + uv2]
        gprev[slot, 1 - half, :C] = g[:, -1] if nf else gprev[slot, half, :C]
    return out, gains


# ---------------------------------------------------------------------------------------------------------------- the banks
class _BankStages:
    """The two stages and their state on host arrays of the backend's dtype; _HipBankStages states the same on the device."""

    def _tables(self):
        return ([native.transposed_table(r, MODEL_RATE) for r in self.rates], [native.transposed_table(MODEL_RATE, r) for r in self.rates])

    def _upload(self, sections: list) -> dict:
        return dict(sections)

    def _down(self, x, tabs: dict, n_y: int, blocks: int):
        return numpy_bank_down(self._hist, x, tabs["front"], self._ftabs, n_y)

    def _up_add(self, r, x, tabs: dict, n_out: int, blocks: int):
        return numpy_bank_up_add(self._rhist, self._pend, r, x, tabs["back"], tabs["gain"], self._btabs, n_out)

    def _floor_up_add(self, r, x, tabs: dict, n_out: int, n_gains: int, blocks: int):
        out, gains = numpy_bank_floor_up_add(self._rhist, self._pend, self._uhold, self._gprev, np.asarray(r), x, tabs["back"], tabs["gain"],
                                             self._btabs, self.inner.hop, self._crho, n_out, n_gains)
        return out.astype(self._pend.dtype), gains


class _HipBankStages(_BankStages):
    """The stages as one launch each on the inner bank's device; the rate tables are native.tables' cached device tensors."""

    def _tables(self):
        pairs = [native.tables(r, self._arr.device) for r in self.rates]
        front, back = [p[0] for p in pairs], [p[1] for p in pairs]
        self._frates = (_lib.WvNativeRate * len(front))(*[_lib.WvNativeRate(t[0].data_ptr(), *t[1:]) for t in front])
        self._brates = (_lib.WvNativeRate * len(back))(*[_lib.WvNativeRate(t[0].data_ptr(), *t[1:]) for t in back])
        return front, back

    def _upload(self, sections: list) -> dict:
        return self.inner._upload(sections)

    def _down(self, x, tabs: dict, n_y: int, blocks: int):
        torch, dev = self._arr.torch, self._arr.device
        y = torch.empty(n_y, dtype=torch.float32, device=dev)
        desc = tabs["front"]
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wv_native_bank_down(
                self._hist.data_ptr(), self.capacity, self._hist.shape[2], x.data_ptr() if x.numel() else None, x.numel(), self._frates,
                len(self.rates), desc.data_ptr(), desc.shape[0], blocks, y.data_ptr() if n_y else None, n_y, _lib.stream()), "wv_native_bank_down")
        return y

    def _up_add(self, r, x, tabs: dict, n_out: int, blocks: int):
        torch, dev = self._arr.torch, self._arr.device
        out = torch.empty(n_out, dtype=torch.float32, device=dev)
        desc = tabs["back"]
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wv_native_bank_up_add(
                self._rhist.data_ptr(), self._rhist.shape[2], self._pend.data_ptr(), self._pend.shape[3], self._pend.shape[2], self.capacity,
                r.data_ptr() if r.numel() else None, r.numel(), x.data_ptr() if x.numel() else None, x.numel(), self._brates, len(self.rates),
                desc.data_ptr(), tabs["gain"].data_ptr(), desc.shape[0], blocks, out.data_ptr() if n_out else None, n_out, _lib.stream()),
                "wv_native_bank_up_add")
        return out

    def _floor_up_add(self, r, x, tabs: dict, n_out: int, n_gains: int, blocks: int):
        torch, dev = self._arr.torch, self._arr.device
        out = torch.empty(n_out, dtype=torch.float32, device=dev)
        gains = torch.empty(n_gains, dtype=torch.float32, device=dev)
        desc = tabs["back"]
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wv_native_bank_floor_up_add(
                self._rhist.data_ptr(), self._rhist.shape[2], self._pend.data_ptr(), self._pend.shape[3], self._uhold.data_ptr(), self._uhold.shape[2],
                self._gprev.data_ptr(), self._pend.shape[2], self.capacity, r.data_ptr() if r.numel() else None, r.numel(),
                x.data_ptr() if x.numel() else None, x.numel(), self._brates, len(self.rates), desc.data_ptr(), tabs["gain"].data_ptr(), desc.shape[0],
                blocks, self.inner.hop, self._crho, out.data_ptr() if n_out else None, n_out, gains.data_ptr() if n_gains else None, n_gains,
                _lib.stream()), "wv_native_bank_floor_up_add")
        return out, gains


class HostFrontBank(_BankStages):
    """The front stage in front of a 16 kHz bank `inner` (session.StreamBank or a subclass): open(*inner's arguments, sample_rate, channels) ->
    slot; push({slot: x [C, n]}) at each slot's own rate -> inner.push of the 16 kHz samples that became final, per slot (a slot whose stage
    emitted nothing still pushes an empty array, so the result has every pushed slot); close(slot) -> the rest, then inner.close.  Whatever the
    inner bank returns stays on the 16 kHz time line.  The slot table is the inner bank's: open_slots() and the open-slot check are its own.
    The stages' arrays live on the inner bank's backend; dtype: numpy arrays of that dtype instead."""

    def __init__(self, inner, rates, max_channels: int = 2, dtype=None):
        self.rates = check_rates(rates)
        if not 1 <= int(max_channels) <= 64:
            raise ValueError(f"max_channels must be within [1, 64], got {max_channels}")
        self.inner, self.capacity, self.max_channels = inner, inner.capacity, int(max_channels)
        self.open_slots, self._check_slot = inner.open_slots, inner._check_slot         # the inner bank's own: no mirror, no second call per slot
        self._arr = inner._arr if dtype is None else NumpyArrays(dtype)
        self._ftabs, self._btabs = self._tables()
        self._plans = [None] * self.capacity
        self._rate = [0] * self.capacity
        self._chan = [1] * self.capacity
        self._half = [0] * self.capacity
        self.stats = {"ticks": 0, "uploads": 0, "front_launches": 0, "back_launches": 0}
        self._new_state()

    # ---- state: allocated once, sized by the largest table of the bank's rates
    def _new_state(self) -> None:
        self._hist = self._arr.zeros(self.capacity, 2, max(t[3] for t in self._ftabs))

    def _new_plan(self, sample_rate: int):
        return StagePlan(*native.table_geometry(sample_rate, MODEL_RATE))

    # ---- slots
    def open(self, *args, sample_rate: int = MODEL_RATE, channels: int = 1) -> int:
        """open(*the inner bank's arguments, sample_rate=, channels=) -> the inner bank's lowest free slot, a stream of `channels` channels at
        `sample_rate` (one of the bank's rates) starting from nothing: its plan is new, so whatever state the slot's last stream left in either
        half is never read.  Refusals, the inner bank's among them, come before any state changes."""
        if int(sample_rate) not in self.rates:
            raise ValueError(f"sample rate {sample_rate} Hz is not one of this bank's rates {self.rates}")
        if not 1 <= int(channels) <= self.max_channels:
            raise ValueError(f"channels must be within [1, {self.max_channels}], got {channels}")
        plan = self._new_plan(int(sample_rate))
        slot = self.inner.open(*args)                                      # RuntimeError when every slot is open
        self._plans[slot], self._rate[slot], self._chan[slot] = plan, self.rates.index(int(sample_rate)), int(channels)
        return slot

    def sample_rate(self, slot: int) -> int:
        self._check_slot(slot)
        return self.rates[self._rate[slot]]

    def channels(self, slot: int) -> int:
        self._check_slot(slot)
        return self._chan[slot]

    def samples_in(self, slot: int) -> int:
        """Samples the slot's stream has pushed, at its own rate."""
        self._check_slot(slot)
        return self._plans[slot].t_in

    # ---- ticks
    def _checked(self, items: dict) -> dict:
        for slot, x in items.items():
            self._check_slot(slot)
            if len(x.shape) != 2 or x.shape[0] != self._chan[slot]:
                raise ValueError(f"slot {slot}: expected new samples of shape [{self._chan[slot]}, n], got {tuple(x.shape)}")
        return {s: items[s] for s in sorted(items)}

    def _packed(self, ticks: dict, count) -> tuple:
        """-> ({slot: offset}, total) of the tick's slots packed one after another, count(slot, tick) floats each."""
        off, total = {}, 0
        for s, t in ticks.items():
            off[s] = total
            total += count(s, t)
        return off, total

    def _front_tick(self, xs: dict, ticks: dict, extra=()):
        """One upload and one front launch for the tick's slots (ticks {slot: StageTick}) -> (the packed x, {slot: its 16 kHz samples, a view
        of the tick's y arena}, the uploaded tables).  extra: further sections of the same upload (the back stage's)."""
        self.stats["ticks"] += 1
        x_off, _ = self._packed(ticks, lambda s, t: self._chan[s] * t.n)
        y_off, n_y = self._packed(ticks, lambda s, t: t.n_out)
        front = np.array([down_row(s, self._rate[s], self._chan[s], t, x_off[s], y_off[s], self._half[s]) for s, t in ticks.items()],
                         np.int64).reshape(-1, 12)
        x = self._arr.cat([self._arr.take(xs[s]).reshape(-1) for s in ticks if ticks[s].n])
        tabs = self._upload([("front", front)] + list(extra))
        self.stats["uploads"] += 1
        y = self._down(x, tabs, n_y, down_blocks(front))
        self.stats["front_launches"] += 1
        for s in ticks:
            self._half[s] ^= 1
        return x, {s: y[y_off[s]:y_off[s] + t.n_out] for s, t in ticks.items()}, tabs

    def _join(self, a, b):
        return b

    def push(self, items: dict):
        """{slot: x [C, n]}, any n per slot -> the inner bank's result per slot.  Everything is checked before any stream's state changes."""
        xs = self._checked(items)
        if not xs:
            return self.inner.push({})
        ticks = {s: self._plans[s].push(int(x.shape[1])) for s, x in xs.items()}
        return self.inner.push(self._front_tick(xs, ticks)[1])

    def close(self, slot: int):
        """The stream's last 16 kHz samples (zeros past its end, as the file kernels take them), then the inner bank's close; frees the slot."""
        self._check_slot(slot)
        ys = self._front_tick({slot: self._arr.zeros(self._chan[slot], 0)}, {slot: self._plans[slot].flush()})[1]
        first = self.inner.push(ys)
        return self._join(None if first is None else first[slot], self.inner.close(slot))


class HostEmbedBank(HostFrontBank):
    """Watermark up to `capacity` live streams, each at its own rate and channel count: open(message, sample_rate, channels, strength) -> slot;
    push({slot: x [C, n]}) -> {slot: [C, k]}, the watermarked samples that no later input can change, each x + strength * (the generator's
    residual brought to the slot's rate) on every channel; close(slot) -> the rest, after which as many samples have come out as went in and their
    concatenation is that of a NativeEmbedSession given the same pushes.  `inner` returns the RESIDUAL of its new frames per slot.
    set_channel_snr_floor(min_snr_db), before the first open(): the per-channel SNR floor of channel_floor.py on every slot (DESIGN.md section
    7d-13).  A sample then leaves only when its whole native frame has its residual, latency_samples(slot) grows by one nominal frame, and per
    stream the concatenated output is channel_floor.numpy_channel_floor on everything the stream pushed; gains(slot) is the trace."""

    channel_snr_floor_db = None
    _ever_opened = False

    def _new_plan(self, sample_rate: int):
        return EmbedPlan(sample_rate, self.inner.hop, self.inner.H, self.channel_snr_floor_db is not None)

    def _new_state(self) -> None:
        super()._new_state()
        zeros = self._arr.zeros
        plans = [self._new_plan(r) for r in self.rates]
        self._rhist = zeros(self.capacity, 2, max(t[3] for t in self._btabs))
        self._pend = zeros(self.capacity, 2, self.max_channels, max(p.pcap for p in plans))
        self._strength = [1.0] * self.capacity
        if self.channel_snr_floor_db is not None:
            self._uhold = zeros(self.capacity, 2, max(p.ucap for p in plans))
            self._gprev = zeros(self.capacity, 2, self.max_channels)
            self._gains = [None] * self.capacity

    def set_channel_snr_floor(self, min_snr_db) -> None:
        """The per-channel floor in dB for every slot (None: off).  Only before the bank's first open().  With set_snr_floor also in force the
        inner bank carries each slot's strength and this floor's cap is 1, as the file route composes the two."""
        if self._ever_opened:
            raise RuntimeError("set_channel_snr_floor is legal only before the bank's first open()")
        db = snr_floor.check_db(min_snr_db)
        if db is not None:
            for r, t in zip(self.rates, self._btabs):
                if floor_tile_frames(*(int(v) for v in t[1:4]), self.inner.hop) < 1:
                    raise ValueError(f"the channel floor's frame at {r} Hz under hop {self.inner.hop} does not fit the kernel's LDS")
        self.channel_snr_floor_db = db
        self._crho = None if db is None else snr_floor.rho_of(db)
        self._new_state()

    def gains(self, slot: int):
        """The channel floor's gains [C, nf] of the native frames the slot's last push or close emitted ([C, 0] where it emitted none): the live
        form of the file route's return_gains."""
        if self.channel_snr_floor_db is None:
            raise RuntimeError("gains() is the channel floor's trace: call set_channel_snr_floor first")
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or not 0 <= slot < self.capacity or self._gains[slot] is None:
            raise ValueError(f"slot {slot!r} has not been opened")
        return self._gains[slot]

    def _floored(self) -> bool:
        """Whether the inner bank shapes its residual under an SNR floor (session.EmbedBank.set_snr_floor): it then applies each slot's own
        strength itself, and the back stage's gains are 1."""
        return getattr(self.inner, "snr_floor_db", None) is not None

    def set_snr_floor(self, min_snr_db) -> None:
        """session.EmbedBank.set_snr_floor on the 16 kHz frames: only before the first open().  The floor is defined on the 16 kHz mono time
        line; the per-channel SNR at a slot's own rate is not bounded by it."""
        self.inner.set_snr_floor(min_snr_db)

    def open(self, message, sample_rate: int = MODEL_RATE, channels: int = 1, strength: float = 1.0) -> int:
        strength = float(strength)
        if (self._floored() or self.channel_snr_floor_db is not None) and not (np.isfinite(strength) and strength >= 0):
            raise ValueError(f"under an SNR floor strength must be finite and >= 0, got {strength}")
        slot = super().open(message, sample_rate=sample_rate, channels=channels)
        self._ever_opened = True
        self._strength[slot] = strength
        if self.channel_snr_floor_db is not None:
            self._gains[slot] = self._arr.zeros(int(channels), 0)
        if self._floored():
            self.inner._strength[slot] = strength
        return slot

    def latency_samples(self, slot: int) -> int:
        """The slot's output lags its input by fewer than this many samples at its own rate."""
        self._check_slot(slot)
        return self._plans[slot].latency_samples

    def samples_out(self, slot: int) -> int:
        self._check_slot(slot)
        return self._plans[slot].t_out

    def _residual_offsets(self, ticks: dict) -> dict:
        """Where the inner bank will put each slot's residual in its packed output of this tick: session.plan_tick on the inner ticks."""
        plan = plan_tick({s: t.inner[0] for s, t in ticks.items()}, {s: t.front.n_out for s, t in ticks.items()}, self.inner.pad_limit)
        return {s: plan.out[s][0] for s in ticks}

    def _floor_embed_tick(self, xs: dict, ticks: dict, final: bool) -> dict:
        """_embed_tick under the channel floor: the same single upload and front launch, the back launch wv_native_bank_floor_up_add."""
        r_off = {s: 0 for s in ticks} if final else self._residual_offsets(ticks)
        x_off, _ = self._packed(ticks, lambda s, t: self._chan[s] * t.front.n)
        out_off, n_out = self._packed(ticks, lambda s, t: self._chan[s] * t.floor.k)
        g_off, n_gains = self._packed(ticks, lambda s, t: self._chan[s] * t.floor.nf)
        back = [floor_up_row(s, self._rate[s], self._chan[s], t, r_off[s], x_off[s], t.front.n, out_off[s], self._half[s], g_off[s])
                for s, t in ticks.items()]
        x, ys, tabs = self._front_tick(xs, {s: t.front for s, t in ticks.items()},
                                       [("back", np.array(back, np.int64).reshape(-1, FLOOR_DESC)),
                                        ("gain", np.array([1.0 if self._floored() else self._strength[s] for s in ticks], np.float32))])
        r = self._residuals(ys, ticks, r_off, final)
        out, gains = self._floor_up_add(r, x, tabs, n_out, n_gains, floor_up_blocks(back, [t[1:] for t in self._btabs], self.inner.hop))
        self.stats["back_launches"] += 1
        for s, t in ticks.items():
            self._gains[s] = gains[g_off[s]:g_off[s] + self._chan[s] * t.floor.nf].reshape(self._chan[s], t.floor.nf)
        return {s: out[out_off[s]:out_off[s] + self._chan[s] * t.floor.k].reshape(self._chan[s], t.floor.k) for s, t in ticks.items()}

    def _embed_tick(self, xs: dict, ticks: dict, final: bool) -> dict:
        if self.channel_snr_floor_db is not None:
            return self._floor_embed_tick(xs, ticks, final)
        r_off = {s: 0 for s in ticks} if final else self._residual_offsets(ticks)
        x_off, _ = self._packed(ticks, lambda s, t: self._chan[s] * t.front.n)
        out_off, n_out = self._packed(ticks, lambda s, t: self._chan[s] * t.back.n_out)
        back = [up_row(s, self._rate[s], self._chan[s], t, r_off[s], x_off[s], t.front.n, out_off[s], self._half[s]) for s, t in ticks.items()]
        x, ys, tabs = self._front_tick(xs, {s: t.front for s, t in ticks.items()},
                                       [("back", np.array(back, np.int64).reshape(-1, 15)),
                                        ("gain", np.array([1.0 if self._floored() else self._strength[s] for s in ticks], self._arr.dtype))])
        r = self._residuals(ys, ticks, r_off, final)
        out = self._up_add(r, x, tabs, n_out, up_blocks(back))
        self.stats["back_launches"] += 1
        return {s: out[out_off[s]:out_off[s] + self._chan[s] * t.back.n_out].reshape(self._chan[s], t.back.n_out) for s, t in ticks.items()}

    def _residuals(self, ys: dict, ticks: dict, r_off: dict, final: bool):
        """The inner bank's residuals of the tick as ONE packed array whose offsets are r_off."""
        if final:
            (s, t), = ticks.items()
            r = self._arr.cat([v.reshape(-1) for v in (self.inner.push(ys)[s], self.inner.close(s)) if v is not None])
            assert r.shape[0] == t.n_res, (r.shape, t.n_res)
            return r
        res = self.inner.push(ys)
        r = self._arr.zeros(max((r_off[s] + t.n_res for s, t in ticks.items()), default=0))
        for s, t in ticks.items():
            assert (0 if res[s] is None else res[s].shape[-1]) == t.n_res, (s, t.n_res)
            if t.n_res:
                r[r_off[s]:r_off[s] + t.n_res] = res[s].reshape(-1)
        return r

    def push(self, items: dict) -> dict:
        xs = self._checked(items)
        if not xs:
            return {}
        return self._embed_tick(xs, {s: self._plans[s].push(int(x.shape[1])) for s, x in xs.items()}, False)

    def close(self, slot: int):
        self._check_slot(slot)
        return self._embed_tick({slot: self._arr.zeros(self._chan[slot], 0)}, {slot: self._plans[slot].flush()}, True)[slot]


# ---------------------------------------------------------------------------------------------------------------- on the device
class NativeEmbedBank(_HipBankStages, HostEmbedBank):
    """HostEmbedBank on a HipNet generator: open(message or watermark id, sample_rate, channels, strength); everything stays on the device.  A tick
    uploads ONE table for the native stages (front descriptors, back descriptors, gains) and makes one front and one back launch, whatever the
    mix of rates; the values of a push are views of one tensor."""

    def __init__(self, net, rates, capacity: int = 64, max_channels: int = 2, precision: str = "f32", pad_limit: float = 1.5,
                 messages=None):
        rates = check_rates(rates)                                         # refused before anything is built on the device
        HostEmbedBank.__init__(self, EmbedBank(net, capacity, precision, pad_limit, messages, add_input=False), rates, max_channels)

    def _residuals(self, ys: dict, ticks: dict, r_off: dict, final: bool):
        if final:
            return HostEmbedBank._residuals(self, ys, ticks, r_off, final)
        res = self.inner.push(ys)
        live = [(s, res[s]) for s, t in ticks.items() if t.n_res]
        if not live:
            return self._arr.zeros(0)
        # the inner bank's views of its own packed output: that tensor is the r arena, the views' offsets the rows' r_off
        base = live[0][1].untyped_storage().data_ptr()
        for s, v in live:
            assert v.untyped_storage().data_ptr() == base and v.storage_offset() == r_off[s] and v.shape[0] == ticks[s].n_res, s
        return live[0][1].as_strided((max(r_off[s] + ticks[s].n_res for s, _ in live),), (1,), 0)


class NativeDetectBank(_HipBankStages, HostFrontBank):
    """Detect the watermark in up to `capacity` live streams at their own rates: push({slot: x [C, n]}) -> {slot: session.DetectState over the
    16 kHz frames that stream has completed} (samples_seen counts 16 kHz samples)."""

    def __init__(self, net, rates, capacity: int = 64, max_channels: int = 2, precision: str = "f32", pad_limit: float = 1.5):
        rates = check_rates(rates)
        HostFrontBank.__init__(self, DetectBank(net, capacity, precision, pad_limit), rates, max_channels)


class NativeLocateBank(_HipBankStages, HostFrontBank):
    """Locate the watermark in up to `capacity` live streams at their own rates: push({slot: x [C, n]}) -> {slot: locator logits of the 16 kHz
    frames that push completed [k]}; the logits stay on the 16 kHz time line."""

    def __init__(self, net, rates, capacity: int = 64, max_channels: int = 2, precision: str = "f32", pad_limit: float = 1.5):
        rates = check_rates(rates)
        HostFrontBank.__init__(self, LocateBank(net, capacity, precision, pad_limit), rates, max_channels)

    def _join(self, a, b):
        return self._arr.cat([a, b])


class NativeSegmentBank(_HipBankStages, HostFrontBank):
    """Watermarked segments of up to `capacity` live streams at their own rates: push({slot: x [C, n]}) returns nothing; poll(), open_segments()
    and close() are session.SegmentBank's on the 16 kHz samples the front stage has made final, so a Segment's frames count 16 kHz detector
    frames and its start_s / end_s are seconds on the stream's own clock.  A caller's gate has no native-rate form and is refused."""

    def __init__(self, detector, locator, rates, capacity: int = 64, max_channels: int = 2, gated: bool = False, **kw):
        if gated:
            raise ValueError("a gate is given per 16 kHz sample; a bank at the streams' own rates takes none")
        rates = check_rates(rates)
        HostFrontBank.__init__(self, SegmentBank(detector, locator, capacity, gated=False, sample_rate=MODEL_RATE, **kw), rates, max_channels)

    def push(self, items: dict) -> None:
        for slot, item in items.items():
            if isinstance(item, (tuple, list)):
                raise ValueError(f"slot {slot}: a gate is given per 16 kHz sample; a bank at the streams' own rates takes none")
        HostFrontBank.push(self, items)

    def poll(self) -> dict:
        return self.inner.poll()

    def open_segments(self) -> dict:
        return self.inner.open_segments()

    def set_split(self, rule) -> None:
        """session.SegmentBank.set_split on the 16 kHz frames: only before the first open()."""
        self.inner.set_split(rule)
