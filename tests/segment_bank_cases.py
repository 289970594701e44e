"""Segment banks: the shared schedules and patterns of tests/test_segment_bank_cpu.py and tests/test_gpu_segment_bank.py (a plain module, fixed
seeds, importable without a GPU).

bank_ticks()        per-slot frame sums and chunkings -> the ticks of wv_bank_segment_track's interface: one arena per tick whose blocks have
                    different Fr_stride and fsum_off, NaN wherever no descriptor points, and the descriptor rows
bad_track_rows()    a good descriptor row changed so that one condition of the contract alone fails
count_net()         a count-only "net" for the state-machine tests: frame sums straight from the gate
stream_gate()       the 0 / 1 gate of a stream of the mixed schedule: runs of on frames with a frame exactly at min_on
ring_gates()        twelve segments per slot on three slots at different phases"""
from __future__ import annotations

import numpy as np

import bank_cases as BK                                            # noqa: F401  (the schedules the state-machine tests play)
import segment_session_cases as SC
import window_cases as W                                           # noqa: F401  (the nets they play them on)

HOP = 10                                                           # of the raw tracker cases, as in test_gpu_segment_session
KERNEL_CAPACITY = 9


# ---- the descriptor interface ---------------------------------------------------------------------------------------------------------------
def bank_ticks(streams, nb, hop, rng):
    """streams [(slot, fsum [nb + 1, Fr] float32, last_valid, chunks [(f_lo, f_hi)], first tick)] -> [(arena [n] float32, desc [P, 8] int64)].
    Stream i's chunk c is served at tick first + c; its block holds the chunk's frames behind 0 .. 2 columns that belong to nobody and before
    0 .. 2 more, so Fr_stride, f_lo and fsum_off differ from row to row and from tick to tick; the rows of a tick come in rotating order; the
    arena starts with a few floats nobody reads and has gaps.  Everything no descriptor points at is NaN.  The last chunk of a stream is its
    final tick (SC.chunks_of's convention); it carries last_valid where it holds the recording's last frame."""
    n_ticks = max(first + len(chunks) for _, _, _, chunks, first in streams)
    out = []
    for t in range(n_ticks):
        n, rows, blocks = int(rng.integers(0, 4)), [], []
        order = streams[t % len(streams):] + streams[:t % len(streams)]
        for slot, fsum, last_valid, chunks, first in order:
            c = t - first
            if not 0 <= c < len(chunks):
                continue
            lo, hi = chunks[c]
            final = c == len(chunks) - 1
            pre, post = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            Fr = pre + hi - lo + post
            block = np.full((nb + 1, Fr), np.nan, np.float32)
            block[:, pre:pre + hi - lo] = fsum[:, lo:hi]
            ends_here = final and hi == fsum.shape[1] and hi > lo
            rows.append([slot, n, Fr, pre, pre + hi - lo, lo, last_valid if ends_here else hop, int(final)])
            blocks.append((n, block))
            n += block.size + int(rng.integers(0, 3))
        arena = np.full(n, np.nan, np.float32)
        for off, block in blocks:
            arena[off:off + block.size] = block.reshape(-1)
        out.append((arena, np.array(rows, np.int64).reshape(-1, 8)))
    return out


def bad_track_rows(row, capacity, nb, hop, n_fsum):
    """-> [(why, row)]: a served row {slot, fsum_off, Fr_stride, f_lo, f_hi, frame0, last_valid, final} with one condition broken."""
    slot, off, Fr, f_lo, f_hi, frame0, lv, final = (int(v) for v in row)
    return [
        ("slot == capacity", (capacity, off, Fr, f_lo, f_hi, frame0, lv, final)),
        ("slot < 0", (-1, off, Fr, f_lo, f_hi, frame0, lv, final)),
        ("f_lo < 0", (slot, off, Fr, -1, f_hi, frame0, lv, final)),
        ("f_hi < f_lo", (slot, off, Fr, f_hi + 1, f_hi, frame0, lv, final)),
        ("f_hi > Fr_stride", (slot, off, Fr, f_lo, Fr + 1, frame0, lv, final)),
        ("Fr_stride < 0", (slot, off, -1, 0, 0, frame0, lv, final)),
        ("Fr_stride beyond 2^31 - 1", (slot, 0, 2 ** 31, f_lo, f_hi, frame0, lv, final)),
        ("fsum_off < 0", (slot, -1, Fr, f_lo, f_hi, frame0, lv, final)),
        ("the block ends past n_fsum", (slot, n_fsum - (nb + 1) * Fr + 1, Fr, f_lo, f_hi, frame0, lv, final)),
        ("fsum_off near 2^63", (slot, 2 ** 63 - 1, Fr, f_lo, f_hi, frame0, lv, final)),
        ("frame0 < 0", (slot, off, Fr, f_lo, f_hi, -1, lv, final)),
        ("last_valid > hop", (slot, off, Fr, f_lo, f_hi, frame0, hop + 1, final)),
        ("last_valid < 0", (slot, off, Fr, f_lo, f_hi, frame0, -1, final)),
    ]


def lockstep_events(fsum, hop, last_valid, min_on, G, ml, dtype=np.float32):
    """One stream's whole array [nb + 1, Fr] through a one-stream localize.SegmentTracker -> its events."""
    from waveverify_amd.localize import SegmentTracker
    t = SegmentTracker(1, fsum.shape[0] - 1, hop, min_on, G, ml, dtype=dtype)
    t.advance(fsum[None], 0, fsum.shape[1], last_valid, True)
    return t.poll()[0]


def pattern_streams(nb, G, ml, kind, rng, hop=HOP, min_on=0.5, capacity=KERNEL_CAPACITY):
    """Every named pattern of SC.named_patterns as a stream of its own, `capacity - 1` at a time on scattered slots that start at different
    ticks -> [batch], a batch = [(slot, fsum, last_valid, chunks, first tick)].  One slot of the bank is left to the caller."""
    pats = SC.named_patterns(hop, min_on, G, ml)
    slots = [s for s in (7, 2, 5, 0, 8, 3, 6, 1, 4)][:capacity - 1]
    batches = []
    for b in range(0, len(pats), len(slots)):
        batch = []
        for i, (name, count, last_valid, _) in enumerate(pats[b:b + len(slots)]):
            fsum = SC.sums_for(count, nb, rng)
            chunks = SC.chunks_of(fsum.shape[1], kind, rng, last_valid < hop)
            batch.append((slots[i], fsum, last_valid, chunks, i % 4))
        batches.append(batch)
    return batches


# ---- the state machine's count-only net -------------------------------------------------------------------------------------------------------
def count_net(hop, scale=0.75):
    """frame_sums(win, gate windows [A, L]) -> [A, 2, ceil(L / hop)] float32: one bit whose sum is `scale` times the frame's gated samples."""
    def fs(win, gwin):
        A, L = gwin.shape
        c = np.pad(np.asarray(gwin, np.float64), ((0, 0), (0, -L % hop))).reshape(A, -1, hop).sum(-1)
        return np.stack([c * scale, c], axis=1).astype(np.float32)
    return fs


def stream_gate(T, hop, min_on=0.5):
    """A 0 / 1 gate [T] for the gated state-machine runs at min_gap_frames = min_len_frames = 1: frame 0 holds exactly min_on * hop gated
    samples (on, by the rule's >=); then on frames alternate with off frames, in runs of two from frame 8 on.  A stream of at least three
    frames has at least two segments; a shorter one has what fits."""
    Fr = -(-T // hop)
    g = np.zeros(Fr * hop, np.float32)
    edge = int(min_on * hop)
    assert edge == min_on * hop and edge > 0
    for f in range(Fr):
        on = f % 2 == 0 if f < 8 else f % 4 in (0, 1)
        if f == 0:
            g[:edge] = 1.0
        elif on:
            g[f * hop:(f + 1) * hop] = 1.0
    return g[:T]


def ring_gates(hop, L=1, G=1, n=12, slots=3):
    """-> (gate [slots, T] float32, expected frames per slot): n runs of L on frames, G off frames between them, slot s shifted by s frames."""
    Fr = n * (L + G) + slots
    gate = np.zeros((slots, Fr), np.float32)
    want = []
    for s in range(slots):
        want.append([(s + i * (L + G), s + i * (L + G) + L) for i in range(n)])
        for lo, hi in want[-1]:
            gate[s, lo:hi] = 1.0
    return np.repeat(gate, hop, axis=1), want


def pieces(T, kind, hop):
    """Push sizes of a T-sample stream: "whole", "hop" or the ragged pattern of test_gpu_segment_session."""
    if kind == "whole":
        return [T]
    if kind == "hop":
        return [hop] * (T // hop) + ([T % hop] if T % hop else [])
    out, base, k = [], [1, hop - 1, 0, hop, 3 * hop + 7, 5 * hop - 1, 2], 0
    while sum(out) < T:
        out.append(min(base[k % len(base)], T - sum(out)))
        k += 1
    return out


def play(bank, steps, xs, gates=None, poll_every=0):
    """BK.run for a segment bank -> ({stream: [Segment] in the order they came out}, {stream: slot}).  gates {stream: [T]} on a gated bank;
    poll_every: poll() after every so many pushes (0: close() alone brings the segments)."""
    slot, owner, pos, out, n_push = {}, {}, {}, {}, 0
    for kind, arg in steps:
        if kind == "open":
            slot[arg], pos[arg], out[arg] = bank.open(), 0, []
            owner[slot[arg]] = arg
        elif kind == "close":
            out[arg] += bank.close(slot[arg])
            del owner[slot[arg]]
        else:
            items = {}
            for name, n in arg.items():
                x = xs[name][pos[name]:pos[name] + n]
                items[slot[name]] = x if gates is None else (x, gates[name][pos[name]:pos[name] + n])
                pos[name] += n
            assert bank.push(items) is None
            n_push += 1
            if poll_every and n_push % poll_every == 0:
                by_slot = bank.poll()
                assert sorted(by_slot) == bank.open_slots() == sorted(owner)
                for s, segs in by_slot.items():
                    out[owner[s]] += segs
    return out, slot
