"""Cases of the session-bank fuzz (tests/test_bank_fuzz_cases_cpu.py, tests/test_gpu_bank_fuzz.py): a plain module, fixed seeds, plain tuples,
importable without a GPU.

random_schedule(hop, H, seed)          steps in bank_cases' vocabulary, ("open", stream) | ("push", {stream: n}) | ("close", stream), drawn tick
                                       by tick: bank_cases.run, native_bank_cases.run, segment_bank_cases.play and span_cases.run_switching play
                                       them unchanged
random_native_schedule(hop, H, seed)   the same with a (rate, channels) per stream and every size at that rate
random_switch_plan(steps, hop, H, seed)  the schedule with ("msg", stream, message row or None) steps between its pushes; split_msgs() turns that
                                       into the table span_cases.run_switching takes
events(steps, hop, H) / coverage(...)  what a schedule does, tick by tick, read off the tickers and plan_tick: the conditions the CPU test asserts
random_advance_case / random_detect_case   raw descriptor tables of wv_bank_advance and wv_bank_detect_update"""
from __future__ import annotations

import string

import numpy as np

import bank_cases as BK
import window_cases as W

# per net: the seeds of a list together meet every condition of coverage() on every net that runs them (tests/test_bank_fuzz_cases_cpu.py
# asserts it); of the lists that do, the ones with the shortest schedules
SEEDS = (4, 14, 17)                                              # the exact banks
F16_SEEDS = (2, 6)                                               # the f16 banks
NATIVE_SEEDS = (0, 1, 2)
TABLE_SEEDS = (0, 1, 2, 3)
SWITCH_SEEDS = (1, 2)
CAPACITY = 4
MIN_STREAMS, MAX_STREAMS = 7, 12                                  # more than CAPACITY: every schedule reuses a slot
P_ABSENT, P_CLOSE, P_OPEN, P_CLOSE_AT_ONCE, P_FILL = 0.2, 0.1, 0.6, 0.12, 0.35
NAMES = string.ascii_uppercase


def budget(hop, H):
    """A stream's samples in all: keeps a schedule's float64 oracle in the low seconds."""
    return 2 * (H + hop) + hop


def push_sizes(hop, H):
    """-> (sizes, weights): the sizes around a frame edge; the last is past the history capacity H + hop and drawn with a small weight."""
    sizes = (0, 1, hop - 1, hop, hop + 1, 2 * hop + 3, H + hop + hop // 2 + 1)
    w = np.array([1.0, 1.6, 1.2, 1.0, 1.0, 1.0, 0.7])
    return sizes, w / w.sum()


def random_schedule(hop, H, seed, capacity=CAPACITY, scale=lambda name, n: n, on_open=lambda name, rng, slot: None):
    """One schedule, drawn tick by tick.  A tick: every free slot may open a stream (so the lowest free slot is reused), which may close at
    once without a push; every open stream is absent with probability P_ABSENT, else pushes a size of push_sizes() clipped to what its budget
    has left; every open stream may close after the tick's push.  A stream that is about to close off a hop multiple pushes, with probability
    P_FILL, what brings it to one instead of the size it drew (bank_cases.mixed_schedule's fill_c), so that closes with nothing to emit are
    met on purpose.  Between MIN_STREAMS and MAX_STREAMS streams open in all; then the rest run out their budgets or close.
    scale(name, n): the size as the stream pushes it (native rates); on_open(name, rng, slot): told of every open, in order, with the slot
    the bank will give it."""
    rng = np.random.default_rng(W.seed_of("bank-fuzz", hop, H, seed))
    sizes, weights = push_sizes(hop, H)
    cap = budget(hop, H)
    n_streams = int(rng.integers(MIN_STREAMS, MAX_STREAMS + 1))
    steps, total, slot_of, opened = [], {}, {}, 0                 # total: the open streams' samples so far, in 16 kHz samples
    while opened < n_streams or total:
        for _ in range(capacity - len(slot_of)):                  # opens: a bank gives the lowest free slot
            if opened >= n_streams or rng.random() >= P_OPEN:
                continue
            slot = min(set(range(capacity)) - set(slot_of.values()))
            name = NAMES[opened]
            opened += 1
            steps.append(("open", name))
            on_open(name, rng, slot)
            if rng.random() < P_CLOSE_AT_ONCE:
                steps.append(("close", name))
            else:
                total[name], slot_of[name] = 0, slot
        closing = [n for n in total if total[n] >= cap or rng.random() < (P_CLOSE if opened < n_streams else 2 * P_CLOSE)]
        push = {}
        for name in total:
            if rng.random() < P_ABSENT:
                continue
            n = min(int(rng.choice(sizes, p=weights)), cap - total[name])
            fill = -total[name] % hop
            if name in closing and fill and fill <= cap - total[name] and rng.random() < P_FILL:
                n = fill
            push[name] = n
        if push:
            steps.append(("push", {name: scale(name, n) for name, n in push.items()}))
            for name, n in push.items():
                total[name] += n
        for name in closing:
            steps.append(("close", name))
            del total[name], slot_of[name]
    return steps


def schedules(hop, H, seeds=SEEDS):
    return [(f"seed{seed}", random_schedule(hop, H, seed)) for seed in seeds]


def random_native_schedule(hop, H, seed, capacity=CAPACITY):
    """-> (steps, {stream: (rate, channels)}): random_schedule with each stream at one of native_bank_cases.STREAMS and every size through
    native_bank_cases.scaled.  A stream that opens in a used slot takes, two times in three, a rate other than that slot's last stream's."""
    import native_bank_cases as NBC
    who, last = {}, {}

    def on_open(name, rng, slot):
        pick = [st for st in NBC.STREAMS if st[0] != last.get(slot)] if slot in last and rng.random() < 2 / 3 else list(NBC.STREAMS)
        who[name] = pick[int(rng.integers(len(pick)))]
        last[slot] = who[name][0]
    steps = random_schedule(hop, H, ("native", seed), capacity, lambda name, n: NBC.scaled(n, who[name][0]), on_open)
    return steps, who


# ---- what a schedule does ----------------------------------------------------------------------------------------------------------------
def events(steps, hop, H, capacity=CAPACITY):
    """Plays the tickers alone -> (per stream [(kind, n, samples completed by it)], per push step ({slot: Tick}, {slot: n}), {stream:
    slot}, the push steps at which the bank is full)."""
    from waveverify_amd.session import _Ticker
    tk, ev, slot, taken, ticks, full = {}, {}, {}, {}, [], []
    for kind, arg in steps:
        if kind == "open":
            s = min(set(range(capacity)) - set(taken))
            taken[s], slot[arg], tk[arg], ev[arg] = arg, s, _Ticker(hop, H), []
        elif kind == "close":
            t = tk[arg].flush()
            ev[arg].append(("close", 0, t.wlen - t.keep if t.wlen else 0))
            del taken[slot[arg]]
        else:
            now, sizes = {}, {}
            for name in taken.values():
                if name in arg:
                    t = tk[name].push(arg[name])
                    ev[name].append(("push", arg[name], t.wlen - t.keep if t.wlen else 0))
                    now[slot[name]], sizes[slot[name]] = t, arg[name]
                else:
                    ev[name].append(("absent", 0, 0))
            if len(taken) == capacity:
                full.append(len(ticks))
            ticks.append((now, sizes))
    return ev, ticks, slot, full


def coverage(steps, hop, H, capacity=CAPACITY):
    """-> {condition: whether the schedule meets it}: the conditions a net's seed list must meet between its schedules, from the tickers and plan_tick."""
    from waveverify_amd.session import plan_tick
    ev, ticks, slot, full = events(steps, hop, H, capacity)
    lengths = BK.stream_lengths(steps)
    opens = [arg for kind, arg in steps if kind == "open"]
    closes = [arg for kind, arg in steps if kind == "close"]
    launches = lambda now, sizes, pad: sum(1 for ln in plan_tick(now, sizes, pad).launches if ln.A)      # noqa: E731
    out = {
        "a slot is reused": len(opens) > len({slot[n] for n in opens}),
        "every opened stream is closed": sorted(opens) == sorted(closes),
        "the bank is full on some tick": bool(full),
        "a stream closes with no push": any(not [e for e in ev[n] if e[0] == "push"] for n in opens),
        "a stream closes on a hop multiple": any(lengths[n] > 0 and lengths[n] % hop == 0 and ev[n][-1] == ("close", 0, 0) for n in opens),
        "a stream closes with a partial frame": any(ev[n][-1][0] == "close" and 0 < ev[n][-1][2] < hop for n in opens),
        "a tick where no slot completes a frame": any(now and any(sizes.values()) and not any(t.wlen for t in now.values())
                                                      for now, sizes in ticks),
        "two launches at pad_limit 1.0 become one at inf": any(
            launches(now, sizes, 1.0) >= 2 and launches(now, sizes, float("inf")) == 1 and plan_tick(now, sizes, float("inf")).padded > 0
            for now, sizes in ticks),
        "a push larger than H + hop": any(e[0] == "push" and e[1] > H + hop for n in opens for e in ev[n]),
        "a zero-length push": any(e[:2] == ("push", 0) for n in opens for e in ev[n]),
        "a stream absent between two of its pushes": any(
            "push" in kinds[:i] and "push" in kinds[i + 1:] for n in opens for kinds in [[e[0] for e in ev[n]]] for i, k in enumerate(kinds)
            if k == "absent"),
    }
    return out


PER_SCHEDULE = ("a slot is reused", "every opened stream is closed")


# ---- EmbedBank.set_message ---------------------------------------------------------------------------------------------------------------
SWITCH_PATTERNS = ("open(None)", "id -> None -> other id", "two switches between frames", "a switch on a tick that completes no frame")


def random_switch_plan(steps, hop, H, seed, n_msg=2):
    """-> the schedule with ("msg", stream, message row or None) steps: a stream's state (a row of the message table, or None: pass-through)
    from the next push on; a ("msg", ...) straight after an open is what the stream opens with.  Every third stream opens with None; before
    a push each open stream switches with probability 0.3, by the cycle id -> None -> other id (and on from there); where the stream's next
    push completes no frame it switches, half of the time, once more before the push after that, so two switches fall between two frames."""
    from waveverify_amd.session import _Ticker
    rng = np.random.default_rng(W.seed_of("bank-fuzz switch", hop, H, seed))
    cycle = [0, None, 1, None][: 2 * n_msg]
    out, at, tk, again, fresh = [], {}, {}, set(), set()
    for kind, arg in steps:
        if kind == "open":
            at[arg] = 1 if len(at) % 3 == 2 else int(rng.choice([0, 2]))
            tk[arg] = _Ticker(hop, H)
            fresh.add(arg)
            out += [(kind, arg), ("msg", arg, cycle[at[arg]])]
            continue
        if kind == "push":
            for name in [n for n in tk if not tk[n].closed and n not in fresh]:      # a stream keeps what it opened with for one push step
                if name in again or rng.random() < 0.3:
                    at[name] = (at[name] + 1) % len(cycle)
                    out.append(("msg", name, cycle[at[name]]))
                    again.discard(name)
                    idle = name not in arg or tk[name].t_in + arg[name] < tk[name].t_out + hop
                    if idle and rng.random() < 0.5:
                        again.add(name)
            for name, n in arg.items():
                tk[name].push(n)
            fresh.clear()
        else:
            tk[arg].flush()
            again.discard(arg)
            fresh.discard(arg)
        out.append((kind, arg))
    return out


def split_msgs(msg_steps):
    """-> (the steps without their ("msg", ...), {stream: [state per global push step]} as span_cases.run_switching reads it: entry k is the
    stream's state when push step k starts (and, at the step it opens before, what it opens with))."""
    steps, state, table, n_push = [], {}, {}, sum(1 for s in msg_steps if s[0] == "push")
    k = 0
    for step in msg_steps:
        if step[0] == "msg":
            _, name, st = step
            state[name] = st
            table.setdefault(name, [None] * (n_push + 1))
            table[name][k:] = [st] * (n_push + 1 - k)
            continue
        steps.append(step)
        if step[0] == "push":
            k += 1
    return steps, table


def switch_patterns(msg_steps, hop, H):
    """-> the SWITCH_PATTERNS a plan shows, from the tickers."""
    from waveverify_amd.session import _Ticker
    tk, hist, since, found, fresh = {}, {}, {}, set(), None
    for step in msg_steps:
        kind = step[0]
        if kind == "open":
            tk[step[1]], fresh = _Ticker(hop, H), step[1]
            continue
        if kind == "msg":
            _, name, st = step
            if name == fresh:
                hist[name], since[name] = [st], 0
                if st is None:
                    found.add("open(None)")
            else:
                hist[name].append(st)
                since[name] += 1
                if since[name] >= 2:
                    found.add("two switches between frames")
                h = hist[name]
                if len(h) >= 3 and h[-2] is None and h[-3] is not None and h[-1] is not None and h[-1] != h[-3]:
                    found.add("id -> None -> other id")
                tk[name].switched = True
        elif kind == "push":
            for name, t in tk.items():
                if t.closed:
                    continue
                done = name in step[1] and t.push(step[1][name]).wlen > 0
                if getattr(t, "switched", False) and not done:
                    found.add("a switch on a tick that completes no frame")
                t.switched = False
                if done:
                    since[name] = 0
        else:
            tk[step[1]].flush()
        fresh = None
    return found


# ---- raw tables --------------------------------------------------------------------------------------------------------------------------
def random_advance_case(seed):
    """-> (capacity, hcap, A, Lmax, n_x, rows, bad): a tick's table for wv_bank_advance in shuffled row order: every row inside the contract
    (bank_row_ok) but the one or two taken from bank_cases.bad_rows (bad = their indices), distinct slots and window rows, slots and a
    window row named by nobody, gaps in x, a row of every kind of bank_cases.ROW_KINDS where hcap allows."""
    rng = np.random.default_rng(W.seed_of("bank-fuzz advance", seed))
    hcap = int(rng.choice([7, 33, 255, 256, 257, 1025, 1300]))
    capacity = int(rng.integers(8, 14))
    n_rows = int(rng.integers(4, capacity - 3))                  # with the bad rows' slots, still fewer than capacity
    slots = [int(s) for s in rng.permutation(capacity)[:n_rows]]
    geo = []
    for i, slot in enumerate(slots):
        hv = int(rng.choice([0, 1, hcap // 2, hcap - 1, hcap]))
        n = int(rng.choice([0, 1, 5, hcap // 3 + 1, hcap + 5]))
        if i == 0:
            hv, n = hcap, 0                                       # a still row: nothing moves
        if i == 1:
            hv, n = 0, min(hcap, 13)                              # no history yet
        hv2 = int(rng.integers(0, min(hcap, hv + n) + 1)) if i else hv
        wlen = int(rng.choice([0, min(8, hv + n), hv + n])) if i > 1 else n
        geo.append((slot, hv, n, wlen, hv + n - hv2, hv2))
    windowed = [g for g in geo if g[3] > 0]
    A = len(windowed) + 1                                         # one window row is named by nobody
    win_rows = [int(r) for r in rng.permutation(A)[:len(windowed)]]
    Lmax = max([g[3] for g in windowed] + [1]) + int(rng.integers(0, 4))
    rows, x_off = [], int(rng.integers(0, 4))
    for slot, hv, n, wlen, drop, hv2 in geo:
        rows.append((slot, hv, x_off, n, win_rows.pop() if wlen else 0, wlen, drop, hv2))
        x_off += n + int(rng.integers(0, 3))                      # gaps
    n_x = x_off + 2
    case7 = (capacity, hcap, A, Lmax, n_x, tuple(rows), None)
    donor = max(range(len(rows)), key=lambda i: (rows[i][5] > 0, rows[i][1] + rows[i][3]))
    pool = BK.bad_rows(case7[:5] + ((rows[donor],), ("overlap",)))
    spare = [s for s in range(capacity) if s not in slots]
    bad = []
    for j in rng.permutation(len(pool))[: int(rng.integers(1, 3))]:
        why, row = pool[int(j)]
        if 0 <= row[0] < capacity and spare:                      # a bad row has a slot of its own where its slot is a legal one
            row = (spare.pop(),) + tuple(row[1:])
        bad.append(tuple(row))
    mixed = list(rows) + bad
    order = [int(i) for i in rng.permutation(len(mixed))]
    rows = tuple(mixed[i] for i in order)
    return capacity, hcap, A, Lmax, n_x, rows, tuple(k for k, i in enumerate(order) if i >= len(mixed) - len(bad))


def random_detect_case(seed):
    """-> (capacity, nb, rows (slot, samples)): shuffled, scattered, a slot outside the bank on either side, slots named by nobody, a row that
    adds no samples, one that adds many."""
    rng = np.random.default_rng(W.seed_of("bank-fuzz detect", seed))
    nb = int(rng.choice([1, 16, 36]))
    capacity = int(rng.integers(6, 40))
    n = int(rng.integers(3, capacity - 1))
    rows = [(int(s), int(rng.choice([0, 1, 8, 40, 1000003]))) for s in rng.permutation(capacity)[:n]]
    rows += [(capacity, 8), (-1, 8)]
    return capacity, nb, tuple(rows[int(i)] for i in rng.permutation(len(rows)))


def random_gate(T, hop, seed, min_on=0.5):
    """A 0 / 1 gate [T] float32 for the gated segment banks: frame 0 holds exactly min_on * hop gated samples (on, by the rule's >=), then on
    and off stretches of 1 to 9 whole frames in turn, so that runs are long enough for a split rule's two windows."""
    rng = np.random.default_rng(W.seed_of("bank-fuzz gate", T, hop, seed))
    Fr = -(-T // hop)
    g = np.zeros(Fr * hop, np.float32)
    g[:int(min_on * hop)] = 1.0
    f, on = 1, bool(rng.integers(2))
    while f < Fr:
        k = int(rng.integers(1, 10))
        if on:
            g[f * hop:(f + k) * hop] = 1.0
        f, on = f + k, not on
    return g[:T]


def gap_threshold(logits, lo=0.3, hi=0.7):
    """-> (threshold, margin): the middle of the widest gap between neighbours of the sorted logits from their quantile lo to hi, and half
    that gap: no logit lies closer to the threshold, so a locator whose logits are within `margin` of these gates the same samples."""
    srt = np.sort(np.asarray(logits, np.float64).reshape(-1))
    a, b = int(lo * len(srt)), max(int(hi * len(srt)), int(lo * len(srt)) + 2)
    gaps = np.diff(srt[a:b])
    i = int(np.argmax(gaps))
    return float(0.5 * (srt[a + i] + srt[a + i + 1])), float(0.5 * gaps[i])
