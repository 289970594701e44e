"""Cost of a session bank's tick against the lockstep sessions -> profiles/session_bank_bench.json.

    python tools/sessionbankbench.py [--reps 15] [--out profiles/session_bank_bench.json]

The default full-size nets with seeded random weights, exact and f16, embed and detect.  Every time is the host clock around one push that
ends in a device synchronise; each repetition opens its banks and sessions afresh, repetition 0 warms up, and the figures are medians over
the repetitions with their min and max (the spread).  Within a repetition the contenders take turns push by push (interleaved).
    (a) equal   S = 1, 16, 64 streams that all push 20 ms (320 samples): bank.push of S slots against the lockstep session's push of [S, 320],
                50 pushes, the first 20 (the halo still filling) left out; the difference stands next to the lockstep push's own spread.
    (b) mixed   48 streams, 16 each on 10, 20 and 60 ms packets, all in phase: ONE bank ticked every 10 ms (a slot is named on the ticks its
                packet is due) at pad_limit 1.0, 1.5 and none, against the three lockstep sessions of 16 streams that are the only way to
                run this without a bank.  0.4 s of stream time fills the halos, then the pushes of one second are timed and summed:
                milliseconds of device time per second of audio.  padded_share: samples run only as right padding / samples run.
    (c) kernels wv_bank_advance (64 slots of the generator's history, each pushing 320 samples into a full window) and wv_bank_detect_update
                (64 rows, 16 bits) alone.
No bar is set on any of these: they are recorded, and session.StreamBank's pad_limit default follows from (b)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveverify_amd import _lib  # noqa: E402
from waveverify_amd.core import WaveVerify  # noqa: E402
from waveverify_amd.session import plan_tick  # noqa: E402
from waveverify_amd.window import halo  # noqa: E402

PUSH, PUSHES, SKIP = 320, 50, 20
TICK, PREROLL, TICKS = 160, 40, 100                                  # 10 ms ticks: 0.4 s un-timed, then one second
PACKETS = (160, 320, 960)
PAD_LIMITS = (("1.0", 1.0), ("1.5", 1.5), ("none", float("inf")))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def audio(S, n, seed):
    rng = np.random.default_rng([16000, S, seed])
    return torch.from_numpy(np.clip(0.1 * rng.standard_normal((S, n), dtype=np.float32), -1, 1)).cuda()


def opened(wv, kind, S, pad=1.5):
    """-> (bank with S open slots, lockstep session of S streams)."""
    if kind == "embed":
        bank, sess = wv.open_embed_bank(S, pad), wv.open_embed_session(list(range(1, S + 1)))
        slots = [bank.open(i + 1) for i in range(S)]
    else:
        bank, sess = wv.open_detect_bank(S, pad), wv.open_detect_session(S)
        slots = [bank.open() for _ in range(S)]
    assert slots == list(range(S))
    return bank, sess


def equal(wv, kind, S, reps):
    x = audio(S, PUSH * PUSHES, 0)
    tb, tl = [], []
    for rep in range(reps + 1):
        bank, sess = opened(wv, kind, S)
        pb, pl = [], []
        for i in range(PUSHES):
            xi = x[:, i * PUSH:(i + 1) * PUSH]
            pb.append(timed(lambda: bank.push({s: xi[s] for s in range(S)})))
            pl.append(timed(lambda: sess.push(xi)))
        if rep:
            tb.append(statistics.median(pb[SKIP:]))
            tl.append(statistics.median(pl[SKIP:]))
    b, l = statistics.median(tb), statistics.median(tl)
    return {"bank_push_ms": stat(tb), "lockstep_push_ms": stat(tl), "bank_minus_lockstep_ms": b - l, "bank_over_lockstep": b / l,
            "lockstep_spread_ms": max(tl) - min(tl)}


def mixed(wv, kind, reps):
    S, n = 48, TICK * (PREROLL + TICKS)
    x = audio(S, n, 1)
    packet = [PACKETS[s // 16] for s in range(S)]
    due = lambda tick, p: (tick + 1) * TICK % p == 0                 # a packet is pushed on the tick that completes it
    totals = {name: [] for name, _ in PAD_LIMITS}
    totals["three_lockstep_sessions"] = []
    shares = {}
    for rep in range(reps + 1):
        banks = {name: opened(wv, kind, S, pad)[0] for name, pad in PAD_LIMITS}
        sessions = [opened(wv, kind, 16)[1] for _ in PACKETS]
        if kind == "embed":                                           # the sessions' streams carry the ids of the bank's slots
            sessions = [wv.open_embed_session(list(range(16 * g + 1, 16 * g + 17))) for g in range(3)]
        spent = {name: 0.0 for name in totals}
        for tick in range(PREROLL + TICKS):
            end = (tick + 1) * TICK
            items = {s: x[s, end - packet[s]: end] for s in range(S) if due(tick, packet[s])}
            if tick == PREROLL:
                before = {name: dict(b.stats) for name, b in banks.items()}
            for name, bank in banks.items():                          # interleaved: every contender runs this tick before the next tick
                t = timed(lambda: bank.push(items))
                spent[name] += t if tick >= PREROLL else 0.0
            for g, p in enumerate(PACKETS):
                if due(tick, p):
                    t = timed(lambda: sessions[g].push(x[16 * g: 16 * g + 16, end - p: end]))
                    spent["three_lockstep_sessions"] += t if tick >= PREROLL else 0.0
        if rep:
            for name in totals:
                totals[name].append(spent[name])
            for name, b in banks.items():
                d = {k: b.stats[k] - before[name][k] for k in b.stats}
                shares[name] = {"padded_share": d["padded_samples"] / max(1, d["window_samples"]), "net_launches_per_second": d["launches"]}
    out = {name: {"device_ms_per_second_of_audio": stat(v), **shares.get(name, {})} for name, v in totals.items()}
    ref = statistics.median(totals["three_lockstep_sessions"])
    for name, _ in PAD_LIMITS:
        out[name]["over_three_lockstep_sessions"] = statistics.median(totals[name]) / ref
    out["three_lockstep_sessions"]["spread_ms"] = max(totals["three_lockstep_sessions"]) - min(totals["three_lockstep_sessions"])
    return out


def kernels(wv, reps):
    from waveverify_amd.session import Tick
    lib, dev = _lib.load(), wv.device
    cfg = wv.configs["generator"]
    hop, H = cfg.hop_length, halo(cfg)
    S, hcap = 64, H + hop
    plan = plan_tick({s: Tick(H, H + hop, H, hop, H) for s in range(S)}, {s: PUSH for s in range(S)}, 1.5)
    ln = plan.launches[0]
    desc = torch.from_numpy(plan.desc).to(dev)
    hist, x = torch.zeros((S, hcap), device=dev), audio(1, S * PUSH, 2).reshape(-1)
    win = torch.empty((S, 1, ln.Lmax), device=dev)
    nb = 16
    acc, seen = torch.zeros((S, nb), dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.int64, device=dev)
    psum = torch.rand((S, nb), device=dev) * hop
    ddesc = torch.tensor([[s, hop] for s in range(S)], dtype=torch.int64, device=dev)
    mp, bits = torch.empty((S, nb), device=dev), torch.empty((S, nb), dtype=torch.int32, device=dev)
    adv = lambda: _lib.check(lib.wv_bank_advance(hist.data_ptr(), S, hcap, x.data_ptr(), x.numel(), desc.data_ptr(), S, win.data_ptr(), S, ln.Lmax,
                                                 _lib.stream()))
    upd = lambda: _lib.check(lib.wv_bank_detect_update(acc.data_ptr(), seen.data_ptr(), S, nb, psum.data_ptr(), ddesc.data_ptr(), S, mp.data_ptr(),
                                                       bits.data_ptr(), _lib.stream()))
    ta, tu = [], []
    for rep in range(reps + 1):
        pa, pu = [], []
        for _ in range(PUSHES):
            pa.append(timed(adv))
            pu.append(timed(upd))
        if rep:
            ta.append(statistics.median(pa))
            tu.append(statistics.median(pu))
    return {"bank_advance_64x320_into_64x%d_ms" % ln.Lmax: stat(ta), "bank_detect_update_64x16_ms": stat(tu)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "session_bank_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sessionbankbench needs the GPU: nothing is measured without one")
    wv = WaveVerify.random_init(seed=0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "equal": {}, "mixed": {}, "kernels": kernels(wv, a.reps)}
    for precision in ("f32", "f16"):
        wv.set_precision(precision)
        for kind in ("embed", "detect"):
            for S in (1, 16, 64):
                res["equal"][f"{kind}_S{S}_{precision}"] = equal(wv, kind, S, a.reps)
            res["mixed"][f"{kind}_{precision}"] = mixed(wv, kind, a.reps)
            print(json.dumps({k: v for k, v in res.items() if k in ("equal", "mixed")}), flush=True)
    wv.set_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
