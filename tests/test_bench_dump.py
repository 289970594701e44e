"""bench.py --dump-outputs on the host: the writer's budget, dtypes and fixed sample, and the argument checks that run before any GPU
call.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _total_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole_as_float32(tmp_path):
    g = torch.Generator().manual_seed(0)
    wm, mp = torch.randn(4, 1, 1000, generator=g), torch.rand(4, 16, generator=g)
    m = bench.dump_outputs(str(tmp_path), dict(wm=wm, mean_prob=mp, bits=mp >= 0.5, d64=mp.double()))
    assert sorted(os.listdir(tmp_path)) == ["bits.npy", "d64.npy", "mean_prob.npy", "wm.npy"]
    assert np.array_equal(np.load(tmp_path / "wm.npy"), wm.numpy())
    bits = np.load(tmp_path / "bits.npy")
    assert bits.dtype == np.float32 and np.array_equal(bits, (mp >= 0.5).float().numpy())
    assert np.load(tmp_path / "d64.npy").dtype == np.float64
    assert all("sample" not in e for e in m["arrays"].values())


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    T = 480000                                                  # the longform workload's outputs: 2 x 61 MB
    wm = torch.arange(32 * T, dtype=torch.float32).reshape(32, 1, T)
    out = {}
    for run in ("a", "b"):
        d = str(tmp_path / run)
        m = bench.dump_outputs(d, dict(wm=wm, loc_logits=-wm, mean_prob=torch.zeros(32, 16)))
        assert _total_bytes(d) <= bench.DUMP_BUDGET_BYTES
        out[run] = np.load(os.path.join(d, "wm.npy"))
    s = m["arrays"]["wm"]["sample"]
    assert s["of"] == wm.numel() and out["a"].size == s["elements"] > wm.numel() // 4
    assert np.array_equal(out["a"], out["b"])                   # the same elements on every run
    idx = np.sort(np.random.default_rng(s["seed"]).choice(s["of"], s["elements"], replace=False))
    assert np.array_equal(out["a"], wm.numpy().reshape(-1)[idx])
    assert "sample" not in m["arrays"]["mean_prob"]


def _bench(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=300)


def test_bench_refuses_what_it_cannot_time_or_dump():
    r = _bench(["--steps", "0"])
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr
    for wl in ("grad_allreduce", "rendezvous"):
        r = _bench(["--workload", wl, "--dump-outputs", "unused"])
        assert r.returncode != 0 and "computes no outputs to dump" in r.stderr, (wl, r.stderr[-300:])
