"""data.ClipPool on the GPU: sample()'s info against a CPU restatement of the draw order and the accept rule run on the float64 oracle's
loudness (tests/loudness_cases.py), x bitwise the chosen arena slice, the gate keeping silence out, the cutoff-free route, and the two
callers in the trainer -- fit() against a hand-written loop, validate(loudness=True) against metrics.Loudness."""
import random
from functools import lru_cache

import numpy as np
import pytest
import torch

import loudness_cases as lc
from waveverify_amd import metrics, profile
from waveverify_amd.data import ClipPool

pytestmark = pytest.mark.gpu

FS, T, TRIES, B = 16000, 16000, 8, 8
SEEDS = (0, 1, 2, 3)


@lru_cache(maxsize=None)
def _clips():
    rng = np.random.default_rng(11)
    tail = np.zeros(48000, np.float32)
    tail[-8000:] = 0.1 * rng.standard_normal(8000)
    return (np.zeros(40000, np.float32),                                         # silent
            (0.1 * rng.standard_normal(50000)).astype(np.float32),               # loud noise
            (0.1 * rng.standard_normal(9000)).astype(np.float32),                # shorter than T
            tail)                                                                # silent except for its last 0.5 s


@lru_cache(maxsize=None)
def _pool():
    return ClipPool([torch.from_numpy(c) if i % 2 else c for i, c in enumerate(_clips())], FS)


@lru_cache(maxsize=None)
def _expected(seed):
    """The documented draws and the accept rule, restated, on the oracle's loudness of every candidate."""
    clips = _clips()
    rng = np.random.default_rng(seed)
    c = rng.integers(len(clips), size=B)
    u = rng.random((B, TRIES))
    offset = np.array([[int(np.floor(u[b, k] * (max(len(clips[c[b]]) - T, 0) + 1))) for k in range(TRIES)] for b in range(B)])
    windows = np.zeros((B, TRIES, T), np.float32)
    for b in range(B):
        for k in range(TRIES):
            w = clips[c[b]][offset[b, k]: offset[b, k] + T]
            windows[b, k, : len(w)] = w
    lufs = np.array([[lc.loudness(windows[b, k], FS) for k in range(TRIES)] for b in range(B)])
    assert np.abs(lufs + 40.0).min() > 1e-6                                      # no accept decision can turn on rounding
    choice = np.array([next((k for k in range(TRIES) if lufs[b, k] > -40.0), TRIES - 1) for b in range(B)])
    return {"clip": c, "offset": offset, "lufs": lufs, "choice": choice, "windows": windows}


def test_pool_is_one_immutable_arena():
    pool, clips = _pool(), _clips()
    assert len(pool) == 4 and pool.seconds == sum(len(c) for c in clips) / FS and pool.sample_rate == FS
    assert pool.arena.is_cuda and pool.arena.dtype == torch.float32 and np.array_equal(pool.arena.cpu().numpy(), np.concatenate(clips))
    assert pool.offsets.tolist() == [0, 40000, 90000, 99000] and pool.lengths.tolist() == [40000, 50000, 9000, 48000]
    with pytest.raises(ValueError):
        pool.offsets[0] = 1
    with pytest.raises(AttributeError):
        pool.arena = None
    with pytest.raises(ValueError):
        ClipPool([], FS)
    with pytest.raises(ValueError):
        ClipPool([np.zeros((2, 100))], FS)
    with pytest.raises(ValueError):
        ClipPool([np.zeros(100)], 22055)


@pytest.mark.parametrize("seed", SEEDS)
def test_info_is_the_cpu_restatement_and_x_is_the_chosen_slice(seed):
    want = _expected(seed)
    before = _pool().arena.clone()
    x, info = _pool().sample(B, 1.0, rng=seed)
    rows = np.arange(B)
    assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (B, 1, T)
    assert set(info) == {"clip", "offset", "tries_used", "lufs"} and all(tuple(v.shape) == (B,) for v in info.values())
    assert np.array_equal(info["clip"], want["clip"]) and np.array_equal(info["tries_used"], want["choice"] + 1)
    assert np.array_equal(info["offset"], want["offset"][rows, want["choice"]])
    assert np.abs(info["lufs"] - want["lufs"][rows, want["choice"]]).max() <= 1e-9
    assert np.array_equal(x[:, 0].cpu().numpy().view(np.int32), want["windows"][rows, want["choice"]].view(np.int32))     # bitwise, zero-padded
    assert torch.equal(_pool().arena, before)
    short = want["clip"] == 2
    if short.any():
        assert not x[:, 0].cpu().numpy()[short][:, 9000:].any() and (info["offset"][short] == 0).all()
    # the gate: no silent excerpt while a loud try exists among the eight
    loud_exists = (want["lufs"] > -40.0).any(axis=1)
    assert (info["lufs"][loud_exists] > -40.0).all() and (info["tries_used"][~loud_exists] == TRIES).all()
    again, info2 = _pool().sample(B, 1.0, rng=np.random.default_rng(seed))       # the same seed, the same batch
    assert torch.equal(again, x) and all(np.array_equal(info[k], info2[k]) for k in info)


def test_the_seeds_meet_every_branch():
    c = np.concatenate([_expected(s)["clip"] for s in SEEDS])
    ch = np.concatenate([_expected(s)["choice"] for s in SEEDS])
    lufs = np.concatenate([_expected(s)["lufs"] for s in SEEDS])
    assert set(c.tolist()) == {0, 1, 2, 3}
    assert (ch == 0).any() and ((ch > 0) & (ch < TRIES - 1)).any() and ((lufs > -40.0).any(axis=1) == False).any()   # noqa: E712


def test_without_a_cutoff_try_0_is_taken_and_nothing_is_measured():
    want = _expected(1)
    profile.enable(True)
    profile.reset()
    try:
        x, info = _pool().sample(B, 1.0, rng=1, loudness_cutoff=None)
        names = {e["kernel"] for e in profile.collect()}
        profile.reset()
        _pool().sample(B, 1.0, rng=1)
        gated = {e["kernel"]: e["launches"] for e in profile.collect()}
    finally:
        profile.enable(False)
    assert names == {"pool_sample"} and gated == {"loudness": 1, "pool_sample": 1}                      # one launch each, nothing else
    assert np.array_equal(info["clip"], want["clip"]) and np.array_equal(info["offset"], want["offset"][:, 0])
    assert (info["tries_used"] == 1).all() and np.isnan(info["lufs"]).all()
    assert np.array_equal(x[:, 0].cpu().numpy().view(np.int32), want["windows"][:, 0].view(np.int32))


def test_batches_is_sample_on_one_generator():
    it = _pool().batches(4, 0.5, seed=5)
    a, b = next(it), next(it)
    rng = np.random.default_rng(5)
    assert torch.equal(a, _pool().sample(4, 0.5, rng=rng)[0]) and torch.equal(b, _pool().sample(4, 0.5, rng=rng)[0])
    assert tuple(a.shape) == (4, 1, 8000) and not torch.equal(a, b)


def _trainer():
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import WatermarkTrainer
    small = dict(channels_enc=8, dimension=16, strides=[2, 2], n_fft_base=16)
    cg = default_config("generator", channels_dec=8, n_residual_dec=1, **small)
    cd, cl = default_config("detector", output_dim=8, **small), default_config("locator", output_dim=8, **small)
    return WatermarkTrainer(cg, random_state_dict(cg, 1, parametrized=True), cd, random_state_dict(cd, 1, parametrized=True), cl,
                            random_state_dict(cl, 1, parametrized=True))


def _seed_globals():
    np.random.seed(0)
    random.seed(0)
    torch.manual_seed(0)


def test_fit_is_sample_plus_seeded_messages_plus_step():
    a, b = _trainer(), _trainer()
    _seed_globals()
    got = a.fit(_pool(), steps=2, batch=4, seed=3, duration=0.5)
    _seed_globals()
    rng, gen, want = np.random.default_rng(3), torch.Generator().manual_seed(3), []
    for _ in range(2):
        x, _ = _pool().sample(4, 0.5, rng=rng)
        msg = torch.randint(0, 2, (4, 16), generator=gen).float()
        want.append(b.step(x, msg.cuda()))
    assert len(got) == 2
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key in w:
            if torch.is_tensor(w[key]):
                assert torch.equal(g[key], w[key]), key
    assert torch.equal(a.G.arena, b.G.arena) and torch.equal(a.D.arena, b.D.arena)
    with pytest.raises(ValueError):
        a.fit(ClipPool([np.zeros(48000, np.float32)], 48000), steps=1, batch=2)


def test_validate_with_loudness_adds_three_keys_that_are_the_module():
    tr = _trainer()
    x, _ = _pool().sample(3, 0.5, rng=2)
    msg = torch.from_numpy(np.random.default_rng(0).integers(0, 2, (3, 16)).astype(np.float32)).cuda()
    plain = tr.validate(x, msg, eval_effects=[("identity", {})])
    out = tr.validate(x, msg, eval_effects=[("identity", {})], loudness=True)
    assert set(out) - set(plain) == {"LUFS delta"} and set(out["per_clip"]) - set(plain["per_clip"]) == {"lufs_in", "lufs_wm"}
    assert set(plain) <= set(out) and set(plain["per_clip"]) <= set(out["per_clip"])
    assert set(plain) == {"dec/loss", "loc/loss", "waveform/loss", "loss", "SISNR", "identity/ber", "identity/miou", "per_clip"}
    assert set(plain["per_clip"]) == {"effects", "errors", "valid", "ber", "miou", "sisnr"}
    for k in plain:
        if k != "per_clip":
            assert (torch.equal(out[k], plain[k]) if torch.is_tensor(plain[k]) else out[k] == plain[k]), k
    wm = tr.G.forward(x, msg)
    lin, lwm = metrics.Loudness()(x, FS).cpu().numpy(), metrics.Loudness()(wm, FS).cpu().numpy()
    assert np.array_equal(out["per_clip"]["lufs_in"], lin) and np.array_equal(out["per_clip"]["lufs_wm"], lwm)
    assert out["per_clip"]["lufs_in"].dtype == np.float64 and out["LUFS delta"] == float((lwm - lin).mean())
    for b in range(3):
        assert abs(lin[b] - lc.loudness(x[b, 0].cpu().numpy(), FS)) <= 1e-9
