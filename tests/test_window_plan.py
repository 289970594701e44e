"""Windowed execution on the CPU: halo derivation, planner invariants, and exactness of windows / live sessions against the numpy
oracle (no GPU)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import wv_oracle as O  # noqa: E402
from waveverify_amd.config import default_config  # noqa: E402
from waveverify_amd.init import random_state_dict, synthetic_clips  # noqa: E402
from waveverify_amd.session import StreamSession  # noqa: E402
from waveverify_amd.window import halo, pipeline_hop, plan  # noqa: E402

KINDS = ("generator", "detector", "locator")
SMALL = dict(strides=[2, 2], channels_enc=8, n_fft_base=16)


def _forward(cfg, net, x, msg):
    if cfg.kind == "generator":
        return O.embed(cfg, net, x, msg[: x.shape[0]] if msg.shape[0] > 1 else msg)
    return O.detector_forward(cfg, net, x)


def test_halo_defaults():
    assert [halo(default_config(k)) for k in KINDS] == [5760, 2880, 416]
    assert pipeline_hop([default_config(k) for k in KINDS]) == 320


@pytest.mark.parametrize("kw", [{}, {"dilation_base": 2}, SMALL], ids=["default", "dilation2", "small"])
@pytest.mark.parametrize("kind", KINDS)
def test_halo_bounds_the_receptive_field(kind, kw):
    """Perturbing input sample p changes no output at or beyond p + halo, and none before p's frame start."""
    cfg = default_config(kind, **kw)
    net = O._Net(cfg, random_state_dict(cfg, 3))
    hop, H = cfg.hop_length, halo(cfg)
    assert H % hop == 0
    p = 3 * hop + hop // 3 + 1
    T = p + H + 2 * hop + 17
    x, msg = synthetic_clips(1, T, seed=5)
    y0 = _forward(cfg, net, x, msg)
    x2 = x.copy()
    x2[..., p] += 0.5
    y1 = _forward(cfg, net, x2, msg)
    changed = np.nonzero(np.any(y0 != y1, axis=(0, 1)))[0]
    assert changed.size, "the perturbation reached no output"
    assert changed.max() < p + H
    assert changed.min() >= p // hop * hop


def _tol(ref):
    """1e-6, scaled by the output's magnitude (logits reach a few units; f32 summation order differs between lengths)."""
    return 1e-6 * max(1.0, float(np.abs(ref).max()))


def _check_partition(launches, lengths, hop, max_windows):
    cover = [np.zeros(T, np.int32) for T in lengths]
    for group in launches:
        assert 1 <= len(group) <= max_windows
        assert len({w.length for w in group}) == 1
        for w in group:
            T = lengths[w.clip]
            assert w.start % hop == 0 and w.start >= 0 and w.start + w.length <= T
            assert w.start <= w.keep_lo < w.keep_hi <= w.start + w.length
            assert w.keep_lo % hop == 0
            assert w.keep_hi % hop == 0 or w.keep_hi == T
            if w.keep_hi == T:
                assert w.start + w.length == T
            if w.start + w.length != T:
                assert w.length % hop == 0
            cover[w.clip][w.keep_lo: w.keep_hi] += 1
    for c in cover:
        assert np.all(c == 1)


@pytest.mark.parametrize("kind", KINDS)
def test_plan_invariants_fuzzed(kind):
    cfg = default_config(kind)
    hop, H = cfg.hop_length, halo(cfg)
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = int(rng.integers(1, 6))
        lengths = [int(rng.integers(1, 400000)) for _ in range(n)]
        window = int(rng.integers(H + hop, 200000))
        mw = int(rng.integers(1, 9))
        launches = plan(lengths, window, cfg, mw)
        _check_partition(launches, lengths, hop, mw)
        L = -(-window // hop) * hop
        for group in launches:
            assert group[0].length <= L
            for w in group:
                if lengths[w.clip] > L:
                    assert w.start == 0 and w.keep_lo == 0 or w.keep_lo - w.start >= H


def test_plan_rejects_windows_shorter_than_the_halo():
    with pytest.raises(ValueError):
        plan([100000], 5000, default_config("generator"))


@pytest.mark.parametrize("kind", KINDS)
def test_windowed_oracle_equals_whole_clip(kind):
    """The planner's windows through the numpy oracle, stitched, equal the oracle on the whole clip (4 s ragged, 1 s windows)."""
    cfg = default_config(kind)
    net = O._Net(cfg, random_state_dict(cfg, 0))
    T = 4 * 16000 + 77
    x, msg = synthetic_clips(1, T, seed=9)
    ref = _forward(cfg, net, x, msg)
    out = np.full_like(ref, np.nan)
    launches = plan([T], 16000, cfg, max_windows=2)
    assert sum(len(g) for g in launches) > 3
    for group in launches:
        xw = np.concatenate([x[:, :, w.start: w.start + w.length] for w in group])
        yw = _forward(cfg, net, xw, msg)
        for i, w in enumerate(group):
            out[0, :, w.keep_lo: w.keep_hi] = yw[i, :, w.keep_lo - w.start: w.keep_hi - w.start]
    np.testing.assert_allclose(out, ref, rtol=0, atol=_tol(ref))


@pytest.mark.parametrize("kind", KINDS)
def test_session_state_machine_on_the_oracle(kind):
    """Irregular pushes then flush(): the concatenated outputs equal the whole-clip oracle; each push returns exactly the newly
    completed frames."""
    cfg = default_config(kind)
    net = O._Net(cfg, random_state_dict(cfg, 1))
    hop = cfg.hop_length
    sizes = [1, 319, 320, 641, 5, 7000, 0, 3333]
    T = sum(sizes)
    S = 2
    x, msg = synthetic_clips(S, T, seed=4)
    ref = _forward(cfg, net, x, msg)

    def fwd(win, keep):
        return _forward(cfg, net, win, msg)[:, :, keep:]

    sess = StreamSession(S, hop, halo(cfg), fwd)
    outs, seen = [], 0
    for n in sizes:
        y = sess.push(x[:, 0, seen: seen + n])
        seen += n
        m = seen // hop * hop
        got = 0 if y is None else y.shape[-1]
        assert got == m - sum(o.shape[-1] for o in outs)
        assert sess.samples_seen == m
        if y is not None:
            outs.append(y)
    y = sess.flush()
    if y is not None:
        outs.append(y)
    assert sess.samples_seen == T
    got = np.concatenate(outs, axis=-1)
    np.testing.assert_allclose(got, ref, rtol=0, atol=_tol(ref))
    with pytest.raises(RuntimeError):
        sess.push(x[:, 0, :1])
    sess.reset()
    y = sess.push(x[:, 0, :2 * hop])
    ref2 = _forward(cfg, net, x[:, :, :2 * hop], msg)
    np.testing.assert_allclose(y, ref2, rtol=0, atol=_tol(ref2))
