"""oracle/wv_oracle_h16.py's detector and locator tails on the CPU: against the pinned exact port (oracle/wv_oracle_torch.py) within the
f16 mode's noise, their gate against a table of configurations, and the sensitivity of the head16 restatement the GPU tests rely on."""
import numpy as np
import pytest
import torch

from oracle import wv_oracle_h16 as O16
from oracle import wv_oracle_torch as OT
from waveverify_amd.config import default_config
from waveverify_amd.init import random_state_dict, synthetic_clips


@pytest.mark.parametrize("kind,kw,expect", [
    ("detector", {}, True),                                    # D 128, 16 bits, hop 320
    ("detector", {"nbits": 8}, True),
    ("detector", {"nbits": 20}, True),
    ("detector", {"nbits": 32}, True),
    ("detector", {"nbits": 36}, False),                        # more bits than head16_kernel's waves hold
    ("detector", {"nbits": 64}, False),
    ("detector", {"nbits": 6}, False),                         # nb % 4
    ("detector", {"dimension": 144}, False),                   # D > 128
    ("detector", {"dimension": 40}, False),                    # D % 16
    ("detector", {"dimension": 64}, True),
    ("detector", {"strides": [5, 5, 4, 2]}, False),            # hop 200
    ("detector", {"strides": [8, 4, 2], "channels_enc": 32}, True),
    ("locator", {}, False),                                    # one output channel
    ("generator", {}, False),
])
def test_head16_gate_table(kind, kw, expect):
    assert O16.head16_gate(default_config(kind, **kw)) is expect


def test_spec_post_plan_table():
    assert O16.spec_post16(default_config("detector"))
    assert O16.spec_post16(default_config("locator", channels_enc=96))
    assert not O16.spec_post16(default_config("detector", channels_enc=8, strides=[]))


@pytest.fixture(scope="module")
def nets():
    out = {}
    for kind, kw in (("detector", {}), ("locator", {}), ("detector", {"nbits": 36})):
        cfg = default_config(kind, **kw)
        out[kind + str(cfg.nbits if kind == "detector" else "")] = OT.Net(cfg, random_state_dict(cfg, 0))
    return out


@pytest.mark.parametrize("B,T", [(2, 16000), (1, 12345), (3, 333), (1, 1)])
def test_oracle_tails_vs_the_exact_port(nets, B, T):
    """The f16 mode's tails within f16 noise of the exact path: logits within 1e-3 of max(1, |logits|max) (measured 3.5e-4 at most), mean
    probabilities within 5e-4 (measured 5e-6 .. 1.2e-4, the largest at T = 1 where one sample is the mean)."""
    x = synthetic_clips(B, T, seed=B + T)[0]
    for key in ("detector16", "locator"):
        net = nets[key]
        ex = OT.detector_logits(net, x).double()
        lg = O16.detect_logits(net, x)
        assert lg.shape == ex.shape
        assert float((lg - ex).abs().max()) <= 1e-3 * max(1.0, float(ex.abs().max()))
        if key == "detector16":
            mp = O16.detect_mean_prob(net, x)
            assert mp.shape == (B, 16)
            assert float((mp - torch.sigmoid(ex).mean(-1)).abs().max()) <= 5e-4
            assert float((mp - torch.sigmoid(lg).mean(-1)).abs().max()) <= 5e-4


def test_mean_prob_beyond_the_gate_is_the_f32_tail(nets):
    x = synthetic_clips(2, 3000, seed=1)[0]
    net = nets["detector36"]
    assert torch.equal(O16.detect_mean_prob(net, x), torch.sigmoid(O16.detect_logits(net, x)).mean(-1))


def test_head16_restatement_is_sensitive():
    """What the kernel-level bars (tests/test_gpu_h16_head.py, 1e-6) stand on: the reference without the f16 rounding of z, or with t off
    by one inside a frame, or with two bits' waves swapped, moves per-sample probabilities by orders of magnitude more than the bar."""
    rng = np.random.default_rng(3)
    D, nb, hop, Fr = 64, 16, 32, 70
    lat = rng.standard_normal((1, D, Fr)).astype(np.float32)
    wc = (1.5 / np.sqrt(D) * rng.standard_normal((D, nb * hop))).astype(np.float32)
    bc = (0.5 * rng.standard_normal(nb)).astype(np.float32)
    p = O16.head16_probs(lat, wc, bc)
    assert np.abs(O16.head16_probs(lat, wc, bc, z16=False) - p).max() > 1e-4
    assert np.abs(O16.head16_probs(lat, wc, bc, shift=1) - p).max() > 1e-2
    assert np.abs(p[:, [4, 5, 6, 7, 0, 1, 2, 3] + list(range(8, 16))] - p).max() > 1e-2
    T = Fr * hop - 5
    assert float((O16.head16(lat, wc, bc, T, keep_lo=[0], keep_hi=[T]) - T * O16.head16(lat, wc, bc, T)).abs().max()) < 1e-9
    assert float(O16.head16(lat, wc, bc, T, keep_lo=[64 * hop], keep_hi=[64 * hop]).abs().max()) == 0.0


def test_head16_bounds_hold_the_reference():
    """The interval the GPU tests use: it contains the unmoved reference and is a single value except for frames whose z sits within two f32
    ulps of the scale of an f16 rounding midpoint."""
    rng = np.random.default_rng(4)
    D, nb, hop, Fr, T = 128, 8, 32, 200, 200 * 32 - 3
    lat = rng.standard_normal((2, D, Fr)).astype(np.float32)
    wc = (1.5 / np.sqrt(D) * rng.standard_normal((D, nb * hop))).astype(np.float32)
    bc = (0.5 * rng.standard_normal(nb)).astype(np.float32)
    ref = O16.head16(lat, wc, bc, T).numpy()
    lo, hi = O16.head16_bounds(lat, wc, bc, T)
    assert (lo <= ref + 1e-15).all() and (ref <= hi + 1e-15).all()
    assert float((hi - lo).max()) < 1e-5
    lo, hi = O16.head16_bounds(lat, wc, bc, T, keep_lo=[0, 7], keep_hi=[T, 7])
    assert (hi[1] == 0).all() and (lo[1] == 0).all()
    np.testing.assert_allclose(lo[0] / T, O16.head16_bounds(lat[:1], wc, bc, T)[0][0], rtol=1e-12)
