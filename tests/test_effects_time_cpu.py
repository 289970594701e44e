"""Host side of the time-domain effects (waveverify_amd/effects.py), no GPU: the random draws reproduce what the reference drew for
tests/golden/effects_time.npz under the same seeds (make_golden_effects_time.py replays the reference's own draw calls and checks the
echo length against the reference's output), the rational `speed` resamples by, and the C ABI's declarations."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from waveverify_amd import _lib
from waveverify_amd import effects as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "effects_time.npz"))
CASES = json.loads(str(GOLD["cases"]))
SR = 16000

NEW_EXPORTS = ("wv_fx_pointwise", "wv_fx_median", "wv_fx_shush", "wv_fx_echo_peaks", "wv_fx_echo_apply", "wv_fx_echo_backward_workspace_bytes",
               "wv_fx_echo_backward", "wv_fx_smooth", "wv_fx_smooth_backward", "wv_fx_scatter_zero", "wv_fx_stretch_linear")


def seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def of(name):
    got = [c for c in CASES if c["name"] == name]
    assert got, name
    return got


def test_echo_plan_reproduces_the_reference_draws():
    for c in of("echo"):
        seed_all(c["seed"])
        n, volume = E.echo_plan(c["T"], SR, **c["params"])
        assert n == int(GOLD[c["key"] + "_n"]) and volume == float(GOLD[c["key"] + "_volume"]), c
        assert 2 <= n <= c["T"] // 2 + 1


def test_smooth_window_reproduces_the_reference_draw():
    for c in of("smooth"):
        seed_all(c["seed"])
        assert E.smooth_window(c["params"]["window_size_range"]) == int(GOLD[c["key"] + "_w"]), c


def test_suppression_indices_reproduce_the_reference_draws():
    for c in of("sample_suppression"):
        seed_all(c["seed"])
        idx = E.suppression_indices(2, 1, c["T"], c["params"]["suppression_percentage"])
        assert idx.dtype == np.int32 and np.array_equal(idx, GOLD[c["key"] + "_idx"]), c
    assert E.suppression_indices(2, 1, 37, 0.0).shape == (2, 0)


def test_pink_noise_host_reproduces_the_reference_generator():
    for c in of("pink_noise"):
        seed_all(c["seed"])
        noise = E.pink_noise_host(2 * c["T"])
        assert noise.dtype == np.float32 and np.array_equal(noise, GOLD[c["key"] + "_noise"].reshape(-1)), c
        assert np.abs(noise).max() == 1.0


def test_speed_ratio_is_the_rational_of_the_speed():
    assert E.speed_ratio(0.8) == (4, 5) and E.speed_ratio(1.25) == (5, 4) and E.speed_ratio(0.9) == (9, 10) and E.speed_ratio(1.0) == (1, 1)
    assert E.resampled_length(16000, *E.speed_ratio(0.8)) == 20000             # T becomes ceil(5 T / 4)
    with pytest.raises(ValueError, match="positive"):
        E.speed_ratio(0.0)


def test_the_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    declared = set(re.findall(r"\b(wv_[a-z0-9_]+)\s*\(", header))
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert int(re.search(r"#define WV_FX_MEDIAN_MAX_K (\d+)", header).group(1)) == E.MEDIAN_MAX_K
    assert int(re.search(r"#define WV_FX_SMOOTH_MAX_W (\d+)", header).group(1)) == E.SMOOTH_MAX_W
    for op, name in ((E.OP_SCALE, "SCALE"), (E.OP_ADD_NOISE, "ADD_NOISE"), (E.OP_QUANTIZE, "QUANTIZE"), (E.OP_MUL, "MUL")):
        assert int(re.search(rf"#define WV_FX_{name} (\d+)", header).group(1)) == op


def test_sixteen_of_the_twenty_effect_names_are_served_and_four_refused():
    served = [n for n in dir(E.AudioEffects) if not n.startswith("_")]
    assert len(served) == 16 and set(E.REFUSED) == {"mp3_lossy_compression", "aac_lossy_compression", "encodec", "random_equalization"}
    assert not set(served) & set(E.REFUSED)
    x = torch.zeros(1, 1, 64)
    for name in E.REFUSED:
        with pytest.raises(NotImplementedError):
            E.apply_effect(name, {}, x, None)
    state = torch.get_rng_state()
    for name in ("speed", "echo", "pink_noise", "median_filter", "smooth", "amplitude_scaling", "quantization", "sample_suppression", "random_noise",
                 "white_noise", "shush"):                 # no CPU fallback: a CPU tensor is refused before anything is drawn or run
        assert name in served
        with pytest.raises(RuntimeError, match="GPU"):
            getattr(E.AudioEffects, name)(x)
    assert torch.equal(torch.get_rng_state(), state)
