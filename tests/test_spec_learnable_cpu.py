"""spec_learnable without a GPU: the checkpoint configuration's flag, and self-checks of tests/golden/spec_learnable.npz -- its
clamped-bin shares, the side rows' gradients, and the formula the kernels implement (spec_learnable_cases.formula_grad) against the
reference's float64 autograd stored in the fixture."""
import json
import os

import numpy as np
import pytest

import spec_learnable_cases as SLC
from waveverify_amd.checkpoint import apply_argbind_config, argbind_config
from waveverify_amd.config import default_config

CASES = [(i, v) for i in range(len(SLC.UNIT_SHAPES)) for v in SLC.VARIANTS]


@pytest.fixture(scope="module")
def fixture():
    return np.load(SLC.FIXTURE)


def test_argbind_config_default_is_unchanged_and_the_flag_is_written_when_asked(golden_dir):
    fx = json.load(open(os.path.join(golden_dir, "state_dict_keys.json")))
    for name, case in fx.items():
        kind = name.split("/")[1]
        cfg = default_config(kind, **case["overrides"])
        assert argbind_config({kind: cfg}) == argbind_config({kind: cfg}, spec_learnable=False) == case["config"], name
        on = argbind_config({kind: cfg}, spec_learnable=True)
        if kind == "generator":
            assert on["Generator.spec_learnable"] is True and case["config"]["Generator.spec_learnable"] is False
            assert {k: v for k, v in on.items() if k != "Generator.spec_learnable"} == {k: v for k, v in case["config"].items() if k != "Generator.spec_learnable"}
            assert apply_argbind_config("generator", cfg, on).to_dict() == apply_argbind_config("generator", cfg, case["config"]).to_dict()
        else:
            assert on == case["config"] and not any(k.endswith("spec_learnable") for k in on)      # only the Generator has the switch


@pytest.mark.parametrize("i,variant", CASES)
def test_fixture_clamped_share_and_side_rows(fixture, i, variant):
    c = SLC.load_unit(fixture, i, variant)
    F = c["n_fft"] // 2 + 1
    assert 0.0 < c["silent_share"] < 0.5 or (c["T"] == 1 and variant == "dft" and c["silent_share"] == 0.5)
    if variant == "noisy":
        side = c["dBasis"][[F, 2 * F - 1]] if c["rows"] is None else c["dBasis"][np.isin(c["rows"], [F, 2 * F - 1])]
        assert side.shape[0] == 2 and float(np.abs(side).max(axis=1).min()) > 1e-3 * c["peak"]


@pytest.mark.parametrize("i,variant", CASES)
def test_formula_reproduces_the_reference_autograd(fixture, i, variant):
    """C = Basis @ frames; p = re^2 + im^2; dC = dP {re, im} / (std p) where p > 1e-10; dBasis = sum_{b,t} dC frames^T -- evaluated in
    float64 on the CPU against the reference's float64 autograd: 1e-10 of the peak where the fixture holds float64, the float32
    storage rounding (2^-23 of the peak) where it holds float32; peak, Frobenius norm and clamped share of the whole tensor to 1e-10."""
    c = SLC.load_unit(fixture, i, variant)
    g, share = SLC.formula_grad(c["basis"], c["wav"], c["dP"], c["n_fft"], c["hop"])
    assert share == c["silent_share"]
    assert abs(float(np.abs(g).max()) - c["peak"]) <= 1e-10 * c["peak"] and abs(float(np.sqrt((g ** 2).sum())) - c["fro"]) <= 1e-10 * c["fro"]
    got = g if c["rows"] is None else g[c["rows"]]
    e = float(np.abs(got - c["dBasis"]).max()) / c["peak"]
    print(f"MEASURE formula vs reference autograd, u{i} {variant}: {e:.2e}")
    assert e <= (1e-10 if c["stored_f64"] else 2.0 ** -23)


def test_fixture_net_case(fixture):
    g = fixture
    keys = [k[len("net_f64_g:"):] for k in g.files if k.startswith("net_f64_g:")]
    assert len(keys) == len(SLC.NET["strides"]) + 1
    for k in keys:
        g64, g32 = g["net_f64_g:" + k], g["net_f32_g:" + k].astype(np.float64)
        assert g64.dtype == np.float64 and float(np.abs(g64).max()) > 0.0
        assert float(np.abs(g32 - g64).max()) <= 1e-4 * float(np.abs(g64).max())           # the reference's own float32 run meets the project's bar
        moved = float(np.abs(g["net_basis2:" + k] - g["net_basis1:" + k]).max())
        assert 0.0 < moved <= 1.01 * SLC.NET_LR + 1e-6                                     # one AdamW step moves an entry by at most ~lr
    assert float(g["net_loss2"]) < float(g["net_loss1"])
