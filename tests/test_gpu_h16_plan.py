"""The launch plan of every net-level entry point, pinned: tests/golden/h16_launch_plan.json holds, for each case of h16_plan_cases, the
(kernel|role, launches) rows the profiler recorded -- or the refusal code -- as the build BEFORE the f16 plan moved into pack_model
produced them (tests/golden/make_golden_h16_plan.py).  This library must launch the same kernels under the same roles the same number of
times, need the same workspace and refuse the same calls.  A stage of the f16 plan that falls to its slower route (the STFT kernel + a
1x1 instead of spec16, the f32 tail instead of head16) changes no numeric test's verdict; it changes these rows."""
import json
import os

import pytest

from h16_plan_cases import net_configs, run_net

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "h16_launch_plan.json")) as f:
    GOLDEN = json.load(f)
NETS = net_configs()


def test_the_golden_covers_exactly_the_cases():
    nets = {k.split("/")[0] for k in GOLDEN}
    assert nets == set(NETS), nets ^ set(NETS)
    refused = [k for k, v in GOLDEN.items() if "refused" in v]
    assert refused and all(k.startswith("narrow16.") and k.endswith("/f16") for k in refused), refused
    assert len([k for k in GOLDEN if k.startswith("narrow16.") and k.endswith("/f16")]) == len(refused)


@pytest.mark.parametrize("net_id", list(NETS))
def test_launch_plan_matches_the_golden(net_id):
    got = run_net(net_id, NETS[net_id])
    want = {k: v for k, v in GOLDEN.items() if k.split("/")[0] == net_id}
    assert set(got) == set(want), set(got) ^ set(want)
    for key, rec in sorted(got.items()):
        exp = want[key]
        if "workspace_bytes" in exp:
            assert rec == exp, (key, rec, exp)
        elif "refused" in exp:
            assert rec.get("refused") == exp["refused"], (key, rec, exp)
        else:
            assert "rows" in rec, (key, rec)
            assert rec["rows"] == exp["rows"], (key, [r for r in rec["rows"] if r not in exp["rows"]], [r for r in exp["rows"] if r not in rec["rows"]])
