#!/usr/bin/env python3
"""h16_launch_plan.json: the (kernel|role, launches) rows, workspace sizes and refusals of tests/h16_plan_cases.py, as the built library
of a checkout produces them.  Needs the MI355X.

    python tests/golden/make_golden_h16_plan.py [--tree DIR] [--out FILE]

--tree: the checkout whose waveverify_amd (with its built library) is recorded; default: this one.  The file in git was recorded from
the commit before the f16 plan moved into pack_model, so that tests/test_gpu_h16_plan.py holds every later build to that commit's launches."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(HERE)))
ap.add_argument("--out", default=os.path.join(HERE, "h16_launch_plan.json"))
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(HERE))                        # tests/: h16_plan_cases, test_gpu_h16
sys.path.insert(0, os.path.abspath(a.tree))                      # the recorded waveverify_amd

from h16_plan_cases import net_configs, run_net                  # noqa: E402

out = {}
for net_id, cfg in net_configs().items():
    for key, rec in run_net(net_id, cfg).items():
        rec.pop("error", None)
        out[key] = rec
with open(a.out, "w") as f:
    f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in out.items()) + "\n}\n")
print(f"{len(out)} records, {sum('refused' in v for v in out.values())} refused -> {a.out}")
