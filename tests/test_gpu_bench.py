"""bench.py end to end at a small size: a plain run prints the headline alone, `--full` adds the profiled pass, the other passes and
the CPU baseline after the timed steps, and both return the same outputs from their last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"}
FULL_ONLY = {
    "f32": {"with_locator", "roofline", "roofline_film", "kernels", "profiled_pass", "cpu_baseline", "parity", "reduced_precision"},
    "f16": {"with_locator", "roofline", "kernels", "profiled_pass", "vs_f32_mode", "cpu_baseline", "parity"},
}


def _bench(args, dump_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "4", "--cpu-clips", "2",
                        "--dump-outputs", str(dump_dir)] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path, precision):
    plain = _bench(["--precision", precision], tmp_path / "plain")
    full = _bench(["--precision", precision, "--full"], tmp_path / "full")
    assert HEADLINE <= plain.keys() and not FULL_ONLY[precision] & plain.keys(), sorted(plain)
    assert FULL_ONLY[precision] <= full.keys(), sorted(full)
    for k in HEADLINE - {"value", "ms_per_step"}:
        assert plain[k] == full[k], k
    assert plain["dtype"] == precision and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert full["parity"]["clips_checked"] == 2
    if precision == "f32":
        assert full["parity"]["ber_vs_oracle"] == 0.0 and full["reduced_precision"]["bits_compared"] == 4 * 16
    for name in ("wm", "mean_prob", "bits"):
        assert np.array_equal(np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")), name
