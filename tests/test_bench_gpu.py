"""GPU: a plain bench.py run (no --full) does only what its headline figure needs - set up, warm up, time the steps,
print the line - and stays within 30 s of wall time outside its steps; what a --full run adds is not on its line."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "kernels", "cpu_baseline", "pcie_inclusive", "host_enqueue_ms_per_step",
             "chain_frac_of_measured_peak")


def test_plain_bench_run_is_lean(built):
    steps, warmup = 4, 2
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"] == "filtered frames/sec, 1080p YUV420p NLMeans+decomb chain"
    assert line["unit"] == "output frames/s" and line["higher_is_better"] is True and line["dtype"].startswith("u8")
    assert line["steps"] == steps and line["warmup"] == warmup and line["value"] > 0
    # value counts the output frames of the timed steps: 32 per step
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 32) < 0.01 * 32
    for k in FULL_ONLY:
        assert k not in line, k
    assert "eedi2_mask_density" not in line["config"]
    outside = wall - (steps + warmup) * line["ms_per_step"] / 1e3
    assert outside < 30.0, f"{outside:.1f} s outside the steps"
