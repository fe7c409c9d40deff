"""-m gpu: what a plain `bench.py` run reports and what only `--full` adds.  A plain run is set-up, warm-up, timed steps,
--dump-outputs and the headline line; the side measurements run after the timed steps of a --full run, so both runs time and
dump the same steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config", "step_ms")
SIDE = ("roofline", "kernels", "power", "single_stream", "fp32_mfma_everywhere", "bf16x3_exact", "roofline_loss", "other_configs",
        "inference", "cpu_baseline")


def _run(extra, dump_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "3", "--batch", "2", "--size", "64",
           "--dump-outputs", str(dump_dir)] + extra
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only_and_full_adds_the_side_measurements(tmp_path):
    plain = _run([], tmp_path / "plain")
    assert all(k in plain for k in HEADLINE), sorted(plain)
    assert not [k for k in SIDE if k in plain], sorted(plain)
    assert plain["unit"] == "images/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert abs(plain["value"] - (2 + 2) / (plain["ms_per_step"] * 1e-3)) / plain["value"] < 0.02      # 2 labelled + 2 unlabelled per step

    full = _run(["--full", "--analysis-steps", "1", "--exact-steps", "1", "--no-power-log"], tmp_path / "full")
    for k in ("roofline", "kernels", "single_stream", "fp32_mfma_everywhere", "bf16x3_exact", "cpu_baseline"):
        assert k in full, (k, sorted(full))
    assert full["kernels"] and full["cpu_baseline"]["value"] > 0
    assert all(k in full for k in HEADLINE)

    # the side measurements come after the timed steps: both runs computed the same steps
    assert plain["config"]["final_loss"] == full["config"]["final_loss"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and names == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        assert np.array_equal(np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)), n
