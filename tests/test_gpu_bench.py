"""bench.py on the device: a plain run measures the headline and nothing after its timed steps; --full adds the side
measurements (small batch here: the structure of the JSON line is under test, not the figures)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SIDE = ("roofline", "opt_in_modes", "with_optimizer", "fresh_batches")
FULL_ONLY = SIDE + ("counters", "other_workloads", "cpu_baseline", "comm")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--batch", "4",
                        "--npoints", "1024"] + list(extra), capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE) and out["value"] > 0 and out["steps"] == 3 and out["warmup"] == 2, out
    return out


def test_plain_run_measures_the_headline_only():
    out = _bench()
    assert not set(FULL_ONLY) & set(out), sorted(set(FULL_ONLY) & set(out))


def test_full_run_adds_the_side_measurements():
    out = _bench("--full", "--no-cpu-baseline", "--no-side-workloads")
    assert all(k in out for k in SIDE), sorted(set(SIDE) - set(out))
    assert out["roofline"]["launches_per_step"] > 0 and out["fresh_batches"]["value"] > 0, out
    assert out["with_optimizer"]["value"] > 0 and out["opt_in_modes"]["bf16"] > 0, out
