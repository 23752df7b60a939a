"""GPU: a plain bench.py run measures the headline figure and nothing else; --full adds the per-kernel, roofline, reference-caller, render,
structure and trace-counter fields after the same timed steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--gaussians", "20000", "--env-gaussians", "8192", "--res", "128"]


def _bench(extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True, env=env, cwd=ROOT, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_plain_run_only_times_the_steps_full_run_adds_the_rest():
    plain = _bench([])
    full = _bench(["--full", "--no-cpu-baseline"])          # (the CPU baselines take minutes; --full runs them unless told not to)
    for d in (plain, full):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["ms_per_step_spread"]["timed_steps"] == 3
        assert d["unit"] == "iters/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert plain["metric"] == full["metric"]
    for k in ("kernels", "roofline", "cpu_baseline", "bvh", "trace_counts", "render_mpix_per_s", "exchange", "launches"):
        assert plain[k] is None, k
    for k in ("reference_caller_ms_per_step", "extension_ms_per_step", "pmc_summary"):
        assert plain["config"][k] is None, k
    assert full["kernels"] and full["roofline"] is not None and full["bvh"] is not None and full["trace_counts"] is not None
    assert full["render_mpix_per_s"] > 0 and full["config"]["reference_caller_ms_per_step"] > 0 and full["config"]["extension_ms_per_step"] > 0
    assert full["cpu_baseline"] is None and full["exchange"] is None                # (--no-cpu-baseline; N = 1)
