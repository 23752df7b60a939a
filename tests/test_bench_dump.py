"""bench.py --dump-outputs and --steps: the dump stays within its budget, is float32 and samples large arrays at the same seeded indices on
every run (CPU); end to end, --steps is the number of timed steps and two runs with the same arguments dump the same outputs (GPU)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_dump_outputs_budget_dtype_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # (bench.py sets this default on import)
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {"big%d" % i: torch.randn(300000, 48, generator=g) for i in range(3)}
    arrays["img"] = torch.randn(3, 800, 800, generator=g)
    arrays["radii"] = torch.arange(1000, dtype=torch.int32)
    out = {}
    bench.flatten_outputs("out", {"base": {"img": arrays["img"], "radii": arrays["radii"]}, "pair": (arrays["big0"], 1)}, out)
    assert sorted(out) == ["out.base.img", "out.base.radii", "out.pair.0"]
    runs = []
    for d in ("a", "b"):
        n = bench.dump_outputs(str(tmp_path / d), arrays)
        assert n <= bench.DUMP_BUDGET_BYTES
        assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / d / "*.npy"))) <= 64_000_000
        runs.append(_load(str(tmp_path / d)))
    assert sorted(runs[0]) == sorted(arrays)
    cap = bench.DUMP_BUDGET_BYTES // 4 // len(arrays)
    for k, a in runs[0].items():
        assert a.dtype == np.float32 and np.array_equal(a, runs[1][k])
        if arrays[k].numel() > cap:
            assert a.shape == (cap,) and np.isin(a, arrays[k].numpy()).all()      # a sample of the array's own elements
        else:
            assert np.array_equal(a, arrays[k].numpy().astype(np.float32))      # small arrays whole, shape kept


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_steps_and_dump_outputs_repeat(tmp_path, monkeypatch):
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # (bench.py sets this default on import)
    lines, dumps = [], []
    for d in ("a", "b"):
        out = str(tmp_path / d)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--gaussians", "20000",
               "--env-gaussians", "8192", "--res", "128", "--no-cpu-baseline", "--no-render", "--no-reference-caller", "--dump-outputs", out]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=280)
        assert r.returncode == 0, r.stderr[-3000:]
        js = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(js) == 1, r.stdout[-2000:]
        lines.append(json.loads(js[0]))
        dumps.append(_load(out))
    for d in lines:
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        assert d["ms_per_step_spread"]["repeats"] == 1                             # one timed region ...
        assert d["ms_per_step_spread"]["timed_steps"] == 3                         # ... in which bench.py's step() really ran --steps times
    a, b = dumps
    assert sorted(a) == sorted(b)
    for k in ("out.rgb", "out.base.allmap", "grad.means3D", "grad.env.shs", "param.means3D", "param.env.means3D"):
        assert k in a, sorted(a)
    # same seeded inputs: the runs differ only by the order of floating-point atomic sums -- the last bits of the forward's accumulated maps and
    # of the gradients.  Adam's first update moves every element by at most its lr, whatever the gradient's size, so where a noise-level gradient
    # flips sign the two parameters end up to 2 x lr apart: that, plus rounding, bounds the parameters element by element
    import bench
    tol = {"out": 1e-6, "grad": 1e-5}
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape == b[k].shape and np.isfinite(a[k]).all(), k
        diff = np.abs(a[k].astype(np.float64) - b[k])
        rel = float(diff.max() / (np.abs(b[k]).max() + 1e-12))
        group = k.split(".")[0]
        if group == "param":
            bound = 2 * bench.LR_OF[k.split(".")[-1]] * (1 + 1e-5) + 4 * np.finfo(np.float32).eps * np.abs(b[k])     # (m/sqrt(v) is +-1 to a few ulp)
            record("bench_dump_run_to_run", k, rel, "(|a-b| <= 2 lr + 4 ulp elementwise)")
            assert (diff <= bound).all(), (k, float(diff.max()))
        else:
            record("bench_dump_run_to_run", k, rel, "(tol %.0e)" % tol[group])
            assert rel <= tol[group], (k, rel)
    assert any(np.abs(a[k]).max() > 0 for k in a if k.startswith("grad."))
