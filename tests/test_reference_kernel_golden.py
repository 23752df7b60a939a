"""GPU: the fixture format of tests/golden/dump_reference_kernel_golden.py and the loader that feeds such a fixture to the HIP path.

The sources of the real CUDA/OptiX extensions are not available (the reference tree carries them as empty submodules), so no fixture of
their outputs exists and the oracle's kernel-body arithmetic is "parity unpinned" (DESIGN.md section 5).  Whoever dumps one where that build
is installed commits it under tests/golden/ together with a test that passes it to `_compare_file` (radii bit-exact, every other output and
gradient within 1e-4 of the tensor's scale; a fixture dumped with --allow-local, from this repository's own packages, is refused there).  Until then `test_dump_script_and_loader_agree` keeps the two halves honest against each other:
it runs the dump script over this repository's own drop-in packages (--allow-local) into a temporary file and consumes that file with the
same loader."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import check_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tests", "golden", "dump_reference_kernel_golden.py")
TOL = 1e-4

n = lambda t: t.detach().cpu().numpy()


def _close(test, name, got, want, tol=TOL):
    """Plain contract against a foreign implementation: |a - b| <= tol * (|b| + mean|b|) elementwise (no oracle floors exist for these fixtures)."""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    return check_close(test, name, got, want, tol=tol)


def _run_raster(case, dev):
    import importlib
    mod = importlib.import_module(case["package"])
    st = mod.GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in case["settings"].items()})
    leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in case["inputs"].items()}
    m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, radii, allmap, weight = mod.GaussianRasterizer(raster_settings=st)(
        means3D=leaves["means3D"], means2D=m2, shs=leaves.get("shs"), colors_precomp=leaves.get("colors_precomp"), opacities=leaves["opacities"],
        scales=leaves["scales"], rotations=leaves["rotations"], cov3D_precomp=None)
    up = case["upstream"]
    ((color * up["color"].to(dev)).sum() + (allmap * up["allmap"].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["means2D"] = m2.grad
    return dict(color=color, radii=radii, allmap=allmap, weight=weight), grads


def _run_tracer(case, dev):
    import diff_surfel_tracing as mod
    from envgs_amd import synth
    st = mod.SurfelTracingSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in case["settings"].items()})
    inp = case["inputs"]
    leaves = {k: inp[k].to(dev).clone().requires_grad_(True) for k in ("means3D", "shs", "colors_precomp", "others_precomp", "opacities", "scales", "rotations")
              if inp.get(k) is not None}
    o = inp["ray_o"].to(dev).clone().requires_grad_(True); d = inp["ray_d"].to(dev).clone().requires_grad_(True)
    g3 = torch.zeros_like(leaves["means3D"], requires_grad=True)
    v, f = synth.get_disks(leaves["means3D"].detach(), leaves["scales"].detach(), leaves["rotations"].detach())
    tracer = mod.SurfelTracer()
    tracer.build_acceleration_structure(v.detach().clone(), f.detach().clone(), rebuild=True)
    outs = tracer(o, d, v, means3D=leaves["means3D"], grads3D=g3, shs=leaves.get("shs"), colors_precomp=leaves.get("colors_precomp"),
                  others_precomp=leaves.get("others_precomp"), opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"],
                  cov3D_precomp=None, tracer_settings=st, start_from_first=case["start_from_first"])
    names = ("rgb", "dpt", "acc", "norm", "dist", "aux", "mid", "wet")
    res = dict(zip(names, outs))
    up = case["upstream"]
    sum((res[k] * up[k].to(dev)).sum() for k in ("rgb", "dpt", "acc", "norm", "aux")).backward()
    torch.cuda.synchronize()
    grads = {k: t.grad for k, t in leaves.items()}
    grads.update(ray_o=o.grad, ray_d=d.grad, grads3D=g3.grad)
    return res, grads


def _compare_file(path, test, allow_local=False):
    """Feed the stored inputs of a dump-script fixture to the HIP path and compare.  A fixture dumped from this repository's own packages
    (--allow-local) pins nothing: it is refused unless `allow_local` says the caller is testing the script itself."""
    data = torch.load(path, map_location="cpu", weights_only=False)
    assert data["meta"]["schema"] == 1
    assert allow_local or not data["meta"].get("local_packages"), "%s was dumped from this repository's own packages (--allow-local): it pins nothing" % path
    dev = torch.device("cuda:0")
    for case in data["raster"]:
        outs, grads = _run_raster(case, dev)
        tag = "%s.raster.%s" % (test, case["name"])
        assert np.array_equal(n(outs["radii"]), n(case["outputs"]["radii"])), case["name"]           # index work: bit-exact
        for k in ("color", "allmap", "weight"):
            _close(tag, k, n(outs[k]), n(case["outputs"][k]))
        for k, want in case["grads"].items():
            if want is None:
                assert grads.get(k) is None or float(grads[k].abs().max()) == 0.0, (case["name"], k)
                continue
            assert grads.get(k) is not None, (case["name"], k)
            _close(tag, "d" + k, n(grads[k]), n(want))
    for case in data["tracer"]:
        outs, grads = _run_tracer(case, dev)
        tag = "%s.tracer.%s" % (test, case["name"])
        for k in ("rgb", "dpt", "acc", "norm", "dist", "aux", "mid", "wet"):
            assert tuple(outs[k].shape) == tuple(case["outputs"][k].shape), (case["name"], k)      # the 8-tuple's layout (optix_utils.py:240-265)
            _close(tag, k, n(outs[k]), n(case["outputs"][k]))
        for k, want in case["grads"].items():
            if want is None:
                continue
            assert grads.get(k) is not None, (case["name"], k)
            _close(tag, "d" + k, n(grads[k]), n(want))
    return data["meta"]


def test_dump_script_and_loader_agree(tmp_path):
    out = str(tmp_path / "self_golden.pt")
    r = subprocess.run([sys.executable, SCRIPT, "--allow-local", "--out", out], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    meta = _compare_file(out, "dump_self_test", allow_local=True)
    assert meta["local_packages"] and len(meta["packages"]) == 4
    with pytest.raises(AssertionError, match="pins nothing"):           # as a committed fixture, the same file is refused
        _compare_file(out, "dump_self_test")
    # without --allow-local the script must refuse this repository's own same-named packages (it would pin nothing)
    r2 = subprocess.run([sys.executable, SCRIPT, "--out", out + ".x"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r2.returncode != 0 and not os.path.exists(out + ".x")
