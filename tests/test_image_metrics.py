"""CPU: the image metrics' float64 oracle against the reference's own results (tests/golden/image_metrics_golden.npz, made by
tests/golden/make_image_metrics_golden.py from easyvolcap/utils/metric_utils.py), the bands of the GPU tests measured on the reference itself,
the argument checks of envgs_amd.metrics, the table's summary and file, and the C-ABI's validation -- none of which needs a GPU."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from envgs_amd import metrics
from tests import image_metrics_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_TOL = 1e-4            # |ssim - ssim64|: the project's elementwise parity bar (README, "Parity")
MSE_RTOL = 1e-4            # |mse - mse64| <= 1e-4 mse64
PSNR_TOL = 4.4e-4          # dB: 10 / ln 10 x 1e-4 = 4.34e-4


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "image_metrics_golden.npz"))


def images_of(gold, name):
    """-> x, y as (B, H, W, C) arrays, the evaluator's [..., :3] slice taken for the 4-channel case."""
    x, y = gold["x_" + name], gold["y_" + name]
    if name == "rgba":
        x, y = x[..., :3], y[..., :3]
    return (x[None], y[None]) if x.ndim == 3 else (x, y)


def psnr_of(mse):
    return 10.0 * np.log10(1.0 / np.maximum(mse, 1e-10))


def test_golden_holds_the_cases_the_tests_need(gold):
    names = list(gold["cases"])
    for bg in ("white", "black", "smooth", "edge", "noise"):
        for a in ("1e-1", "1e-2", "1e-3"):
            assert "%s_%s" % (bg, a) in names
    for name in ("same", "tiny", "rgba", "batch3", "u8"):
        assert name in names
    assert gold["x_tiny"].shape == (7, 5, 3) and gold["x_rgba"].shape[-1] == 4 and gold["x_batch3"].shape[0] == 3
    assert gold["y_u8"].dtype == np.uint8 and gold["x_u8"].dtype == np.float32
    assert np.array_equal(gold["x_same"], gold["y_same"]) and gold["psnr32_same"][0] == pytest.approx(100.0, abs=1e-4)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "image_metrics_golden.npz")) < 256 * 1024


def test_window_of_the_oracle_and_of_the_kernel_is_the_reference_window(gold):
    win = gold["win"]
    assert win.dtype == np.float32 and win.shape == (11,)
    assert np.array_equal(orc.window(), win)
    src = open(os.path.join(ROOT, "envgs_amd", "csrc", "metrics.hip")).read()
    body = src[src.index("kMetricWin[11]"):]
    taps = [float.fromhex(h) for h in re.findall(r"(0x1\.[0-9a-f]+p-\d+)f", body[:body.index("};")])]
    assert np.array_equal(np.array(taps, np.float32), win) and np.array_equal(np.array(taps, np.float64), win.astype(np.float64))


def test_oracle_reproduces_the_reference_in_float64(gold):
    for name in gold["cases"]:
        x, y = images_of(gold, name)
        got = orc.batch_metrics(x, y)
        assert np.abs(got[:, 2] - gold["ssim64_" + name]).max() <= 1e-9, name
        assert np.allclose(got[:, 0], gold["mse64_" + name], rtol=1e-9, atol=0), name
        assert np.abs(got[:, 1] - psnr_of(gold["mse64_" + name])).max() <= 1e-9, name


def test_uint8_rule_of_the_oracle_is_the_float_twin(gold):
    y8 = gold["y_u8"]
    twin = (torch.from_numpy(y8).float() / 255).numpy()
    assert np.array_equal(orc.as_float(y8), twin.astype(np.float64))
    assert orc.image_metrics(gold["x_u8"], y8) == orc.image_metrics(gold["x_u8"], twin)


def test_reference_float32_results_lie_inside_the_bands(gold):
    """The bands the GPU kernel is held to, applied to the reference's own float32 evaluation: it passes them with room to spare, so they ask nothing
    of the kernel that float32 arithmetic of this form cannot give."""
    worst_s = worst_p = 0.0
    for name in gold["cases"]:
        worst_s = max(worst_s, float(np.abs(gold["ssim32_" + name] - gold["ssim64_" + name]).max()))
        worst_p = max(worst_p, float(np.abs(gold["psnr32_" + name] - psnr_of(gold["mse64_" + name])).max()))
    assert worst_s <= SSIM_TOL / 2 and worst_p <= PSNR_TOL / 10, (worst_s, worst_p)


def test_batch_semantics_of_the_reference(gold):
    """On a batch the reference's psnr comes from the batch-wide mse and its ssim is the batch-wide mean: what metrics.psnr / metrics.ssim return."""
    m = gold["mse64_batch3"]
    assert abs(float(gold["psnr32_batch_batch3"]) - float(psnr_of(m.mean()))) <= PSNR_TOL
    assert abs(float(gold["ssim32_batch_batch3"]) - float(gold["ssim64_batch3"].mean())) <= SSIM_TOL


def test_argument_checks():
    x = torch.zeros(2, 8, 9, 3)
    with pytest.raises(ValueError, match="layout"):
        metrics.image_metrics(x, x, layout="nhwc")
    with pytest.raises(ValueError, match="same shape"):
        metrics.image_metrics(x, torch.zeros(2, 8, 9, 4))
    with pytest.raises(ValueError, match="3-D"):
        metrics.image_metrics(torch.zeros(8, 9), torch.zeros(8, 9))
    for bad in (torch.int32, torch.int8, torch.bool):
        with pytest.raises(ValueError, match="float tensor or uint8"):
            metrics.image_metrics(x, torch.zeros(2, 8, 9, 3, dtype=bad))
    with pytest.raises(ValueError, match="pred must be a float"):
        metrics.image_metrics(x.to(torch.uint8), x)
    with pytest.raises(RuntimeError, match="no CPU path"):              # CPU tensors: refuse, never fall back
        metrics.image_metrics(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.image_metrics(x, x.to(torch.uint8), layout="chw")
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.psnr(x[0], x[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.ImageMetricTable().add(x, x)
    with pytest.raises(ValueError, match="labels"):
        metrics.ImageMetricTable().add(x, x, camera=[1, 2, 3])
    with pytest.raises(ValueError, match="capacity"):
        metrics.ImageMetricTable(capacity=0)
    with pytest.raises(ValueError, match="cameras for"):
        metrics.evaluate_views([1, 2], [x[0]], {}, {}, 0, None, None)
    assert not hasattr(metrics, "lpips")                                # a stated gap, not a stub


def test_summary_and_json_of_a_hand_made_table(tmp_path):
    psnr = np.array([31.25, 28.5, 40.125, 100.0, 22.0625])
    ssim = np.array([0.91, 0.875, 0.99, 1.0, 0.5])
    vals = np.stack([10.0 ** (-psnr / 10.0), psnr, ssim], 1)
    t = metrics.ImageMetricTable.from_host(vals, cameras=[3, 3, 4, 4, 5], frames=[0, 1, 0, 1, 0])
    assert len(t) == 5
    s = t.summary()
    assert sorted(s) == ["psnr_mean", "psnr_std", "ssim_mean", "ssim_std"]
    assert s["psnr_mean"] == float(np.mean(psnr)) and s["psnr_std"] == float(np.std(psnr))               # the population form
    assert s["ssim_mean"] == float(np.mean(ssim)) and s["ssim_std"] == float(np.std(ssim))
    assert s["psnr_std"] != pytest.approx(float(np.std(psnr, ddof=1)))
    rows = t.rows()
    assert rows[2] == dict(psnr=40.125, ssim=0.99, camera=4, frame=0) and [r["frame"] for r in rows] == [0, 1, 0, 1, 0]
    path = str(tmp_path / "metrics.json")
    t.save_json(path)
    doc = json.load(open(path))
    assert sorted(doc) == ["metrics", "summary"] and doc["summary"] == s and doc["metrics"] == rows
    assert all(sorted(r) == ["camera", "frame", "psnr", "ssim"] for r in doc["metrics"])                 # no lpips key, no stand-in
    empty = metrics.ImageMetricTable()
    assert empty.rows() == [] and empty.summary() == {} and len(empty) == 0


def test_abi_validation_without_a_gpu():
    from envgs_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "envgs_metrics.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"^#define\s+ENVGS_METRICS_(\w+)\s+(\d+)", hdr, re.M)}
    assert codes == dict(GT_F32=metrics.GT_F32, GT_U8=metrics.GT_U8, MSE=metrics.MSE, PSNR=metrics.PSNR, SSIM=metrics.SSIM, COLS=metrics.COLS)
    count = lib.envgs_image_metrics_partial_count
    assert count(1, 3, 16, 16) == 3 and count(2, 3, 17, 15) == 12 and count(1, 1, 1, 1) == 1 and count(100, 3, 1200, 1600) == 100 * 3 * 75 * 100
    assert count(0, 3, 16, 16) == 0 and count(1, 0, 16, 16) == 0 and count(1, 3, 0, 16) == 0 and count(1, 3, 16, -1) == 0
    s = (ctypes.c_int64 * 4)(1, 1, 1, 1)
    one = ctypes.c_void_p(64)                    # a non-NULL pointer that is never dereferenced: every call below returns before a launch
    f = lib.envgs_image_metrics
    assert f(0, 3, 8, 8, None, None, None, None, 0, None, None, None) == 0                       # B = 0: success, nothing to do
    for B, C, H, W in ((1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8), (0, 3, 0, 8)):
        assert f(B, C, H, W, one, s, one, s, 0, one, one, None) == -1
    for dtype in (2, -1, 255):
        assert f(1, 3, 8, 8, one, s, one, s, dtype, one, one, None) == -1
        assert f(0, 3, 8, 8, one, s, one, s, dtype, one, one, None) == -1
    args = [one, s, one, s, 0, one, one]
    for i in (0, 1, 2, 3, 5, 6):
        a = list(args); a[i] = None
        assert f(1, 3, 8, 8, *a, None) == -1
    assert f(1 << 20, 3, 1 << 14, 1 << 14, one, s, one, s, 0, one, one, None) == -1               # more tiles than a grid has workgroups
    assert math.isclose(float(orc.window().astype(np.float64).sum()), 1.0, abs_tol=1e-7)
