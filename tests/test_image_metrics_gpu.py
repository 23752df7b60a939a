"""GPU: envgs_amd.metrics (csrc/metrics.hip) against the reference's results (tests/golden/image_metrics_golden.npz) and the float64 oracle
(tests/image_metrics_oracle.py) at the bands of tests/test_image_metrics.py; layouts, batch independence and reproducibility to the bit; the C-ABI
on guard-banded buffers; the device table; and evaluate_views over the EnvGS forward."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from envgs_amd import metrics
from tests import image_metrics_oracle as orc
from tests.test_image_metrics import MSE_RTOL, PSNR_TOL, SSIM_TOL, psnr_of
from tests.util import check_close, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "image_metrics_golden.npz"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _bits(a, b):
    """Byte for byte, NaNs included."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.int64) == b.view(torch.int64)).all())


def _pair(B, H, W, C, seed, dev, amp=0.05):
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(B, H, W, C, generator=g)
    x = (y + amp * torch.randn(B, H, W, C, generator=g)).clamp(0, 1)
    return x.to(dev), y.to(dev)


def _assert_bands(test, got, want, tag=""):
    """got, want: (n, 3) float64 rows mse, psnr, ssim.  The issue's bands, absolute for SSIM and PSNR, relative for the mse."""
    e_s = np.abs(got[:, 2] - want[:, 2])
    e_m = np.abs(got[:, 0] - want[:, 0]) / np.maximum(want[:, 0], 1e-300)
    e_m = np.where(want[:, 0] == 0, np.abs(got[:, 0]), e_m)             # x == y: the mse is exactly 0 on both sides
    e_p = np.abs(got[:, 1] - want[:, 1])
    print("%s%s: max |dssim| %.3e  max rel dmse %.3e  max |dpsnr| %.3e dB" % (test, tag, e_s.max(), e_m.max(), e_p.max()))
    assert e_s.max() <= SSIM_TOL and e_m.max() <= MSE_RTOL and e_p.max() <= PSNR_TOL, (test, tag, e_s.max(), e_m.max(), e_p.max())
    return float(e_s.max()), float(e_m.max()), float(e_p.max())


# ---- parity with the reference ---------------------------------------------------------------------------------------------------------------
def test_parity_with_the_golden_on_every_case(gold, dev):
    test = "image_metrics_golden"
    got, want = [], []
    for name in gold["cases"]:
        x, y = gold["x_" + name], gold["y_" + name]
        xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        if name == "rgba":
            xt, yt = xt[..., :3], yt[..., :3]                                # the evaluator's slice, read in place
        rows = metrics.image_metrics(xt, yt).cpu().numpy()
        m64 = gold["mse64_" + name]
        ref = np.stack([m64, psnr_of(m64), gold["ssim64_" + name]], 1)
        assert rows.shape == ref.shape and rows.dtype == np.float64
        _assert_bands(test, rows, ref, "[%s]" % name)
        got.append(rows); want.append(ref)
    got, want = np.concatenate(got), np.concatenate(want)
    same = got[list(gold["cases"]).index("same")]
    assert same[0] == 0.0 and same[1] == 100.0 and same[2] == 1.0            # x == y: numerator and denominator of the SSIM map are the same bits
    e_s, e_m, e_p = _assert_bands(test, got, want)
    record(test, "ssim abs", e_s, "max |ssim - ssim64| over %d images (bound %.0e)" % (len(got), SSIM_TOL))
    record(test, "psnr abs dB", e_p, "max |psnr - psnr64| (bound %.1e dB)" % PSNR_TOL)
    check_close(test, "ssim", got[:, 2], want[:, 2], tol=SSIM_TOL)
    nz = want[:, 0] > 0
    check_close(test, "mse", got[nz, 0], want[nz, 0], tol=MSE_RTOL, floor=1e-30)
    # the reference's own callables: a Python float, batch-wide on a batch
    xb, yb = torch.from_numpy(gold["x_batch3"]).to(dev), torch.from_numpy(gold["y_batch3"]).to(dev)
    assert isinstance(metrics.psnr(xb, yb), float) and isinstance(metrics.ssim(xb[0], yb[0]), float)
    assert abs(metrics.psnr(xb, yb) - float(psnr_of(gold["mse64_batch3"].mean()))) <= PSNR_TOL
    assert abs(metrics.ssim(xb, yb) - float(gold["ssim64_batch3"].mean())) <= SSIM_TOL
    assert abs(metrics.psnr(xb, yb) - float(gold["psnr32_batch_batch3"])) <= 2 * PSNR_TOL
    assert abs(metrics.ssim(xb[1], yb[1]) - float(gold["ssim64_batch3"][1])) <= SSIM_TOL
    assert metrics.psnr(yb, yb) == 100.0


# ---- shapes around the tile and the halo -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (11, 11), (16, 16), (17, 15), (26, 27), (33, 47)])
def test_shapes_around_the_tile_and_the_halo(H, W, C, B, dev):
    x, y = _pair(B, H, W, C, 1000 + 97 * H + 13 * W + 5 * C + B, dev)
    got = metrics.image_metrics(x, y).cpu().numpy()
    want = orc.batch_metrics(x.cpu().numpy(), y.cpu().numpy())
    e_s, e_m, _ = _assert_bands("image_metrics_shapes", got, want, "[%dx%dx%d B%d]" % (H, W, C, B))
    record("image_metrics_shapes", "ssim abs", e_s)
    record("image_metrics_shapes", "mse rel", e_m)


# ---- layouts: read in place, the same bytes as a contiguous copy ---------------------------------------------------------------------------------
def test_layouts_give_the_bytes_of_a_contiguous_copy(dev):
    B, H, W, C = 2, 21, 35, 3
    x, y = _pair(B, H, W, C, 7, dev)
    base = metrics.image_metrics(x, y)
    # "chw" views of the same data, and channel-first storage seen as "hwc"
    assert _bits(metrics.image_metrics(x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2), layout="chw"), base)
    xc, yc = x.permute(0, 3, 1, 2).contiguous(), y.permute(0, 3, 1, 2).contiguous()
    assert _bits(metrics.image_metrics(xc, yc, layout="chw"), base)
    assert _bits(metrics.image_metrics(xc.permute(0, 2, 3, 1), yc.permute(0, 2, 3, 1)), base)
    assert _bits(metrics.image_metrics(xc.permute(0, 2, 3, 1), y), base)                       # pred and gt with different strides
    # the evaluator's [..., :3] slice of a 4-channel image
    x4 = torch.cat([x, torch.rand(B, H, W, 1, device=dev)], -1); y4 = torch.cat([y, torch.rand(B, H, W, 1, device=dev)], -1)
    assert not x4[..., :3].is_contiguous()
    assert _bits(metrics.image_metrics(x4[..., :3], y4[..., :3]), base)
    assert _bits(metrics.image_metrics(x4[0, ..., :3], y4[0, ..., :3]), base[:1])             # a 3-D input is a batch of one
    # a transposed view: (B, W, H, C) storage
    xt, yt = x.transpose(1, 2).contiguous(), y.transpose(1, 2).contiguous()
    assert not xt.transpose(1, 2).is_contiguous()
    assert _bits(metrics.image_metrics(xt.transpose(1, 2), yt.transpose(1, 2)), base)
    # every second row and column of a larger image
    big_x = torch.zeros(B, 2 * H, 2 * W, C, device=dev); big_y = torch.ones(B, 2 * H, 2 * W, C, device=dev)
    big_x[:, ::2, ::2] = x; big_y[:, ::2, ::2] = y
    assert _bits(metrics.image_metrics(big_x[:, ::2, ::2], big_y[:, ::2, ::2]), base)
    # other float dtypes of pred and gt are converted first
    assert _bits(metrics.image_metrics(x.double(), y.double()), base)
    assert _bits(metrics.image_metrics(x.half(), y), metrics.image_metrics(x.half().float(), y))


def test_uint8_ground_truth_is_its_float_twin(gold, dev):
    y8 = torch.from_numpy(gold["y_u8"]).to(dev)
    x = torch.from_numpy(gold["x_u8"]).to(dev)
    every = torch.arange(256, dtype=torch.uint8, device=dev).reshape(1, 16, 16, 1).expand(1, 16, 16, 3)       # each of the 256 codes
    xe = torch.rand(1, 16, 16, 3, device=dev)
    for a, b in ((x, y8), (xe, every)):
        # the twin is divided on the HOST: torch's device kernel multiplies by the rounded reciprocal of a scalar divisor, which is not the
        # correctly rounded quotient the 8-bit rule asks for (k * fl(1 / 255) differs from fl(k / 255) in the last bit for 126 of the 256 codes)
        twin = (b.cpu().float() / 255).to(dev)
        assert np.array_equal(twin.cpu().numpy().astype(np.float64), orc.as_float(b.cpu().numpy()))
        assert _bits(metrics.image_metrics(a, b), metrics.image_metrics(a, twin))
    y4 = torch.cat([y8, y8[..., :1]], -1)
    assert _bits(metrics.image_metrics(x, y4[..., :3]), metrics.image_metrics(x, y8))                         # a strided uint8 view
    assert _bits(metrics.image_metrics(x.permute(2, 0, 1), y8.permute(2, 0, 1), layout="chw"), metrics.image_metrics(x, y8))


# ---- batch independence and reproducibility ----------------------------------------------------------------------------------------------------
def test_rows_are_independent_and_reproducible_to_the_bit(dev):
    x, y = _pair(3, 37, 50, 3, 11, dev)
    rows = metrics.image_metrics(x, y)
    assert _bits(metrics.image_metrics(x, y), rows)
    for b in range(3):
        assert _bits(metrics.image_metrics(x[b], y[b]), rows[b:b + 1])
        assert _bits(metrics.image_metrics(x[b:b + 1].clone(), y[b:b + 1].clone()), rows[b:b + 1])
    xn = x.clone(); xn[1, 20, 30, 2] = float("nan")
    bad = metrics.image_metrics(xn, y)
    assert _bits(bad[0], rows[0]) and _bits(bad[2], rows[2])
    assert bool(torch.isnan(bad[1]).all())
    yn = y.clone(); yn[1, 0, 0, 0] = float("nan")                                                              # in the ground truth, at the image's corner
    bad = metrics.image_metrics(x, yn)
    assert _bits(bad[0], rows[0]) and _bits(bad[2], rows[2]) and bool(torch.isnan(bad[1]).all())


# ---- edge cases and the table ------------------------------------------------------------------------------------------------------------------
def test_empty_batch(dev):
    out = metrics.image_metrics(torch.zeros(0, 8, 9, 3, device=dev), torch.zeros(0, 8, 9, 3, dtype=torch.uint8, device=dev))
    assert tuple(out.shape) == (0, 3) and out.dtype == torch.float64 and out.device.type == "cuda"
    t = metrics.ImageMetricTable()
    t.add(torch.zeros(0, 8, 9, 3, device=dev), torch.zeros(0, 8, 9, 3, device=dev))
    assert len(t) == 0 and t.rows() == [] and t.summary() == {}


CANARY = 0x7FF8A5A5A5A5A5A5          # a NaN no arithmetic here produces
GUARD = 2048


class _Guarded:
    """GUARD canary doubles, n doubles, GUARD canary doubles."""

    def __init__(self, n, dev):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int64, device=dev)

    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr() + 8 * GUARD)

    def body(self):
        host = self.raw.cpu()
        assert bool((host[:GUARD] == CANARY).all()) and bool((host[GUARD + self.n:] == CANARY).all()), "written outside its %d doubles" % self.n
        body = host[GUARD:GUARD + self.n]
        assert bool((body != CANARY).all()), "elements left unwritten"
        return body.view(torch.float64)


@pytest.mark.parametrize("B,C,H,W,u8", [(3, 3, 17, 15, False), (2, 1, 1, 1, True), (1, 3, 33, 47, True)])
def test_c_abi_on_guard_banded_buffers(B, C, H, W, u8, dev):
    from envgs_amd import _lib
    lib = _lib.load()
    x, y = _pair(B, H, W, C, 23, dev)
    if u8:
        y = (y * 255).round().to(torch.uint8)
    want = metrics.image_metrics(x, y)
    count = lib.envgs_image_metrics_partial_count(B, C, H, W)
    assert count == B * C * ((H + 15) // 16) * ((W + 15) // 16)
    partial, out = _Guarded(2 * count, dev), _Guarded(3 * B, dev)
    s = (ctypes.c_int64 * 4)(H * W * C, 1, W * C, C)
    st = _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert lib.envgs_image_metrics(B, C, H, W, _lib.ptr(x), s, _lib.ptr(y), s, int(u8), partial.ptr(), out.ptr(), st) == 0
    torch.cuda.synchronize()
    assert _bits(out.body().reshape(B, 3), want)
    rec = partial.body().reshape(B, -1, 2)
    assert bool(torch.isfinite(rec).all())
    n = C * H * W
    assert np.allclose(rec[:, :, 1].sum(1).numpy() / n, want[:, 0].cpu().numpy(), rtol=1e-12, atol=0)          # the records are the tiles' sums
    assert np.allclose(rec[:, :, 0].sum(1).numpy() / n, want[:, 2].cpu().numpy(), rtol=1e-12, atol=0)


def _sync_warnings(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return out, [w for w in rec if "called a synchronizing" in str(w.message)]        # (not the notice set_sync_debug_mode itself prints)


def test_table_across_a_doubling_equals_direct_calls_with_one_read_back(dev, tmp_path):
    x, y = _pair(7, 19, 23, 3, 31, dev)
    y8 = (y * 255).round().to(torch.uint8)
    direct = torch.cat([metrics.image_metrics(x[:1], y[:1]), metrics.image_metrics(x[1:4], y8[1:4]), metrics.image_metrics(x[4:], y[4:])])
    t = metrics.ImageMetricTable(capacity=2)

    def fill():
        t.add(x[0], y[0], camera=5, frame=0)
        t.add(x[1:4], y8[1:4], camera=[6, 7, 8], frame=1)           # 1 + 3 > 2: grows to 4
        t.add(x[4:], y[4:], camera=9, frame=[2, 3, 4])              # 4 + 3 > 4: grows to 8
    _, syncs = _sync_warnings(fill)
    assert syncs == [], [str(w.message) for w in syncs]
    assert len(t) == 7 and t.capacity == 8
    rows, syncs = _sync_warnings(t.rows)
    assert len(syncs) == 1, [str(w.message) for w in syncs]           # the one read-back
    (summary, _), syncs = _sync_warnings(lambda: (t.summary(), t.save_json(str(tmp_path / "m.json"))))
    assert syncs == []                                                # served from the rows already read
    assert _bits(torch.from_numpy(t.values()), direct)
    d = direct.cpu().numpy()
    assert [r["psnr"] for r in rows] == list(d[:, 1]) and [r["ssim"] for r in rows] == list(d[:, 2])
    assert [r["camera"] for r in rows] == [5, 6, 7, 8, 9, 9, 9] and [r["frame"] for r in rows] == [0, 1, 1, 1, 2, 3, 4]
    assert summary["psnr_mean"] == float(np.mean(d[:, 1])) and summary["ssim_std"] == float(np.std(d[:, 2]))
    out = torch.full((9, 3), -1.0, dtype=torch.float64, device=dev)                   # `out`: rows of a larger table
    got = metrics.image_metrics(x[1:4], y8[1:4], out=out[2:5])
    assert got.data_ptr() == out[2:5].data_ptr() and _bits(out[2:5], direct[1:4]) and bool((out[:2] == -1).all()) and bool((out[5:] == -1).all())
    with pytest.raises(ValueError, match="out must be"):
        metrics.image_metrics(x[1:4], y[1:4], out=out[:2])


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_views_scores_what_the_forward_renders(dev):
    import diff_surfel_rasterization_wet_ch05 as pkg
    import diff_surfel_tracing as tpkg
    from envgs_amd import envgs_step, synth
    H, W = 48, 64
    base = synth.base_gaussians(2000, seed=3)
    base["scales"] = base["scales"] * 5.0
    env = synth.env_gaussians(2000, seed=4, bound=12.0)
    base, env = ({k: v.to(dev) for k, v in d.items()} for d in (base, env))
    cams = [synth.orbit_camera(v, H=H, W=W, fx=1111.1 * W / 800.0, device=dev) for v in (1, 4)]
    bg, env_bg, deg = torch.zeros(3, device=dev), torch.tensor([0.1, 0.2, 0.3], device=dev), 3
    g = torch.Generator().manual_seed(5)
    photos = [torch.randint(0, 256, (H, W, 4), generator=g, dtype=torch.uint8).to(dev) for _ in cams]          # 8-bit RGBA ground truth
    was = envgs_step.FUSED["on"]
    envgs_step.FUSED["on"] = True
    try:
        tracer = tpkg.SurfelTracer()
        with torch.no_grad():
            renders = [envgs_step.envgs_forward(pkg, tpkg, tracer, cam, synth.get_rays(cam), base, env, bg, env_bg, deg)["rgb"].clone() for cam in cams]
        table = metrics.evaluate_views(cams, photos, base, env, deg, bg, env_bg, labels=[(7, 0), (8, 0)])
        same = metrics.evaluate_views(cams, renders, base, env, deg, bg, env_bg)
    finally:
        envgs_step.FUSED["on"] = was
    assert tuple(renders[0].shape) == (H, W, 3) and float(renders[0].std()) > 0.01                                 # a picture, not a constant
    direct = torch.cat([metrics.image_metrics(r, p[..., :3]) for r, p in zip(renders, photos)])
    assert _bits(torch.from_numpy(table.values()), direct)
    rows = table.rows()
    assert [(r["camera"], r["frame"]) for r in rows] == [(7, 0), (8, 0)] and all(3.0 < r["psnr"] < 20.0 for r in rows)
    for r in same.rows():
        assert r["psnr"] == 100.0 and abs(r["ssim"] - 1.0) <= 1e-6
    assert [(r["camera"], r["frame"]) for r in same.rows()] == [(0, 0), (1, 0)]
