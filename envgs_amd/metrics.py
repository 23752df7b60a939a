"""Image evaluation on the device: per-image MSE, PSNR and SSIM of a batch (include/envgs_metrics.h, csrc/metrics.hip), a device-side table
that costs one read-back per test set, and a driver that renders cameras through the EnvGS forward and scores them.

Semantics: the reference's evaluator metrics, easyvolcap/utils/metric_utils.py -- psnr (:21-25: 10 log10(1 / clip(mse, 1e-10)), mse in
loss_utils.py:311-312) and ssim (:28-64: 11-tap sigma-1.5 float32 Gaussian, zero padding of 5, per channel, C1 = 0.01^2, C2 = 0.03^2, mean over
channels and pixels) -- per image.  runners/evaluators/volumetric_video_evaluator.py computes ['PSNR', 'SSIM', 'LPIPS'] per view and writes
metrics.json; ImageMetricTable.save_json writes the same layout.

LPIPS is NOT here: it is a VGG network with learned weights, and neither the weights nor a way to fetch them is part of this project.
A metrics.json from this module has no 'lpips' key; nothing stands in for it."""
import ctypes
import json

import numpy as np
import torch

from . import _lib

GT_F32, GT_U8 = 0, 1                                   # ENVGS_METRICS_GT_*
MSE, PSNR, SSIM = 0, 1, 2                              # ENVGS_METRICS_* columns
COLS = 3


def _as_batch(t, name):
    if not torch.is_tensor(t):
        raise TypeError("%s must be a tensor, got %s" % (name, type(t).__name__))
    if t.dim() == 3:
        return t.unsqueeze(0)
    if t.dim() != 4:
        raise ValueError("%s must be one image (3-D) or a batch of images (4-D), got shape %s" % (name, tuple(t.shape)))
    return t


def _strides(t, layout):
    """Element strides in the kernel's order (batch, channel, row, column)."""
    s = t.stride()
    return (ctypes.c_int64 * 4)(*((s[0], s[3], s[1], s[2]) if layout == "hwc" else (s[0], s[1], s[2], s[3])))


def image_metrics(pred, gt, layout="hwc", out=None):
    """pred, gt: (H, W, C) / (B, H, W, C) images with layout="hwc", (C, H, W) / (B, C, H, W) with layout="chw"; a 3-D input is a batch of one.
    pred: any float dtype (other than float32: converted first).  gt: a float dtype, or uint8, read as k / 255 in float32 (img.float() / 255) --
    a test set of 8-bit photographs stays 8-bit on the device.  Any strides: a [..., :3] slice of a 4-channel image, a permuted or transposed
    view are read in place, without a copy.
    -> (B, 3) float64 device tensor, columns mse, psnr, ssim (MSE, PSNR, SSIM), or `out` (a (B, 3) float64 contiguous device tensor, e.g. rows of
    a larger table) filled and returned.  Two launches, no host synchronisation; the result of image b depends on image b alone and is the same
    bytes on every call.  GPU tensors only: there is no CPU path."""
    if layout not in ("hwc", "chw"):
        raise ValueError("layout must be 'hwc' or 'chw', got %r" % (layout,))
    pred, gt = _as_batch(pred, "pred"), _as_batch(gt, "gt")
    if pred.shape != gt.shape:
        raise ValueError("pred and gt must have the same shape, got %s and %s" % (tuple(pred.shape), tuple(gt.shape)))
    if not pred.dtype.is_floating_point:
        raise ValueError("pred must be a float tensor, got %s" % pred.dtype)
    if gt.dtype != torch.uint8 and not gt.dtype.is_floating_point:
        raise ValueError("gt must be a float tensor or uint8, got %s" % gt.dtype)
    B = pred.shape[0]
    (H, W, C) = pred.shape[1:] if layout == "hwc" else (pred.shape[2], pred.shape[3], pred.shape[1])
    if B > 0 and min(H, W, C) < 1:
        raise ValueError("empty images: shape %s" % (tuple(pred.shape),))
    if pred.device.type != "cuda" or gt.device != pred.device:
        raise RuntimeError("image_metrics needs GPU tensors on one device; there is no CPU path (pred on %s, gt on %s)" % (pred.device, gt.device))
    dev = pred.device
    if out is None:
        out = torch.empty(B, COLS, dtype=torch.float64, device=dev)
    elif (not torch.is_tensor(out) or out.dtype != torch.float64 or out.device != dev or tuple(out.shape) != (B, COLS) or not out.is_contiguous()):
        raise ValueError("out must be a contiguous (%d, %d) float64 tensor on %s" % (B, COLS, dev))
    if B == 0:
        return out
    lib = _lib.load()
    pred = pred.detach().to(torch.float32)
    gt = gt.detach() if gt.dtype == torch.uint8 else gt.detach().to(torch.float32)
    count = lib.envgs_image_metrics_partial_count(B, C, H, W)
    partial = torch.empty(count, 2, dtype=torch.float64, device=dev)
    stream = _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.envgs_image_metrics(B, C, H, W, _lib.ptr(pred), _strides(pred, layout), _lib.ptr(gt), _strides(gt, layout),
                                       GT_U8 if gt.dtype == torch.uint8 else GT_F32, _lib.ptr(partial), _lib.ptr(out), stream), "envgs_image_metrics")
    return out


def psnr(x, y):
    """Metrics.PSNR of the reference: (H, W, C) or (B, H, W, C) images -> a Python float (one read-back).  On a batch the mse is batch-wide, as
    loss_utils.mse's mean is."""
    m = image_metrics(x, y)[:, MSE].mean().item()
    return float("nan") if m != m else 10.0 * float(np.log10(1.0 / max(m, 1e-10)))


def ssim(x, y):
    """Metrics.SSIM of the reference: (H, W, C) or (B, H, W, C) images -> a Python float (one read-back), the mean over the whole batch."""
    return image_metrics(x, y)[:, SSIM].mean().item()


class ImageMetricTable:
    """Metric rows of a test set, kept on the device: add() scores views straight into the next rows, rows() makes the ONE read-back."""

    def __init__(self, capacity=256):
        if int(capacity) < 1:
            raise ValueError("capacity must be at least 1, got %r" % (capacity,))
        self.capacity = int(capacity)
        self._buf = None                 # (capacity, 3) float64 on the device of the first add
        self._n = 0
        self._meta = []                  # (camera, frame) per row
        self._host = None                # (n, 3) float64 on the host, valid until the next add

    def __len__(self):
        return self._n

    @classmethod
    def from_host(cls, values, cameras=None, frames=None):
        """A table of rows already on the host: values (n, 3) columns mse, psnr, ssim.  Needs no GPU."""
        values = np.asarray(values, np.float64).reshape(-1, COLS)
        n = values.shape[0]
        t = cls(capacity=max(n, 1))
        t._n, t._host = n, values.copy()
        t._meta = list(zip(cameras if cameras is not None else [None] * n, frames if frames is not None else [None] * n))
        if len(t._meta) != n:
            raise ValueError("cameras and frames must have one entry per row")
        return t

    def _reserve(self, n, dev):
        if self._buf is None:
            if self._n:
                raise RuntimeError("a table made by from_host holds host rows only; it cannot take device rows")
            while self.capacity < n:
                self.capacity *= 2
            self._buf = torch.empty(self.capacity, COLS, dtype=torch.float64, device=dev)
        elif self._buf.device != dev:
            raise RuntimeError("the table lives on %s, the images on %s" % (self._buf.device, dev))
        if n > self.capacity:
            while self.capacity < n:
                self.capacity *= 2
            grown = torch.empty(self.capacity, COLS, dtype=torch.float64, device=dev)
            grown[:self._n].copy_(self._buf[:self._n])               # on the stream, no synchronisation
            self._buf = grown

    def add(self, pred, gt, camera=None, frame=None, layout="hwc"):
        """Scores one view, or a batch, into the next rows; camera / frame: one label, or one per image of the batch.  No host synchronisation.
        -> the new rows, a (B, 3) view of the device table (valid until the table grows)."""
        B = _as_batch(pred, "pred").shape[0]
        labels = []
        for name, v in (("camera", camera), ("frame", frame)):
            v = list(v) if isinstance(v, (list, tuple)) else [v] * B
            if len(v) != B:
                raise ValueError("%s has %d labels for %d images" % (name, len(v), B))
            labels.append(v)
        dev = pred.device
        if dev.type != "cuda":
            raise RuntimeError("ImageMetricTable.add needs GPU tensors; there is no CPU path")
        self._reserve(self._n + B, dev)
        rows = image_metrics(pred, gt, layout=layout, out=self._buf[self._n:self._n + B])
        self._n += B
        self._meta += list(zip(*labels))
        self._host = None
        return rows

    def values(self):
        """(n, 3) float64 on the host, columns mse, psnr, ssim: the one read-back (kept until the next add)."""
        if self._host is None:
            self._host = np.zeros((0, COLS)) if self._buf is None else self._buf[:self._n].cpu().numpy()
        return self._host

    def rows(self):
        v = self.values()
        return [dict(psnr=float(v[i, PSNR]), ssim=float(v[i, SSIM]), camera=self._meta[i][0], frame=self._meta[i][1]) for i in range(self._n)]

    def summary(self):
        """psnr_mean, psnr_std, ssim_mean, ssim_std; the population standard deviation (np.std), as the reference's summarize()."""
        v = self.values()
        if not len(v):
            return {}
        return dict(psnr_mean=float(np.mean(v[:, PSNR])), psnr_std=float(np.std(v[:, PSNR])),
                    ssim_mean=float(np.mean(v[:, SSIM])), ssim_std=float(np.std(v[:, SSIM])))

    def save_json(self, path):
        """{"summary": ..., "metrics": [...]}: the layout of the reference's metrics.json (without its lpips and time entries)."""
        doc = dict(summary=self.summary(), metrics=self.rows())
        with open(path, "w") as f:
            json.dump(doc, f, indent=4)
        return doc


def evaluate_views(cameras, images, base, env, sh_degree, bg, env_bg, labels=None, pkg=None, tpkg=None, tracer=None):
    """Renders every camera through envgs_step.envgs_forward under torch.no_grad() and scores the blended rgb, unclipped (the reference's evaluator
    does not clip either), against images[i]: (H, W, C >= 3) float or uint8 on the device, the first three channels in place.  -> ImageMetricTable.

    cameras: synth.make_camera records (their rays are synth.get_rays); base / env: the surfel dicts envgs_forward takes;
    labels: per camera (camera, frame), default (i, 0).  The raster package (diff_surfel_rasterization_wet_ch05), the tracer package and ONE
    SurfelTracer are created once for all views unless passed in.  The caller form (envgs_step.FUSED and its other switches) is left as it is set.

    Host synchronisation: scoring adds none -- the table is read once, by the caller's rows() / summary() / save_json().  What remains per view is the
    forward's own: the rasterizer waits for its instance count (an event behind the projection kernel, envgs_amd/raster.py), and a sh_degree
    passed as a device tensor is read once per tensor object (cached).  The tracer's forward reads nothing back."""
    from . import envgs_step, synth
    if len(cameras) != len(images):
        raise ValueError("%d cameras for %d images" % (len(cameras), len(images)))
    if pkg is None:
        import diff_surfel_rasterization_wet_ch05 as pkg
    if tpkg is None:
        import diff_surfel_tracing as tpkg
    if tracer is None:
        tracer = tpkg.SurfelTracer()
    table = ImageMetricTable()
    with torch.no_grad():
        for i, (cam, img) in enumerate(zip(cameras, images)):
            out = envgs_step.envgs_forward(pkg, tpkg, tracer, cam, synth.get_rays(cam), base, env, bg, env_bg, sh_degree)
            camera, frame = (i, 0) if labels is None else labels[i]
            table.add(out["rgb"], img[..., :3], camera=camera, frame=frame)
    return table
