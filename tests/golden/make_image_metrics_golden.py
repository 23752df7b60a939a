"""Generate tests/golden/image_metrics_golden.npz by IMPORTING the reference's evaluator metrics, easyvolcap/utils/metric_utils.py (psnr, ssim), the
way the other makers import theirs (authoring container only; what that container lacks and the two functions never touch is mocked).

Per case: the inputs (float32, or uint8 for the 8-bit ground truth), and per image of the case
  psnr32, ssim32   the reference's own results on the float32 inputs                (what a user of the reference reports)
  ssim64           the reference's ssim on .double() inputs                         (the float64 yardstick for SSIM)
  mse64            mean((x - y)^2) in float64 by this file's own arithmetic         (the reference's mse casts to float32: it cannot be the yardstick)
and for the batch case the reference's batch-wide psnr32 / ssim32 as well (psnr from the batch-wide mse, ssim the batch-wide mean).
"win" is the reference's float32 window, metric_utils.gaussian(11, 1.5).  Fixture = inputs + the reference's outputs; data only.

Cases (images 27 x 22 x 3: one full 16 x 16 tile and a ragged one in each direction, every pixel within reach of the zero padding or not):
  <bg>_<a>   bg in white, black, smooth (an 8-bit ramp plus sinusoid), edge (a hard edge), noise (uniform); prediction clamp(y + a randn, 0, 1), a = 1e-1, 1e-2, 1e-3
  same       x == y bit for bit: 100 dB
  tiny       7 x 5: the window hangs over zeros on every side of every pixel
  rgba       a 4-channel image scored through its [..., :3] slice (stored with its fourth channel)
  batch3     three images in one call
  u8         a uint8 ground truth; the reference is given its float twin, y.float() / 255"""
import json
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
for name in ("pdbr", "pdbr.utils", "ruamel", "ruamel.yaml", "plyfile", "skimage", "skimage.metrics", "lpips", "torchvision", "torchvision.models",
             "torchvision.models.vgg"):
    sys.modules.setdefault(name, MagicMock())
sys.modules.setdefault("ujson", json)

H, W, C = 27, 22, 3
BACKGROUNDS = ("white", "black", "smooth", "edge", "noise")
AMPS = ("1e-1", "1e-2", "1e-3")


def smooth_image(h=H, w=W, c=C):
    """A ramp plus a sinusoid per channel, inside [0.1, 0.9], as an 8-bit image (k / 255): what a photograph of a rendered surface looks like."""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    ch = [0.5 + 0.3 * (xx / max(w - 1, 1) - 0.5) + 0.1 * torch.sin(yy / 6.0 + k) + 0.05 * torch.cos((xx + 2.0 * yy) / (9.0 + k)) for k in range(c)]
    return torch.round(torch.stack(ch, -1) * 255.0) / 255.0


def background(bg, g, h=H, w=W, c=C):
    if bg == "white":
        return torch.ones(h, w, c)
    if bg == "black":
        return torch.zeros(h, w, c)
    if bg == "edge":
        y = torch.zeros(h, w, c); y[:, :w // 2] = 1.0                     # left half 1, right half 0
        return y
    if bg == "noise":
        return torch.rand(h, w, c, generator=g, dtype=torch.float32)
    return smooth_image(h, w, c)


def noisy(y, amp, g):
    return (y + amp * torch.randn(y.shape, generator=g, dtype=torch.float32)).clamp(0, 1)


def cases():
    """-> list of (name, x, y): x float32, y float32 or uint8; (H, W, C), or (B, H, W, C) for the batch."""
    out = []
    seed = 0
    for bg in BACKGROUNDS:
        for amp in AMPS:
            g = torch.Generator().manual_seed(500 + seed); seed += 1
            y = background(bg, g)
            out.append(("%s_%s" % (bg, amp), noisy(y, float(amp), g), y))
    y = smooth_image()
    out.append(("same", y.clone(), y))
    g = torch.Generator().manual_seed(600)
    y = background("noise", g, 7, 5)
    out.append(("tiny", noisy(y, 0.05, g), y))
    g = torch.Generator().manual_seed(601)
    y = smooth_image(H, W, 4)
    out.append(("rgba", noisy(y, 0.03, g), y))
    g = torch.Generator().manual_seed(602)
    ys = torch.stack([background("noise", g), smooth_image(), background("edge", g)])
    out.append(("batch3", torch.stack([noisy(ys[0], 0.1, g), noisy(ys[1], 0.01, g), noisy(ys[2], 0.03, g)]), ys))
    g = torch.Generator().manual_seed(603)
    y8 = torch.randint(0, 256, (H, W, C), generator=g, dtype=torch.uint8)
    out.append(("u8", noisy(y8.float() / 255, 0.02, g), y8))
    return out


def main():
    torch.set_num_threads(1)
    from easyvolcap.utils import metric_utils as mu
    res = {"win": mu.gaussian(11, 1.5).numpy()}
    assert res["win"].dtype == np.float32
    names = []
    for name, x, y in cases():
        names.append(name)
        assert x.dtype == torch.float32 and float(x.min()) >= 0 and float(x.max()) <= 1
        res["x_" + name] = x.numpy(); res["y_" + name] = y.numpy()
        yf = y.float() / 255 if y.dtype == torch.uint8 else y
        xs, ys = (x, yf) if name != "rgba" else (x[..., :3], yf[..., :3])           # the evaluator's slice
        if xs.dim() == 3:
            xs, ys = xs[None], ys[None]
        res["psnr32_" + name] = np.array([mu.psnr(a, b) for a, b in zip(xs, ys)], np.float64)
        res["ssim32_" + name] = np.array([mu.ssim(a, b) for a, b in zip(xs, ys)], np.float64)
        res["ssim64_" + name] = np.array([mu.ssim(a.double(), b.double()) for a, b in zip(xs, ys)], np.float64)
        res["mse64_" + name] = np.array([float(((a.double() - b.double()) ** 2).mean()) for a, b in zip(xs, ys)], np.float64)
        if xs.shape[0] > 1:
            res["psnr32_batch_" + name] = np.float64(mu.psnr(xs, ys)); res["ssim32_batch_" + name] = np.float64(mu.ssim(xs, ys))
        m = res["mse64_" + name]
        p64 = 10 * np.log10(1 / np.maximum(m, 1e-10))
        print("%-12s psnr %s  ssim %s   fp32 reference: |dpsnr| %.1e dB  |dssim| %.1e" % (
            name, np.round(p64, 4), np.round(res["ssim64_" + name], 6), np.abs(res["psnr32_" + name] - p64).max(),
            np.abs(res["ssim32_" + name] - res["ssim64_" + name]).max()))
    res["cases"] = np.array(names)
    path = os.path.join(HERE, "image_metrics_golden.npz")
    np.savez_compressed(path, **res)
    print(os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
