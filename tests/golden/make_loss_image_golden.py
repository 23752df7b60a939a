"""Generate tests/golden/loss_image_golden.npz by IMPORTING the reference's image loss exactly as make_loss_golden.py does (authoring container
only), on IMAGE-LIKE inputs: saturated white / black backgrounds, a smooth ramp + sinusoid, a hard edge, with x within 1e-2 .. 1e-3 of y.
There B2 = s1 + s2 + C2 of SSIM is dominated by C2 = 9e-4 and the float32 variances E[x^2] - mu^2 cancel, so the reference's own float32
evaluation is itself off by up to 1.7e-2 (loss_golden.npz holds white noise only, where it is exact to 5e-8).

Per case: the seeded inputs x, y (float32 values, stored as float32), the reference's float64 l1 / ssim / loss / grad, and the reference's own
float32 loss / grad (the same code on .float() tensors) -- the yardstick the fused kernel's float32 error is measured with.
Fixture = inputs + the reference's outputs; data only.

Size (the file stays below loss_golden.npz): a float64 gradient of noise does not compress, so it is stored as its distance from the float32
one, dgrad = float32(grad64 - grad32): grad64 = grad32 + dgrad in float64.  The distance is 1e-4 .. 1e-7 of the gradient, so its float32
rounding is below 1e-10 of it (asserted below; the CPU test compares at 1e-9, the GPU tests at 1e-4 and above).  The smooth ground truth is
an 8-bit image (k / 255), as a photograph is."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

C, H, W = 3, 40, 36
CASES = ("white_1e-2", "white_1e-3", "black_1e-2", "smooth_1e-2", "smooth_1e-3", "edge_1e-2", "same")


def smooth_image():
    """A ramp plus a sinusoid per channel, inside [0.1, 0.9]: what a rendered surface looks like."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ch = [0.5 + 0.3 * (xx / (W - 1) - 0.5) + 0.1 * torch.sin(yy / 6.0 + c) + 0.05 * torch.cos((xx + 2.0 * yy) / (9.0 + c)) for c in range(C)]
    return torch.round(torch.stack(ch) * 255.0) / 255.0                   # the ground truth is an 8-bit image


def inputs(tag, seed):
    g = torch.Generator().manual_seed(100 + seed)
    noise = torch.randn(C, H, W, generator=g, dtype=torch.float32)
    if tag.startswith("white"):
        y = torch.ones(C, H, W)
    elif tag.startswith("black"):
        y = torch.zeros(C, H, W)
    elif tag.startswith("edge"):
        y = torch.zeros(C, H, W); y[:, :, :W // 2] = 1.0                  # a hard vertical edge: left half 1, right half 0
    else:
        y = smooth_image()
    if tag == "same":
        return y.clone(), y                                                # x == y bit for bit
    amp = float(tag.split("_")[1])
    return (y + amp * noise).clamp(0, 1), y


def main():
    import importlib.util
    torch.set_num_threads(1)
    spec = importlib.util.spec_from_file_location("ref_ssim_utils", "/root/reference/easyvolcap/utils/ssim_utils.py")
    ssim_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ssim_utils)

    def evaluate(x, y):
        x = x[None].clone().requires_grad_(True); y = y[None]
        l1 = (x - y).abs().mean()                                          # loss_utils.l1 -> l1_reg
        s = ssim_utils.ssim(x, y, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03))
        loss = 0.8 * l1 + 0.2 * (1.0 - s)
        loss.backward()
        return l1.item(), s.item(), loss.item(), x.grad[0].numpy()

    out = {"cases": np.array(CASES)}
    for seed, tag in enumerate(CASES):
        x, y = inputs(tag, seed)
        assert x.dtype == torch.float32 and float(x.min()) >= 0 and float(x.max()) <= 1
        l1, s, loss, grad = evaluate(x.double(), y.double())
        _, _, loss32, grad32 = evaluate(x, y)
        assert grad.dtype == np.float64 and grad32.dtype == np.float32
        out["x_" + tag] = x.numpy(); out["y_" + tag] = y.numpy()
        out["l1_" + tag] = l1; out["ssim_" + tag] = s; out["loss_" + tag] = loss
        out["loss32_" + tag] = np.float32(loss32); out["grad32_" + tag] = grad32
        dgrad = (grad - grad32.astype(np.float64)).astype(np.float32)
        assert np.all(np.abs(grad32.astype(np.float64) + dgrad.astype(np.float64) - grad) <= 1e-10 * np.abs(grad) + 1e-15)   # (the CPU test: rtol 1e-9, atol 1e-14)
        out["dgrad_" + tag] = dgrad
        gm = np.abs(grad).mean()
        if tag == "same":                                                  # the optimum: loss and gradient are rounding residue of 0
            print("%-12s loss %.3e (fp32 %.3e)  max|grad| %.3e (fp32 %.3e)" % (tag, loss, loss32, np.abs(grad).max(), np.abs(grad32).max()))
            continue
        print("%-12s loss %.9e  fp32 rel err %.2e   grad fp32 err (floor mean|g|) %.2e" % (
            tag, loss, abs(loss32 - loss) / abs(loss), float((np.abs(grad32 - grad) / (np.abs(grad) + gm)).max())))
    path = os.path.join(HERE, "loss_image_golden.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
