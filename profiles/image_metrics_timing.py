"""Image evaluation at the sizes of a test set: B = 1, 8 and 100 images of 800 x 800 x 3 and of 1200 x 1600 x 3, a float32 prediction against a
uint8 ground truth (random values generated on the device: nothing is read from disk).

  fused        metrics.image_metrics(pred, gt): csrc/metrics.hip, two launches for the whole batch, no host sync; the device time of the call
  fused+read   the same followed by the ONE read-back of the (B, 3) table
  torch/view   the same formulas as torch expressions on the same GPU, one view at a time with an .item() per metric, as an evaluator that scores
               each view when it is rendered does: five grouped conv2d with the 11 x 11 window (zero padding 5), the elementwise SSIM map and
               its mean; mse and the clipped log for PSNR.  The ground truth is converted with .float() / 255 inside the window.
  torch/batch  those expressions on the whole batch at once, one read-back (what they cost without the per-view syncs; B x the temporaries)

All in one process, alternating, warmed up; device events around each whole call (host work and read-backs are inside the window: this is time per
call, not kernel time); median of REPEATS with the spread.  Also reported: bytes per second against the least traffic, 4 + 1 bytes per element
read once -- a whole-call rate, not a kernel's share of peak -- and the largest difference between the fused and the torch results.
    python profiles/image_metrics_timing.py [--repeats 10] [--out FILE]
Needs a GPU; there is no CPU path."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]          # profiles/numbers.py must not stand in for the standard library's
sys.path.insert(0, os.path.dirname(HERE))

import argparse  # noqa: E402
import math  # noqa: E402
import statistics  # noqa: E402

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def window2d(C, dev):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).expand(C, 1, 11, 11).contiguous().to(dev)


def torch_maps(x, y, win):
    """x, y (B, H, W, C) float32 -> per-image mse (B,) and ssim (B,), as torch expressions."""
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
    x, y = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    C = x.shape[1]
    blur = lambda t: F.conv2d(t, win, padding=5, groups=C)
    mu1, mu2 = blur(x), blur(y)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    v1, v2, v12 = blur(x * x) - m11, blur(y * y) - m22, blur(x * y) - m12
    smap = ((2 * m12 + 0.01 ** 2) * (2 * v12 + 0.03 ** 2)) / ((m11 + m22 + 0.01 ** 2) * (v1 + v2 + 0.03 ** 2))
    return mse, smap.mean(dim=(1, 2, 3))


def torch_per_view(pred, gt, win):
    rows = []
    for b in range(pred.shape[0]):
        mse, s = torch_maps(pred[b:b + 1], gt[b:b + 1].float() / 255, win)
        psnr = ((1 / mse.clip(1e-10)).log() * 10 / math.log(10)).item()             # the evaluator's two read-backs per view
        rows.append((psnr, s.item()))
    return rows


def torch_batched(pred, gt, win):
    mse, s = torch_maps(pred, gt.float() / 255, win)
    return torch.stack([(1 / mse.clip(1e-10)).log() * 10 / math.log(10), s], 1).cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_metrics_timing.py needs a GPU")
    from envgs_amd import metrics
    dev = torch.device("cuda", 0)
    lines = ["image metrics: float32 prediction, uint8 ground truth, C = 3", "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]
    win = window2d(3, dev)
    for H, W in ((800, 800), (1200, 1600)):
        g = torch.Generator(device=dev).manual_seed(H)
        gt_all = torch.randint(0, 256, (100, H, W, 3), generator=g, dtype=torch.uint8, device=dev)
        pred_all = (gt_all.float() / 255 + 0.02 * torch.randn(100, H, W, 3, generator=g, device=dev)).clamp(0, 1)
        for B in (1, 8, 100):
            pred, gt = pred_all[:B], gt_all[:B]
            forms = {"fused": lambda: metrics.image_metrics(pred, gt), "fused+read": lambda: metrics.image_metrics(pred, gt).cpu(),
                     "torch/view": lambda: torch_per_view(pred, gt, win), "torch/batch": lambda: torch_batched(pred, gt, win)}
            for _ in range(2):
                outs = {k: f() for k, f in forms.items()}
            torch.cuda.synchronize()
            times = {k: [] for k in forms}
            for _ in range(args.repeats):
                for k, f in forms.items():
                    times[k].append(timed(f)[0])
            fused = outs["fused+read"]
            twin = torch.tensor(outs["torch/view"], dtype=torch.float64)
            d_psnr, d_ssim = (fused[:, 1] - twin[:, 0]).abs().max().item(), (fused[:, 2] - twin[:, 1]).abs().max().item()
            model = B * H * W * 3 * 5
            lines.append("%d x %d x 3, B = %d: %.1f Mpix, least traffic %.3f GB; fused vs torch/view: max |dpsnr| %.2e dB, max |dssim| %.2e"
                         % (H, W, B, B * H * W / 1e6, model / 1e9, d_psnr, d_ssim))
            for k in forms:
                t = times[k]
                med = statistics.median(t)
                syncs = {"fused": 0, "fused+read": 1, "torch/view": 2 * B, "torch/batch": 1}[k]
                lines.append("  %-11s  median %9.3f ms  min %9.3f  max %9.3f  (%d repeats)   %.1f Mpix/s   %.1f GB/s of the least traffic   host syncs per call: %d"
                             % (k, med, min(t), max(t), len(t), B * H * W / 1e6 / (med * 1e-3), model / (med * 1e-3) / 1e9, syncs))
            lines.append("  ratio torch/view : fused+read (medians): %.1f    torch/batch : fused+read: %.1f"
                         % (statistics.median(times["torch/view"]) / statistics.median(times["fused+read"]),
                            statistics.median(times["torch/batch"]) / statistics.median(times["fused+read"])))
        del gt_all, pred_all, pred, gt, outs
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
