"""Depth fusion at the sizes of a DTU / Tanks-and-Temples run: VIEWS views of 1200 x 1600 and of 544 x 960 with S = 4 sources each, the analytic
depth of a sphere seen from an arc of cameras one degree apart (generated on the device from a formula: nothing is read from disk).

  fused   mesh.fuse_depth_points(depth, cameras, rgb=rgb, sources=...): csrc/mesh_fuse.hip, one host sync (the read-back of N)
  torch   the same rule written as torch expressions on the same GPU, view by view with the S sources batched -- the (S, H W, 3) temporaries,
          grid_sample and one nonzero() per view of the route a user had before: the torch form of tests/mesh_fuse_oracle.py in float32

Both in one process, alternating, warmed up; device events around each whole call (host work and read-backs are inside the window: this is time per
call, not kernel time); median of REPEATS with the spread.  Also reported: the achieved bytes per second against the model of the issue --
(1 + S) 4 H W read plus 5 H W written per view -- which is a whole-call rate, not a kernel's share of peak; the host syncs of each form; and that the
two forms keep the same pixels up to the pairs on a threshold.
    python profiles/mesh_fuse_timing.py [--views 100] [--repeats 20] [--out FILE]
Needs a GPU; there is no CPU path."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]          # profiles/numbers.py must not stand in for the standard library's
sys.path.insert(0, os.path.dirname(HERE))

import argparse  # noqa: E402
import math  # noqa: E402
import statistics  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

S = 4


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def rig(V, H, W, dev):
    """V cameras on an arc, one degree apart, looking at the unit sphere from 3.2 away -> (cameras, K, R, T float64, depth (V,H,W) on the device)."""
    from envgs_amd import synth
    f = 0.95 * min(H, W) * 3.2 / 2.2
    K = np.array([[f, 0.0, W / 2 - 0.29], [0.0, 1.03 * f, H / 2 + 0.17], [0.0, 0.0, 1.0]])
    cams, Ks, Rs, Ts = [], [], [], []
    for v in range(V):
        az, el = math.radians(v - 0.5 * (V - 1) + 0.3 * (v % 2)), math.radians(12.0 + 4.0 * (v % 3))
        c = 3.2 * (1.0 + 0.002 * v) * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(fwd, (0.0, 0.0, 1.0))
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd]).astype(np.float32).astype(np.float64)
        T = (-R @ c).astype(np.float32).astype(np.float64)
        cams.append(synth.make_camera(K, R, T, H, W, 0.5, 10.0))
        Ks.append(K.astype(np.float32).astype(np.float64)); Rs.append(R); Ts.append(T)
    K, R, T = np.stack(Ks), np.stack(Rs), np.stack(Ts)
    depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    py, px = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64) + 0.5, torch.arange(W, device=dev, dtype=torch.float64) + 0.5, indexing="ij")
    for v in range(V):
        d = torch.stack([(px - K[v, 0, 2]) / K[v, 0, 0], (py - K[v, 1, 2]) / K[v, 1, 1], torch.ones_like(px)], -1)
        cc = torch.tensor(T[v], device=dev)
        dd, dc = (d * d).sum(-1), d @ cc
        disc = dc * dc - dd * (cc @ cc - 1.0)
        depth[v] = torch.where(disc > 0, (dc - disc.clamp_min(0).sqrt()) / dd, torch.zeros_like(dd)).float()
    return cams, K, R, T, depth


def torch_form(depth, rgb, fwd, back, view, sources, th):
    """The twin's rule as torch expressions, float32, one view at a time with its sources batched.  fwd, back: (V,S,12), view: (V,12) on the device."""
    V, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=depth.device, dtype=torch.float32) + 0.5,
                            torch.arange(W, device=depth.device, dtype=torch.float32) + 0.5, indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1).reshape(-1, 3)                      # (HW,3)
    n_min = math.ceil(th["geo_sum_thresh"] * sources.shape[1])
    pts, cols = [], []
    for r in range(V):
        d = depth[r].reshape(1, -1, 1)
        A, b, B, bb = fwd[r, :, :9].reshape(-1, 3, 3), fwd[r, :, None, 9:], back[r, :, :9].reshape(-1, 3, 3), back[r, :, None, 9:]
        p = d * (pix @ A.mT) + b                                                             # (S,HW,3)
        uv = p[..., :2] / p[..., 2:]
        grid = torch.stack([uv[..., 0] / W * 2 - 1, uv[..., 1] / H * 2 - 1], -1).reshape(-1, H, W, 2)
        sampled = torch.nn.functional.grid_sample(depth[sources[r]][:, None], grid, padding_mode="border", align_corners=False).reshape(-1, H * W, 1)
        q = sampled * (torch.cat([uv, torch.ones_like(uv[..., :1])], -1) @ B.mT) + bb
        z = q[..., 2]
        dist = torch.sqrt((q[..., 0] / z - pix[:, 0]) ** 2 + (q[..., 1] / z - pix[:, 1]) ** 2)
        ok = (dist < th["geo_abs_thresh"]) & ((z - d[..., 0]).abs() / d[..., 0] < th["geo_rel_thresh"]) & (sampled[..., 0] > 0) & (d[..., 0] > 0)
        count = ok.sum(0)
        avg = (torch.where(ok, z, torch.zeros_like(z)).sum(0) + d[0, :, 0]) / (count + 1)
        keep = ((count >= n_min) & (d[0, :, 0] > th["pho_abs_thresh"])).nonzero()[:, 0]       # a host sync per view
        pts.append(view[r, 9:] + avg[keep, None] * (pix[keep] @ view[r, :9].reshape(3, 3).mT))
        cols.append(rgb[r].reshape(3, -1)[:, keep].mT)
    return torch.cat(pts), torch.cat(cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_fuse_timing.py needs a GPU")
    from envgs_amd import mesh
    dev = torch.device("cuda", 0)
    th = dict(geo_abs_thresh=1.0, geo_rel_thresh=0.01, geo_sum_thresh=0.75, pho_abs_thresh=0.0)
    V = args.views
    lines = ["depth fusion, %d views, S = %d, thresholds %s" % (V, S, th), "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]
    for H, W in ((1200, 1600), (544, 960)):
        cams, K, R, T, depth = rig(V, H, W, dev)
        rgb = torch.rand(V, 3, H, W, device=dev)
        sources = mesh.nearest_views(cams, S)
        fwd, back = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in mesh.fuse_pair_maps(K, R, T, sources.numpy()))
        view = torch.from_numpy(mesh.fuse_view_maps(K, R, T).astype(np.float32)).to(dev)
        src_dev = sources.to(dev)
        fused = lambda: mesh.fuse_depth_points(depth, cams, rgb=rgb, sources=sources, **th)
        twin = lambda: torch_form(depth, rgb, fwd, back, view, src_dev, th)
        for _ in range(2):
            a, b = fused(), twin()
        torch.cuda.synchronize()
        times = {"fused": [], "torch": []}
        for _ in range(args.repeats):
            times["fused"].append(timed(fused)[0])
            times["torch"].append(timed(twin)[0])
        n_f, n_t = a[0].shape[0], b[0].shape[0]
        model = V * ((1 + S) * 4 * H * W + 5 * H * W)
        lines.append("%d x %d: %d pixels, kept %d (fused) / %d (torch form), model traffic %.3f GB" % (H, W, V * H * W, n_f, n_t, model / 1e9))
        for form in ("fused", "torch"):
            t = times[form]
            med = statistics.median(t)
            lines.append("  %-5s  median %9.3f ms  min %9.3f  max %9.3f  (%d repeats)   %.1f GB/s of the model traffic   host syncs per call: %d"
                         % (form, med, min(t), max(t), len(t), model / (med * 1e-3) / 1e9, 1 if form == "fused" else V))
        lines.append("  ratio torch / fused (medians): %.1f" % (statistics.median(times["torch"]) / statistics.median(times["fused"])))
        del depth, rgb, a, b
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
