"""The mesh rasteriser at the sizes of a DTU run: the extract() of an analytic sphere's TSDF at a voxel size that gives on the order of 10^6 faces
(generated on the device from a formula: nothing is read from disk), through 8 and through 100 views of 1200 x 1600.

  full     mesh.render_mesh(mesh, cameras) with its default outputs (depth, face, normal, color): csrc/mesh_raster.hip, no host sync
  raster   the same call with no outputs: the key image is cleared and filled, and the resolve pass only reads the keys -- the raster pass's
           share by subtraction (full - raster = what resolving and writing the maps costs)
  seen     mesh.visible_faces(): the cull's flag alone

Device events around each whole call, warmed up; median of REPEATS with the spread, and the median per view.  Also reported, from the counters the
raster pass adds to on request (a run of its own, not timed): the fragments covered, the 64-bit atomics issued (a plain load of the key rules the
rest out) and the pixels that end up covered.  Then the same mesh plus ONE triangle that covers every image, which is the large-face path: one
workgroup walks 1.9 M pixels per view.  No bound is asserted: the numbers are written down as measured.
    python profiles/mesh_raster_timing.py [--voxel 0.008] [--repeats 10] [--out FILE]
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

H, W = 1200, 1600


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def sphere_mesh(voxel, dev):
    """extract() of the unit sphere's TSDF on [-1.1, 1.1]^3, coloured by position."""
    from envgs_amd import mesh
    n = int(math.ceil(2.2 / voxel)) + 1
    ax = -1.1 + voxel * torch.arange(n, device=dev, dtype=torch.float32)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    trunc = 5.0 * voxel
    tsdf = ((torch.sqrt(x * x + y * y + z * z) - 1.0) / trunc).clamp(-1.0, 1.0).contiguous()
    rgb = torch.stack([0.5 + 0.45 * x, 0.5 + 0.45 * y, 0.5 + 0.45 * z]).contiguous()
    vol = mesh.TSDFVolume.from_tensors(tsdf, torch.ones_like(tsdf), rgb, (-1.1, -1.1, -1.1), voxel, trunc)
    return vol.extract()


def rig(V):
    """V cameras on a ring around the sphere, 3.2 away, the sphere filling most of the shorter side."""
    from envgs_amd import synth
    f = 0.9 * min(H, W) * 3.2 / 2.2
    K = np.array([[f, 0.0, W / 2 - 0.29], [0.0, 1.03 * f, H / 2 + 0.17], [0.0, 0.0, 1.0]])
    cams = []
    for v in range(V):
        az, el = 2.0 * math.pi * v / V, math.radians(-20.0 + 20.0 * (v % 3))
        c = 3.2 * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(fwd, (0.0, 0.0, 1.0))
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        cams.append(synth.make_camera(K, R, -R @ c, H, W, 0.5, 10.0))
    return cams


def with_whole_image_triangle(m, cams):
    """The mesh plus ONE huge triangle behind the sphere as camera 0 sees it: it covers all of camera 0's image and large parts of its neighbours';
    a camera it crosses or lies behind does not draw it (there is no clipping)."""
    from envgs_amd import mesh
    cam = cams[0]
    R, T = cam.R.double().numpy(), cam.T.double().numpy().reshape(3)
    corners_cam = np.array([[-60.0, -40.0, 6.0], [60.0, -40.0, 6.0], [0.0, 80.0, 6.0]])
    corners = (corners_cam - T) @ R                                                      # R^T (x_cam - T)
    dev = m.vertices.device
    V = m.vertices.shape[0]
    vertices = torch.cat([m.vertices, torch.tensor(corners, dtype=torch.float32, device=dev)])
    colors = torch.cat([m.colors, torch.full((3, 3), 0.5, device=dev)])
    faces = torch.cat([m.faces, torch.tensor([[V, V + 1, V + 2]], dtype=torch.int32, device=dev)])
    return mesh.Mesh(vertices=vertices, faces=faces, colors=colors)


def measure(lines, label, m, cams, repeats):
    from envgs_amd import mesh
    dev = m.vertices.device
    forms = {"full": lambda: mesh.render_mesh(m, cams), "raster": lambda: mesh._raster(m, cams, None, 0.0, (), "timing"),
             "seen": lambda: mesh.visible_faces(m, cams)}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            times[k].append(timed(fn)[0])
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    r = mesh._raster(m, cams, None, 0.0, ("face", "seen"), "timing", stats=stats)
    covered, issued = stats.tolist()
    pixels = int((r.face >= 0).sum())
    lines.append("%s: %d faces, %d views of %d x %d (%d launch groups)" % (label, m.faces.shape[0], len(cams), H, W, (len(cams) + 7) // 8))
    med = {}
    for k in forms:
        t = times[k]
        med[k] = statistics.median(t)
        lines.append("  %-6s  median %9.3f ms  min %9.3f  max %9.3f  (%d repeats)   %.3f ms per view" % (k, med[k], min(t), max(t), len(t), med[k] / len(cams)))
    lines.append("  raster share of the full call (medians): %.0f %%; resolve and map writes by subtraction: %.3f ms (%.3f per view)"
                 % (100.0 * med["raster"] / med["full"], med["full"] - med["raster"], (med["full"] - med["raster"]) / len(cams)))
    lines.append("  fragments covered %d, atomics issued %d (%.1f %%), pixels covered %d of %d: %.2f fragments and %.2f atomics per covered pixel; faces seen %d"
                 % (covered, issued, 100.0 * issued / max(covered, 1), pixels, len(cams) * H * W, covered / max(pixels, 1), issued / max(pixels, 1),
                    int(r.seen.sum())))
    del r
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.008)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_raster_timing.py needs a GPU")
    from envgs_amd import _lib
    dev = torch.device("cuda", 0)
    m = sphere_mesh(args.voxel, dev)
    lines = ["mesh rasteriser, unit sphere at voxel %g: %d vertices, %d faces; SMALL_MAX = %d" % (args.voxel, m.vertices.shape[0], m.faces.shape[0],
                                                                                               _lib.load().envgs_mesh_raster_small_max()),
             "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]
    print("\n".join(lines), flush=True)
    for V in (8, 100):
        cams = rig(V)
        for label, mm in (("sphere", m), ("sphere + one whole-image triangle", with_whole_image_triangle(m, cams))):
            done = len(lines)
            measure(lines, label, mm, cams, args.repeats)
            print("\n".join(lines[done:]), flush=True)
    text = "\n".join(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
