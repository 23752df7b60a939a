"""Device time of the mesh-extraction kernels (csrc/mesh.hip) next to their byte models:  python profiles/mesh_timing.py [--sizes 256 512] [--reps 20]

Per volume size N^3 (bounds [-1,1]^3, colour on):
  integrate   one launch fusing 8 views of 800x800 (analytic sphere depth + a colour map): median of `reps` launches, HIP events
  torch       the same arithmetic written in torch on the device, one view at a time (the baseline the speed-up is quoted against)
  extract     envgs_mesh_count + the read-back + envgs_mesh_extract of the fused volume
  components  envgs_mesh_components of that mesh + the read-back of C;  select: envgs_mesh_select_count + read-back + envgs_mesh_select_emit of its largest
              component;  clean: mesh.clean with its defaults (components, the rule in torch, select)
  simplify    mesh.simplify of that mesh on cells of 2 voxels (envgs_mesh_simplify_cluster + the selection), with the grid given and with the grid
              sized from a read-back;  torch: the same clustering in torch ops (torch_simplify below)
The byte model of integrate: every voxel's tsdf, weight and rgb read once (20 B), and written back (20 B) in the 16 B granules where a voxel changed;
of extract: 8 B read + 1 B written (classify), 1 B read + 3 B written (count), 4 B read (emit) per voxel, plus 24 B per vertex and 12 B per face
written.  Fractions are of 6.3 TB/s (the achievable HBM rate, not the 8 TB/s peak).  Nothing is asserted; the table goes to DESIGN.md."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]          # profiles/numbers.py must not stand in for the standard library's
sys.path.insert(0, os.path.dirname(HERE))

import argparse  # noqa: E402

import torch  # noqa: E402

from envgs_amd import mesh, synth  # noqa: E402

ACHIEVABLE = 6.3e12
H = W = 800
FX = 1111.1


def sphere_depth(cam, radius, dev):
    """z-depth of a sphere at the origin through the pixel centres, 0 where the ray misses."""
    cc = cam.T.reshape(3).double()
    py, px = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    d = torch.stack([(px - W / 2) / FX, (py - H / 2) / FX, torch.ones_like(px)], dim=-1)
    dd, dc = (d * d).sum(-1), d @ cc
    disc = dc * dc - dd * (cc @ cc - radius ** 2)
    t = (dc - disc.clamp_min(0).sqrt()) / dd
    return torch.where(disc > 0, t, torch.zeros_like(t)).float().to(dev)


def torch_integrate_view(vol, grid, depth, rgb, K, R, T):
    """Steps 1-10 of include/envgs_mesh.h in torch ops, one view."""
    X, Y, Z = grid
    xc = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z + T[0]
    yc = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z + T[1]
    zc = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + T[2]
    u = torch.floor(K[0, 0] * (xc / zc) + K[0, 2])
    v = torch.floor(K[1, 1] * (yc / zc) + K[1, 2])
    ok = (zc > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    pix = torch.where(ok, v * W + u, torch.zeros_like(u)).long()
    d = depth.reshape(-1)[pix]
    sdf = d - zc
    ok = ok & (d > 0) & ~(sdf < -vol.trunc)
    val = torch.clamp_max(sdf / vol.trunc, 1.0)
    w1 = vol.weight + 1
    vol.tsdf.copy_(torch.where(ok, (vol.weight * vol.tsdf + val) / w1, vol.tsdf))
    for c in range(3):
        vol.rgb[c].copy_(torch.where(ok, (vol.weight * vol.rgb[c] + rgb[c].reshape(-1)[pix]) / w1, vol.rgb[c]))
    vol.weight.copy_(torch.where(ok, torch.clamp_max(w1, vol.w_max), vol.weight))


def torch_simplify(m, origin, cell, dims):
    """The clustering of include/envgs_mesh.h ("simplification") in torch ops: float means (index_add_, so neither bit-defined nor reproducible),
    the same face rules.  -> (vertices, faces, colors)"""
    v, dev = m.vertices, m.vertices.device
    o = torch.tensor(origin, dtype=torch.float32, device=dev)
    n = torch.tensor(dims, dtype=torch.int64, device=dev)
    ijk = torch.minimum(torch.floor((v - o) / cell).clamp_min(0).long(), n - 1)
    lin = ijk[:, 0] + n[0] * (ijk[:, 1] + n[1] * ijk[:, 2])
    _, cluster, members = torch.unique(lin, return_inverse=True, return_counts=True)
    C = members.shape[0]
    mean = lambda a: torch.zeros(C, 3, dtype=torch.float32, device=dev).index_add_(0, cluster, a) / members[:, None]
    cl_v, cl_c = mean(v), mean(m.colors)
    f = cluster[m.faces.long()]
    ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    first = f.argmin(dim=1, keepdim=True)
    rot = torch.gather(f, 1, (first + torch.arange(3, device=dev)[None, :]) % 3)          # the smallest cluster first
    key = (rot[:, 0] * C + rot[:, 1]) * C + rot[:, 2]
    _, klass = torch.unique(key, return_inverse=True)
    idx = torch.arange(f.shape[0], device=dev)
    lowest = torch.full((int(klass.max()) + 1,), f.shape[0], dtype=torch.int64, device=dev).scatter_reduce_(0, klass[ok], idx[ok], "amin")
    g = f[ok & (lowest[klass] == idx)]
    used = torch.zeros(C, dtype=torch.bool, device=dev)
    used[g.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    return cl_v[used], new[g].int(), cl_c[used]


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cams = [synth.orbit_camera(v, n_views=8, radius=4.0, H=H, W=W, fx=FX) for v in range(8)]
    depth = torch.stack([sphere_depth(c, 0.7, dev) for c in cams])
    py, px = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
    rgb = torch.stack([torch.stack([0.5 + 0.5 * torch.sin(0.01 * px + v), 0.5 + 0.5 * torch.cos(0.013 * py), (px + py) / (H + W)]) for v in range(8)]).contiguous()
    K, R, T = torch.stack([c.K for c in cams]), torch.stack([c.R for c in cams]), torch.stack([c.T.reshape(3) for c in cams])
    print("%-6s %-10s %10s %12s %10s   %s" % ("N", "kernel", "ms", "model MB", "of 6.3TB/s", "note"))
    for N in args.sizes:
        voxel = 2.0 / (N - 1)
        vol = mesh.TSDFVolume((-1, -1, -1), (-1 + voxel * (N - 1 - 1e-3),) * 3, voxel, device=dev)
        assert vol.dims == (N, N, N), vol.dims
        n = N ** 3
        vol.integrate(depth, K, R, T, rgb=rgb)
        changed = float((vol.weight > 0).float().mean())
        t_int = median_ms(lambda: vol.integrate(depth, K, R, T, rgb=rgb), args.reps)
        by = n * 20.0 * (1.0 + changed) + depth.numel() * 16.0
        print("%-6d %-10s %10.3f %12.1f %9.1f%%   8 views per launch; %.1f %% of the voxels change" % (N, "integrate", t_int, by / 1e6, 100 * by / (t_int * 1e-3) / ACHIEVABLE, 100 * changed))
        x = torch.arange(N, dtype=torch.float32, device=dev)
        grid = tuple(vol.origin[a] + g * vol.voxel_size for a, g in enumerate(torch.meshgrid(x, x, x, indexing="ij")[::-1]))

        def torch_all():
            for b in range(8):
                torch_integrate_view(vol, grid, depth[b], rgb[b], K[b], R[b], T[b])
        t_torch = median_ms(torch_all, args.torch_reps)
        print("%-6d %-10s %10.3f %12s %10s   same arithmetic in torch, 8 views one at a time: %.1fx the fused launch" % (N, "torch", t_torch, "-", "-", t_torch / t_int))
        del grid
        vol.reset()
        vol.integrate(depth, K, R, T, rgb=rgb)
        m = vol.extract()
        V, F = m.vertices.shape[0], m.faces.shape[0]
        t_ext = median_ms(lambda: vol.extract(), args.reps)
        by = n * 17.0 + V * 24.0 + F * 12.0
        print("%-6d %-10s %10.3f %12.1f %9.1f%%   V %d F %d; includes the (V, F) read-back and the output allocation" % (N, "extract", t_ext, by / 1e6, 100 * by / (t_ext * 1e-3) / ACHIEVABLE, V, F))
        # the clean-up of that mesh (csrc/mesh_clean.hip); the models count the streaming reads and writes of the passes, not the union-find's chases
        comp = mesh.components(m)
        t_cc = median_ms(lambda: mesh.components(m), args.reps)
        by = V * 36.0 + F * 48.0
        print("%-6d %-10s %10.3f %12.1f %9.1f%%   %d components, the largest %d faces; includes the read-back of C and the output allocation"
              % (N, "components", t_cc, by / 1e6, 100 * by / (t_cc * 1e-3) / ACHIEVABLE, comp.count, int(comp.faces.max()) if comp.count else 0))
        keep = comp.face_label == int(comp.faces.argmax()) if comp.count else torch.zeros(F, dtype=torch.bool, device=dev)
        s = mesh.select_faces(m, keep)
        t_sel = median_ms(lambda: mesh.select_faces(m, keep), args.reps)
        by = F * 26.0 + V * 4.0 + s.vertices.shape[0] * 48.0 + s.faces.shape[0] * 15.0
        print("%-6d %-10s %10.3f %12.1f %9.1f%%   the largest component: V' %d F' %d; includes the (V', F') read-back and the output allocation"
              % (N, "select", t_sel, by / 1e6, 100 * by / (t_sel * 1e-3) / ACHIEVABLE, s.vertices.shape[0], s.faces.shape[0]))
        t_clean = median_ms(lambda: mesh.clean(m), args.reps)
        print("%-6d %-10s %10.3f %12s %10s   components + the rule in torch (sort of C counts, gather of F labels) + select: %.2fx the extraction"
              % (N, "clean", t_clean, "-", "-", t_clean / t_ext))
        # the simplification of that mesh (csrc/mesh_simplify.hip) on cells of 2 voxels from the volume's origin.  Model: 41 B per vertex (assign and
        # accumulate read it twice, vertex_cluster written, colours read), 3 B per cell (cleared, scanned, rank written), 144 B per row of the sums
        # (cleared, read, representative written), 79 B per face (map, enter with one probe, keep), 4 B per slot, plus the selection's own model
        cell = 2 * vol.voxel_size
        dims = tuple((d - 1) // 2 + 1 for d in vol.dims)
        sm = mesh.simplify(m, cell, origin=vol.origin, dims=dims)
        Vs, Fs = sm.vertices.shape[0], sm.faces.shape[0]
        cells = dims[0] * dims[1] * dims[2]
        rows = min(V, cells)
        slots = 2
        while slots < 2 * F:
            slots *= 2
        t_simp = median_ms(lambda: mesh.simplify(m, cell, origin=vol.origin, dims=dims), args.reps)
        by = V * 41.0 + cells * 3.0 + rows * 144.0 + F * 79.0 + slots * 4.0 + F * 26.0 + rows * 4.0 + Vs * 48.0 + Fs * 15.0
        print("%-6d %-10s %10.3f %12.1f %9.1f%%   cells of 2 voxels, grid given: V' %d F' %d; includes the (V', F') read-back and the output allocation"
              % (N, "simplify", t_simp, by / 1e6, 100 * by / (t_simp * 1e-3) / ACHIEVABLE, Vs, Fs))
        t_auto = median_ms(lambda: mesh.simplify(m, cell), args.reps)
        print("%-6d %-10s %10.3f %12s %10s   the same with origin=None: the grid is sized from the read-back of the vertex extrema" % (N, "simplify*", t_auto, "-", "-"))
        ts = torch_simplify(m, vol.origin, cell, dims)
        t_ts = median_ms(lambda: torch_simplify(m, vol.origin, cell, dims), args.torch_reps)
        print("%-6d %-10s %10.3f %12s %10s   the same clustering in torch (unique on cell keys, index_add_ means, unique on face keys): V' %d F' %d, %.1fx simplify"
              % (N, "torch", t_ts, "-", "-", ts[0].shape[0], ts[1].shape[0], t_ts / t_simp))
        del vol, m, comp, s, sm, ts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
