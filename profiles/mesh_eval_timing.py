"""Nearest-point search of the mesh evaluation at 2^18 queries x 2^18 points, both surface samples (two seeds) of a torus extracted from a volume of
the `big` shape of tests/mesh_cases.py (81 x 65 x 51 voxels):

  grid   envgs_amd.mesh.PointGrid(points, max_distance, cell_size) + .nearest(queries): the build, its read-back of the extrema, and the search;
  cdist  what a user could do before it existed: torch.cdist over chunks of the queries with a running minimum, on the same GPU.

Both in one process, alternating, warmed up; device events around each call; median of REPEATS, with the spread.  Then the grid alone at other
cell sizes, to see where the default lies.
    python profiles/mesh_eval_timing.py [--repeats 5] [--out FILE]
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

DIMS, VOXEL, ORIGIN = (81, 65, 51), 0.05, (-1.17, 0.43, 2.01)
RING, TUBE = 20.0, 8.0                                            # voxels
N = 2 ** 18
MAX_DISTANCE = 0.05
CHUNK = 4096                                                      # queries per cdist call: a 4 GiB distance matrix


def torus_mesh(dev):
    from envgs_amd import mesh
    nx, ny, nz = DIMS
    z, y, x = torch.meshgrid(torch.arange(nz, dtype=torch.float64), torch.arange(ny, dtype=torch.float64), torch.arange(nx, dtype=torch.float64), indexing="ij")
    ring = torch.sqrt((x - 0.49 * nx) ** 2 + (y - 0.47 * ny) ** 2) - RING
    tsdf = (0.05 * (torch.sqrt(ring ** 2 + (z - 0.52 * nz) ** 2) - TUBE)).float().to(dev).contiguous()
    return mesh.TSDFVolume.from_tensors(tsdf, torch.ones_like(tsdf), None, ORIGIN, VOXEL).extract()


def cdist_nearest(queries, points, max_distance):
    d2 = torch.empty(queries.shape[0], dtype=torch.float32, device=queries.device)
    index = torch.empty(queries.shape[0], dtype=torch.int64, device=queries.device)
    for s in range(0, queries.shape[0], CHUNK):
        d, i = torch.cdist(queries[s:s + CHUNK], points).min(dim=1)
        d2[s:s + CHUNK], index[s:s + CHUNK] = d * d, i
    miss = d2 > max_distance * max_distance
    return torch.where(miss, float("inf"), d2), torch.where(miss, -1, index)


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_eval_timing.py needs a GPU")
    from envgs_amd import mesh
    dev = torch.device("cuda", 0)
    m = torus_mesh(dev)
    area = 4 * math.pi ** 2 * RING * TUBE * VOXEL ** 2
    density = 1.03 * N / area
    queries, points = [mesh.sample_surface(m, density, seed=s)[0][:N].contiguous() for s in (0, 1)]
    assert queries.shape[0] == N and points.shape[0] == N, (queries.shape, points.shape)
    grid = mesh.PointGrid(points, MAX_DISTANCE)
    grid_form = lambda cell=None: mesh.PointGrid(points, MAX_DISTANCE, cell).nearest(queries)
    cdist_form = lambda: cdist_nearest(queries, points, MAX_DISTANCE)
    gd, gi = grid_form()
    cd, ci = cdist_form()
    found = gi >= 0
    lines = ["nearest point, %d queries x %d points: surface samples of a torus mesh (V %d, F %d) at density %.0f, max_distance %g" % (N, N, m.vertices.shape[0], m.faces.shape[0], density, MAX_DISTANCE),
             "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "default cell_size %.6g -> grid %s = %d cells" % (grid.cell_size, grid.dims, math.prod(grid.dims)),
             "found %d of %d; index equal to cdist's argmin on %d; max |sqrt(dist2) - cdist| %.3g" % (
                 int(found.sum()), N, int((gi.long() == ci).sum()), float((gd[found].sqrt() - cd[found].sqrt()).abs().max()))]
    for _ in range(2):
        grid_form(); cdist_form()
    torch.cuda.synchronize()
    times = {"grid": [], "cdist": []}
    for _ in range(args.repeats):
        times["cdist"] += timed(cdist_form, 1)
        times["grid"] += timed(grid_form, 1)
    for form in ("cdist", "grid"):
        t = times[form]
        lines.append("%-5s  median %.3f ms  min %.3f  max %.3f  (%d repeats: %s)" % (form, statistics.median(t), min(t), max(t), len(t), " ".join("%.3f" % v for v in t)))
    lines.append("ratio cdist / grid (medians): %.1f" % (statistics.median(times["cdist"]) / statistics.median(times["grid"])))
    for factor in (0.25, 0.5, 1.0, 2.0, 4.0):
        cell = factor * grid.cell_size
        try:
            g = mesh.PointGrid(points, MAX_DISTANCE, cell)
        except ValueError as e:
            lines.append("cell_size %.6g (%.2f x default): %s" % (cell, factor, str(e)[:60]))
            continue
        d, i = g.nearest(queries)
        assert torch.equal(d, gd) and torch.equal(i, gi)
        build = timed(lambda: mesh.PointGrid(points, MAX_DISTANCE, cell), args.repeats)
        search = timed(lambda: g.nearest(queries), args.repeats)
        lines.append("cell_size %.6g (%.2f x default), grid %s: build median %.3f ms, search median %.3f ms, same bytes" % (
            cell, factor, g.dims, statistics.median(build), statistics.median(search)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
