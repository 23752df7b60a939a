"""Thinning of the DTU protocol at 2^18 points: surface samples of the torus of profiles/mesh_eval_timing.py, radius = their mean spacing.

  device  envgs_amd.mesh.thin_points(points, radius, seed): the grid, its read-back of the extrema, the rounds and their count read-backs;
  host    what a user could do before it existed: neighbour lists from torch.cdist over chunks of the points on the same GPU, then the literal
          DTU loop over them on the host, in the same key order.

Both in one process, alternating, warmed up; device events around each call; median of REPEATS, with the spread.  Also recorded: the rounds and the
undecided points after each (one read-back per round for this listing only), and the time at other cell sizes.
    python profiles/mesh_thin_timing.py [--repeats 5] [--out FILE]
Needs a GPU; there is no CPU path."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]          # profiles/numbers.py must not stand in for the standard library's
sys.path.insert(0, os.path.dirname(HERE))

import argparse  # noqa: E402
import importlib.util  # noqa: E402
import math  # noqa: E402
import statistics  # noqa: E402

import torch  # noqa: E402

N = 2 ** 18
CHUNK = 4096                                                      # rows per cdist call: a 4 GiB distance matrix


def _eval_timing():
    spec = importlib.util.spec_from_file_location("mesh_eval_timing", os.path.join(HERE, "mesh_eval_timing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def thin_keys(n, seed, dev):
    """key(i) = h(seed, i, 0xFFFFFFFE) of include/envgs_mesh.h, in int64 arithmetic masked to 32 bits."""
    m = 0xFFFFFFFF

    def mix(x):
        x = x ^ (x >> 16)
        x = (x * 0x7FEB352D) & m
        x = x ^ (x >> 15)
        x = (x * 0x846CA68B) & m
        return x ^ (x >> 16)

    i = torch.arange(n, dtype=torch.int64, device=dev)
    return mix(mix(mix(torch.full((1,), seed, dtype=torch.int64, device=dev)) ^ i) ^ 0xFFFFFFFE)


def exact_near(a, points, radius):
    """The header's d2 <= r2, operation for operation in fp32 (cdist takes its matrix-product form at this size and is off near the radius)."""
    dx, dy, dz = (a[:, None, e] - points[None, :, e] for e in range(3))
    return ((dx * dx) + (dy * dy)) + (dz * dz) <= torch.tensor(radius, dtype=torch.float32, device=a.device) ** 2


def host_thin(points, radius, seed, exact=False):
    """Neighbour pairs by chunked cdist on the device (exact: by the header's d2), the sequential loop on the host."""
    n = points.shape[0]
    rows, cols = [], []
    for s in range(0, n, 1024 if exact else CHUNK):
        near = (exact_near(points[s:s + 1024], points, radius) if exact else torch.cdist(points[s:s + CHUNK], points) <= radius).nonzero()
        rows.append(near[:, 0] + s)
        cols.append(near[:, 1])
    rows, cols = torch.cat(rows).cpu().numpy(), torch.cat(cols).cpu().numpy()      # sorted by row
    start = [0] * (n + 1)
    for r in rows.tolist():
        start[r + 1] += 1
    for i in range(n):
        start[i + 1] += start[i]
    cols = cols.tolist()
    alive, keep = [True] * n, [False] * n
    for i in torch.argsort(thin_keys(n, seed, points.device)).tolist():
        if alive[i]:
            keep[i] = True
            for j in cols[start[i]:start[i + 1]]:
                alive[j] = False
    return torch.tensor(keep, device=points.device)


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
        raise SystemExit("mesh_thin_timing.py needs a GPU")
    from envgs_amd import mesh
    et = _eval_timing()
    dev = torch.device("cuda", 0)
    m = et.torus_mesh(dev)
    area = 4 * math.pi ** 2 * et.RING * et.TUBE * et.VOXEL ** 2
    points = mesh.sample_surface(m, 1.03 * N / area, seed=0)[0][:N].contiguous()
    assert points.shape[0] == N, points.shape
    radius = math.sqrt(area / N)
    device_form = lambda cell=None: mesh.thin_points(points, radius, seed=0, cell_size=cell)
    host_form = lambda: host_thin(points, radius, 0)
    keep = device_form()
    host_keep = host_form()
    exact_keep = host_thin(points, radius, 0, exact=True)
    history = []
    _, rounds = mesh._thin(points, radius, 0, None, 1, history)
    grid = mesh.PointGrid(points, radius, _default_cell=radius * 1.002)
    lines = ["thinning, %d points: surface samples of a torus mesh (V %d, F %d), radius %.6g (their mean spacing), seed 0" % (N, m.vertices.shape[0], m.faces.shape[0], radius),
             "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "default cell_size %.6g -> grid %s = %d cells, shells %d" % (grid.cell_size, grid.dims, math.prod(grid.dims), mesh._thin_shells(radius, grid.cell_size, grid.dims)),
             "kept %d of %d; rows that differ from the host loop over cdist pairs: %d; over pairs by the exact fp32 d2: %d" % (
                 int(keep.sum()), N, int((keep != host_keep).sum()), int((keep != exact_keep).sum())),
             "rounds %d; undecided after each round: %s" % (rounds, " ".join(str(h) for h in history))]
    for _ in range(2):
        device_form()
    torch.cuda.synchronize()
    times = {"device": [], "host": []}
    for _ in range(args.repeats):
        times["host"] += timed(host_form, 1)
        times["device"] += timed(device_form, 1)
    for form in ("host", "device"):
        t = times[form]
        lines.append("%-6s  median %.3f ms  min %.3f  max %.3f  (%d repeats: %s)" % (form, statistics.median(t), min(t), max(t), len(t), " ".join("%.3f" % v for v in t)))
    lines.append("ratio host / device (medians): %.1f" % (statistics.median(times["host"]) / statistics.median(times["device"])))
    for factor in (0.5, 1.0, 2.0, 4.0):
        cell = factor * grid.cell_size
        try:
            assert torch.equal(device_form(cell), keep)
        except ValueError as e:
            lines.append("cell_size %.6g (%.2f x default): %s" % (cell, factor, str(e)[:60]))
            continue
        lines.append("cell_size %.6g (%.2f x default): median %.3f ms, same bytes" % (cell, factor, statistics.median(timed(lambda: device_form(cell), args.repeats))))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
