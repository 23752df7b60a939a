"""One registration iteration at 1 M source x 1 M target points next to PointGrid.nearest alone at the same size: surface samples of the torus of
profiles/mesh_eval_timing.py, two independent draws, the source displaced by 0.5 degrees and 0.002 (well inside max_distance).

  nearest    grid.nearest(moved): the parent's kernel over the rows transform_points wrote -- the yardstick: what an iteration cannot avoid
  iteration  mesh.register_sums(source, grid, T): the transformation, the same walk, the 18 sums in double, the final workgroup and the read-back
             of 18 doubles (the host sync of an iteration is part of the figure)

Both in one process, alternating, warmed up; device events around each call; median of REPEATS, with the spread.  Also recorded: that the matches of
the two are the same bytes, a whole register() call, and the iteration at other cell sizes (same bytes asserted).
    python profiles/mesh_register_timing.py [--repeats 9] [--out FILE]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

N = 1_000_000


def _eval_timing():
    spec = importlib.util.spec_from_file_location("mesh_eval_timing", os.path.join(HERE, "mesh_eval_timing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def displacement(degrees, shift):
    t = math.radians(degrees)
    T = np.eye(4)
    T[:3, :3] = [[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = shift
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_register_timing.py needs a GPU")
    from envgs_amd import mesh
    et = _eval_timing()
    dev = torch.device("cuda", 0)
    m = et.torus_mesh(dev)
    area = 4 * math.pi ** 2 * et.RING * et.TUBE * et.VOXEL ** 2
    target = mesh.sample_surface(m, 1.03 * N / area, seed=0)[0][:N].contiguous()
    source = mesh.sample_surface(m, 1.03 * N / area, seed=1)[0][:N].contiguous()
    assert target.shape[0] == N and source.shape[0] == N, (target.shape, source.shape)
    spacing = math.sqrt(area / N)
    max_distance = 8.0 * spacing
    T = displacement(0.5, (0.002, -0.001, 0.0015))
    grid = mesh.PointGrid(target, max_distance)
    moved = mesh.transform_points(source, T)
    nearest_form = lambda g=grid: g.nearest(moved)
    iteration_form = lambda g=grid: mesh.register_sums(source, g, T)
    sums, rows, dist2, index = mesh.register_sums(source, grid, T, return_rows=True)
    near = nearest_form()
    same = torch.equal(rows, moved) and torch.equal(near[0], dist2) and torch.equal(near[1], index)
    lines = ["registration, %d source x %d target points: two draws of surface samples of a torus mesh (V %d, F %d), mean spacing %.6g, max_distance %.6g"
             % (N, N, m.vertices.shape[0], m.faces.shape[0], spacing, max_distance),
             "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "default cell_size %.6g -> grid %s = %d cells" % (grid.cell_size, grid.dims, math.prod(grid.dims)),
             "matched %d of %d, inlier rmse %.6g; rows, dist2 and index of the iteration equal transform_points + nearest: %s"
             % (int(sums[0]), N, math.sqrt(sums[1] / max(sums[0], 1.0)), same)]
    for _ in range(3):
        nearest_form()
        iteration_form()
    torch.cuda.synchronize()
    times = {"nearest": [], "iteration": []}
    for _ in range(args.repeats):
        times["nearest"] += timed(nearest_form, 1)
        times["iteration"] += timed(iteration_form, 1)
    for form in ("nearest", "iteration"):
        t = times[form]
        lines.append("%-9s  median %.3f ms  min %.3f  max %.3f  (%d repeats: %s)" % (form, statistics.median(t), min(t), max(t), len(t), " ".join("%.3f" % v for v in t)))
    lines.append("ratio iteration / nearest (medians): %.2f" % (statistics.median(times["iteration"]) / statistics.median(times["nearest"])))
    whole = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        result = mesh.register(source, grid, max_distance, init=T)
        e1.record()
        torch.cuda.synchronize()
        whole.append(e0.elapsed_time(e1))
    lines.append("register() from the displacement, grid passed in: %d evaluations, converged %s, fitness %.4f, inlier rmse %.6g; median %.3f ms of 3 (%s)"
                 % (len(result.history), result.converged, result.fitness, result.inlier_rmse, statistics.median(whole), " ".join("%.3f" % v for v in whole)))
    for factor in (0.5, 2.0, 4.0):
        cell = factor * grid.cell_size
        try:
            other = mesh.PointGrid(target, max_distance, cell)
        except ValueError as e:
            lines.append("cell_size %.6g (%.2f x default): %s" % (cell, factor, str(e)[:60]))
            continue
        assert iteration_form(other).tobytes() == sums.tobytes()
        lines.append("cell_size %.6g (%.2f x default): nearest %.3f ms, iteration %.3f ms (medians of %d), same bytes"
                     % (cell, factor, statistics.median(timed(lambda: nearest_form(other), args.repeats)),
                        statistics.median(timed(lambda: iteration_form(other), args.repeats)), args.repeats))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
