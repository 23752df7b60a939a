"""Round 9, step 0: what handing R6's / R7's tiles to persistent workgroups heaviest first can save, predicted from the per-tile work of the eight
bench views at the flagship raster shapes (GPU for the counts, the schedules are simulated on the CPU).

    python profiles/raster_schedule_model.py --out profiles/r09_raster_schedule_model.txt [--save-counts DIR]

Per tile: the list length (`ranges`; R6's queue key), the entries R6 walks before every pixel of the tile has stopped (the deepest last
contributor, `n_contrib`; closer to R6's time than the list length) and the (quadrant, splat) passes of R7 (popcount of `contrib_mask` over the
tile's list; R7's key and its time).  A tile's time is taken as proportional to its work; list scheduling on 1280 (R6: 256 CUs x 5) and 1024
(R7: x 4) slots, an eighth of them per XCD:

  (a) today's dispatch: one workgroup per tile, dispatched in order and round robin over the XCDs, workgroup b -> XCD b % 8 -> tile
      (b % 8) * per + b / 8; a workgroup starts when its XCD has a free slot and every earlier workgroup has started;
  (b) persistent slots, one queue per XCD band, heaviest of 32 classes first (tile index ascending inside a class), a slot whose queue is dry
      takes from the next band's;
  (c) persistent slots, one global queue in the same order.

Reported per view: makespan / ideal (ideal = total work / slots) and heaviest tile / ideal."""
import argparse
import heapq
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [os.path.dirname(HERE)] + [p for p in sys.path if os.path.abspath(p or ".") != HERE]      # (profiles/numbers.py would shadow the stdlib's)

import numpy as np  # noqa: E402

CLASSES = 32


def by_class(key, tiles):
    """`tiles` heaviest class first, tile index ascending inside a class (the order build_tile_order writes)."""
    cls = (key.astype(np.int64) * CLASSES) // (int(key.max()) + 1)
    return sorted(tiles, key=lambda t: (-cls[t], t))


def fixed_dispatch(cost, slots):
    n = len(cost)
    per = (n + 7) // 8
    free = [[0.0] * (slots // 8) for _ in range(8)]
    started, end = 0.0, 0.0
    for b in range(8 * per):
        x, t = b & 7, (b & 7) * per + (b >> 3)
        if t >= n:
            continue
        started = max(started, heapq.heappop(free[x]))
        heapq.heappush(free[x], started + cost[t])
        end = max(end, started + cost[t])
    return end


def persistent(cost, key, slots, banded, steal=True):
    n = len(cost)
    per = (n + 7) // 8
    if banded:
        queues = [by_class(key, range(x * per, min(n, (x + 1) * per))) for x in range(8)]
    else:
        queues = [by_class(key, range(n))] + [[] for _ in range(7)]
    heads = [0] * 8
    workers = [(0.0, w & 7) for w in range(slots)]
    heapq.heapify(workers)
    end = 0.0
    while workers:
        now, x = heapq.heappop(workers)
        for k in range(8 if (steal or not banded) else 1):
            q = (x + k) & 7 if banded else 0
            if heads[q] < len(queues[q]):
                t = queues[q][heads[q]]
                heads[q] += 1
                end = max(end, now + cost[t])
                heapq.heappush(workers, (now + cost[t], x))
                break
    return end


def report(name, cost, key, slots, out):
    cost = cost.astype(np.float64)
    ideal = cost.sum() / slots
    a = fixed_dispatch(cost, slots)
    b = persistent(cost, key, slots, True)
    b0 = persistent(cost, key, slots, True, steal=False)
    c = persistent(cost, key, slots, False)
    out("    %-34s ideal %8.0f  heaviest/ideal %.2f   makespan/ideal  (a) %.3f  (b) %.3f  (b, no stealing) %.3f  (c) %.3f" % (
        name, ideal, cost.max() / ideal, a / ideal, b / ideal, b0 / ideal, c / ideal))
    return a, b, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--save-counts", default=None, help="directory for the per-view count arrays (.npy)")
    ap.add_argument("--from-counts", default=None, help="directory of saved count arrays: no GPU")
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--res", type=int, default=800)
    a = ap.parse_args()
    lines = []
    out = lambda s="": (lines.append(s), print(s, flush=True))
    P, H, W, C = a.gaussians, a.res, a.res, 5
    out("R6 / R7 tile schedules simulated from the per-tile work, %d base surfels, %dx%d, the eight bench views" % (P, H, W))
    out("R6 on 1280 slots, R7 on 1024; makespan in units of work (entries / passes); see profiles/raster_schedule_model.py")
    out()
    if not a.from_counts:
        import torch
        from envgs_amd import raster, synth
        dev = torch.device("cuda:0")
        g = synth.base_gaussians(P, seed=0, device=dev)
        pkg = importlib.import_module("diff_surfel_rasterization_wet_ch05")
        sh_degree = torch.tensor([3], device=dev)
    tot = {"R6 by list length": [0.0] * 3, "R6 by walked entries": [0.0] * 3, "R7": [0.0] * 3}
    for v in range(8):
        if a.from_counts:
            inst, walked, pas = np.load(os.path.join(a.from_counts, "raster_tiles_view%d.npy" % v)).T
        else:
            cam = synth.orbit_camera(v, n_views=8, H=H, W=W, fx=1111.1 * W / 800.0, device=dev)
            st = pkg.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(C, device=dev),
                                                   scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                                                   sh_degree=sh_degree, campos=cam.camera_center, prefiltered=False, debug=False)
            with torch.no_grad():
                _, sv = raster.rasterize_forward(C, g["means3D"], None, torch.zeros(P, C, device=dev), g["opacities"], g["scales"], g["rotations"], None, st)
            rg = sv["ranges"].view(-1, 2).long().cpu().numpy()
            cm = sv["contrib_mask"][:sv["N"]].cpu().numpy()
            inst = rg[:, 1] - rg[:, 0]
            gx, gy = (W + 15) // 16, (H + 15) // 16
            last = torch.zeros(gy * 16, gx * 16, dtype=torch.int32, device=dev)
            last[:H, :W] = sv["n_contrib"][0]
            walked = last.view(gy, 16, gx, 16).amax(dim=(1, 3)).reshape(-1).long().cpu().numpy()
            # (R6 stops flushing contrib_mask once every pixel of the tile has stopped: entries behind the deepest last contributor are not
            #  written, and R7 does not read them)
            c_pas = np.concatenate([[0], np.cumsum(np.unpackbits(cm[:, None], axis=1).sum(1))])
            pas = c_pas[rg[:, 0] + np.minimum(walked, inst)] - c_pas[rg[:, 0]]
            if sv.get("tile_queue") is not None:
                assert np.array_equal(raster.tile_queue_views(sv)["tile_cost"].cpu().numpy().astype(np.int64), pas)
            if a.save_counts:
                os.makedirs(a.save_counts, exist_ok=True)
                np.save(os.path.join(a.save_counts, "raster_tiles_view%d.npy" % v), np.stack([inst, walked, pas], 1))
        out("view %d: %d tiles, %d instances, %d walked, %d passes; per tile mean / max: instances %.0f / %d, walked %.0f / %d, passes %.0f / %d" % (
            v, len(inst), inst.sum(), walked.sum(), pas.sum(), inst.mean(), inst.max(), walked.mean(), walked.max(), pas.mean(), pas.max()))
        for name, cost, key, slots in (("R6 by list length", inst, inst, 1280), ("R6 by walked entries", walked, inst, 1280), ("R7", pas, pas, 1024)):
            r = report("%s (queue key = %s)" % (name, "passes" if name == "R7" else "list length"), cost, key, slots, out)
            tot[name] = [x + y for x, y in zip(tot[name], r)]
    out()
    out("summed makespan over the eight views, (b) and (c) against (a):")
    for name, (sa, sb, sc) in tot.items():
        out("    %-22s (a) %10.0f  (b) %10.0f = %.3f (a)  (c) %10.0f = %.3f (a)" % (name, sa, sb, sb / sa, sc, sc / sa))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
