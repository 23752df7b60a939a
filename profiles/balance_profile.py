"""Round 7: how evenly the coarse work of the flagship step is spread, measured on the eight bench views at the flagship shapes (GPU).

    python profiles/balance_profile.py --out profiles/r07_balance_before.txt [--save-counts DIR]

Tracer backward: the per-batch entry counts of the environment trace (tracing.LAST_STATS["n_entries"]) and what profiles/sched_model.py
makes of them.  Raster: per tile, the instances (`ranges`), the instances some pixel blended and the (quadrant, splat) passes R7 walks (both
from `contrib_mask`), summed over the eight contiguous bands xcd_tile() gives the XCDs.
"""
import argparse
import importlib
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [os.path.dirname(HERE)] + [p for p in sys.path if os.path.abspath(p or ".") != HERE]      # (profiles/numbers.py would shadow the stdlib's)

import numpy as np  # noqa: E402
import torch  # noqa: E402

_spec = importlib.util.spec_from_file_location("sched_model", os.path.join(HERE, "sched_model.py"))
sched_model = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sched_model)
from envgs_amd import envgs_step, raster, synth, tracing  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--save-counts", default=None, help="directory for the per-view count arrays (.npy)")
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--env-gaussians", type=int, default=163840)
    ap.add_argument("--res", type=int, default=800)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, H, W, C = a.gaussians, a.res, a.res, 5
    g = synth.base_gaussians(P, seed=0, device=dev)
    ge = synth.env_gaussians(a.env_gaussians, seed=1, device=dev)
    cams = [synth.orbit_camera(v, n_views=8, H=H, W=W, fx=1111.1 * W / 800.0, device=dev) for v in range(8)]
    names = ["means3D", "shs", "opacities", "scales", "rotations"]
    params = {k: g[k].clone().requires_grad_(True) for k in names}
    params["specular"] = g["specular"].repeat(1, C - 4).contiguous().clone().requires_grad_(True)
    params["roughness"] = g["roughness"].clone().requires_grad_(True)
    env = {k: ge[k].clone().requires_grad_(True) for k in names}
    pkg = importlib.import_module("diff_surfel_rasterization_wet_ch05")
    import diff_surfel_tracing as tpkg
    envgs_step.FUSED["on"] = True
    tracer = tpkg.SurfelTracer()
    bg = torch.zeros(3, device=dev)
    sh_degree = torch.tensor([3], device=dev)
    lines = []
    out = lambda s="": (lines.append(s), print(s, flush=True))
    out("balance of the coarse work, %d base / %d environment surfels, %dx%d, the eight bench views" % (P, a.env_gaussians, H, W))
    out()
    out("== tracer backward: entries per 64-ray batch of the environment trace ==")
    for v, cam in enumerate(cams):
        for _ in range(2):                                   # (the second call runs with the list capacities the first one published)
            envgs_step.envgs_forward(pkg, tpkg, tracer, cam, synth.get_rays(cam), params, env, bg, bg, sh_degree)
        torch.cuda.synchronize()
        tracing.join_deferred_gradients()
        ne = tracing.LAST_STATS["n_entries"].cpu().numpy().astype(np.int64)
        if a.save_counts:
            os.makedirs(a.save_counts, exist_ok=True)
            np.save(os.path.join(a.save_counts, "n_entries_view%d.npy" % v), ne)
        out("view %d" % v)
        out(sched_model.format_report(sched_model.report(ne)).rstrip("\n"))
    out()
    out("== raster: per-tile work summed over the eight XCD bands of xcd_tile() ==")
    out("(instances = entries of the tile's list; contributing = entries some pixel of the tile blended; passes = (8x8 quadrant, splat) passes of R7)")
    for v, cam in enumerate(cams):
        st = pkg.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(C, device=dev),
                                               scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                                               sh_degree=sh_degree, campos=cam.camera_center, prefiltered=False, debug=False)
        with torch.no_grad():
            _, sv = raster.rasterize_forward(C, g["means3D"], None, torch.zeros(P, C, device=dev), g["opacities"], g["scales"], g["rotations"], None, st)
        rg = sv["ranges"].view(-1, 2).long().cpu().numpy()
        cm = sv["contrib_mask"][:sv["N"]].cpu().numpy()
        inst = rg[:, 1] - rg[:, 0]
        c_con = np.concatenate([[0], np.cumsum(cm != 0)])
        c_pas = np.concatenate([[0], np.cumsum(np.unpackbits(cm[:, None], axis=1)[:, 4:].sum(1))])
        con = c_con[rg[:, 1]] - c_con[rg[:, 0]]
        pas = c_pas[rg[:, 1]] - c_pas[rg[:, 0]]
        ntiles = len(inst)
        per = (ntiles + 7) // 8
        if a.save_counts:
            np.save(os.path.join(a.save_counts, "tiles_view%d.npy" % v), np.stack([inst, con, pas], 1))
        out("view %d: %d tiles, %d instances, %d contributing, %d passes" % (v, ntiles, inst.sum(), con.sum(), pas.sum()))
        for name, arr in (("instances", inst), ("contributing", con), ("passes", pas)):
            bands = np.array([arr[x * per:(x + 1) * per].sum() for x in range(8)], dtype=np.float64)
            nz = arr[arr > 0]
            out("    %-12s band / mean: %s   max / mean %.3f   per tile: mean %.0f  p50 %.0f  p90 %.0f  max %d" % (
                name, " ".join("%.2f" % (b / bands.mean()) for b in bands), bands.max() / bands.mean(), arr.mean(),
                np.percentile(nz, 50) if nz.size else 0, np.percentile(nz, 90) if nz.size else 0, arr.max()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
