"""Generate tests/golden/fuse_golden.npz from the reference's own depth fusion (authoring container only):

    python tests/golden/make_fuse_golden.py <root of the reference tree>

The reference's functions are loaded FROM THE REFERENCE TREE AT RUN TIME: easyvolcap/utils/fusion_utils.py imports cv2, trimesh and mcubes at the
top, so the function definitions named below are taken out of their files through `ast` (decorators dropped: torch.jit.script needs a source file)
and executed in a namespace that holds only torch.  Nothing of the reference's text is written anywhere; the fixture holds the inputs of
tests/mesh_fuse_cases.py and the outputs the reference computes from them, in float32 and in float64.

Per case <c> (sphere, holes, border, s3):
  <c>/depth K R T sources thresholds        the inputs (thresholds: geo_abs, geo_rel, geo_sum, pho_abs)
  <c>/depth_avg32 photo geo final           compute_consistency in float32 (the masks of the float64 run are identical unless flips says otherwise)
  <c>/pair_mask z32                         depth_geometry_consistency in float32: the per-pair mask and depth_reprojected (0 where the pair fails)
  <c>/depth_avg64 z64                       the float64 run (depth_avg64 not for "holes", z64 only for "border" and "s3": the file's size)
  <c>/diff                                  largest float32-vs-float64 relative difference of depth_reprojected, dist, depth_est_averaged, and the
                                            number of pair decisions and final bits that differ between the two runs
  <c>/similarity                            compute_camera_similarity(c2ws, c2ws)[1]
rays/...                                    get_rays(z_depth=True) of view 0 of the sphere rig: centres and directions
band                                        4 x the largest of the diff entries over all cases ("Depth fusion")

How the differences are measured.  depth_reprojected and dist are compared over the pairs IN PLAY: sampled positive in both runs, and in the
float64 run within twice geo_rel_thresh and twice geo_abs_thresh -- the pairs that pass, and those that fail by less than a factor of two.  A pair
far outside (a silhouette sample that mixes the surface with the empty background, a point that returns pixels away) decides nothing near a
threshold, and its rounding -- a bilinear weight of 0.03 carries the coordinate's absolute error thirty-fold -- says nothing about the pairs that
do.  depth_reprojected: |z32 - z64| / |z64|.  dist: |dist32 - dist64| / max(dist64, geo_abs_thresh) -- dist is a length in pixels near 0 for an
agreeing pair, its error is that of a pixel coordinate and it is decided against geo_abs_thresh, so that is its scale.  depth_est_averaged:
|a32 - a64| / |a64| over the pixels whose pair decisions agree."""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import mesh_fuse_cases as cases  # noqa: E402

WANTED = {"easyvolcap/utils/fusion_utils.py": ["depth_reprojection", "depth_geometry_consistency", "compute_consistency"],
          "easyvolcap/utils/ray_utils.py": ["create_meshgrid", "get_rays", "get_rays_from_ij"],
          "easyvolcap/utils/math_utils.py": ["affine_inverse", "torch_inverse_3x3", "normalize"],
          "easyvolcap/utils/cam_utils.py": ["compute_camera_similarity"]}


def load_reference(root):
    ns = {"torch": torch, "F": torch.nn.functional, "np": np}
    for rel, names in WANTED.items():
        tree = ast.parse(open(os.path.join(root, rel)).read())
        found = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        missing = set(names) - {n.name for n in found}
        if missing:
            raise SystemExit("%s has no %s" % (rel, sorted(missing)))
        for n in found:
            n.decorator_list = []
        exec(compile(ast.Module(body=found, type_ignores=[]), rel, "exec"), ns)
    return ns


def run(ref, case, dtype):
    V, S = case.sources.shape
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    depth, K = t(case.depth), t(case.K)
    ext = torch.eye(4, dtype=dtype).repeat(V, 1, 1)
    ext[:, :3, :3], ext[:, :3, 3] = t(case.R), t(case.T)
    th = case.thresholds
    out = dict(avg=[], photo=[], geo=[], final=[], pair=[], z=[], zraw=[], dist=[], proj=[])
    for r in range(V):
        src = torch.from_numpy(case.sources[r])
        a = (depth[r][None], K[r][None], ext[r][None], depth[src][None], K[src][None], ext[src][None])
        avg, photo, geo, final = ref["compute_consistency"](*a, th["geo_abs_thresh"], th["geo_rel_thresh"], th["geo_sum_thresh"], th["pho_abs_thresh"])
        mask, z, _, _ = ref["depth_geometry_consistency"](*a, th["geo_abs_thresh"], th["geo_rel_thresh"])
        zraw, x2, y2, _, _, proj = ref["depth_reprojection"](*a)
        ij = ref["create_meshgrid"](case.H, case.W, device=depth.device, dtype=dtype)
        dist = torch.sqrt((x2 - ij[..., 1]) ** 2 + (y2 - ij[..., 0]) ** 2)
        for k, val in zip(("avg", "photo", "geo", "final", "pair", "z", "zraw", "dist", "proj"), (avg, photo, geo, final, mask, z, zraw, dist, proj)):
            out[k].append(val[0].numpy())
    return {k: np.stack(v) for k, v in out.items()}


def main(root):
    ref = load_reference(root)
    store, worst = {}, 0.0
    for name in cases.GOLDEN:
        case = cases.golden_case(name)
        o32, o64 = run(ref, case, torch.float32), run(ref, case, torch.float64)
        th = case.thresholds
        with np.errstate(all="ignore"):
            d64 = case.depth.astype(np.float64)[:, None]
            play = (o32["proj"] & o64["proj"] & (np.abs(o64["zraw"] - d64) / d64 < 2 * th["geo_rel_thresh"]) & (o64["dist"] < 2 * th["geo_abs_thresh"])
                    & np.isfinite(o32["zraw"]) & np.isfinite(o32["dist"]))
            dz = np.where(play, np.abs(o32["zraw"] - o64["zraw"]) / np.abs(o64["zraw"]), 0.0).max()
            dd = np.where(play, np.abs(o32["dist"] - o64["dist"]) / np.maximum(o64["dist"], th["geo_abs_thresh"]), 0.0).max()
            same = (o32["pair"] == o64["pair"]).all(1) & np.isfinite(o64["avg"]) & (o64["avg"] != 0)
            da = np.where(same, np.abs(o32["avg"] - o64["avg"]) / np.abs(o64["avg"]), 0.0).max()
        flips = [int((o32["pair"] != o64["pair"]).sum()), int((o32["final"] != o64["final"]).sum())]
        print("%-7s depth_reprojected %.3g  dist %.3g  depth_est_averaged %.3g  pair flips %d  final flips %d  kept %d of %d"
              % (name, dz, dd, da, flips[0], flips[1], int(o32["final"].sum()), o32["final"].size))
        worst = max(worst, dz, dd, da)
        p = name + "/"
        store.update({p + "depth": case.depth.astype(np.float32), p + "K": case.K.astype(np.float32), p + "R": case.R.astype(np.float32),
                      p + "T": case.T.astype(np.float32), p + "sources": case.sources,
                      p + "thresholds": np.array([th["geo_abs_thresh"], th["geo_rel_thresh"], th["geo_sum_thresh"], th["pho_abs_thresh"]], np.float64),
                      p + "depth_avg32": o32["avg"].astype(np.float32), p + "photo": o32["photo"], p + "geo": o32["geo"], p + "final": o32["final"],
                      p + "pair_mask": o32["pair"], p + "z32": o32["z"].astype(np.float32),
                      p + "diff": np.array([dz, dd, da] + flips, np.float64)})
        if name != "holes":
            store[p + "depth_avg64"] = o64["avg"]
        if name in ("border", "s3"):
            store[p + "z64"] = o64["z"]
        c2w = torch.eye(4, dtype=torch.float64).repeat(len(case.K), 1, 1)
        c2w[:, :3, :3] = torch.from_numpy(case.R).mT
        c2w[:, :3, 3] = torch.from_numpy(-np.einsum("vji,vj->vi", case.R, case.T))
        store[p + "similarity"] = ref["compute_camera_similarity"](c2w, c2w)[1].numpy().astype(np.int64)
    case = cases.golden_case("sphere")
    t = lambda a: torch.from_numpy(a[0])
    ray_o, ray_d = ref["get_rays"](case.H, case.W, t(case.K), t(case.R), t(case.T).reshape(3, 1), z_depth=True)
    store["rays/origin"], store["rays/direction"] = ray_o[0, 0].numpy(), ray_d.numpy().astype(np.float32)
    store["band"] = np.array(4.0 * worst)
    print("band = 4 x %.3g = %.3g" % (worst, 4.0 * worst))
    path = os.path.join(HERE, "fuse_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
