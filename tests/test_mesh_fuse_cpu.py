"""CPU: the depth-fusion oracle (tests/mesh_fuse_oracle.py) against the reference's recorded outputs (tests/golden/fuse_golden.npz), the fragile
share of every case, and the host side of envgs_amd.mesh's depth fusion: nearest_views, the count threshold, the composed maps, the point-cloud
PLY and the argument checks."""
import numpy as np
import pytest
import torch

from tests import mesh_fuse_cases as cases
from tests import mesh_fuse_oracle as fo


def _cameras(c):
    from envgs_amd import synth
    return [synth.make_camera(c.K[v], c.R[v], c.T[v], c.H, c.W, 0.5, 10.0) for v in range(len(c.K))]


@pytest.mark.parametrize("name", cases.GOLDEN)
def test_oracle_matches_the_reference(name):
    g = cases.golden()
    c = g.cases[name]
    o = fo.consistency(c.depth, c.K, c.R, c.T, c.sources, band=g.band, **c.thresholds)
    share = float(o.fragile.mean())
    pair_bad = int((o.pair_mask != c.pair_mask)[~o.pair_fragile].sum())
    print("%s: band %.3g, fragile pixels %d of %d (%.3f %%), fragile pairs %d, pair decisions that differ off them %d, reference float32-vs-float64 %s"
          % (name, g.band, int(o.fragile.sum()), o.fragile.size, 100 * share, int(o.pair_fragile.sum()), pair_bad, c.diff.tolist()))
    assert share <= 0.01                                                        # the condition of the issue, per case
    assert c.diff[3] == 0 and c.diff[4] == 0                                    # the reference's two precisions decided alike: one set of masks
    assert pair_bad == 0
    assert np.array_equal(o.photo_mask, c.photo)
    assert np.array_equal(o.geo_mask[~o.fragile_geo], c.geo[~o.fragile_geo])
    assert np.array_equal(o.final_mask[~o.fragile_final], c.final[~o.fragile_final])
    assert o.min_count == {"sphere": 3, "holes": 3, "border": 3, "s3": 3}[name]
    same = (o.pair_mask == c.pair_mask).all(1)                                  # float64 against float64: equal decisions, equal values
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))
    if hasattr(c, "depth_avg64"):
        e = rel(o.depth_avg[same], c.depth_avg64[same])
        print("%s: depth_avg against the reference's float64: %.3g" % (name, e))
        assert same.mean() > 0.99 and e <= 1e-12
    if hasattr(c, "z64"):
        both = o.pair_mask & c.pair_mask
        e = rel(o.z[both], c.z64[both])
        print("%s: depth_reprojected against the reference's float64: %.3g" % (name, e))
        assert both.any() and e <= 1e-12
    # the reference's own float32 run sits inside the band it set (a quarter of it, by construction)
    keep = ~o.fragile
    e32 = rel(c.depth_avg32.astype(np.float64)[keep], o.depth_avg[keep])
    both = o.pair_mask & c.pair_mask
    z32 = rel(c.z32.astype(np.float64)[both], o.z[both])
    print("%s: the reference's float32 depth_avg %.3g and depth_reprojected %.3g from the oracle" % (name, e32, z32))
    assert e32 <= g.band and z32 <= g.band


def test_golden_covers_what_it_is_for():
    g = cases.golden()
    assert 0 < g.band < 1e-2
    assert abs(g.band - 4 * max(c.diff[:3].max() for c in g.cases.values())) <= 1e-12 * g.band
    for name, c in g.cases.items():
        live = cases.golden_case(name)                                          # the fixture holds the inputs tests/mesh_fuse_cases.py builds
        assert np.array_equal(c.sources, live.sources) and np.allclose(c.K, live.K, rtol=1e-6) and np.allclose(c.depth, live.depth, rtol=1e-5, atol=1e-6)
        assert 0.05 < c.final.mean() < 0.9
    holes, sphere = g.cases["holes"], g.cases["sphere"]
    assert (holes.depth == 0).sum() > (sphere.depth == 0).sum() and holes.final.sum() < sphere.final.sum()
    # border: a good part of the surface a view sees projects outside its sources' images
    c = g.cases["border"]
    o = fo.consistency(c.depth, c.K, c.R, c.T, c.sources, band=g.band, **c.thresholds)
    outside = 0
    for r in range(len(c.K)):
        for k, s in enumerate(c.sources[r]):
            p = fo.pair(c.depth[r].astype(np.float64), c.depth[s].astype(np.float64), *fo.pair_maps(c.K.astype(np.float64), c.R.astype(np.float64),
                        c.T.astype(np.float64), r, int(s)), 1.0, 0.01, g.band)
            seen = c.depth[r] > 0
            outside += int((seen & ((p.u < 0.5) | (p.u > c.W - 0.5) | (p.v < 0.5) | (p.v > c.H - 0.5))).sum())
    print("border: %d (pixel, source) pairs sample under the border clip" % outside)
    assert outside > 200 and o.final_mask.any()


def test_device_cases_stay_inside_the_fragile_limit():
    """The cases tests/test_mesh_fuse_gpu.py runs are ones its check can judge: from the float64 audit alone, at most 1 % of the pixels are fragile,
    and each case keeps some pixels and drops some."""
    band = cases.golden().band
    todo = [("%dx%d" % s, cases.shape_case(*s, 3, 2)) for s in cases.SHAPES]
    todo += [("V %d S %d" % vs, cases.shape_case(17, 31, *vs)) for vs in ((3, 0), (3, 1), (3, 8), (3, 9), (1, 0), (2, 1))]
    todo += [("bad values", cases.bad_values_case()), ("far border", cases.far_border_case())]
    for what, c in todo:
        o = fo.consistency(c.depth, c.K, c.R, c.T, c.sources, band=band, **c.thresholds)
        print("%s: fragile %d of %d, kept %d" % (what, int(o.fragile.sum()), o.fragile.size, int(o.final_mask.sum())))
        assert o.fragile.mean() <= 0.01, what
        assert o.final_mask.any() and (what == "1x1" or not o.final_mask.all()), what
    assert fo.consistency(cases.shape_case(17, 31, 3, 9).depth, *[getattr(cases.shape_case(17, 31, 3, 9), k) for k in "KRT"],
                          cases.shape_case(17, 31, 3, 9).sources, band=band, geo_rel_thresh=0.03).count.max() == 9


@pytest.mark.parametrize("name", cases.GOLDEN)
def test_nearest_views(name):
    from envgs_amd import mesh
    c = cases.golden().cases[name]
    n = c.sources.shape[1]
    got = mesh.nearest_views(_cameras(c), n)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(c.K), n)
    assert np.array_equal(got.numpy(), c.similarity[:, 1:1 + n])                # the reference's compute_camera_similarity
    assert np.array_equal(got.numpy(), c.sources)
    assert (c.similarity[:, 0] == np.arange(len(c.K))).all()                    # distinct centres: the reference drops the view itself
    assert tuple(mesh.nearest_views(_cameras(c), 99).shape) == (len(c.K), len(c.K) - 1)
    assert tuple(mesh.nearest_views(_cameras(c), 0).shape) == (len(c.K), 0)


def test_nearest_views_with_coincident_centres_excludes_the_view_itself():
    from envgs_amd import mesh
    c = cases.golden().cases["s3"]
    cams = _cameras(c)
    cams[2] = cams[0]                                                           # views 0 and 2 share a centre
    got = mesh.nearest_views(cams, 3).numpy()
    assert all(v not in got[v] for v in range(4))
    assert got[0, 0] == 2 and got[2, 0] == 0                                    # distance 0 comes first, and it is the OTHER camera


@pytest.mark.parametrize("thresh", [0.5, 0.75, 1.0])
def test_min_count_is_the_reference_comparison(thresh):
    from envgs_amd import mesh
    for S in range(1, 11):
        counts = torch.arange(S + 2)
        passing = (counts >= (thresh * S)).nonzero().reshape(-1)                # the reference's expression on an integer tensor
        want = int(passing[0])
        assert mesh.fuse_min_count(thresh, S) == want and fo.min_count(thresh, S) == want
    assert mesh.fuse_min_count(0.75, 0) == 0 and mesh.fuse_min_count(0.75, 3) == 3 and mesh.fuse_min_count(0.75, 4) == 3


def test_composed_maps_and_back_projection():
    from envgs_amd import mesh
    g = cases.golden()
    c = g.cases["sphere"]
    K, R, T = (a.astype(np.float64) for a in (c.K, c.R, c.T))
    fwd_all, back_all = mesh.fuse_pair_maps(K, R, T, c.sources)
    assert fwd_all.shape == back_all.shape == c.sources.shape + (12,)
    for r in range(len(K)):
        for k, s in enumerate(c.sources[r]):
            for a, b in zip((fwd_all[r, k], back_all[r, k]), fo.pair_maps(K, R, T, r, int(s))):
                assert np.allclose(a, b, rtol=1e-13, atol=1e-13)
    k = list(c.sources[1]).index(2)
    fwd, back = fwd_all[1, k], back_all[1, k]
    # a point of depth d in front of pixel (x, y) of view 1 goes to view 2 and comes back
    pix, d = np.array([20.5, 17.5, 1.0]), 2.4
    p = d * (fwd[:9].reshape(3, 3) @ pix) + fwd[9:]
    q = p[2] * (back[:9].reshape(3, 3) @ (p / p[2])) + back[9:]
    assert np.allclose(q / q[2], pix, rtol=0, atol=1e-5) and abs(q[2] - d) < 1e-6          # the float32 rotations are orthogonal to 1e-7 only
    M = mesh.fuse_view_maps(K, R, T)
    assert np.allclose(M, fo.view_maps(K, R, T), rtol=1e-13, atol=1e-13)
    # get_rays(z_depth=True) of the reference (its inverse of K is float32 with an epsilon on the determinant: 1e-5)
    xc, yc = fo.pixel_centres(c.H, c.W)
    ray = np.stack([xc, yc, np.ones_like(xc)], -1) @ M[0, :9].reshape(3, 3).T
    assert np.allclose(M[0, 9:], g.rays_origin, atol=1e-6)
    assert np.abs(ray - g.rays_direction).max() <= 1e-5
    idx = np.array([0, 5 * c.W + 7, c.H * c.W - 1])
    pts, bound = fo.points(np.full((1, c.H, c.W), 2.0), K[:1], R[:1], T[:1], idx, g.band)
    assert np.allclose(pts, g.rays_origin + 2.0 * g.rays_direction.reshape(-1, 3)[idx], atol=3e-5) and (bound > 0).all()


def test_points_ply_round_trip(tmp_path):
    from envgs_amd import ckpt
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(257, 3)).astype(np.float32)
    col = rng.random((257, 3)).astype(np.float32)
    col[0], col[1] = (-0.5, 0.0, 1.5), (0.5, 1.0 / 255.0, 0.499 / 255.0)
    nrm = rng.normal(size=(257, 3)).astype(np.float32)
    want = np.rint(np.clip(col.astype(np.float64), 0, 1) * 255).astype(np.uint8)
    for colors, normals in ((None, None), (col, None), (None, nrm), (torch.from_numpy(col), torch.from_numpy(nrm))):
        path = str(tmp_path / "cloud.ply")
        ckpt.save_points_ply(path, torch.from_numpy(pts), colors, normals)
        p, c, n = ckpt.load_points_ply(path)
        assert p.dtype == np.float32 and np.array_equal(p, pts)
        assert (c is None) == (colors is None) and (n is None) == (normals is None)
        if c is not None:
            assert c.dtype == np.uint8 and np.array_equal(c, want)
        if n is not None:
            assert np.array_equal(n, nrm)
        head = open(path, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
        names = [l.split()[2] for l in head if l.startswith("property")]
        assert head[1] == "format binary_little_endian 1.0" and names == (["x", "y", "z"] + (["nx", "ny", "nz"] if normals is not None else [])
                                                                          + (["red", "green", "blue"] if colors is not None else []))
        v, f, mc = ckpt.load_mesh_ply(path)                                     # the mesh reader takes it as a cloud without faces
        assert np.array_equal(v, pts) and f.shape == (0, 3)
    ckpt.save_points_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    p, c, n = ckpt.load_points_ply(str(tmp_path / "empty.ply"))
    assert p.shape == (0, 3) and c.shape == (0, 3) and n is None
    with pytest.raises(ValueError):
        ckpt.save_points_ply(str(tmp_path / "bad.ply"), pts, col[:5])
    with pytest.raises(ValueError):
        ckpt.save_points_ply(str(tmp_path / "bad.ply"), pts, None, nrm[:5])


def test_argument_checks_raise_value_error():
    from envgs_amd import mesh
    c = cases.golden().cases["s3"]
    cams = _cameras(c)
    depth = torch.from_numpy(c.depth)                                           # a CPU tensor
    V, H, W = depth.shape
    for fn in (mesh.depth_consistency, mesh.fuse_depth_points):
        with pytest.raises(ValueError, match="GPU"):
            fn(depth, cams)
        with pytest.raises(ValueError, match="float32"):
            fn(depth.double(), cams)
        with pytest.raises(ValueError, match="float32"):
            fn(depth[0], cams)                                                  # rank
        with pytest.raises(ValueError, match="per camera"):
            fn(depth[:3], cams)
        with pytest.raises(ValueError, match="share one size"):
            fn([depth[0], depth[1], depth[2, :, :-1], depth[3]], cams)
        with pytest.raises(ValueError, match="out of range"):
            fn(depth, cams, sources=[[1, 2], [0, 4], [0, 1], [0, 1]])
        with pytest.raises(ValueError, match="out of range"):
            fn(depth, cams, sources=torch.tensor([[1, 2], [0, -1], [0, 1], [0, 1]]))
        with pytest.raises(ValueError, match="own source"):
            fn(depth, cams, sources=[[1, 2], [0, 1], [0, 1], [0, 1]])
        with pytest.raises(ValueError, match="table"):
            fn(depth, cams, sources=[[1, 2], [0, 2], [0, 1]])                   # one row short
        for key in ("geo_abs_thresh", "geo_rel_thresh", "geo_sum_thresh", "pho_abs_thresh"):
            for bad in (float("nan"), float("inf"), 1e300):                     # 1e300 is not finite as the float the kernel takes
                with pytest.raises(ValueError, match="finite"):
                    fn(depth, cams, **{key: bad})
        with pytest.raises(ValueError, match="2\\^31"):
            fn(torch.zeros(1, dtype=torch.float32).expand(4, 2 ** 15, 2 ** 15), cams)                    # one element of storage: only the shape is read
    with pytest.raises(TypeError):
        mesh.fuse_depth_points(depth, cams, voxel_size=0.1)
    with pytest.raises(ValueError):
        mesh.nearest_views([], 2)
