"""GPU: the depth fusion (csrc/mesh_fuse.hip, envgs_amd.mesh "depth fusion") against its float64 twin (tests/mesh_fuse_oracle.py) and against the
reference's recorded outputs (tests/golden/fuse_golden.npz), by the convention of DESIGN.md section 5: decisions exactly off the audited fragile
set, values within the measured band, points within the derived fp32 bound.  Shapes are the smallest at which the kernels change path: a
workgroup is 256 pixels, the compaction scans one counter per workgroup."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_fuse_cases as cases
from tests import mesh_fuse_oracle as fo

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, TEMP_TOO_SMALL = -1, -2


def _cameras(c):
    from envgs_amd import synth
    return [synth.make_camera(c.K[v], c.R[v], c.T[v], c.H, c.W, 0.5, 10.0, device=DEV) for v in range(len(c.K))]


def _np(t):
    return None if t is None else t.cpu().numpy()


def _maps(V, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.random((V, 3, H, W), dtype=np.float32), rng.normal(size=(V, 3, H, W)).astype(np.float32)


def fuse_and_check(c, what, depth_avg_ref=None, masks_ref=None):
    """depth_consistency and fuse_depth_points of a case on the device, each twice (identical bytes), against the audited oracle; with the
    reference's recorded depth_avg / masks when given.  -> (the device's consistency as arrays, the oracle's, points, index)."""
    from envgs_amd import mesh
    band = cases.golden().band
    cams = _cameras(c)
    depth = torch.from_numpy(np.ascontiguousarray(c.depth, np.float32)).to(DEV)
    V, H, W = depth.shape
    rgb, nrm = _maps(V, H, W, 3)
    rgb_t, nrm_t = torch.from_numpy(rgb).to(DEV), torch.from_numpy(nrm).to(DEV)
    kw = dict(sources=c.sources, **c.thresholds)
    runs = []
    for _ in range(2):
        o = mesh.depth_consistency(depth, cams, **kw)
        p = mesh.fuse_depth_points(depth, cams, rgb=rgb_t, normal=nrm_t, return_index=True, **kw)
        runs.append([_np(o.depth_avg), _np(o.count), _np(o.photo_mask), _np(o.geo_mask), _np(o.final_mask)] + [_np(t) for t in p])
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: two runs differ" % what
    got = SimpleNamespace(**dict(zip(("depth_avg", "count", "photo_mask", "geo_mask", "final_mask", "points", "colors", "normals", "index"), runs[0])))
    assert got.depth_avg.dtype == np.float32 and got.count.dtype == np.uint8 and got.final_mask.dtype == np.bool_ and got.index.dtype == np.int64
    want = fo.consistency(c.depth, c.K, c.R, c.T, c.sources, band=band, **c.thresholds)
    fo.check(got, want, band, what)
    if depth_avg_ref is not None:                               # the reference's own float32 outputs
        ref = SimpleNamespace(count=want.count, fragile=want.fragile, fragile_geo=want.fragile_geo, fragile_final=want.fragile_final,
                              depth_avg=want.depth_avg, **masks_ref)
        fo.check(got, ref, band, what + " (reference)", depth_avg_ref=depth_avg_ref)
    assert not np.isnan(got.depth_avg[got.final_mask]).any()    # no NaN reaches a kept pixel
    # compaction: ascending (view, row, column), gathers at the index
    assert np.array_equal(got.index, np.flatnonzero(got.final_mask.reshape(-1)))
    N = len(got.index)
    assert got.points.shape == (N, 3) and got.colors.shape == (N, 3) and got.normals.shape == (N, 3)
    v, r = got.index // (H * W), got.index % (H * W)
    assert np.array_equal(got.colors, rgb.reshape(V, 3, H * W)[v, :, r]) and np.array_equal(got.normals, nrm.reshape(V, 3, H * W)[v, :, r])
    source = want.depth_avg if depth_avg_ref is None else np.asarray(depth_avg_ref, np.float64)
    pts, bound = fo.points(source, c.K, c.R, c.T, got.index, band)
    keep = ~want.fragile.reshape(-1)[got.index]
    excess = float(np.max((np.abs(got.points - pts) / bound)[keep], initial=0.0))
    print("%s: %d points, largest error / bound %.3g" % (what, N, excess))
    assert excess <= 1.0, "%s: a point is %.3g bounds from the oracle (band %.3g)" % (what, excess, band)
    return got, want


# ---- 1. image sizes around one workgroup and one scan block ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_image_sizes(H, W):
    fuse_and_check(cases.shape_case(H, W, 3, 2), "%dx%d" % (H, W))


# ---- 2. source counts: none, one launch, and the accumulate launch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,S", [(3, 0), (3, 1), (3, 2), (3, 8), (3, 9), (1, 0), (2, 1)])
def test_source_counts(V, S):
    c = cases.shape_case(17, 31, V, S)
    assert c.sources.shape == (V, S)
    got, want = fuse_and_check(c, "V %d S %d" % (V, S))
    if S == 0:                                                  # what the reference's expressions give without sources
        assert np.array_equal(got.depth_avg, c.depth) and got.geo_mask.all() and not got.count.any()
        assert np.array_equal(got.final_mask, c.depth > 0)
    if S == 9:                                                  # sources repeat: the count passes 8 only through the second launch
        assert want.count.max() == 9 and got.count.max() == 9
    if (V, S) == (2, 1):
        assert c.sources.tolist() == [[1], [0]]


# ---- 3. the golden cases: the reference's recorded float32 outputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.GOLDEN)
def test_golden_cases_against_the_reference(name):
    c = cases.golden().cases[name]
    fuse_and_check(c, name, depth_avg_ref=c.depth_avg32, masks_ref=dict(photo_mask=c.photo, geo_mask=c.geo, final_mask=c.final))


# ---- 4. holes and non-finite values -------------------------------------------------------------------------------------------------------------------
def test_holes_and_non_finite_depths():
    c = cases.bad_values_case()
    got, want = fuse_and_check(c, "bad values")
    bad = ~(np.isfinite(c.depth) & (c.depth > 0))
    assert bad.sum() > 100 and np.isnan(c.depth).any() and np.isinf(c.depth).any() and (c.depth < 0).any()
    assert not got.final_mask[bad].any() and not got.count[bad].any()           # such a reference pixel keeps nothing
    assert got.final_mask.any()
    # such a tap makes its pair fail: wherever the oracle saw a non-finite sample, the pair did not pass, and the device counted alike (fuse_and_check)
    assert (want.count < c.sources.shape[1])[~bad].any()


# ---- 5. border ------------------------------------------------------------------------------------------------------------------------------------------
def test_border_and_a_source_behind_the_surface():
    c = cases.far_border_case()
    got, want = fuse_and_check(c, "far border")
    behind = 0
    for r in range(3):
        k = list(c.sources[r]).index(3)
        fwd, _ = fo.pair_maps(c.K, c.R, c.T, r, 3)
        xc, yc = fo.pixel_centres(c.H, c.W)
        z = c.depth[r] * (fwd[6] * xc + fwd[7] * yc + fwd[8]) + fwd[11]
        seen = c.depth[r] > 0
        behind += int((seen & (z < 0)).sum())
        assert not want.pair_mask[r, k][seen & (z < 0)].any()
    assert behind > 50                                          # the case is what it claims to be; the device's counts equal the oracle's


# ---- 6. order and compaction ------------------------------------------------------------------------------------------------------------------------------
def test_nothing_kept_and_everything_kept():
    from envgs_amd import mesh
    base = cases.shape_case(17, 31, 3, 0)
    cams = _cameras(base)
    for fill, n in ((0.0, 0), (2.5, 3 * 17 * 31)):
        depth = torch.full((3, 17, 31), fill, dtype=torch.float32, device=DEV)
        pts, col, nrm, idx = mesh.fuse_depth_points(depth, cams, sources=base.sources, return_index=True)
        assert pts.shape == (n, 3) and col is None and nrm is None and idx.shape == (n,)
        assert torch.equal(idx.cpu(), torch.arange(n))
        if n:
            want, bound = fo.points(np.full((3, 17, 31), fill), base.K, base.R, base.T, np.arange(n), 0.0)
            assert (np.abs(pts.cpu().numpy() - want) <= bound).all()
    assert mesh.fuse_depth_points(depth, cams, sources=base.sources)[1:] == (None, None)


# ---- 7. the C ABI on guarded buffers ----------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _guarded(n, dtype):
    """A buffer of n elements between two runs of canary bytes -> (whole, payload view)."""
    size = torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((2 * GUARD + n * size + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + n * size].view(dtype)


def _untouched(whole):
    return bool((whole == 0xA5).all())


def _guards_intact(whole, n_bytes):
    return bool((whole[:GUARD] == 0xA5).all()) and bool((whole[GUARD + n_bytes:] == 0xA5).all())


def test_c_abi_on_guarded_buffers():
    from envgs_amd import _lib, mesh
    lib = _lib.load()
    c = cases.shape_case(17, 31, 3, 2)
    V, H, W = c.depth.shape
    n = V * H * W
    depth = torch.from_numpy(c.depth).to(DEV)
    p, s = _lib.ptr, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    K, R, T = c.K, c.R, c.T

    def pack(r, srcs, H_=H, W_=W):
        ps = _lib.FuseSources()
        ps.count = len(srcs)
        all_fwd, all_back = mesh.fuse_pair_maps(K, R, T, np.array([srcs if v == r else [(v + 1) % V] * len(srcs) for v in range(V)], np.int64))
        for q, j in enumerate(srcs):
            fwd, back = all_fwd[r, q], all_back[r, q]
            ps.v[q].depth, ps.v[q].H, ps.v[q].W = depth[j].data_ptr(), H_, W_
            ps.v[q].fwd, ps.v[q].back = (ctypes.c_float * 12)(*fwd), (ctypes.c_float * 12)(*back)
        return ps

    cnt_w, cnt = _guarded(n, torch.uint8)
    sum_w, tot = _guarded(n, torch.float32)
    # every invalid call is rejected and writes nothing
    good = pack(0, [1, 2])
    nine, minus, null_src, other_size = pack(0, [1, 2]), pack(0, [1, 2]), pack(0, [1, 2]), pack(0, [1, 2], W_=W - 1)
    nine.count, minus.count = 9, -1
    null_src.v[1].depth = None
    for args in ((H, W, p(depth[0]), nine), (H, W, p(depth[0]), minus), (H, W, p(depth[0]), null_src), (H, W, p(depth[0]), other_size),
                 (0, W, p(depth[0]), good), (H, 0, p(depth[0]), good), (65536, 65536, p(depth[0]), good), (H, W, None, good), (H, W, p(depth[0]), None)):
        assert lib.envgs_fuse_consistency(*args, 1.0, 0.01, 0, p(cnt), p(tot), s) == BAD_ARG
    assert lib.envgs_fuse_consistency(H, W, p(depth[0]), good, 1.0, 0.01, 0, None, p(tot), s) == BAD_ARG
    assert lib.envgs_fuse_consistency(H, W, p(depth[0]), good, 1.0, 0.01, 0, p(cnt), None, s) == BAD_ARG
    torch.cuda.synchronize()
    assert _untouched(cnt_w) and _untouched(sum_w)
    # the valid calls: one per view, inside the guards
    for r in range(V):
        assert lib.envgs_fuse_consistency(H, W, p(depth[r]), pack(r, [int(j) for j in c.sources[r]]), 1.0, 0.01, 0, p(cnt[r * H * W:]), p(tot[r * H * W:]), s) == 0
    want = fo.consistency(c.depth, K, R, T, c.sources, band=cases.golden().band)
    keep = ~want.fragile.reshape(-1)
    assert _guards_intact(cnt_w, n) and _guards_intact(sum_w, 4 * n)
    assert np.array_equal(cnt.cpu().numpy()[keep], want.count.reshape(-1)[keep])
    # count / emit
    tb = lib.envgs_fuse_temp_bytes(V, H, W)
    assert tb > 0 and lib.envgs_fuse_temp_bytes(0, H, W) == 0 and lib.envgs_fuse_temp_bytes(V, 65536, 65536) == 0 and lib.envgs_fuse_temp_bytes(4, 32768, 16384) == 0
    temp = torch.empty(tb + 16, dtype=torch.uint8, device=DEV)
    avg_w, avg = _guarded(n, torch.float32)
    fin_w, fin = _guarded(n, torch.uint8)
    tot_w, total = _guarded(1, torch.int64)
    d = p(depth)
    for args in ((0, H, W, d, p(cnt), p(tot), 2, 0.0, p(avg), p(fin), p(temp), tb, p(total)), (V, H, W, None, p(cnt), p(tot), 2, 0.0, p(avg), p(fin), p(temp), tb, p(total)),
                 (V, H, W, d, None, p(tot), 2, 0.0, p(avg), p(fin), p(temp), tb, p(total)), (V, H, W, d, p(cnt), p(tot), 2, 0.0, None, p(fin), p(temp), tb, p(total)),
                 (V, H, W, d, p(cnt), p(tot), 2, 0.0, p(avg), p(fin), None, tb, p(total)), (V, H, W, d, p(cnt), p(tot), 2, 0.0, p(avg), p(fin), p(temp[4:]), tb, p(total)),
                 (V, H, W, d, p(cnt), p(tot), 2, 0.0, p(avg), p(fin), p(temp), tb, None)):
        assert lib.envgs_fuse_count(*args, s) == BAD_ARG
    assert lib.envgs_fuse_count(V, H, W, d, p(cnt), p(tot), 2, 0.0, p(avg), p(fin), p(temp), tb - 1, p(total), s) == TEMP_TOO_SMALL
    torch.cuda.synchronize()
    assert _untouched(avg_w) and _untouched(fin_w) and _untouched(tot_w)
    assert lib.envgs_fuse_count(V, H, W, d, p(cnt), p(tot), 2, 0.0, p(avg), p(fin), p(temp), tb, p(total), s) == 0
    N = int(total.item())
    assert _guards_intact(avg_w, 4 * n) and _guards_intact(fin_w, n) and _guards_intact(tot_w, 8)
    assert N == int(fin.sum()) and 0 < N < n
    maps = torch.from_numpy(mesh.fuse_view_maps(K, R, T).astype(np.float32)).to(DEV)
    rgb = torch.from_numpy(_maps(V, H, W, 4)[0]).to(DEV)
    pts_w, pts = _guarded(3 * N, torch.float32)
    col_w, col = _guarded(3 * N, torch.float32)
    idx_w, idx = _guarded(N, torch.int64)
    for args in ((V, H, W, p(avg), p(fin), p(temp), tb, p(maps), None, None, n + 1, p(pts), None, None, None),          # more rows than pixels
                 (V, H, W, p(avg), p(fin), p(temp), tb, p(maps), None, None, N, p(pts), p(col), None, None),              # colours without their map
                 (V, H, W, p(avg), p(fin), p(temp), tb, p(maps), None, None, N, p(pts), None, p(col), None),              # normals without their map
                 (V, H, W, p(avg), p(fin), p(temp), tb, None, None, None, N, p(pts), None, None, None),
                 (V, H, W, p(avg), p(fin), p(temp), tb, p(maps), None, None, N, None, None, None, None),
                 (V, H, W, None, p(fin), p(temp), tb, p(maps), None, None, N, p(pts), None, None, None),
                 (V, 0, W, p(avg), p(fin), p(temp), tb, p(maps), None, None, N, p(pts), None, None, None)):
        assert lib.envgs_fuse_emit(*args, s) == BAD_ARG
    assert lib.envgs_fuse_emit(V, H, W, p(avg), p(fin), p(temp), tb - 1, p(maps), None, None, N, p(pts), None, None, None, s) == TEMP_TOO_SMALL
    torch.cuda.synchronize()
    assert _untouched(pts_w) and _untouched(col_w) and _untouched(idx_w)
    # NULL optional pointers are allowed: points alone, then everything
    assert lib.envgs_fuse_emit(V, H, W, p(avg), p(fin), p(temp), tb, p(maps), None, None, N, p(pts), None, None, None, s) == 0
    alone = pts.clone()
    assert _guards_intact(pts_w, 12 * N) and _untouched(col_w) and _untouched(idx_w)
    assert lib.envgs_fuse_emit(V, H, W, p(avg), p(fin), p(temp), tb, p(maps), p(rgb), None, N, p(pts), p(col), None, p(idx), s) == 0
    assert _guards_intact(pts_w, 12 * N) and _guards_intact(col_w, 12 * N) and _guards_intact(idx_w, 8 * N)
    assert torch.equal(alone, pts) and torch.equal(idx, fin.nonzero().reshape(-1))
    # a smaller N than counted: the rows beyond it are left alone
    pts.fill_(7.0)
    assert lib.envgs_fuse_emit(V, H, W, p(avg), p(fin), p(temp), tb, p(maps), None, None, N - 1, p(pts), None, None, None, s) == 0
    assert torch.equal(pts[:3 * (N - 1)], alone[:3 * (N - 1)]) and bool((pts[3 * (N - 1):] == 7.0).all())


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------------------------------
def test_fuse_surfel_points_end_to_end(tmp_path):
    from envgs_amd import ckpt, mesh, synth
    from tests.test_mesh_gpu import _sphere_surfels
    band = cases.golden().band
    rig = cases.arc_rig(4, 32, 32, f=64.0, distance=3.0)
    cams = [synth.make_camera(rig.K[v], rig.R[v], rig.T[v], 32, 32, 0.5, 6.0, device=DEV) for v in range(4)]
    surfels = _sphere_surfels()
    # geo_rel_thresh 0.03, not the script's 0.01: a surfel's Gaussian spans two pixels here, so two views blend the sphere's depth differently by
    # about 1 % -- at 0.01 the threshold cuts through the bulk and 7.3 % of the pixels are fragile (measured on these maps; 0.29 % at 0.03)
    kw = dict(n_srcs=3, geo_rel_thresh=0.03)
    cloud, maps = mesh.fuse_surfel_points(cams, surfels, sh_degree=0, alpha_min=0.5, **kw)
    assert len(maps) == 4 and all(m.normal.shape == (3, 32, 32) and m.rgb.shape == (3, 32, 32) for m in maps)
    depth = np.stack([m.depth.cpu().numpy() for m in maps])
    alpha = np.stack([m.alpha.cpu().numpy() for m in maps])
    assert (depth[alpha <= 0.5] == 0).all() and (depth > 0).mean() > 0.1
    # the cloud is the oracle applied to the maps it returned
    src = mesh.nearest_views(cams, 3).numpy()
    want = fo.consistency(depth, rig.K, rig.R, rig.T, src, band=band, geo_rel_thresh=kw["geo_rel_thresh"])
    N = cloud.points.shape[0]
    final = np.zeros(4 * 32 * 32, bool)
    final[cloud.index.cpu().numpy()] = True
    share = float(want.fragile.mean())
    print("end to end: %d points, fragile %.3f %%" % (N, 100 * share))
    assert share <= 0.01 and N > 100
    assert np.array_equal(final.reshape(4, 32, 32)[~want.fragile_final], want.final_mask[~want.fragile_final])
    idx = cloud.index.cpu().numpy()
    pts, bound = fo.points(want.depth_avg, rig.K, rig.R, rig.T, idx, band)
    keep = ~want.fragile.reshape(-1)[idx]
    assert (np.abs(cloud.points.cpu().numpy() - pts) <= bound)[keep].all()
    v, r = idx // 1024, idx % 1024
    rgb = np.stack([m.rgb.cpu().numpy() for m in maps]).reshape(4, 3, 1024)
    nrm = np.stack([m.normal.cpu().numpy() for m in maps]).reshape(4, 3, 1024)
    assert np.array_equal(cloud.colors.cpu().numpy(), rgb[v, :, r]) and np.array_equal(cloud.normals.cpu().numpy(), nrm[v, :, r])
    # the rendered normal, in world space, points out of the sphere and towards the camera side
    n_unit = cloud.normals / cloud.normals.norm(dim=1, keepdim=True).clamp_min(1e-12)
    radial = cloud.points / cloud.points.norm(dim=1, keepdim=True)
    assert float((n_unit * radial).sum(1).abs().median()) > 0.9
    # the cloud goes straight into the evaluation: against itself every distance is zero
    score = mesh.evaluate(cloud.points, cloud.points, max_distance=0.1, threshold=0.01)
    assert score.accuracy == 0.0 and score.completeness == 0.0 and score.fscore == 1.0 and score.n_pred == N
    path = str(tmp_path / "cloud.ply")
    ckpt.save_points_ply(path, cloud.points, cloud.colors, cloud.normals)
    p, c, n = ckpt.load_points_ply(path)
    assert np.array_equal(p, cloud.points.cpu().numpy()) and np.array_equal(n, cloud.normals.cpu().numpy())
    assert np.array_equal(c, np.rint(np.clip(cloud.colors.cpu().numpy().astype(np.float64), 0, 1) * 255).astype(np.uint8))
