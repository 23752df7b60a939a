"""GPU: the DTU protocol (csrc/mesh_eval.hip: thinning and culling; envgs_amd.mesh.thin_points / cull_to_masks / in_box / in_volume / above_plane /
evaluate_dtu) against the independent oracle (tests/mesh_thin_oracle.py).  Every comparison of masks is exact -- `keep` is a function of the points,
the radius and the keys alone -- and every product call runs twice and must give identical bytes.  PARITY UNPINNED (DESIGN.md "DTU protocol")."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_thin_cases as tc
from tests import mesh_thin_oracle as to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CANARY = 0x5A
BELOW = lambda x: float(np.nextafter(F32(x), F32(0)))


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def check_thin(points, radius, seed, want=None, cell_size=None, label=""):
    """thin_points twice: identical bytes, equal to the oracle's loop.  -> (keep NumPy, rounds)"""
    from envgs_amd import mesh
    p = _t(np.asarray(points, F32).reshape(-1, 3))
    want = to.thin(points, radius, seed) if want is None else want
    for run in range(2):
        keep, rounds = mesh.thin_points(p, radius, seed=seed, cell_size=cell_size, return_rounds=True)
        assert keep.dtype == torch.bool and tuple(keep.shape) == want.shape, (label, run)
        bad = np.flatnonzero(_np(keep) != want)
        assert bad.size == 0, (label, run, seed, cell_size, bad[:8], want[bad[:8]])
        assert 0 <= rounds <= max(p.shape[0], 0)
    assert torch.equal(mesh.thin_points(p, radius, seed=seed, cell_size=cell_size), keep)
    return _np(keep), rounds


# ---- 1. small counts --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000])
def test_small_counts(N):
    points = tc.cube(N, 100 + N)
    radius = tc.cube_radius(max(N, 8), 6)
    for seed in (0, 1, None):
        keep, rounds = check_thin(points, radius, seed, label="N %d" % N)
        assert keep.shape == (N,) and (N == 0 or keep.any()) and (rounds > 0) == (N > 0)


# ---- 2. the cell size changes nothing -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cloud():
    points, radius = tc.cube(5000, 81), tc.cube_radius(5000, 8)
    return points, radius, {seed: to.thin(points, radius, seed) for seed in (0, None)}


@pytest.mark.parametrize("cell", ["radius / 4", "default", "3 radius", "one cell"])
def test_random_cloud_at_every_cell_size(cell):
    points, radius, want = _cloud()
    cell_size = {"radius / 4": radius / 4, "default": None, "3 radius": 3 * radius, "one cell": 2.0}[cell]
    for seed in (0, None):
        keep, _ = check_thin(points, radius, seed, want=want[seed], cell_size=cell_size, label=cell)
        assert 0.1 < keep.mean() < 0.9


# ---- 3. the inclusive bound, where d2 is exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1.0, BELOW(1.0), 2.0, BELOW(2.0)])
def test_lattice(radius):
    base = tc.lattice()
    for points, cell_size in ((base, 1.0), (base, None), (base * F32(0.5) + F32(3.5), 0.5)):      # cell 1 / 0.5: every point on a cell wall
        r = radius if cell_size != 0.5 else radius * 0.5         # the halved copy: halves and quarters, still exact
        for seed in (0, None):
            keep, _ = check_thin(points, r, seed, cell_size=cell_size, label="lattice r %r cell %r" % (r, cell_size))
            if radius < 1.0:
                assert keep.all()                                  # one step below the spacing: nobody has a neighbour
            if radius == 1.0:
                assert not keep.all()
    if radius in (1.0, 2.0):                                      # the bound is inclusive: the step below keeps strictly more
        assert to.thin(base, radius, 0).sum() < to.thin(base, BELOW(radius), 0).sum()


# ---- 4, 5. duplicates, rows that are not finite, one dense cluster ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, None])
def test_duplicates_and_non_finite_rows_at_radius_zero(seed):
    points, which = tc.duplicates()
    keep, _ = check_thin(points, 0.0, seed, label="duplicates")
    key = to.keys(points.shape[0], seed)
    assert keep.sum() == 50 and not keep[which < 0].any()
    for pos in range(50):
        rows = np.flatnonzero(which == pos)
        assert keep[rows].sum() == 1 and keep[rows[np.argmin(key[rows])]]
    none = np.full((70, 3), np.nan, F32)
    keep, rounds = check_thin(none, 1.0, seed, label="no finite point")
    assert not keep.any() and rounds == 0


@pytest.mark.parametrize("seed", [0, None])
def test_one_cluster_has_one_survivor(seed):
    points = tc.cluster()
    keep, _ = check_thin(points, 0.1, seed, label="cluster")
    assert keep.sum() == 1 and keep[np.argmin(to.keys(points.shape[0], seed))]


# ---- 6. the adversarial order ---------------------------------------------------------------------------------------------------------------------------------------
def test_collinear_points_in_index_order_and_hashed():
    points = tc.collinear()
    keep, rounds = check_thin(points, tc.COLLINEAR_RADIUS, None, label="collinear, index order")
    assert keep.sum() == 300 and keep[::2].all() and 1 <= rounds <= tc.COLLINEAR_N
    keep, rounds = check_thin(points, tc.COLLINEAR_RADIUS, 0, label="collinear, seed 0")
    print("collinear: %d rounds under the hash order" % rounds)
    assert rounds <= 12


# ---- 7, 8. large coordinates; a surface ---------------------------------------------------------------------------------------------------------------------------------
def test_large_coordinates_small_radius():
    points = tc.offset_cloud()
    for seed in (0, None):
        keep, _ = check_thin(points, 0.01, seed, label="offset 1000")
        assert 0.3 < keep.mean() < 0.95
    check_thin(points, 0.01, 0, cell_size=0.004, label="offset 1000, cell 0.004")


def test_surface_samples_at_their_mean_spacing():
    points, spacing = tc.torus(6000)
    keep, rounds = check_thin(points, spacing, 0, label="torus")
    print("torus: kept %d of %d in %d rounds" % (keep.sum(), keep.shape[0], rounds))
    assert 0.2 < keep.mean() < 0.8 and rounds <= 16
    check_thin(points, spacing, None, label="torus, index order")


# ---- 9. the C-ABI: canaries and the caller's stream ---------------------------------------------------------------------------------------------------------------------
def _guarded(rows, width, dtype, pad, fill=None):
    size = torch.empty(0, dtype=dtype).element_size()
    buf = torch.full(((rows + 2 * pad) * width * size,), CANARY, dtype=torch.uint8, device=DEV).view(dtype)
    if fill is not None:
        buf[pad * width:(pad + rows) * width] = torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)).to(DEV)
    return buf


def _untouched(buf, width, rows, pad):
    b, e = buf.view(torch.uint8), buf.element_size()
    return bool((b[:pad * width * e] == CANARY).all()) and bool((b[(pad + rows) * width * e:] == CANARY).all())


def _raw_thin(points, radius, seed, cell, group, pad=64, stream=None):
    """The grid and the four thinning calls of the C-ABI on canary-guarded buffers; the scratch is canary-filled too, and the bytes between its
    parts (state | worklist | worklist | counters, each rounded up to 256 B) and after it must survive."""
    from envgs_amd import _lib
    lib = _lib.load()
    N = points.shape[0]
    lo = points.min(axis=0)
    dims = [int(math.floor((float(h) - float(l)) / cell)) + 1 for l, h in zip(lo, points.max(axis=0))]
    cells = math.prod(dims)
    shells = 0
    while F32(F32(F32(shells) * F32(cell)) * F32(0.9990234375)) < F32(radius) and shells < max(dims) - 1:
        shells += 1
    p = _guarded(N, 3, torch.float32, pad, points)
    ce, rec = _guarded(cells, 1, torch.int32, pad), _guarded(N, 4, torch.float32, pad)
    keep, count = _guarded(N, 1, torch.uint8, pad), _guarded(2, 1, torch.int32, pad)
    at = lambda buf, width: _lib.ctypes.c_void_p(buf.data_ptr() + pad * width * buf.element_size())
    s = _lib.ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream.cuda_stream)
    o = [float(x) for x in lo]
    gb = lib.envgs_points_grid_temp_bytes(N, *dims)
    gtemp = torch.empty(gb, dtype=torch.uint8, device=DEV)
    assert lib.envgs_points_grid_build(N, at(p, 3), o[0], o[1], o[2], cell, *dims, _lib.ptr(gtemp), gb, at(ce, 1), at(rec, 4), s) == 0
    tb = lib.envgs_points_thin_temp_bytes(N)
    part = (4 * N + 255) // 256 * 256
    assert tb == 3 * part + 256
    temp = torch.full((tb + 512,), CANARY, dtype=torch.uint8, device=DEV)
    toff = (-temp.data_ptr()) % 256
    tp = _lib.ctypes.c_void_p(temp.data_ptr() + toff)
    assert lib.envgs_points_thin_begin(N, at(p, 3), tp, tb, at(count, 1), s) == 0
    undecided, launched, rounds = N, 0, 0
    while undecided:
        assert launched <= N
        assert lib.envgs_points_thin_round(N, at(p, 3), radius, int(seed is not None), seed or 0, o[0], o[1], o[2], cell, *dims, shells, at(ce, 1), at(rec, 4),
                                           tp, tb, launched, group, undecided, at(count, 1), s) == 0
        launched += group
        torch.cuda.synchronize()
        undecided, rounds = count[pad:pad + 2].tolist()
    assert lib.envgs_points_thin_keep(N, tp, tb, at(keep, 1), s) == 0
    torch.cuda.synchronize()
    assert _untouched(keep, 1, N, pad) and _untouched(count, 1, 2, pad) and _untouched(p, 3, N, pad) and _untouched(ce, 1, cells, pad) and _untouched(rec, 4, N, pad)
    body = temp[toff:toff + tb]
    assert bool((temp[:toff] == CANARY).all()) and bool((temp[toff + tb:] == CANARY).all())
    for k in range(3):                                            # after the states and after either worklist
        assert bool((body[k * part + 4 * N:(k + 1) * part] == CANARY).all()), "the scratch was written beyond row N of part %d" % k
    assert bool((body[3 * part + 16:] == CANARY).all())
    state = body[:4 * N].view(torch.int32)
    assert int(state.min()) >= 1 and int(state.max()) <= 2        # every point is KEPT or DROPPED
    return keep[pad:pad + N].cpu().numpy().astype(bool), rounds


def test_thinning_writes_nothing_outside_the_documented_rows_and_runs_on_the_callers_stream():
    points, radius, want = _cloud()
    points = points[:4999]                                        # 4 x 4999 is no multiple of 256: the parts of the scratch have gaps
    want0 = to.thin(points, radius, 0)
    rounds = {}
    for group in (1, 4):
        for _ in range(2):
            keep, rounds[group] = _raw_thin(points, radius, 0, radius * 1.5, group)
            assert np.array_equal(keep, want0)
    print("rounds, one per read-back: %d; four per read-back: %d" % (rounds[1], rounds[4]))      # what a lane sees of its own launch may save a round, never change a result
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        check_thin(points, radius, 0, want=want0, label="side stream")
    side.synchronize()
    keep, _ = _raw_thin(points, radius, None, radius * 1.5, 4, stream=side)
    assert np.array_equal(keep, to.thin(points, radius, None))


def test_bad_arguments_are_rejected():
    from envgs_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(8192, dtype=torch.uint8, device=DEV)
    p = _lib.ptr(buf)
    odd = _lib.ctypes.c_void_p(buf.data_ptr() + 4)
    assert lib.envgs_points_thin_temp_bytes(2 ** 31) == 0 and lib.envgs_points_thin_temp_bytes(0) == 256
    assert lib.envgs_points_thin_begin(1, None, p, 8192, p, None) == -1
    assert lib.envgs_points_thin_begin(1, p, odd, 8188, p, None) == -1
    assert lib.envgs_points_thin_begin(1, p, p, 16, p, None) == -2
    round_ = lambda radius=1.0, cell=1.0, nx=2, shells=1, temp=p, tb=8192: lib.envgs_points_thin_round(1, p, radius, 1, 0, 0, 0, 0, cell, nx, 2, 2, shells, p, p, temp, tb,
                                                                                                 0, 1, 1, p, None)
    assert round_(radius=-1.0) == -1 and round_(radius=float("inf")) == -1 and round_(radius=float("nan")) == -1
    assert round_(cell=0.0) == -1 and round_(nx=1025) == -1 and round_(shells=-1) == -1 and round_(shells=1024) == -1
    assert round_(temp=odd) == -1 and round_(tb=16) == -2
    assert lib.envgs_points_thin_keep(1, p, 8192, None, None) == -1 and lib.envgs_points_thin_keep(1, p, 16, p, None) == -2
    views = _lib.CullViews()
    views.count = 9
    assert lib.envgs_mesh_cull_vertices(1, p, views, 0, p, None) == -1
    views.count = 1                                               # a NULL mask
    assert lib.envgs_mesh_cull_vertices(1, p, views, 0, p, None) == -1
    assert lib.envgs_mesh_cull_faces(2 ** 31, 1, p, p, p, None) == -1 and lib.envgs_mesh_cull_faces(3, 1, None, p, p, None) == -1
    torch.cuda.synchronize()


# ---- 10. a large cloud, by its two defining properties ------------------------------------------------------------------------------------------------------------------
def test_two_hundred_thousand_samples_are_independent_and_maximal():
    from envgs_amd import mesh
    pts, spacing = tc.torus(200000)
    p = _t(pts)
    keep, rounds = mesh.thin_points(p, spacing, seed=3, return_rounds=True)
    again = mesh.thin_points(p, spacing, seed=3)
    assert torch.equal(keep, again)
    kept, dropped = p[keep].contiguous(), p[~keep].contiguous()
    print("200 000 samples: kept %d in %d rounds" % (kept.shape[0], rounds))
    assert 0.2 < kept.shape[0] / p.shape[0] < 0.8 and rounds <= 24
    _, idx = mesh.PointGrid(kept, spacing).nearest(dropped)       # maximal: every dropped point has a kept one within the radius
    assert bool((idx >= 0).all())
    r2 = torch.tensor(spacing, dtype=torch.float32, device=DEV) ** 2
    pairs = 0
    for s in range(0, kept.shape[0], 1024):                       # independent: within the radius of a kept point lies no kept point but itself
        a = kept[s:s + 1024]
        dx, dy, dz = (a[:, None, e] - kept[None, :, e] for e in range(3))
        pairs += int((((dx * dx) + (dy * dy)) + (dz * dz) <= r2).sum())
    assert pairs == kept.shape[0]


# ---- 11. culling ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _look_at(eye, target):
    z = np.asarray(target, np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R.astype(F32), (-R @ np.asarray(eye, np.float64)).astype(F32)


@functools.lru_cache(maxsize=None)
def _cull_case(n_views):
    rng = np.random.default_rng(90 + n_views)
    H, W = 30, 41
    K = np.array([[35, 0, 20.5], [0, 35, 15], [0, 0, 1]], F32)
    views, masks = [], []
    for i in range(n_views):
        a = 2 * math.pi * i / n_views
        R, T = _look_at([3 * math.cos(a), 3 * math.sin(a), 0.7 + 0.1 * i], [0, 0, 0])
        views.append((K, R, T))
        yy, xx = np.mgrid[:H, :W]
        masks.append(((xx - 20) ** 2 + (yy - 14.5) ** 2 <= (9 + i) ** 2).astype(np.uint8))      # a disc, a different one per view
    # view 0 by hand: identity rotation at the origin, so that the roles below can be placed exactly
    views[0] = (np.array([[10, 0, 4], [0, 10, 3], [0, 0, 1]], F32), np.eye(3, dtype=F32), np.zeros(3, F32))
    masks[0] = np.zeros((H, W), np.uint8)
    masks[0][:, 4:] = 1
    hand = np.array([[0, 0, -1], [0, 0, 0], [-1, 0, 1], [0.5, 2.69, 1], [0.5, 2.7, 1], [-0.01, 0, 1], [0, 0, 1], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf]], F32)
    #               behind     zc = 0     off image   last pixel row  row H or H-1    px 3: out      px 4: in   not finite
    v = np.concatenate([hand, rng.uniform(-1.2, 1.2, (2000, 3)).astype(F32)])
    f = rng.integers(0, v.shape[0], (6000, 3)).astype(np.int32)
    f[:10] = [[i, (i + 1) % 10, 10 + i] for i in range(10)]
    f[17], f[18] = [-1, 3, 4], [1, v.shape[0], 2]
    colors = rng.random(v.shape, dtype=F32)
    vk = to.cull_vertices(v, views, masks)
    want = to.select_faces(v, f, colors, to.cull_faces(v.shape[0], f, vk))
    return SimpleNamespace(vertices=v, faces=f, colors=colors, views=views, masks=np.stack(masks), vertex_keep=vk, want=want)


@pytest.mark.parametrize("n_views", [1, 3, 9])
def test_cull_to_masks(n_views):
    from envgs_amd import mesh
    c = _cull_case(n_views)
    first = to.cull_vertices(c.vertices[:10], c.views[:1], c.masks[:1]).tolist()      # the hand-placed roles, in the view they were placed for
    assert first[:4] == [True, True, True, True] and first[5:] == [False, True, False, False, False]
    assert 0.02 < c.vertex_keep.mean() < 0.98 and 0 < c.want.faces.shape[0] < c.faces.shape[0]
    dm = mesh.Mesh(vertices=_t(c.vertices), faces=_t(c.faces), colors=_t(c.colors))
    cams = [SimpleNamespace(K=torch.from_numpy(K), R=torch.from_numpy(R), T=torch.from_numpy(T)) for K, R, T in c.views]
    for masks in (_t(c.masks), _t(c.masks.astype(bool))):
        for run in range(2):
            got, index = mesh.cull_to_masks(dm, cams, masks, return_index=True)
            assert np.array_equal(_np(index), c.want.index) and np.array_equal(_np(got.faces), c.want.faces)
            assert np.array_equal(_np(got.vertices).view(np.uint32), c.want.vertices.view(np.uint32))
            assert np.array_equal(_np(got.colors).view(np.uint32), c.want.colors.view(np.uint32))
    plain = mesh.cull_to_masks(dm, cams, _t(c.masks))
    assert torch.equal(plain.faces, got.faces)
    keep = torch.from_numpy(to.cull_faces(c.vertices.shape[0], c.faces, c.vertex_keep)).to(DEV)
    same = mesh.select_faces(dm, keep)                            # the face and vertex order is that of select_faces on the oracle's mask
    assert torch.equal(same.faces, got.faces) and torch.equal(same.vertices.view(torch.int32), got.vertices.view(torch.int32))
    with pytest.raises(ValueError):
        mesh.cull_to_masks(dm, cams + cams[:1], _t(c.masks))


# ---- 12. the protocol ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_filters_against_the_oracle():
    from envgs_amd import mesh
    rng = np.random.default_rng(95)
    p = rng.uniform(-0.2, 1.2, (4000, 3)).astype(F32)
    p[:64] = np.round(p[:64] * 32) / 32                           # rows on the lattice of half voxels: every other one a tie of rint
    p[64:70] = [[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5]]
    vol = rng.random((16, 16, 16)) < 0.6
    origin, voxel = (0.125, 0.0, -0.0625), 0.0625
    plane = (0.25, -0.5, 1.0, -0.375)
    d = _t(p)
    for _ in range(2):
        assert np.array_equal(_np(mesh.in_box(d, (0, 0, 0), (1, 1, 1))), to.in_box(p, (0, 0, 0), (1, 1, 1)))
        assert np.array_equal(_np(mesh.in_volume(d, _t(vol), origin, voxel)), to.in_volume(p, vol, origin, voxel))
        assert np.array_equal(_np(mesh.in_volume(d, _t(vol.astype(np.uint8)), origin, 0.07)), to.in_volume(p, vol, origin, 0.07))
        assert np.array_equal(_np(mesh.above_plane(d, plane)), to.above_plane(p, plane))
    assert 0.1 < to.in_volume(p, vol, origin, voxel).mean() < 0.9 and 0.1 < to.above_plane(p, plane).mean() < 0.9


@functools.lru_cache(maxsize=None)
def _dtu_case():
    rng = np.random.default_rng(96)
    pred = rng.random((3000, 3), dtype=F32)
    scan = (rng.random((2500, 3), dtype=F32) * F32(0.9) + F32(0.05))
    kw = dict(radius=0.05, max_distance=0.04, seed=5, observed=(rng.random((16, 16, 16)) < 0.7, (0.1, 0.1, 0.1), 0.05), box=((0.05, 0.05, 0.05), (0.95, 0.9, 0.95)),
              plane=(0.0, 0.1, 1.0, -0.3), threshold=0.025)
    return pred, scan, kw, to.evaluate_dtu(pred, scan, **kw)


COUNTS = ("n_samples", "n_thinned", "n_in", "n_pred", "n_scan", "n_ref", "found_pred", "found_ref", "within_pred", "within_ref")
METRICS = ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore")


def test_evaluate_dtu_against_the_oracle():
    from envgs_amd import mesh
    pred, scan, kw, want = _dtu_case()
    assert want.n_samples > want.n_thinned > want.n_in > want.n_pred > want.found_pred > 0 and want.n_scan > want.n_ref > want.found_ref > 0
    dkw = {**kw, "observed": (_t(kw["observed"][0]),) + kw["observed"][1:]}
    for _ in range(2):
        got = mesh.evaluate_dtu(_t(pred), _t(scan), **dkw)
        for k in COUNTS:
            assert getattr(got, k) == getattr(want, k), k
        for k in METRICS:                                         # float64 sums of at most 10^4 terms, added in two orders
            assert abs(getattr(got, k) - getattr(want, k)) <= 1e-9 * abs(getattr(want, k)), (k, getattr(got, k), getattr(want, k))
        assert np.allclose(_np(got.d_pred), want.d_pred, rtol=1e-15, atol=0) and np.allclose(_np(got.d_ref), want.d_ref, rtol=1e-15, atol=0)
    bare = mesh.evaluate_dtu(_t(pred), _t(scan), 0.05, 0.04, seed=5)
    assert not hasattr(bare, "fscore") and bare.n_in == bare.n_thinned == bare.n_pred == want.n_thinned and bare.n_ref == bare.n_scan


def test_evaluate_dtu_without_filters_reproduces_evaluate():
    from envgs_amd import mesh
    pred, scan, _, _ = _dtu_case()
    assert np.unique(pred, axis=0).shape[0] == pred.shape[0]
    a = mesh.evaluate_dtu(_t(pred), _t(scan), 0.0, 0.12, threshold=0.06)
    b = mesh.evaluate(_t(pred), _t(scan), 0.12, 0.06)
    assert a.n_samples == a.n_thinned == a.n_pred == b.n_pred and a.n_ref == b.n_ref
    for k in METRICS + ("found_pred", "found_ref", "within_pred", "within_ref"):
        assert getattr(a, k) == getattr(b, k), k
    assert torch.equal(a.d_pred, b.d_pred) and torch.equal(a.d_ref, b.d_ref)


def test_evaluate_dtu_on_a_mesh():
    from envgs_amd import mesh
    v = _t(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F32))
    m = mesh.Mesh(vertices=v, faces=_t(np.array([[0, 1, 2], [0, 2, 3]], np.int32)), colors=None)
    g = np.arange(0, 1.0001, 0.05)
    scan = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    samples = mesh.sample_surface(m, 4000.0, seed=2)[0]
    want = to.evaluate_dtu(_np(samples), scan, 0.03, 0.2, seed=2)
    got = mesh.evaluate_dtu(m, _t(scan), 0.03, 0.2, density=4000.0, seed=2)
    assert (got.n_samples, got.n_thinned, got.found_pred, got.found_ref) == (want.n_samples, want.n_thinned, want.found_pred, want.found_ref)
    assert got.n_thinned < got.n_samples and abs(got.chamfer - want.chamfer) <= 1e-9 * want.chamfer
    assert got.accuracy <= 0.05 * math.sqrt(2) / 2 + 1e-6         # no sample of the square is farther from the lattice than half a diagonal


# ---- 13. what raises --------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_value_errors():
    from envgs_amd import mesh
    p = _t(tc.cube(1000, 1100))
    for bad in (-1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError):
            mesh.thin_points(p, bad)
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError):
            mesh.thin_points(p, 0.1, seed=bad)
    with pytest.raises(ValueError, match="smallest admissible cell_size"):
        mesh.thin_points(p, 0.1, cell_size=1e-4)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            mesh.thin_points(p, 0.1, cell_size=bad)
    with pytest.raises(ValueError):
        mesh.evaluate_dtu(p, p, 0.1, 0.2, threshold=0.3)
    with pytest.raises(ValueError):
        mesh.evaluate_dtu(mesh.Mesh(vertices=p, faces=torch.zeros(1, 3, dtype=torch.int32, device=DEV), colors=None), p, 0.1, 0.2)      # a mesh needs a density
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.thin_points(torch.zeros(4, 3), 0.1)
    keep = mesh.thin_points(p, 1e-7)                              # a tiny radius: the default cell is raised until the grid limits hold
    assert bool(keep.all())
