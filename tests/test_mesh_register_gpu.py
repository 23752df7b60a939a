"""GPU: registration and the Tanks-and-Temples protocol (csrc/mesh_register.hip; envgs_amd.mesh.transform_points / register / voxel_downsample /
in_polygon_volume / evaluate_tnt) against the independent oracle (tests/mesh_register_oracle.py).  Matches, cells, masks and voxel means are compared
exactly; the 18 sums against math.fsum within a summation bound computed from the data; the registration against the truth within the oracle's own
deviation.  Every device buffer the front end allocates during a test stands between canary rows.  PARITY UNPINNED (DESIGN.md "Registration")."""
import contextlib
import functools
import json
import math

import numpy as np
import pytest
import torch

from tests import mesh_eval_oracle as eo
from tests import mesh_register_oracle as ro
from tests import mesh_simplify_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
CANARY, GUARD = 0x5A, 256


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


class _GuardedTorch:
    """Stands in for the `torch` name of envgs_amd.mesh: every torch.empty on the device comes out of a larger byte buffer filled with a canary."""

    def __init__(self):
        self.buffers = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=torch.float32, device=None):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        if device is None or torch.device(device).type != "cuda":
            return torch.empty(shape, dtype=dtype, device=device)
        nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device=device)
        self.buffers.append((raw, nbytes))
        return raw[GUARD:GUARD + nbytes].view(dtype).reshape(shape)

    def check(self):
        assert self.buffers
        for raw, nbytes in self.buffers:
            assert bool((raw[:GUARD] == CANARY).all()) and bool((raw[GUARD + nbytes:] == CANARY).all()), "a canary row around a %d-byte buffer" % nbytes


@contextlib.contextmanager
def guarded():
    from envgs_amd import mesh
    guard, real = _GuardedTorch(), mesh.torch
    mesh.torch = guard
    try:
        yield guard
    finally:
        mesh.torch = real
    guard.check()


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------------------------------------
SUM_T = ro.similarity((2, -1, 3), 4.0, (0.05, -0.02, 0.03), 1.01)


@functools.lru_cache(maxsize=None)
def _sum_target():
    return np.random.default_rng(40).uniform(-1, 1, (400, 3)).astype(F32)


def check_sums(source, target, T, max_distance, cell_size=None, label=""):
    """register_sums twice: identical bytes; n exact; the matches and the moved rows equal the oracle's bit for bit; every float sum within
    Q 2^-52 sum |term| of the exact sum.  -> the oracle's evaluation"""
    from envgs_amd import mesh
    source, target = np.asarray(source, F32).reshape(-1, 3), np.asarray(target, F32).reshape(-1, 3)
    Q = source.shape[0]
    want = ro.sums(source, target, T, max_distance, ro.center(target))
    runs = []
    with guarded():
        grid = mesh.PointGrid(_t(target), max_distance, cell_size)
        assert np.array_equal(np.array(grid.center), ro.center(target)), label
        for run in range(2):
            got, moved, dist2, index = mesh.register_sums(_t(source), grid, T, return_rows=True)
            runs.append((got.tobytes(), _np(moved).tobytes(), _np(dist2).tobytes(), _np(index).tobytes()))
        plain = mesh.register_sums(_t(source), grid, T)
        near = grid.nearest(moved)
    assert runs[0] == runs[1] and plain.tobytes() == runs[0][0], label
    assert got.dtype == F64 and got.shape == (18,)
    assert _np(moved).tobytes() == want.moved.tobytes(), label
    assert np.array_equal(_np(index), want.index) and _np(dist2).tobytes() == want.dist2.tobytes(), label
    assert torch.equal(near[0], dist2) and torch.equal(near[1], index), label            # the rule of envgs_points_nearest, by the kernel itself
    assert got[0] == want.n, (label, got[0], want.n)
    bound = ro.sums_bound(Q, want.abs)
    err = np.abs(got - want.sums)
    print("%s: Q %d n %d, largest error / bound %.3g" % (label, Q, want.n, float((err[1:] / np.maximum(bound[1:], 1e-300)).max()) if want.n else 0.0))
    assert (err[1:] <= bound[1:]).all(), (label, err, bound)
    return want


@pytest.mark.parametrize("Q", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 773, 65793])
def test_sums_at_every_size(Q):
    source = np.random.default_rng(100 + Q).uniform(-1.1, 1.1, (Q, 3)).astype(F32)
    want = check_sums(source, _sum_target(), SUM_T, 0.25, label="Q %d" % Q)
    assert Q < 63 or 0 < want.n < Q                               # matched and unmatched rows both occur


def test_sums_with_rows_that_are_not_finite():
    rng = np.random.default_rng(41)
    source = rng.uniform(-1, 1, (700, 3)).astype(F32)
    target = _sum_target().copy()
    source[::7, 0] = np.nan
    source[3::11, 2] = np.inf
    source[5::13] = -np.inf
    target[::5, 1] = np.nan
    target[2::9] = np.inf
    want = check_sums(source, target, SUM_T, 0.3, label="not finite")
    assert 0 < want.n < 700 and (want.index[::7] == -1).all()


def test_sums_without_any_match_and_on_an_empty_target():
    source = np.random.default_rng(42).uniform(-1, 1, (300, 3)).astype(F32)
    far = ro.similarity((0, 0, 1), 0.0, (10.0, 0.0, 0.0))
    for target, T, label in ((_sum_target(), far, "far"), (np.zeros((0, 3), F32), SUM_T, "empty target")):
        want = check_sums(source, target, T, 0.25, label=label)
        assert want.n == 0 and not want.sums.any()


@pytest.mark.parametrize("cell", [None, 0.05, 4.0])
def test_sums_at_distance_zero_on_coincident_clouds(cell):
    target = _sum_target()
    source = np.concatenate([target[::2], target[:50] + F32(0.001)])      # the identity moves nothing: 200 exact hits, 50 misses
    want = check_sums(source, target, np.eye(4), 0.0, cell_size=cell, label="coincident, cell %r" % cell)
    assert want.n == 200 and want.sums[1] == 0.0
    assert np.array_equal(want.index[:200], np.arange(0, 400, 2))


def test_bad_arguments_are_rejected_before_any_gpu_work():
    import ctypes
    from envgs_amd import _lib
    lib = _lib.load()
    M = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    nan = (ctypes.c_float * 12)(*([float("nan")] * 12))
    c = (ctypes.c_double * 3)(0, 0, 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = _lib.ptr(buf)
    assert lib.envgs_points_transform(4, p, None, p, None) == -1 and lib.envgs_points_transform(4, p, nan, p, None) == -1
    assert lib.envgs_points_transform(2 ** 31, p, M, p, None) == -1 and lib.envgs_points_transform(4, None, M, p, None) == -1
    ok = dict(Q=4, source=p, M=M, r=0.5, o=(0.0, 0.0, 0.0), cell=1.0, n=(1, 1, 1), ce=p, rec=p, c=c, temp=p, tb=4096, sums=p)
    call = lambda a: lib.envgs_points_register_sums(a["Q"], a["source"], a["M"], a["r"], *a["o"], a["cell"], *a["n"], a["ce"], a["rec"], a["c"], a["temp"],
                                                    a["tb"], a["sums"], None, None, None, None)
    for bad in (dict(M=None), dict(M=nan), dict(r=-1.0), dict(r=float("inf")), dict(cell=0.0), dict(n=(0, 1, 1)), dict(n=(1025, 1, 1)), dict(ce=None),
                dict(c=None), dict(temp=None), dict(sums=None), dict(source=None), dict(Q=2 ** 31)):
        assert call({**ok, **bad}) == -1, bad
    assert call({**ok, "tb": 16}) == -2
    assert lib.envgs_points_voxel_keys(4, p, 0.0, 0.0, 0.0, 1.0, 2 ** 21 + 1, 1, 1, p, None) == -1
    assert lib.envgs_points_voxel_keys(4, p, 0.0, 0.0, 0.0, float("nan"), 1, 1, 1, p, None) == -1
    assert lib.envgs_points_voxel_cluster(4, p, 0.0, 0.0, 0.0, 1.0, 1, 1, 1, p, p, p, 16, None, p, None) == -2
    assert lib.envgs_points_voxel_cluster(4, p, 0.0, 0.0, 0.0, 1.0, 1, 1, 1, p, p, p, 4096, None, None, None) == -1
    assert lib.envgs_points_voxel_finish(4, p, 0.0, 0.0, 0.0, 1.0, 1, 1, 1, p, 4096, 5, p, None) == -1
    for axis, M_, poly in ((3, 4, p), (-1, 4, p), (0, 2, p), (0, 257, p), (0, 4, None)):
        assert lib.envgs_points_in_polygon(4, p, axis, 0.0, 1.0, M_, poly, p, None) == -1
    assert lib.envgs_points_in_polygon(4, p, 0, float("nan"), 1.0, 4, p, p, None) == -1
    torch.cuda.synchronize()


# ---- 2. the registration ----------------------------------------------------------------------------------------------------------------------------------------
def _history_bytes(r):
    return b"".join(h.transformation.tobytes() + h.sums.tobytes() for h in r.history) + r.transformation.tobytes()


@functools.lru_cache(maxsize=None)
def _registered(name):
    """One product run and one oracle run per case, shared by the tests below and left unchanged."""
    from envgs_amd import mesh
    c = ro.cases()[name]
    with guarded():
        got = mesh.register(_t(c.source), _t(c.target), c.max_distance, with_scale=c.with_scale)
    want = ro.icp(c.source, c.target, c.max_distance, ro.center(c.target), with_scale=c.with_scale)
    return c, got, want


@pytest.mark.parametrize("cell", ["again", "max_distance / 4", "3 max_distance", "one cell"])
def test_register_gives_identical_bytes_at_every_cell_size(cell):
    from envgs_amd import mesh
    c, first, _ = _registered("cube")
    cell_size = {"again": None, "max_distance / 4": c.max_distance / 4, "3 max_distance": 3 * c.max_distance, "one cell": 4.0}[cell]
    grid = mesh.PointGrid(_t(c.target), c.max_distance, cell_size)
    assert (grid.dims == (1, 1, 1)) == (cell == "one cell")
    again = mesh.register(_t(c.source), grid, c.max_distance, with_scale=c.with_scale)      # the grid passed in, built once
    assert _history_bytes(again) == _history_bytes(first) and len(again.history) == len(first.history) > 2
    assert (again.fitness, again.inlier_rmse, again.iterations, again.converged) == (first.fitness, first.inlier_rmse, first.iterations, first.converged)
    with pytest.raises(ValueError):
        mesh.register(_t(c.source), grid, 2 * c.max_distance)


@pytest.mark.parametrize("name", ["cube", "cube+scale", "surface", "outliers"])
def test_the_chain_under_the_products_own_decisions(name):
    """For every k: the oracle's exact sums at the product's recorded T_k against the product's, and T_{k+1} = rigid_from_sums(sums_k) T_k to the bit."""
    from envgs_amd import mesh
    c, got, _ = _registered(name)
    ctr = ro.center(c.target)
    assert np.array_equal(got.center, ctr)
    Q = c.source.shape[0]
    for k, h in enumerate(got.history):
        want = ro.sums(c.source, c.target, h.transformation, c.max_distance, ctr)
        assert h.sums[0] == want.n and (np.abs(h.sums - want.sums)[1:] <= ro.sums_bound(Q, want.abs)[1:]).all(), (name, k)
        assert h.fitness == want.n / Q and h.inlier_rmse == math.sqrt(h.sums[1] / h.sums[0])
        if k + 1 < len(got.history):
            step = mesh.rigid_from_sums(h.sums, c.with_scale, got.center) @ h.transformation
            assert step.tobytes() == got.history[k + 1].transformation.tobytes(), (name, k)
    assert got.transformation.tobytes() == got.history[-1].transformation.tobytes() and got.iterations == len(got.history) - 1


@pytest.mark.parametrize("name", ["cube", "cube+scale", "surface", "outliers"])
def test_recovery(name):
    c, got, want = _registered(name)
    assert got.converged and want.converged and got.iterations == want.iterations <= 20
    assert got.fitness == c.fitness and (name == "outliers") == (got.fitness == 1000 / 1300) and (name == "outliers" or got.fitness == 1.0)
    last = ro.sums(c.source, c.target, got.transformation, c.max_distance, ro.center(c.target))
    bound = ro.rmse_bound(c.source, got.transformation, last.index)
    deviation, own = float(np.abs(got.transformation - c.truth).max()), float(np.abs(want.transformation - c.truth).max())
    print("%s: %d iterations, inlier_rmse %.3g (fp32 bound %.3g), |T - truth| %.3g (the oracle's own %.3g)"
          % (name, got.iterations, got.inlier_rmse, bound, deviation, own))
    assert 0.0 < got.inlier_rmse <= bound
    assert deviation <= 4.0 * own


def test_register_stops_without_pairs_and_after_max_iterations():
    from envgs_amd import mesh
    c = ro.cases()["cube"]
    none = mesh.register(_t(c.source + F32(50.0)), _t(c.target), c.max_distance)
    assert not none.converged and none.iterations == 0 and none.fitness == 0.0 and len(none.history) == 1
    assert np.array_equal(none.transformation, np.eye(4))
    short = mesh.register(_t(c.source), _t(c.target), c.max_distance, max_iterations=2)
    full = _registered("cube")[1]
    assert not short.converged and short.iterations == 2 and len(short.history) == 3
    assert short.transformation.tobytes() == full.history[2].transformation.tobytes()
    empty = mesh.register(_t(np.zeros((0, 3), F32)), _t(c.target), c.max_distance, init=c.truth)
    assert not empty.converged and empty.fitness == 0.0 and np.array_equal(empty.transformation, c.truth)


# ---- 3. transform_points -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 257, 3000])
def test_transform_points(N):
    from envgs_amd import mesh
    rng = np.random.default_rng(50 + N)
    points = (rng.normal(size=(N, 3)) * 10.0 ** rng.uniform(-3, 3, (N, 1))).astype(F32)
    if N > 8:
        points[1, 0], points[2, 1], points[3, 2], points[4] = np.nan, np.inf, -np.inf, np.inf
    T = ro.similarity((1, 2, -2), 33.0, (0.7, -11.0, 3.0), 1.3)
    T[0, 1] = 0.0                                                 # a zero entry times an infinity is a NaN: the row stays not finite
    want = ro.transform(points, T)
    with guarded():
        got = mesh.transform_points(_t(points), T)
        rows = mesh.register_sums(_t(points), mesh.PointGrid(_t(_sum_target()), 0.25), T[:3], return_rows=True)[1]
    assert _np(got).tobytes() == want.tobytes() and _np(rows).tobytes() == want.tobytes()
    assert (np.isfinite(want).all(axis=1) | ~np.isfinite(want).any(axis=1) | ~np.isfinite(points).all(axis=1)).all()
    assert not np.isfinite(want[~np.isfinite(points).all(axis=1)]).any()
    for bad in (np.eye(3), np.full((4, 4), np.nan), np.eye(4) * 1e300):
        with pytest.raises(ValueError):
            mesh.transform_points(_t(points), bad)


# ---- 4. voxel_downsample -------------------------------------------------------------------------------------------------------------------------------------------
def _voxel_cloud(N, seed):
    rng = np.random.default_rng(seed)
    points = rng.uniform(-1, 1, (N, 3)).astype(F32)
    if N >= 64:
        points[N // 2:N // 2 + N // 8] = points[:N // 8]          # exact duplicates
        points[5, 1], points[9] = np.nan, np.inf
    return points


def check_voxel(points, voxel, origin=None, label=""):
    from envgs_amd import mesh
    want = ro.voxel_downsample(points, voxel, origin)
    outs = []
    with guarded():
        for run in range(2):
            got, cluster = mesh.voxel_downsample(_t(points), voxel, origin=origin, return_index=True)
            outs.append((_np(got).tobytes(), _np(cluster).tobytes()))
        assert torch.equal(mesh.voxel_downsample(_t(points), voxel, origin=origin), got)
    assert outs[0] == outs[1], label
    assert got.dtype == torch.float32 and tuple(got.shape) == want.points.shape, (label, got.shape, want.points.shape)
    assert _np(got).tobytes() == want.points.tobytes(), label
    assert cluster.dtype == torch.int32 and np.array_equal(_np(cluster), want.cluster), label
    return want, got


@pytest.mark.parametrize("N", [0, 1, 2, 64, 65, 257, 5000])
def test_voxel_downsample_equals_the_oracle_and_ignores_the_order(N):
    from envgs_amd import mesh
    points = _voxel_cloud(N, 60 + N)
    want, got = check_voxel(points, 0.23, label="N %d" % N)
    if N >= 64:
        fin = np.isfinite(points).all(axis=1)
        members = np.bincount(want.cluster[fin])
        assert (want.cluster[~fin] == -1).all() and (~fin).sum() == 2 and members.max() > 1
        single = np.flatnonzero(members == 1)                      # a cell of one member keeps its bits
        owner = np.array([np.flatnonzero(want.cluster == s)[0] for s in single[:20]])
        assert single.size and _np(got)[single[:20]].tobytes() == points[owner].tobytes()
    perm = np.random.default_rng(61).permutation(N)
    lo = so.grid_of(points, 0.23)[0]
    again, cluster = mesh.voxel_downsample(_t(points[perm]), 0.23, origin=lo, return_index=True)
    assert _np(again).tobytes() == want.points.tobytes() and np.array_equal(_np(cluster), want.cluster[perm])


def test_voxel_downsample_on_an_explicit_origin_and_in_one_cell():
    points = _voxel_cloud(900, 62)
    check_voxel(points, 0.31, origin=(-1.5, -1.25, -1.0), label="origin")
    check_voxel(points, 0.31, origin=(0.0, 0.1, -0.2), label="origin inside the cloud: clamped below at 0")
    want, _ = check_voxel(points, 8.0, label="one cell")
    assert want.points.shape == (1, 3)
    same = np.tile(points[:1], (300, 1))
    want, _ = check_voxel(same, 0.1, label="all equal")
    assert want.points.shape == (1, 3)


def test_voxel_downsample_equals_the_dense_clustering_of_simplify():
    """Rows 0 .. C-1 of cl_vertices of envgs_mesh_simplify_cluster, on the same origin and cell with F = 0, are the same bytes."""
    from envgs_amd import _lib, mesh
    points = _voxel_cloud(5000, 63)
    p = _t(points)
    for voxel in (0.23, 0.07):
        origin, dims = mesh.voxel_grid(p, voxel)
        assert (origin, dims) == so.grid_of(points, voxel)
        sparse = mesh.voxel_downsample(p, voxel)
        lib = _lib.load()
        V, R = points.shape[0], min(points.shape[0], math.prod(dims))
        tb = lib.envgs_mesh_simplify_temp_bytes(V, 0, *dims)
        temp = torch.empty(tb, dtype=torch.uint8, device=DEV)
        cl_vertices = torch.zeros(R, 3, dtype=torch.float32, device=DEV)
        vertex_cluster = torch.empty(V, dtype=torch.int32, device=DEV)
        count = torch.empty(1, dtype=torch.int32, device=DEV)
        q = _lib.ptr
        _lib.check(lib.envgs_mesh_simplify_cluster(V, 0, q(p), None, None, *origin, voxel, *dims, q(temp), tb, q(cl_vertices), None, None, None,
                                                   q(vertex_cluster), q(count), None), "envgs_mesh_simplify_cluster")
        torch.cuda.synchronize()
        C = int(count.item())
        assert C == sparse.shape[0] > 100 and _np(cl_vertices[:C]).tobytes() == _np(sparse).tobytes()


def test_voxel_downsample_beyond_the_dense_grid_and_beyond_its_own():
    from envgs_amd import mesh
    rng = np.random.default_rng(64)
    points = rng.uniform(0, 1, (1000, 3)).astype(F32)
    points[0], points[1] = 0.0, 1.0
    points[500:520] = points[480:500] + F32(2.0 ** -22)          # neighbours that share a cell of 2^-20
    voxel = 2.0 ** -20 * (1 - 2.0 ** -12)                          # just above 2^20 cells per axis
    want, got = check_voxel(points, voxel, label="2^20 cells per axis")
    assert min(want.dims) > 2 ** 20 and 900 < got.shape[0] < 1000
    with pytest.raises(ValueError):
        mesh.simplify_grid(_t(points), voxel)                     # the dense path refuses
    with pytest.raises(ValueError) as info:
        mesh.voxel_downsample(_t(points), 2.0 ** -22)
    smallest = float(str(info.value).rsplit(" ", 1)[1])
    assert 2.0 ** -21 * 0.99 < smallest < 2.0 ** -21 * 1.01
    mesh.voxel_grid(_t(points), smallest)                        # the named voxel is admissible
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            mesh.voxel_downsample(_t(points), bad)


# ---- 5. in_polygon_volume ------------------------------------------------------------------------------------------------------------------------------------------
def _polygon(kind, axis):
    """(M,3) float64 in the plane of (u, v), the orthogonal coordinate arbitrary."""
    if kind == "convex":
        uv = [(0.9 * math.cos(a) + 0.05, 0.7 * math.sin(a) - 0.1) for a in np.linspace(0, 2 * math.pi, 7, endpoint=False)]
    elif kind == "L":
        uv = [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.0), (0.0, 0.0), (0.0, 0.5), (-0.5, 0.5)]
    elif kind == "triangle":
        uv = [(-0.75, -0.5), (0.75, -0.25), (0.0, 0.8)]
    else:                                                          # 256 vertices of a star: concave at every second vertex
        uv = [((0.9 if j % 2 else 0.55) * math.cos(2 * math.pi * j / 256), (0.9 if j % 2 else 0.55) * math.sin(2 * math.pi * j / 256)) for j in range(256)]
    w, u, v = ro.UV[axis]
    poly = np.zeros((len(uv), 3))
    poly[:, u], poly[:, v], poly[:, w] = [p[0] for p in uv], [p[1] for p in uv], np.linspace(-3, 3, len(uv))
    return poly


def check_polygon(points, axis, lo, hi, poly, label=""):
    from envgs_amd import mesh
    want = ro.in_polygon(points, axis, lo, hi, poly)
    with guarded():
        got = mesh.in_polygon_volume(_t(np.asarray(points, F32).reshape(-1, 3)), axis, lo, hi, poly)
    assert got.dtype == torch.bool and np.array_equal(_np(got), want), (label, np.flatnonzero(_np(got) != want)[:8])
    return want


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
@pytest.mark.parametrize("kind", ["convex", "L", "triangle", "star 256"])
def test_in_polygon_volume(axis, kind):
    poly = _polygon(kind, axis)
    w, u, v = ro.UV[axis]
    rng = np.random.default_rng(70)
    points = rng.uniform(-1, 1, (4000, 3)).astype(F32)
    points[7, 0], points[8, 1], points[9, 2] = np.nan, np.inf, -np.inf
    edge = points[:600].copy()                                    # on the vertices, on the edges' supporting lines and on the horizontal edges
    edge[:, u] = F32(poly[np.arange(600) % poly.shape[0], u])
    edge[:300, v] = F32(poly[np.arange(300) % poly.shape[0], v])
    band = points[:400].copy()                                    # at axis_min and axis_max exactly, and one step outside
    band[:100, w], band[100:200, w] = F32(-0.25), F32(0.5)
    band[200:300, w], band[300:, w] = np.nextafter(F32(-0.25), F32(-1)), np.nextafter(F32(0.5), F32(1))
    allp = np.concatenate([points, edge, band])
    want = check_polygon(allp, axis, -0.25, 0.5, poly, label="%s %s" % (axis, kind))
    assert 0.05 < want[:4000].mean() < 0.6 and not want[[7, 8, 9]].any()
    inside_uv = ro.in_polygon(band, axis, -np.inf, np.inf, poly)
    assert np.array_equal(want[4600:4800], inside_uv[:200]) and not want[4800:].any()      # the bounds are inclusive
    if kind == "L":                                               # the notch is outside, the arms are inside
        probe = np.zeros((3, 3), F32)
        probe[:, u], probe[:, v] = [0.25, -0.25, 0.25], [0.25, 0.25, -0.25]
        assert check_polygon(probe, axis, -1, 1, poly).tolist() == [False, True, True]


@pytest.mark.parametrize("N", [0, 1, 257])
def test_in_polygon_volume_small_counts(N):
    from envgs_amd import mesh
    points = np.random.default_rng(71 + N).uniform(-1, 1, (N, 3)).astype(F32)
    check_polygon(points, "Y", -0.5, 0.5, _polygon("L", "Y"), label="N %d" % N)
    for bad in (dict(axis="W"), dict(polygon=np.zeros((2, 3))), dict(polygon=np.zeros((257, 3))), dict(polygon=np.full((4, 3), np.nan)), dict(axis_min=float("nan"))):
        kw = dict(axis="Y", axis_min=-0.5, axis_max=0.5, polygon=_polygon("L", "Y"))
        kw.update(bad)
        with pytest.raises(ValueError):
            mesh.in_polygon_volume(_t(points), kw["axis"], kw["axis_min"], kw["axis_max"], kw["polygon"])


def test_load_crop_volume(tmp_path):
    from envgs_amd import mesh
    poly = _polygon("L", "Y")
    path = tmp_path / "crop.json"
    path.write_text(json.dumps({"axis_max": 0.5, "axis_min": -0.25, "bounding_polygon": poly.tolist(), "class_name": "SelectionPolygonVolume",
                                "orthogonal_axis": "Y", "version_major": 1, "version_minor": 0}))
    crop = mesh.load_crop_volume(str(path))
    assert (crop.axis, crop.axis_min, crop.axis_max) == ("Y", -0.25, 0.5) and np.array_equal(crop.polygon, poly)
    points = np.random.default_rng(72).uniform(-1, 1, (500, 3)).astype(F32)
    got = mesh.in_polygon_volume(_t(points), crop.axis, crop.axis_min, crop.axis_max, crop.polygon)
    assert np.array_equal(_np(got), ro.in_polygon(points, "Y", -0.25, 0.5, poly))


# ---- 6. evaluate_tnt -----------------------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_tnt():
    """The surface case with a square crop and an init that is 1 degree off: the three stages run, the transformation meets the recovery bound, and
    the scores equal evaluate() applied by hand to clouds the oracle prepared under the product's final transformation."""
    from types import SimpleNamespace
    from envgs_amd import mesh
    c = ro.cases()["surface"]
    tau = 0.02
    crop = SimpleNamespace(axis="Z", axis_min=-1.0, axis_max=1.0, polygon=np.array([[-0.8, -0.8, 0], [0.8, -0.8, 0], [0.8, 0.8, 0], [-0.8, 0.8, 0]], F64))
    init = ro.similarity((1, 0, 1), 1.0, (0.004, -0.003, 0.002)) @ c.truth
    pred = c.source                                               # row i is the partner of scan row 3 i: every 3rd scan row keeps all partners
    with guarded():
        got = mesh.evaluate_tnt(_t(pred), _t(c.target), tau, init=init, crop=crop, max_points=1000)
    assert len(got.registrations) == 3 and all(len(r.history) >= 2 for r in got.registrations)
    total = init
    for r in got.registrations:
        total = r.transformation @ total
    assert total.tobytes() == got.transformation.tobytes()

    cropf = lambda p: p[ro.in_polygon(p, crop.axis, crop.axis_min, crop.axis_max, crop.polygon)]
    moved = ro.voxel_downsample(cropf(ro.transform(pred, got.transformation)), tau / 2).points
    scan = ro.voxel_downsample(cropf(c.target), tau / 2).points
    want = eo.evaluate(moved, scan, tau, tau)
    for name in ("precision", "recall", "fscore", "n_pred", "n_ref", "within_pred", "within_ref", "found_pred", "found_ref"):
        assert getattr(got, name) == getattr(want, name), (name, getattr(got, name), getattr(want, name))
    assert 0.9 < got.precision <= 1.0 and 0.2 < got.recall < 1.0 and 500 < got.n_pred < 1000 and got.n_ref < 3000      # the crop cut both
    by_hand = mesh.evaluate(_t(moved), _t(scan), max_distance=tau, threshold=tau)
    assert (by_hand.precision, by_hand.recall, by_hand.fscore) == (got.precision, got.recall, got.fscore)

    # the third stage, again by the oracle under the product's own second-stage result: every k-th row, moved, cropped
    T2 = got.registrations[1].transformation @ got.registrations[0].transformation @ init
    k = -(-pred.shape[0] // 1000)
    src3, tgt3 = cropf(ro.transform(pred[::k], T2)), cropf(c.target[::-(-c.target.shape[0] // 1000)])
    want3 = ro.icp(src3, tgt3, 2 * tau, ro.center(tgt3))
    own = float(np.abs(want3.transformation @ T2 - c.truth).max())
    deviation = float(np.abs(got.transformation - c.truth).max())
    print("evaluate_tnt: |T - truth| %.3g (the oracle's own %.3g), P %.4f R %.4f F %.4f" % (deviation, own, got.precision, got.recall, got.fscore))
    assert got.registrations[2].converged and deviation <= 4.0 * own
    again = mesh.evaluate_tnt(_t(pred), _t(c.target), tau, init=init, crop=crop, max_points=1000)
    assert again.transformation.tobytes() == got.transformation.tobytes() and again.fscore == got.fscore
