"""GPU: the mesh evaluation kernels (csrc/mesh_eval.hip) through envgs_amd.mesh.sample_surface / PointGrid / nearest_points / evaluate and through
the C-ABI, against the independent oracle (tests/mesh_eval_oracle.py).  Every comparison of samples and of nearest points is exact -- integers and
float words defined bit for bit by include/envgs_mesh.h -- and every product call runs twice and must give identical bytes.  PARITY UNPINNED
(DESIGN.md "Mesh evaluation"): the semantics are this project's."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_eval_cases as ec
from tests import mesh_eval_oracle as eo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CANARY = 0x5A


def _bits(a):
    """float arrays compared as words: NaN payloads and the sign of zero count."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _same(got, want):
    got, want = _np(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_mesh(m):
    from envgs_amd import mesh
    return mesh.Mesh(vertices=_t(m.vertices), faces=_t(m.faces), colors=_t(m.colors))


@functools.lru_cache(maxsize=None)
def _oracle_samples(name):
    m = ec.SEEDED[name]() if name in ec.SEEDED else ec.HAND[name][0]
    return eo.sample_surface(m.vertices, m.faces, m.colors, m.density, m.seed)


# ---- 1. sampling ----------------------------------------------------------------------------------------------------------------------------------------
def check_sample(m, want, label):
    """sample_surface twice with the faces and once without: identical bytes, equal to the oracle."""
    from envgs_amd import mesh
    dm = _device_mesh(m)
    for run in range(2):
        points, colors, face = mesh.sample_surface(dm, m.density, seed=m.seed, return_face=True)
        assert points.dtype == torch.float32 and face.dtype == torch.int32 and tuple(points.shape) == want.points.shape, (label, run)
        assert _same(face, want.face), (label, run)
        assert _same(points, want.points), (label, run)
        assert (colors is None) == (want.colors is None) and (colors is None or _same(colors, want.colors)), (label, run)
    plain = mesh.sample_surface(dm, m.density, seed=m.seed)
    assert len(plain) == 2 and _same(plain[0], want.points)
    return points, colors, face


@pytest.mark.parametrize("name", list(ec.HAND))
def test_hand_made_meshes(name):
    m, counts = ec.HAND[name]
    _, _, face = check_sample(m, _oracle_samples(name), name)
    assert np.bincount(_np(face), minlength=len(counts)).tolist() == counts


def test_empty_meshes_and_no_samples():
    from envgs_amd import mesh
    tri = ec.HAND["one right triangle"][0]
    empty = [ec._case(np.zeros((0, 3)), np.zeros((0, 3), np.int32), 5.0), ec._case(np.zeros((0, 3)), [[0, 1, 2], [0, 0, 0]], 5.0),
             ec._case(tri.vertices, np.zeros((0, 3), np.int32), 5.0, colors=tri.colors), ec._case(tri.vertices, tri.faces, 1e-9, colors=tri.colors)]
    for m in empty:
        want = eo.sample_surface(m.vertices, m.faces, m.colors, m.density, m.seed)
        points, colors, face = check_sample(m, want, "V %d F %d" % (m.vertices.shape[0], m.faces.shape[0]))
        assert points.shape == (0, 3) and face.shape == (0,) and (colors is None or colors.shape == (0, 3))
    dm = _device_mesh(tri)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            mesh.sample_surface(dm, bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.sample_surface(mesh.Mesh(vertices=torch.zeros(3, 3), faces=torch.zeros(1, 3, dtype=torch.int32), colors=None), 1.0)


def test_one_huge_face_among_tiny_ones():
    want = _oracle_samples("giant")
    _, _, face = check_sample(ec.giant(), want, "giant")
    c = np.bincount(_np(face), minlength=1000)
    assert 99000 < c[500] < 101000 and np.delete(c, 500).max() <= 1


def test_more_than_1024_workgroup_totals():
    m = ec.many()
    assert (m.faces.shape[0] + 255) // 256 > 1024
    want = _oracle_samples("many")
    check_sample(m, want, "many")
    bare = SimpleNamespace(**{**vars(m), "colors": None})
    bare_want = SimpleNamespace(**{**vars(want), "colors": None})
    points, colors, _ = check_sample(bare, bare_want, "many, no colours")
    assert colors is None and want.face[-1] >= m.faces.shape[0] - 300      # the last workgroups emit too


def test_an_indexed_mesh_with_bad_faces_and_the_seed():
    from envgs_amd import mesh
    m = ec.soup()
    points, _, face = check_sample(m, _oracle_samples("soup"), "soup")
    assert not np.isin(_np(face), [5, 77, 100]).any() and bool(torch.isfinite(points).all())
    other = SimpleNamespace(**{**vars(m), "seed": 1})
    want = eo.sample_surface(m.vertices, m.faces, m.colors, m.density, 1)
    p1, _, _ = check_sample(other, want, "soup, seed 1")
    assert p1.shape != points.shape or not torch.equal(p1.view(torch.int32), points.view(torch.int32))
    with pytest.raises(ValueError):
        mesh.sample_surface(_device_mesh(m), m.density, seed=2 ** 32)


def test_limits_raise():
    from envgs_amd import mesh
    tri = ec.HAND["one right triangle"][0]
    dm = _device_mesh(tri)
    with pytest.raises(ValueError, match="2\\^24"):
        mesh.sample_surface(dm, 2.0 ** 23)                       # area 2: 2^24 + u
    assert mesh.sample_surface(dm, 2.0 ** 10)[0].shape[0] in (2048, 2049)
    many = ec._case(tri.vertices, np.tile(tri.faces, (300, 1)), 8.0e6)       # 300 x 1.6e7 = 4.8e9: past 2^32, caught by the 64-bit total
    assert not eo.face_counts(many.vertices, many.faces, many.density, 0).over
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.sample_surface(_device_mesh(many), many.density)


def _guarded(rows, width, dtype, pad, fill=None):
    size = torch.empty(0, dtype=dtype).element_size()
    buf = torch.full(((rows + 2 * pad) * width * size,), CANARY, dtype=torch.uint8, device=DEV).view(dtype)
    if fill is not None:
        buf[pad * width:(pad + rows) * width] = torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)).to(DEV)
    return buf


def _untouched(buf, width, rows, pad):
    b, e = buf.view(torch.uint8), buf.element_size()
    return bool((b[:pad * width * e] == CANARY).all()) and bool((b[(pad + rows) * width * e:] == CANARY).all())


def _raw_sample(m, pad=64, stream=None):
    """The two sampling calls of the C-ABI on buffers with `pad` canary rows before and after every array the library reads by index or writes."""
    from envgs_amd import _lib
    lib = _lib.load()
    V, F = m.vertices.shape[0], m.faces.shape[0]
    v, c, f = _guarded(V, 3, torch.float32, pad, m.vertices), _guarded(V, 3, torch.float32, pad, m.colors), _guarded(F, 3, torch.int32, pad, m.faces)
    tb = lib.envgs_mesh_sample_temp_bytes(V, F)
    temp = torch.full((tb + 512,), CANARY, dtype=torch.uint8, device=DEV)
    toff = (-temp.data_ptr()) % 256
    tp = _lib.ctypes.c_void_p(temp.data_ptr() + toff)
    totals = _guarded(2, 1, torch.int64, pad)
    at = lambda buf, width: _lib.ctypes.c_void_p(buf.data_ptr() + pad * width * buf.element_size())
    s = _lib.ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream.cuda_stream)
    assert lib.envgs_mesh_sample_count(V, F, at(v, 3), at(f, 3), m.density, m.seed, tp, tb, at(totals, 1), s) == 0
    torch.cuda.synchronize()
    S, over = totals[pad:pad + 2].tolist()
    assert not over and _untouched(totals, 1, 2, pad)
    pts, col, face = _guarded(S, 3, torch.float32, pad), _guarded(S, 3, torch.float32, pad), _guarded(S, 1, torch.int32, pad)
    assert lib.envgs_mesh_sample_emit(V, F, at(v, 3), at(c, 3), at(f, 3), m.seed, tp, tb, S, at(pts, 3), at(col, 3), at(face, 1), s) == 0
    torch.cuda.synchronize()
    assert _untouched(pts, 3, S, pad) and _untouched(col, 3, S, pad) and _untouched(face, 1, S, pad), "rows at or beyond S were written"
    assert _untouched(v, 3, V, pad) and _untouched(c, 3, V, pad) and _untouched(f, 3, F, pad)
    assert bool((temp[:toff] == CANARY).all()) and bool((temp[toff + tb:] == CANARY).all())
    body = lambda buf, width: buf[pad * width:(pad + S) * width].reshape(S, width).cpu().numpy()
    return SimpleNamespace(points=body(pts, 3), colors=body(col, 3), face=body(face, 1).reshape(-1))


@pytest.mark.parametrize("name", ["soup", "giant"])
def test_sampling_writes_nothing_outside_the_documented_rows(name):
    """In soup the indices -1 and V stand beside canary-guarded vertex arrays whose canary words read as valid numbers."""
    m, want = ec.SEEDED[name](), _oracle_samples(name)
    for _ in range(2):
        got = _raw_sample(m)
        assert _same(got.face, want.face) and _same(got.points, want.points) and _same(got.colors, want.colors)


def test_sampling_on_the_callers_stream():
    m, want = ec.soup(), _oracle_samples("soup")
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        check_sample(m, want, "side stream")
    side.synchronize()
    got = _raw_sample(m, stream=side)
    assert _same(got.points, want.points)


# ---- 2. nearest -------------------------------------------------------------------------------------------------------------------------------------------
def check_nearest(queries, points, max_distance, cell_size=None, label="", want=None):
    """PointGrid + nearest twice and nearest_points once: identical bytes, equal to brute force.  -> (dist2, index) NumPy"""
    from envgs_amd import mesh
    q, p = _t(np.asarray(queries, F32).reshape(-1, 3)), _t(np.asarray(points, F32).reshape(-1, 3))
    want = eo.nearest(queries, points, max_distance) if want is None else want
    grid = mesh.PointGrid(p, max_distance, cell_size)
    for run in range(2):
        d2, idx = grid.nearest(q)
        assert d2.dtype == torch.float32 and idx.dtype == torch.int32
        bad = np.flatnonzero((_np(idx) != want[1]) | (_bits(_np(d2)) != _bits(want[0])))
        assert bad.size == 0, (label, run, grid.dims, bad[:5], _np(idx)[bad[:5]], want[1][bad[:5]], _np(d2)[bad[:5]], want[0][bad[:5]])
    d2, idx = mesh.nearest_points(q, p, max_distance, cell_size)
    assert _same(d2, want[0]) and _same(idx, want[1]), label
    return want


@pytest.mark.parametrize("N", [0, 1, 257])
def test_small_counts(N):
    rng = np.random.default_rng(N)
    points = (0.25 + 0.5 * rng.random((N, 3))).astype(F32)        # all in ONE cell of edge 4
    for Q in (0, 1, 65, 300):
        queries = rng.random((Q, 3)).astype(F32)
        d2, idx = check_nearest(queries, points, 0.3, cell_size=4.0, label="N %d Q %d" % (N, Q))
        assert idx.shape == (Q,) and (N > 0 or (idx == -1).all())
        check_nearest(queries, points, 0.3, label="N %d Q %d, default cell" % (N, Q))


@pytest.mark.parametrize("max_distance", [1.0, float(np.nextafter(F32(1), F32(0))), 5.0, float(np.nextafter(F32(5), F32(0))), 0.7, 0.0, 3000.0])
def test_lattice(max_distance):
    """Points on the cell walls; queries on walls, at midpoints (ties: the lowest index), at the grid's corners, 1 000 cells outside, and at exact
    lattice distances 1 and 5 from their nearest point, with the radius on the distance (inclusive) and one fp32 step below it."""
    p, q = ec.lattice(), ec.lattice_queries()
    for cell in (1.0, 0.25, 2.5, 100.0):
        d2, idx = check_nearest(q, p, max_distance, cell_size=cell, label="lattice r %r cell %g" % (max_distance, cell))
    edge = q[-6:]
    got = dict(zip(("x-", "z-", "x+", "345", "345+", "diag"), zip(d2[-6:].tolist(), idx[-6:].tolist())))
    if max_distance == 1.0:
        assert got["x-"] == (1.0, 0 + ec.L * (2 + ec.L * 2))      # (0, 2, 2), x fastest
        assert got["z-"][0] == 1.0 and got["x+"][0] == 1.0 and got["345"][1] == -1 and got["diag"][1] == -1
    if 0.99 < max_distance < 1.0:
        assert got["x-"][1] == -1 and got["z-"][1] == -1 and got["x+"][1] == -1
    if max_distance == 5.0:
        assert got["345"][0] == 25.0 and got["345+"][0] == 25.0 and got["diag"][0] == 2.0
    if 4.99 < max_distance < 5.0:
        assert got["345"][1] == -1 and got["345+"][1] == -1 and got["diag"][0] == 2.0
    if max_distance == 3000.0:
        assert (idx >= 0).all()                                  # the queries 1 000 cells outside find the border points
    assert edge.shape == (6, 3)


def test_duplicates_and_non_finite_values():
    p = np.concatenate([ec.lattice(), ec.lattice()[::-1]])        # every point twice: the lowest index wins
    q = ec.lattice_queries()
    _, idx = check_nearest(q, p, 1.5, cell_size=1.0, label="duplicates")
    assert idx.max() < ec.lattice().shape[0] * 2 and (idx >= 0).any()
    on = check_nearest(ec.lattice(), p, 0.0, cell_size=0.5, label="duplicates, radius 0")
    assert (on[0] == 0).all() and np.array_equal(on[1], np.arange(216))      # never the copy at 431 - i
    ps, qs = ec.with_specials(p, 41), ec.with_specials(q, 42)
    d2, idx = check_nearest(qs, ps, 1.5, label="NaN and inf")
    nf = ~np.isfinite(qs).all(axis=1)
    assert nf.sum() == 9 and (idx[nf] == -1).all() and np.isinf(d2[nf]).all()
    assert not np.isin(idx, np.flatnonzero(~np.isfinite(ps).all(axis=1))).any()
    none = np.full((5, 3), np.nan, F32)
    d2, idx = check_nearest(q[:70], none, 1.0, label="no finite point")
    assert (idx == -1).all()


@functools.lru_cache(maxsize=None)
def _cloud_truth():
    c = ec.cloud()
    return eo.nearest(c.queries, c.points, c.max_distance)


@pytest.mark.parametrize("factor", [1 / 16, 1.0, 7.0, None, "default"])
def test_random_cloud_at_every_cell_size(factor):
    """5 000 points x 3 000 queries against brute force; the result is the same BYTES at every cell size (each compared with the one truth)."""
    c = ec.cloud()
    cell = None if factor == "default" else (2.0 if factor is None else factor * c.max_distance)      # 2.0: one cell for the whole cloud
    d2, idx = check_nearest(c.queries, c.points, c.max_distance, cell_size=cell, label="cloud, cell %r" % cell, want=_cloud_truth())
    assert 0.2 < (idx >= 0).mean() < 0.999                        # some queries have no neighbour within the radius


def test_large_coordinates_small_cells():
    c = ec.offset_cloud()
    d2, idx = check_nearest(c.queries, c.points, c.max_distance, cell_size=c.cell_size, label="offset 1000")
    assert (idx >= 0).mean() > 0.9
    check_nearest(c.queries, c.points, c.max_distance, label="offset 1000, default cell")


def test_cell_size_limits():
    from envgs_amd import mesh
    p = _t(ec.cloud().points)
    with pytest.raises(ValueError, match="smallest admissible cell_size"):
        mesh.PointGrid(p, 0.05, 1e-4)                            # 10^4 cells per axis
    with pytest.raises(ValueError, match="smallest admissible cell_size"):
        mesh.PointGrid(p, 0.05, 1.5e-3)                          # 667 per axis, 2.9e8 in all
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            mesh.PointGrid(p, 0.05, bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mesh.PointGrid(p, bad)
    g = mesh.PointGrid(p, 1e-6)                                   # the default is raised until the limits hold
    assert max(g.dims) <= 1024 and math.prod(g.dims) <= 2 ** 27
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.PointGrid(torch.zeros(4, 3), 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.nearest(torch.zeros(4, 3))


def _raw_nearest(queries, points, max_distance, cell, pad=64, stream=None):
    from envgs_amd import _lib
    lib = _lib.load()
    N, Q = points.shape[0], queries.shape[0]
    lo = points.min(axis=0)
    dims = [int(math.floor((float(h) - float(l)) / cell)) + 1 for l, h in zip(lo, points.max(axis=0))]
    cells = math.prod(dims)
    p, q = _guarded(N, 3, torch.float32, pad, points), _guarded(Q, 3, torch.float32, pad, queries)
    ce, rec = _guarded(cells, 1, torch.int32, pad), _guarded(N, 4, torch.float32, pad)
    d2, idx = _guarded(Q, 1, torch.float32, pad), _guarded(Q, 1, torch.int32, pad)
    tb = lib.envgs_points_grid_temp_bytes(N, *dims)
    temp = torch.full((tb + 512,), CANARY, dtype=torch.uint8, device=DEV)
    toff = (-temp.data_ptr()) % 256
    at = lambda buf, width: _lib.ctypes.c_void_p(buf.data_ptr() + pad * width * buf.element_size())
    s = _lib.ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream.cuda_stream)
    o = [float(x) for x in lo]
    assert lib.envgs_points_grid_build(N, at(p, 3), o[0], o[1], o[2], cell, *dims, _lib.ctypes.c_void_p(temp.data_ptr() + toff), tb, at(ce, 1), at(rec, 4), s) == 0
    assert lib.envgs_points_nearest(Q, at(q, 3), max_distance, o[0], o[1], o[2], cell, *dims, at(ce, 1), at(rec, 4), at(d2, 1), at(idx, 1), s) == 0
    torch.cuda.synchronize()
    assert _untouched(d2, 1, Q, pad) and _untouched(idx, 1, Q, pad), "rows at or beyond Q were written"
    assert _untouched(ce, 1, cells, pad) and _untouched(rec, 4, N, pad) and _untouched(p, 3, N, pad) and _untouched(q, 3, Q, pad)
    assert bool((temp[:toff] == CANARY).all()) and bool((temp[toff + tb:] == CANARY).all())
    assert int(ce[pad + cells - 1]) == N                          # the end of the last cell: every (finite) point has a slot
    return d2[pad:pad + Q].cpu().numpy(), idx[pad:pad + Q].cpu().numpy()


def test_nearest_writes_nothing_outside_the_documented_rows_and_runs_on_the_callers_stream():
    c = ec.cloud()
    want = _cloud_truth()
    q, w = c.queries[:301], (want[0][:301], want[1][:301])
    for _ in range(2):
        d2, idx = _raw_nearest(q, c.points, c.max_distance, 0.03)
        assert _same(d2, w[0]) and _same(idx, w[1])
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        check_nearest(q, c.points, c.max_distance, label="side stream", want=w)
    side.synchronize()
    d2, idx = _raw_nearest(q, c.points, c.max_distance, 0.03, stream=side)
    assert _same(d2, w[0]) and _same(idx, w[1])


def test_bad_arguments_are_rejected():
    from envgs_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = _lib.ptr(buf)
    odd = _lib.ctypes.c_void_p(buf.data_ptr() + 4)
    assert lib.envgs_points_grid_temp_bytes(10, 1025, 1, 1) == 0 and lib.envgs_points_grid_temp_bytes(10, 1024, 1024, 256) == 0
    assert lib.envgs_points_grid_temp_bytes(2 ** 31, 4, 4, 4) == 0 and lib.envgs_points_grid_temp_bytes(10, 0, 4, 4) == 0
    assert lib.envgs_points_grid_build(1, p, 0, 0, 0, 1.0, 1025, 1, 1, p, 4096, p, p, None) == -1
    assert lib.envgs_points_grid_build(1, p, 0, 0, 0, 0.0, 2, 2, 2, p, 4096, p, p, None) == -1
    assert lib.envgs_points_grid_build(1, p, float("nan"), 0, 0, 1.0, 2, 2, 2, p, 4096, p, p, None) == -1
    assert lib.envgs_points_grid_build(1, p, 0, 0, 0, 1.0, 2, 2, 2, odd, 4092, p, p, None) == -1
    assert lib.envgs_points_grid_build(1, None, 0, 0, 0, 1.0, 2, 2, 2, p, 4096, p, p, None) == -1
    assert lib.envgs_points_grid_build(1, p, 0, 0, 0, 1.0, 2, 2, 2, p, 16, p, p, None) == -2
    assert lib.envgs_points_nearest(1, p, -1.0, 0, 0, 0, 1.0, 2, 2, 2, p, p, p, p, None) == -1
    assert lib.envgs_points_nearest(1, p, float("inf"), 0, 0, 0, 1.0, 2, 2, 2, p, p, p, p, None) == -1
    assert lib.envgs_points_nearest(1, None, 1.0, 0, 0, 0, 1.0, 2, 2, 2, p, p, p, p, None) == -1
    assert lib.envgs_mesh_sample_temp_bytes(2 ** 31, 1) == 0
    assert lib.envgs_mesh_sample_count(3, 1, p, p, 0.0, 0, p, 4096, p, None) == -1
    assert lib.envgs_mesh_sample_count(3, 1, p, p, float("inf"), 0, p, 4096, p, None) == -1
    assert lib.envgs_mesh_sample_count(3, 1, None, p, 1.0, 0, p, 4096, p, None) == -1
    assert lib.envgs_mesh_sample_count(3, 1, p, p, 1.0, 0, p, 16, p, None) == -2
    assert lib.envgs_mesh_sample_emit(3, 1, p, None, p, 0, p, 4096, 5, p, p, None, None) == -1      # colours out without colours in
    assert lib.envgs_mesh_sample_emit(3, 1, p, None, p, 0, p, 4096, 2 ** 31, p, None, None, None) == -1
    torch.cuda.synchronize()


# ---- 3. metrics -------------------------------------------------------------------------------------------------------------------------------------------
def test_a_cloud_against_itself():
    from envgs_amd import mesh
    p = _t(ec.cloud().points)
    assert np.unique(ec.cloud().points, axis=0).shape[0] == p.shape[0]
    d2, idx = mesh.nearest_points(p, p, 0.01)
    assert bool((d2 == 0).all()) and torch.equal(idx, torch.arange(p.shape[0], dtype=torch.int32, device=DEV))
    e = mesh.evaluate(p, p, 0.01, 0.0)
    assert e.accuracy == 0.0 and e.completeness == 0.0 and e.chamfer == 0.0 and e.precision == 1.0 and e.recall == 1.0 and e.fscore == 1.0
    assert (e.found_pred, e.within_pred, e.found_ref, e.within_ref, e.n_pred, e.n_ref) == (5000,) * 6
    assert bool((e.d_pred == 0).all()) and e.d_pred.dtype == torch.float64


@pytest.mark.parametrize("seed,n_pred,n_ref,max_distance,threshold", [(51, 900, 1100, 0.1, 0.05), (52, 3000, 700, 0.06, 0.06)])
def test_two_clouds_against_the_oracle(seed, n_pred, n_ref, max_distance, threshold):
    from envgs_amd import mesh
    rng = np.random.default_rng(seed)
    pred, ref = rng.random((n_pred, 3), dtype=F32), rng.random((n_ref, 3), dtype=F32) * F32(0.9)
    want = eo.evaluate(pred, ref, max_distance, threshold)
    for _ in range(2):
        got = mesh.evaluate(_t(pred), _t(ref), max_distance, threshold)
        for k in ("n_pred", "n_ref", "found_pred", "found_ref", "within_pred", "within_ref"):
            assert getattr(got, k) == getattr(want, k), k
        assert 0 < got.within_pred < got.found_pred or threshold == max_distance
        for k in ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore"):      # float64 sums of at most 10^4 terms, added in two orders
            assert abs(getattr(got, k) - getattr(want, k)) <= 1e-9 * abs(getattr(want, k)), (k, getattr(got, k), getattr(want, k))
        assert np.allclose(_np(got.d_pred), want.d_pred, rtol=1e-15, atol=0) and np.allclose(_np(got.d_ref), want.d_ref, rtol=1e-15, atol=0)
    with pytest.raises(ValueError):
        mesh.evaluate(_t(pred), _t(ref), 0.05, 0.06)


def test_a_cloud_beyond_the_radius():
    from envgs_amd import mesh
    c = ec.cloud()
    e = mesh.evaluate(_t(c.points), _t(c.points + F32(3.0)), 0.5, 0.25)
    assert (e.found_pred, e.within_pred, e.found_ref, e.within_ref) == (0, 0, 0, 0)
    assert e.precision == 0.0 and e.recall == 0.0 and e.fscore == 0.0 and math.isnan(e.accuracy) and math.isnan(e.chamfer)
    assert bool(torch.isinf(e.d_pred).all())


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------------------------
def test_extracted_plane_against_a_lattice():
    """The volume of the plane z = c: the level set is linear, so extract() lies on the plane within the suite's 1e-5 voxel.  Against a square
    lattice of spacing s on that plane, reaching beyond the mesh, no surface sample is farther from its lattice point than half a diagonal."""
    from envgs_amd import mesh
    nx, ny, nz, voxel, origin = 20, 18, 10, 0.1, (0.3, -0.2, 1.0)
    c = origin[2] + 4.37 * voxel
    z = (origin[2] + voxel * np.arange(nz, dtype=np.float64) - c) / (5 * voxel)
    tsdf = np.broadcast_to(z[:, None, None], (nz, ny, nx)).astype(F32)
    vol = mesh.TSDFVolume.from_tensors(_t(tsdf), _t(np.ones_like(tsdf)), None, origin, voxel)
    m = vol.extract()
    assert m.faces.shape[0] > 0
    assert float((m.vertices[:, 2].double() - c).abs().max()) <= 1e-5 * voxel + 2.0 ** -22
    s = 0.05
    gx = origin[0] - 0.2 + s * np.arange(int((voxel * (nx - 1) + 0.4) / s) + 2)
    gy = origin[1] - 0.2 + s * np.arange(int((voxel * (ny - 1) + 0.4) / s) + 2)
    X, Y = np.meshgrid(gx, gy, indexing="xy")
    lattice = np.stack([X.reshape(-1), Y.reshape(-1), np.full(X.size, c)], axis=1).astype(F32)
    for _ in range(2):
        e = mesh.evaluate(m, _t(lattice), 2 * s, s, density=2000.0, seed=4)
        area = voxel * (nx - 1) * voxel * (ny - 1)
        assert abs(e.n_pred - 2000.0 * area) <= 3 * math.sqrt(m.faces.shape[0])
        bound = s * math.sqrt(2.0) / 2 + 2e-5 * voxel + 8 * float(np.spacing(F32(np.abs(lattice).max())))
        print("plane: %d samples, max distance %.6f (bound %.6f), accuracy %.6f, completeness %.6f, recall %.4f"
              % (e.n_pred, float(e.d_pred.max()), bound, e.accuracy, e.completeness, e.recall))
        assert float(e.d_pred.max()) <= bound
        assert e.precision == 1.0 and e.found_pred == e.n_pred == e.within_pred
        assert 0.0 < e.recall < 1.0                               # the lattice reaches beyond the mesh
    cmp = mesh.compare_meshes(mesh.simplify(m, 2 * voxel, origin=vol.origin), m, 2 * s, s, density=2000.0)
    assert cmp.n_pred > 0 and cmp.precision == 1.0 and cmp.accuracy <= s      # the simplified plane lies inside the same plane
