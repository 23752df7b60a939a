"""GPU: the mesh simplification kernels (csrc/mesh_simplify.hip) through envgs_amd.mesh.simplify and through the C-ABI, against the independent oracle
(tests/mesh_simplify_oracle.py).  Every comparison is exact -- integers, floats defined bit for bit by include/envgs_mesh.h -- and every product call
runs twice and must give identical bytes.  PARITY UNPINNED (DESIGN.md "Mesh simplification"): the semantics are this project's."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_clean_oracle as co
from tests import mesh_oracle as mo
from tests import mesh_simplify_cases as sc
from tests import mesh_simplify_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _bits(a):
    """float arrays compared as words: NaN payloads and the sign of zero count."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _same(got, want):
    got, want = _np(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _device_mesh(vertices, faces, colors=None):
    from envgs_amd import mesh
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return mesh.Mesh(vertices=t(np.asarray(vertices, F32)), faces=t(np.asarray(faces, np.int32).reshape(-1, 3)), colors=t(colors))


def _assert_equals_oracle(got, index, want, label):
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32 and index.dtype == torch.int32
    assert tuple(got.faces.shape) == want.faces.shape and tuple(got.vertices.shape) == want.vertices.shape, label
    assert _same(got.faces, want.faces), label
    assert _same(got.vertices, want.vertices), label
    assert (got.colors is None) == (want.colors is None) and (want.colors is None or _same(got.colors, want.colors)), label
    assert _same(index, want.vertex_cluster), label


def check_simplify(m, label="", explicit=True):
    """simplify twice, identical bytes, equal to the oracle on the same arrays and the same grid.  explicit: the case's own origin and dims are
    passed; otherwise the wrapper sizes the grid and the oracle follows its documented rule.  -> (product Mesh, oracle namespace)"""
    from envgs_amd import mesh
    dm = _device_mesh(m.vertices, m.faces, m.colors)
    if explicit:
        kw, origin, dims = dict(origin=m.origin, dims=m.dims), m.origin, m.dims
    else:
        kw = {}
        origin, dims = so.grid_of(m.vertices, m.cell)
        g_origin, g_dims = mesh.simplify_grid(dm.vertices, m.cell)
        assert tuple(g_dims) == tuple(dims) and np.array_equal(np.asarray(g_origin, F32), np.asarray(origin, F32))
    want = so.simplify(m.vertices, m.faces, m.colors, origin, m.cell, dims)
    got, index = mesh.simplify(dm, m.cell, return_index=True, **kw)
    again, index2 = mesh.simplify(dm, m.cell, return_index=True, **kw)
    print("%s: V %d -> %d, F %d -> %d, clusters %d" % (label, m.vertices.shape[0], got.vertices.shape[0], m.faces.shape[0], got.faces.shape[0], want.count))
    _assert_equals_oracle(got, index, want, label)
    _assert_equals_oracle(again, index2, want, label + " (second run)")
    plain = mesh.simplify(dm, m.cell, **kw)                      # without the index: a Mesh alone
    assert isinstance(plain, mesh.Mesh) and torch.equal(plain.faces, got.faces) and _same(plain.vertices, want.vertices)
    return got, want


# ---- 1. the hand-made meshes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.HAND))
def test_hand_made_meshes(name):
    m, vertices, faces, colors, vertex_cluster = sc.HAND[name]
    got, _ = check_simplify(m, name)
    assert _same(got.vertices, np.asarray(vertices, F32).reshape(-1, 3)) and got.faces.tolist() == [list(f) for f in faces]
    assert colors is None or _same(got.colors, np.asarray(colors, F32).reshape(-1, 3))
    sized = sc._mesh(m.vertices.copy(), m.faces, m.colors, cell=m.cell)
    if name != "a NaN vertex":
        sized.vertices[-1, 2] = np.inf                          # the extrema leave out every vertex that is not finite
    check_simplify(sized, name + ", grid sized by the wrapper", explicit=False)


def test_empty_meshes():
    from envgs_amd import mesh
    for V, F in ((0, 0), (0, 2), (5, 0)):                       # faces over no vertices are all out of range
        m = sc._mesh(np.full((V, 3), 0.5), np.zeros((F, 3), np.int32), dims=(1, 1, 1))
        for explicit in (True, False):
            got, _ = check_simplify(m, "V %d F %d" % (V, F), explicit=explicit)
            assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.colors is None
    with pytest.raises(ValueError, match="smallest admissible cell_size"):
        mesh.simplify(_device_mesh([[0, 0, 0], [1, 1, 1]], [[0, 1, 0]]), 1e-4)       # 10^4 cells per axis
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            mesh.simplify(_device_mesh([[0, 0, 0], [1, 1, 1]], [[0, 1, 0]]), bad)


# ---- 2. the rank scan ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_one_vertex_per_cell_along_a_row(n):
    """n consecutive occupied cells: the block scan of sc_rank across lane, wavefront and workgroup edges; every vertex is its own cluster."""
    m = sc.row(n)
    got, want = check_simplify(m, "row %d" % n)
    assert want.count == n and want.cluster.tolist() == list(range(n))
    assert got.faces.shape[0] == max(n - 2, 0) and got.vertices.shape[0] == (n if n >= 3 else 0)
    if n >= 3:
        assert _same(got.vertices, m.vertices) and _same(got.colors, m.colors) and _same(got.faces, m.faces)     # singletons: nothing changes


def test_more_than_1024_workgroup_totals():
    m = sc.sparse_grid()
    assert (math.prod(m.dims) + 255) // 256 > 1024
    _, want = check_simplify(m, "sparse 65x65x63")
    lin = so.vertex_cells(m.vertices, m.origin, m.cell, m.dims)[1]
    assert lin.max() == math.prod(m.dims) - 1 and want.keep[-1]   # the last cell is occupied and its face survives


# ---- 3. the sums --------------------------------------------------------------------------------------------------------------------------------------
def test_one_giant_cluster():
    got, want = check_simplify(sc.giant(), "70 000 in one cell + 3")
    assert want.count == 4 and got.faces.tolist() == [[1, 3, 2], [0, 1, 2]]
    got, want = check_simplify(sc.giant(singletons=False), "70 000 in one cell")
    assert want.count == 1 and got.vertices.shape == (0, 3) and got.faces.shape == (0, 3)


def test_runs_of_equal_clusters_under_three_numberings():
    """Cells of 1, 2, 63, 64, 65 and 300 consecutive vertices: runs that start at every lane offset and straddle wavefronts; then the same mesh
    with its vertices numbered backwards and at random, where members of one cell are scattered.  Positions and colours must be the same BYTES:
    a mean summed with float atomics depends on the order of the adds and fails here."""
    m = sc.runs()
    base, want = check_simplify(m, "runs, identity")
    assert np.bincount(want.cluster).tolist() == list(sc.RUNS)
    for kind in ("reversed", "random"):
        got, _ = check_simplify(sc.renumber(m, sc.numbering(kind, m.vertices.shape[0])), "runs, " + kind)
        assert torch.equal(got.vertices.view(torch.int32), base.vertices.view(torch.int32)), kind
        assert torch.equal(got.colors.view(torch.int32), base.colors.view(torch.int32)), kind
        assert torch.equal(got.faces, base.faces), kind


def test_singletons_are_copied_bit_for_bit():
    """cell below the smallest vertex spacing; the wrapper sizes the grid itself (origin None)."""
    m = sc.spread()
    got, want = check_simplify(m, "spread", explicit=False)
    assert want.count == m.vertices.shape[0] and got.faces.shape[0] == int(want.keep.sum())
    used = np.unique(m.faces[want.keep])                         # the vertices a surviving face names
    order = used[np.argsort(want.cluster[used], kind="stable")]
    assert _same(got.vertices, m.vertices[order]) and _same(got.colors, m.colors[order])
    distinct = np.unique(np.sort(m.faces, axis=1), axis=0).shape[0]
    assert got.faces.shape[0] >= distinct                        # no face of distinct corners collapses; only repeats go


def test_fixed_point_range():
    m = sc.colour_range()
    got, want = check_simplify(m, "colour range")
    c = _np(got.colors)
    assert np.isfinite(c).all() and c.min() == 0.0 and c.max() == 255.0
    last = _np(got.vertices)[-1]                                 # the pair on and beyond the upper bound: offset 1 on every axis, both members
    assert last.tolist() == [float(m.dims[0]), 1.0, 1.0]


# ---- 4. faces -----------------------------------------------------------------------------------------------------------------------------------------
def test_face_rules():
    m = sc.face_rules()
    got, want = check_simplify(m, "face rules")
    assert want.keep.tolist() == [f in (0, 7, 10, 14) for f in range(m.faces.shape[0])]
    torch.cuda.synchronize()                                    # the run ends clean


def test_hash_table():
    one = sc._mesh(sc._TRI_V, [[2, 0, 1]], dims=(2, 2, 1))
    got, _ = check_simplify(one, "F = 1")
    assert got.faces.tolist() == [[2, 0, 1]]
    m = sc.rotations()
    got, want = check_simplify(m, "4096 copies")
    assert got.faces.shape[0] == 2 and got.faces[0].tolist() == m.faces[0].tolist() and int(want.keep.sum()) == 2
    d = sc.duplicates()
    assert d.faces.shape[0] == 300000
    got, want = check_simplify(d, "300 000 faces, each four times")
    assert got.faces.shape[0] <= 75000
    perm = np.random.default_rng(9).permutation(d.faces.shape[0])
    shuffled = sc._mesh(d.vertices, d.faces[perm], origin=d.origin, cell=d.cell, dims=d.dims)
    got2, want2 = check_simplify(shuffled, "300 000 faces, permuted")      # the lowest index wins: against the oracle on the permuted input
    assert got2.faces.shape[0] == got.faces.shape[0] and not np.array_equal(want2.keep, want.keep[perm])


# ---- 5. the C-ABI: bounds of writes, indices out of range ---------------------------------------------------------------------------------------------
CANARY = 0x5A


def _raw_cluster(m, pad=64, stream=None):
    """envgs_mesh_simplify_cluster on buffers with `pad` canary rows before and after every array the library reads by index or writes.
    -> namespace of NumPy arrays; asserts that no canary changed."""
    from envgs_amd import _lib
    lib = _lib.load()
    V, F = m.vertices.shape[0], m.faces.shape[0]
    nx, ny, nz = m.dims
    R = min(V, nx * ny * nz)

    def guarded(rows, width, dtype, fill=None):
        size = torch.empty(0, dtype=dtype).element_size()
        buf = torch.full(((rows + 2 * pad) * width * size,), CANARY, dtype=torch.uint8, device=DEV).view(dtype)
        if fill is not None:
            buf[pad * width:(pad + rows) * width] = torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)).to(DEV)
        return buf

    v = guarded(V, 3, torch.float32, m.vertices)
    c = guarded(V, 3, torch.float32, m.colors)
    f = guarded(F, 3, torch.int32, m.faces)
    cl_v, cl_c, cl_f = guarded(R, 3, torch.float32), guarded(R, 3, torch.float32), guarded(F, 3, torch.int32)
    keep, vc, count = guarded(F, 1, torch.uint8), guarded(V, 1, torch.int32), guarded(1, 1, torch.int32)
    tb = lib.envgs_mesh_simplify_temp_bytes(V, F, nx, ny, nz)
    temp = torch.full((tb + 512,), CANARY, dtype=torch.uint8, device=DEV)
    toff = (-temp.data_ptr()) % 256                              # an aligned window with canaries on both sides
    at = lambda buf, width: _lib.ctypes.c_void_p(buf.data_ptr() + pad * width * buf.element_size())
    s = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream.cuda_stream
    rc = lib.envgs_mesh_simplify_cluster(V, F, at(v, 3), at(c, 3), at(f, 3), m.origin[0], m.origin[1], m.origin[2], m.cell, nx, ny, nz,
                                         _lib.ctypes.c_void_p(temp.data_ptr() + toff), tb, at(cl_v, 3), at(cl_c, 3), at(cl_f, 3), at(keep, 1), at(vc, 1),
                                         at(count, 1), _lib.ctypes.c_void_p(s))
    assert rc == 0
    torch.cuda.synchronize()
    C = int(count[pad])
    word = lambda buf: buf.view(torch.uint8)

    def untouched(buf, width, rows):
        b, e = word(buf), buf.element_size()
        return bool((b[:pad * width * e] == CANARY).all()) and bool((b[(pad + rows) * width * e:] == CANARY).all())

    assert untouched(cl_v, 3, C) and untouched(cl_c, 3, C), "rows at or beyond C were written"
    assert untouched(cl_f, 3, F) and untouched(keep, 1, F) and untouched(vc, 1, V) and untouched(count, 1, 1)
    assert untouched(v, 3, V) and untouched(c, 3, V) and untouched(f, 3, F)
    assert bool((temp[:toff] == CANARY).all()) and bool((temp[toff + tb:] == CANARY).all())
    body = lambda buf, width, rows: buf[pad * width:(pad + rows) * width].reshape(rows, width).cpu().numpy()
    return SimpleNamespace(count=C, cl_vertices=body(cl_v, 3, C), cl_colors=body(cl_c, 3, C), mapped=body(cl_f, 3, F), keep=body(keep, 1, F).reshape(-1),
                           cluster=body(vc, 1, V).reshape(-1))


@pytest.mark.parametrize("case", ["face_rules", "runs", "colour_range", "sparse_grid"])
def test_nothing_outside_the_documented_rows_is_written(case):
    """The outputs of the clustering call sit between canaries: rows C .. R-1 of the representatives stay untouched, and so does everything around
    the arrays.  In face_rules the indices -1, V, 2^31 - 1 and -2^31 stand beside canary-guarded vertex and cluster arrays whose canary words
    read as valid numbers: were one dereferenced, the mapped face would not be the oracle's -1."""
    m = getattr(sc, case)()
    want = so.simplify(m.vertices, m.faces, m.colors, m.origin, m.cell, m.dims)
    for _ in range(2):
        got = _raw_cluster(m)
        assert got.count == want.count and (case != "sparse_grid" or got.count < min(m.vertices.shape[0], math.prod(m.dims)))
        assert np.array_equal(got.cluster, want.cluster) and np.array_equal(got.mapped, want.mapped)
        assert np.array_equal(got.keep.astype(bool), want.keep)
        assert np.array_equal(_bits(got.cl_vertices), _bits(want.cl_vertices)) and np.array_equal(_bits(got.cl_colors), _bits(want.cl_colors))


def test_selection_writes_nothing_beyond_the_survivors():
    """simplify() sizes its outputs exactly; here the two selection calls run on the clustered mesh with larger, canary-filled outputs."""
    from envgs_amd import _lib
    lib = _lib.load()
    m = sc.runs()
    want = so.simplify(m.vertices, m.faces, m.colors, m.origin, m.cell, m.dims)
    raw = _raw_cluster(m)
    V, F = m.vertices.shape[0], m.faces.shape[0]
    R = min(V, math.prod(m.dims))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cl_v = torch.zeros(R, 3, device=DEV)
    cl_v[:raw.count] = t(raw.cl_vertices)
    cl_f, keep = t(raw.mapped), t(raw.keep)
    tb = lib.envgs_mesh_select_temp_bytes(R, F)
    temp = torch.empty(tb, dtype=torch.uint8, device=DEV)
    totals = torch.empty(2, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    assert lib.envgs_mesh_select_count(R, F, p(cl_f), p(keep), p(temp), tb, p(totals), None) == 0
    Vo, Fo = totals.tolist()
    assert (Vo, Fo) == (want.vertices.shape[0], want.faces.shape[0])
    out_v = torch.full((Vo + 16, 3), -7.0, device=DEV)
    out_f = torch.full((Fo + 16, 3), -7, dtype=torch.int32, device=DEV)
    assert lib.envgs_mesh_select_emit(R, F, p(cl_v), None, p(cl_f), p(keep), p(temp), tb, Vo, Fo, p(out_v), None, p(out_f), None, None) == 0
    torch.cuda.synchronize()
    assert _same(out_v[:Vo], want.vertices) and _same(out_f[:Fo], want.faces)
    assert bool((out_v[Vo:] == -7.0).all()) and bool((out_f[Fo:] == -7).all())


def test_on_the_callers_stream():
    m = sc.runs()
    base, _ = check_simplify(m, "default stream")
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got, _ = check_simplify(m, "side stream")
    side.synchronize()
    assert torch.equal(got.vertices.view(torch.int32), base.vertices.view(torch.int32)) and torch.equal(got.faces, base.faces)
    want = so.simplify(m.vertices, m.faces, m.colors, m.origin, m.cell, m.dims)
    raw = _raw_cluster(m, stream=side)
    assert np.array_equal(raw.cluster, want.cluster) and np.array_equal(_bits(raw.cl_vertices), _bits(want.cl_vertices))


# ---- 6. tied to the extractor ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.SPHERES))
def test_simplified_extraction_equals_the_oracles(name):
    """The shapes and grids of the "40x36x32" and "37x35x33" volumes of tests/mesh_cases.py with an analytic sphere in them: extracted on the device,
    simplified on the device at 2 and 3 voxels from the volume's origin.  (a) equals the oracle's simplification of the device's own mesh;
    (b) equals the oracle's simplification of the ORACLE's extraction, array for array."""
    from envgs_amd import mesh
    s = sc.sphere(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    vol = mesh.TSDFVolume.from_tensors(t(s.tsdf), t(np.ones_like(s.tsdf)), t(s.rgb), s.origin, s.voxel)
    m = vol.extract()
    gv, gf, gc = _np(m.vertices), _np(m.faces), _np(m.colors)
    print("%s: extraction V %d F %d; device against oracle: faces equal %s, max vertex difference %.3g voxel, max colour difference %.3g"
          % (name, gv.shape[0], gf.shape[0], np.array_equal(gf, s.mesh.faces), np.abs(gv - s.mesh.vertices).max() / s.voxel, np.abs(gc - s.mesh.colors).max()))
    for k in (2, 3):
        cell = k * s.voxel
        got, index = mesh.simplify(m, cell, origin=vol.origin, return_index=True)
        again, index2 = mesh.simplify(m, cell, origin=vol.origin, return_index=True)
        assert torch.equal(got.vertices, again.vertices) and torch.equal(got.faces, again.faces) and torch.equal(got.colors, again.colors)
        assert torch.equal(index, index2)
        origin, dims = so.grid_of(gv, cell, vol.origin)
        own = so.simplify(gv, gf, gc, origin, cell, dims)
        print("%s, %d voxels: V %d -> %d, F %d -> %d" % (name, k, gv.shape[0], got.vertices.shape[0], gf.shape[0], got.faces.shape[0]))
        _assert_equals_oracle(got, index, own, "%s k %d, the device's mesh" % (name, k))
        assert 0 < got.faces.shape[0] < gf.shape[0] and 0 < got.vertices.shape[0] < gv.shape[0]
        dist = (got.vertices.double() - torch.tensor(s.centre, dtype=torch.float64, device=DEV)).norm(dim=1) - s.radius
        assert float(dist.abs().max()) <= cell * math.sqrt(3.0) + 1e-5 * s.voxel
        o_origin, o_dims = so.grid_of(s.mesh.vertices, cell, vol.origin)
        ref = so.simplify(s.mesh.vertices, s.mesh.faces, s.mesh.colors, o_origin, cell, o_dims)
        dv = np.abs(_np(got.vertices) - ref.vertices).max() if tuple(got.vertices.shape) == ref.vertices.shape else float("nan")
        print("%s, %d voxels: against the oracle's simplification of the oracle's extraction: V %d (oracle %d) F %d (oracle %d), max vertex difference %.3g"
              % (name, k, got.vertices.shape[0], ref.vertices.shape[0], got.faces.shape[0], ref.faces.shape[0], dv))
        _assert_equals_oracle(got, index, ref, "%s k %d, the oracle's mesh" % (name, k))


@pytest.fixture(scope="module")
def two_spheres():
    """The scene of tests/test_mesh_clean_gpu.py::test_fuse_extract_clean_end_to_end: the Fibonacci sphere of surfels plus a blob above it, fused
    from eight rendered views and extracted.  -> (volume, mesh)"""
    from envgs_amd import mesh, synth
    from tests.test_mesh_clean_gpu import BLOB_C, BLOB_R, E2E_HI, E2E_LO, E2E_VOXEL
    from tests.test_mesh_gpu import _sphere_surfels
    main, blob = _sphere_surfels(), _sphere_surfels(P=1024, radius=BLOB_R)
    blob["means3D"] = (blob["means3D"] + torch.tensor(BLOB_C, device=DEV)).contiguous()
    blob["scales"] = torch.full_like(blob["scales"], 0.015)
    base = {k: torch.cat([main[k], blob[k]]).contiguous() for k in main}
    cams = [synth.orbit_camera(v, n_views=8, radius=3.0, H=96, W=96, fx=120.0, n=0.5, f=6.0, device=DEV) for v in range(8)]
    vol = mesh.TSDFVolume(E2E_LO, E2E_HI, E2E_VOXEL, device=DEV)
    mesh.fuse_surfels(vol, cams, base, sh_degree=0, alpha_min=0.5)
    return vol, vol.extract()


def test_clean_and_simplify_in_both_orders(two_spheres):
    from envgs_amd import mesh
    vol, m = two_spheres
    arrays = _np(m.vertices), _np(m.faces), _np(m.colors)
    cell = 2 * vol.voxel_size
    kw = dict(keep_largest=1, min_faces=0)
    # simplify(clean(.))
    got = mesh.simplify(mesh.clean(m, **kw), cell, origin=vol.origin)
    c = co.clean(*arrays, **kw)
    origin, dims = so.grid_of(c.vertices, cell, vol.origin)
    want = so.simplify(c.vertices, c.faces, c.colors, origin, cell, dims)
    print("simplify(clean): F %d -> %d -> %d" % (m.faces.shape[0], c.faces.shape[0], got.faces.shape[0]))
    assert _same(got.vertices, want.vertices) and _same(got.faces, want.faces) and _same(got.colors, want.colors)
    assert 0 < got.faces.shape[0] < c.faces.shape[0]
    # clean(simplify(.))
    got = mesh.clean(mesh.simplify(m, cell, origin=vol.origin), **kw)
    origin, dims = so.grid_of(arrays[0], cell, vol.origin)
    s = so.simplify(*arrays, origin, cell, dims)
    want = co.clean(s.vertices, s.faces, s.colors, **kw)
    print("clean(simplify): F %d -> %d -> %d" % (m.faces.shape[0], s.faces.shape[0], got.faces.shape[0]))
    assert _same(got.vertices, want.vertices) and _same(got.faces, want.faces) and _same(got.colors, want.colors)
    assert 0 < got.faces.shape[0] < s.faces.shape[0]


def test_fuse_extract_clean_simplify_end_to_end(two_spheres):
    """Every vertex of the cleaned mesh is within trunc + sqrt(3) voxel of radius 0.6 (tests/test_mesh_clean_gpu.py); a simplified vertex is a mean
    of vertices of one cell (or one of them), so within the cell's diagonal of them."""
    from envgs_amd import mesh
    from tests.test_mesh_clean_gpu import MAIN_R
    vol, m = two_spheres
    cleaned = mesh.clean(m, keep_largest=1, min_faces=0)
    for k in (2, 3):
        cell = k * vol.voxel_size
        got, again = mesh.simplify(cleaned, cell, origin=vol.origin), mesh.simplify(cleaned, cell, origin=vol.origin)
        assert torch.equal(got.vertices, again.vertices) and torch.equal(got.faces, again.faces) and torch.equal(got.colors, again.colors)
        band = vol.trunc + math.sqrt(3.0) * vol.voxel_size + cell * math.sqrt(3.0)
        dev = float((got.vertices.norm(dim=1) - MAIN_R).abs().max())
        print("end to end, %d voxels: V %d -> %d, F %d -> %d, max |radius - 0.6| %.4f (band %.4f)"
              % (k, cleaned.vertices.shape[0], got.vertices.shape[0], cleaned.faces.shape[0], got.faces.shape[0], dev, band))
        assert 0 < got.faces.shape[0] < cleaned.faces.shape[0] and 0 < got.vertices.shape[0] < cleaned.vertices.shape[0]
        assert dev <= band
        assert int(got.faces.min()) == 0 and int(got.faces.max()) == got.vertices.shape[0] - 1
