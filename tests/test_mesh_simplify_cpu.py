"""CPU: the mesh simplification oracle (tests/mesh_simplify_oracle.py) on hand-made meshes whose answers are typed in, its independence of the vertex
numbering, the geometry of a simplified analytic sphere, the face table of csrc/mesh_facehash.h built for the host and run by several threads
against the oracle, the argument checks of the C-ABI that need no GPU, and the grid rule of envgs_amd.mesh.simplify_grid.  (The HIP kernels are
compared against the same oracle in tests/test_mesh_simplify_gpu.py.)"""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_simplify_cases as sc
from tests import mesh_simplify_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run(m):
    return so.simplify(m.vertices, m.faces, m.colors, m.origin, m.cell, m.dims)


# ---- 1. hand-made meshes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.HAND))
def test_oracle_on_hand_made_meshes(name):
    m, vertices, faces, colors, vertex_cluster = sc.HAND[name]
    got = _run(m)
    assert np.array_equal(_bits(got.vertices), _bits(np.asarray(vertices, F32).reshape(-1, 3)))
    assert got.faces.dtype == np.int32 and np.array_equal(got.faces, np.asarray(faces, np.int32).reshape(-1, 3))
    assert got.vertex_cluster.tolist() == vertex_cluster
    if colors is None:
        assert got.colors is None
    else:
        assert np.array_equal(_bits(got.colors), _bits(np.asarray(colors, F32).reshape(-1, 3)))


def test_dedup_keeps_the_lowest_index_of_each_rotation_class():
    mapped = [[3, 1, 2], [1, 2, 3], [2, 1, 3], [2, 3, 1], [1, 3, 2], [5, 5, 6], [1, 2, 3]]
    cand = [True, True, True, True, True, False, False]
    assert so.dedup_faces(mapped, cand).tolist() == [True, False, True, False, False, False, False]
    cand[0] = False                                              # a face dropped earlier hides nothing
    assert so.dedup_faces(mapped, cand).tolist() == [False, True, True, False, False, False, False]


# ---- 2. the numbering of the vertices does not matter -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["runs", "sparse_grid", "colour_range", "face_rules"])
def test_oracle_does_not_depend_on_the_vertex_numbering(case):
    m = getattr(sc, case)()
    base = _run(m)
    assert base.faces.shape[0] > 0
    for kind in ("reversed", "random"):
        perm = sc.numbering(kind, m.vertices.shape[0])
        other = _run(sc.renumber(m, perm))
        assert np.array_equal(_bits(other.vertices), _bits(base.vertices)) and np.array_equal(_bits(other.colors), _bits(base.colors))
        assert np.array_equal(other.faces, base.faces)
        assert np.array_equal(other.vertex_cluster[perm], base.vertex_cluster)


def test_generated_cases_reach_what_they_name():
    r = _run(sc.runs())
    assert np.bincount(r.cluster).tolist() == list(sc.RUNS)
    g = _run(sc.giant())
    assert g.count == 4 and g.faces.tolist() == [[1, 3, 2], [0, 1, 2]] and np.bincount(g.cluster).tolist() == [70000, 1, 1, 1]
    e = _run(sc.giant(singletons=False))
    assert e.count == 1 and e.vertices.shape == (0, 3) and e.faces.shape == (0, 3) and (e.vertex_cluster == -1).all()
    s = sc.sparse_grid()
    cells = math.prod(s.dims)
    assert (cells + 255) // 256 > 1024 and _run(s).cluster.max() == _run(s).count - 1
    assert so.vertex_cells(s.vertices, s.origin, s.cell, s.dims)[1].max() == cells - 1
    rot = _run(sc.rotations())
    assert rot.keep.sum() == 2 and rot.keep[0]
    sp = sc.spread()
    origin, dims = so.grid_of(sp.vertices, sp.cell)
    one = so.simplify(sp.vertices, sp.faces, sp.colors, origin, sp.cell, dims)
    assert one.count == sp.vertices.shape[0] and np.array_equal(_bits(one.cl_vertices[one.cluster]), _bits(sp.vertices))
    assert np.array_equal(_bits(one.cl_colors[one.cluster]), _bits(sp.colors))


# ---- 3. geometry on the analytic sphere -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.SPHERES))
@pytest.mark.parametrize("k", [2, 3])
def test_simplified_sphere_stays_within_a_cell_diagonal(name, k):
    """A mean lies in the convex hull of members that share a cell, so it is within the cell's diagonal of each of them; the members are within the
    extractor's own vertex bound, 1e-5 voxel, of the sphere."""
    s = sc.sphere(name)
    cell = k * s.voxel
    dims = tuple((n - 1) // k + 1 for n in s.dims)
    got = so.simplify(s.mesh.vertices, s.mesh.faces, s.mesh.colors, s.origin, cell, dims)
    V, F = s.mesh.vertices.shape[0], s.mesh.faces.shape[0]
    assert 0 < got.faces.shape[0] < F and 0 < got.vertices.shape[0] < V
    dist = np.abs(np.linalg.norm(got.vertices.astype(np.float64) - np.asarray(s.centre), axis=1) - s.radius)
    assert dist.max() <= cell * math.sqrt(3.0) + 1e-5 * s.voxel
    assert got.faces.min() == 0 and got.faces.max() == got.vertices.shape[0] - 1
    assert (got.colors >= 0).all() and (got.colors <= 1).all()


# ---- 4. the face table on the host ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_facehash(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_facehash")
    exe = str(d / "mesh_facehash_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "envgs_amd", "csrc", "mesh_facehash_host.cpp")], check=True)

    def run(mapped, cand, threads):
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        mapped = np.ascontiguousarray(mapped, np.int32).reshape(-1, 3)
        with open(src, "wb") as f:
            f.write(np.array([mapped.shape[0]], np.uint32).tobytes() + mapped.tobytes() + np.ascontiguousarray(cand, np.uint8).tobytes())
        subprocess.run([exe, src, dst, str(threads)], check=True)
        return np.fromfile(dst, np.uint8).astype(bool)
    return run


@pytest.mark.parametrize("threads", [4, 7])
def test_host_face_table_equals_the_oracle(host_facehash, threads):
    for m in (sc.rotations(), sc.duplicates(unique=20000, side=20), sc.face_rules(), sc.HAND["a face and its reverse"][0]):
        want = _run(m)
        cand = (want.mapped >= 0).all(axis=1) & (want.mapped[:, 0] != want.mapped[:, 1]) & (want.mapped[:, 1] != want.mapped[:, 2]) \
            & (want.mapped[:, 2] != want.mapped[:, 0])
        got = host_facehash(want.mapped, cand, threads)
        assert np.array_equal(got, want.keep)
        assert want.keep.sum() < cand.sum() or m.faces.shape[0] < 10
    assert host_facehash(np.zeros((0, 3), np.int32), np.zeros(0, np.uint8), threads).shape == (0,)


# ---- 5. the C-ABI -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from envgs_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_bad_arguments_are_rejected_before_any_gpu_work(lib):
    FAKE = 0x1000                                               # never dereferenced on the host; rejected calls launch nothing
    BIG = 1 << 31
    inf, nan = float("inf"), float("nan")
    call = lambda V=8, F=4, v=FAKE, c=None, faces=FAKE, o=(0.0, 0.0, 0.0), cell=1.0, dims=(4, 4, 4), temp=FAKE, tb=1 << 40, cv=FAKE, cc=None, cf=FAKE, \
        keep=FAKE, vc=FAKE, count=FAKE: lib.envgs_mesh_simplify_cluster(V, F, v, c, faces, o[0], o[1], o[2], cell, dims[0], dims[1], dims[2], temp, tb, cv, cc,
                                                                        cf, keep, vc, count, None)
    for bad in (dict(V=BIG), dict(F=BIG), dict(v=None), dict(faces=None), dict(temp=None), dict(temp=FAKE + 8), dict(cv=None), dict(cf=None),
                dict(keep=None), dict(vc=None), dict(count=None), dict(cc=FAKE),          # colours asked for, none given
                dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(o=(nan, 0.0, 0.0)), dict(o=(0.0, 0.0, inf)),
                dict(dims=(0, 4, 4)), dict(dims=(4, -1, 4)), dict(dims=(2048, 1024, 1024)), dict(dims=(65536, 65536, 1)),
                dict(dims=(2 ** 31 - 1, 2, 1))):
        assert call(**bad) == -1, bad
    tbytes = lib.envgs_mesh_simplify_temp_bytes
    need = tbytes(1000, 3000, 10, 10, 10)
    slots = 8192                                                 # the power of two >= 2 * 3000
    model = 1000 + 60 * 1000 + 4 * 3000 + 4 * slots              # 1 B per cell, 60 B per row of min(V, cells), 4 B per face, 4 B per slot
    assert model <= need < model + 8192
    assert tbytes(BIG, 4, 2, 2, 2) == 0 and tbytes(4, BIG, 2, 2, 2) == 0 and tbytes(4, 4, 0, 2, 2) == 0 and tbytes(4, 4, 2048, 1024, 1024) == 0
    assert tbytes(4, 4, 2047, 1024, 1024) > 0                    # 2^31 - 2^20 cells: in range
    assert call(V=1000, F=3000, dims=(10, 10, 10), tb=need - 1) == -2


# ---- 6. Python: CPU tensors, the grid --------------------------------------------------------------------------------------------------------------------
def test_simplify_on_cpu_tensors_raises():
    import torch
    from envgs_amd import mesh
    m = mesh.Mesh(vertices=torch.zeros(3, 3), faces=torch.zeros(1, 3, dtype=torch.int32), colors=None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.simplify(m, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.simplify(m, 0.5, origin=(0, 0, 0), return_index=True)
