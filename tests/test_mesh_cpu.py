"""CPU: the mesh oracle's own acceptance test on analytic level sets, the case table of tests/mesh_cases.py on the oracle alone (every
configuration is one the GPU comparison can judge), the mesh PLY round trip, and the argument checks of the mesh C-ABI that need no GPU.
(The HIP kernels are compared against this oracle in tests/test_mesh_gpu.py and tests/test_mesh_shapes_gpu.py.)"""
import ctypes

import numpy as np
import pytest

from tests import mesh_cases as mc
from tests import mesh_oracle as mo

DIMS = (14, 12, 10)
CENTRE = (6.37, 5.61, 4.83)


def _extract(vol):
    return mo.marching_tetrahedra(vol, np.ones_like(vol), None, (0.0, 0.0, 0.0), 1.0)


@pytest.fixture(scope="module")
def sphere():
    return _extract(mo.sphere_volume(DIMS, CENTRE, 3.217))


@pytest.fixture(scope="module")
def torus():
    return _extract(mo.torus_volume(DIMS, CENTRE, 3.1, 1.27))


def test_oracle_sphere_is_a_closed_oriented_sphere(sphere):
    assert sphere.vertices.shape == (566, 3) and sphere.faces.shape == (1128, 3)
    top = mo.mesh_topology(sphere.faces, 566)
    assert top.closed_oriented and top.all_referenced and top.euler == 2


def test_oracle_torus_is_a_closed_oriented_torus(torus):
    assert torus.vertices.shape == (686, 3) and torus.faces.shape == (1372, 3)
    top = mo.mesh_topology(torus.faces, 686)
    assert top.closed_oriented and top.all_referenced and top.euler == 0


def test_oracle_sphere_normals_point_outward(sphere):
    p = sphere.vertices.astype(np.float64)[sphere.faces]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", n, p.mean(axis=1) - np.array(CENTRE)) > 0).all()
    # and every vertex lies on its crossed edge, close to the analytic surface (linear interpolation of a distance field over <= sqrt(3) voxels)
    assert np.abs(np.linalg.norm(p.reshape(-1, 3) - np.array(CENTRE), axis=1) - 3.217).max() < 0.15


def test_oracle_orders_vertices_and_faces_canonically(sphere, torus):
    for m in (sphere, torus):
        key = m.vertex_owner * 7 + m.vertex_slot
        assert (np.diff(key) > 0).all()
        assert (np.diff(m.face_cell) >= 0).all()
        assert np.array_equal(mo.face_cells(m.faces, m.vertex_owner, m.vertex_slot, DIMS), m.face_cell)


def test_oracle_case_table_counts():
    table = mo.case_table()
    assert len(table) == 6 and sorted(set(mo.kuhn_tetrahedra())) == sorted(mo.kuhn_tetrahedra())
    for row in table:
        assert [len(t) for t in row] == [0 if bin(m).count("1") in (0, 4) else 2 if bin(m).count("1") == 2 else 1 for m in range(16)]


def test_oracle_integration_float32_and_float64_agree_off_the_fragile_voxels():
    """One analytic view: the float64 shadow lists the fragile voxels, and everywhere else the float32 run takes the same decisions."""
    dims, voxel, origin = (10, 9, 8), 0.1, (-0.4531, -0.4127, 0.6131)
    H, W = 24, 32
    K = [[30.0, 0, W / 2 + 0.37], [0, 31.1, H / 2 - 0.21], [0, 0, 1]]
    depth = np.full((H, W), 1.0, np.float32)
    depth[:, :5] = 0.0
    view = mo.make_view(depth, K, np.eye(3), np.zeros(3), rgb=np.random.default_rng(0).random((3, H, W), dtype=np.float32), trunc=0.3)
    z = np.ones((dims[2], dims[1], dims[0]), np.float32)
    D32, W32, C32, _ = mo.integrate(z, 0 * z, np.zeros((3,) + z.shape, np.float32), origin, voxel, [view, view], dtype=np.float32)
    D64, W64, C64, frag = mo.integrate(z, 0 * z, np.zeros((3,) + z.shape, np.float32), origin, voxel, [view, view], dtype=np.float64)
    assert frag.mean() < 0.05 and (W64 > 0).any() and (W64 == 0).any()
    keep = ~frag
    assert np.array_equal(W32[keep], W64[keep])
    assert np.abs(D32 - D64)[keep].max() < 1e-6 and np.abs(C32 - C64)[:, keep].max() < 1e-6
    # the scalar restatement equals the vectorised one, voxel by voxel
    for ijk in ((0, 0, 0), (5, 4, 3), (9, 8, 7), (2, 7, 1)):
        d, w, c = mo.integrate_voxel(ijk, (1.0, 0.0, (0.0, 0.0, 0.0)), origin, voxel, [view, view], 64.0, 0.3, [(0, 0, False)] * 2)
        at = (ijk[2], ijk[1], ijk[0])
        assert d == D32[at] and w == W32[at] and all(c[q] == C32[(q,) + at] for q in range(3))


@pytest.mark.parametrize("name", list(mc.INTEGRATION))
def test_integration_case_table_meets_the_conditions_of_check_fused(name):
    """Every integration configuration of tests/mesh_cases.py, on the oracle alone: what test_mesh_gpu.check_fused asserts before it compares
    anything.  The 1 % cap on the fragile share is a condition, not a measurement: a row that breaks it gets another origin, off the cameras'
    symmetry planes."""
    c = mc.oracle_conditions(name)
    print("%s: fragile %d of %d voxels (%.2f %%), observed %d, unobserved %d, f32/f64 weight disagreements off the fragile voxels %d"
          % (name, c.fragile, c.n, 100 * c.share, c.observed, c.unobserved, c.disagree))
    assert c.share <= 0.01
    assert c.observed > 0.02 * c.n
    assert c.unobserved >= 1
    assert c.disagree == 0
    assert c.finite                                             # NaN / inf depth pixels are skipped or give val = 1, never a NaN in the volume
    dims = mc.INTEGRATION[name][0]
    if max(dims) > 4:                                           # beyond the tiny rows: the surface itself is seen, by overlapping views
        assert c.max_weight >= 2.0 and c.min_tsdf < -0.4


def test_integration_case_table_reaches_the_paths_it_names():
    n = {k: int(np.prod(v[0])) for k, v in mc.INTEGRATION.items()}
    assert [n[k] % 4 for k in ("37x35x33", "41x37x33", "5x3x2", "7x5x3", "40x36x32")] == [3, 1, 2, 1, 0]
    assert n["2x3x171"] == 1026 and n["40x36x32"] % 1024 == 0 and mc.INTEGRATION["1027x2x2"][0][0] > 1024
    dims, voxel, lo, _ = mc.INTEGRATION["ragged e2e"]            # the dimensions TSDFVolume(lo, hi, voxel) rounds to: odd on every axis
    assert tuple(int(np.ceil((h - l) / voxel - 1e-9)) + 1 for l, h in zip(lo, mc.E2E_HI)) == dims and all(d % 2 == 1 and d <= 45 for d in dims)
    kinds = {v[3] for v in mc.INTEGRATION.values()}
    assert kinds == {"orbit", "inside", "mixed", "e2e"}
    inside = mc.view_set("inside")
    assert len(inside) == 5
    X, Y, Z = mo.voxel_positions((37, 35, 33), mc.INTEGRATION["inside"][2], 0.05, np.float64)
    for v in inside:                                            # the camera stands inside the sphere: voxels on both sides of its image plane
        centre = -v.R.astype(np.float64).T @ v.T
        assert np.linalg.norm(centre - np.array(mc.base.SPHERE_C)) < mc.base.SPHERE_R
        zc = v.R[2, 0] * X + v.R[2, 1] * Y + v.R[2, 2] * Z + v.T[2]
        assert (zc > 0).mean() > 0.1 and (zc <= 0).mean() > 0.1
        assert np.isnan(v.depth).sum() > 20 and np.isposinf(v.depth).sum() > 20 and (v.depth < 0).sum() > 20
    mixed = mc.view_set("mixed")
    assert len({v.depth.shape for v in mixed}) == 2 and len({float(v.trunc) for v in mixed}) > 2 and len({float(v.depth_max) for v in mixed}) > 2
    assert {v.rgb is None for v in mixed} == {True, False}
    for v in mixed:                                             # depth_max cuts a part of every view it is set on, never all of it
        if np.isfinite(v.depth_max):
            assert ((v.depth > 0) & (v.depth <= v.depth_max)).any() and (v.depth > v.depth_max).any()


@pytest.mark.parametrize("name", mc.EXTRACTION)
def test_extraction_case_table_gives_the_meshes_it_names(name):
    e = mc.extraction(name)
    nz, ny, nx = e.tsdf.shape
    weight = np.ones_like(e.tsdf) if e.weight is None else e.weight
    ref = mo.marching_tetrahedra(e.tsdf, weight, None, e.origin, e.voxel, level=e.level, min_weight=e.min_weight)
    V, F = ref.vertices.shape[0], ref.faces.shape[0]
    top = mo.mesh_topology(ref.faces, V)
    print("%s: V %d F %d, closed %s, euler %d" % (name, V, F, top.closed_oriented, top.euler))
    assert V > 0 and F > 0 and top.all_referenced and np.isfinite(ref.vertices).all()
    assert top.closed_oriented == (e.euler is not None) and (e.euler is None or top.euler == e.euler)
    if name == "thin 2x2x2":
        assert (V, F) == (7, 6)                                 # one corner inside: its 7 edges, the 6 tetrahedra around it
    if name in ("thin 2x2x300", "thin 300x2x2", "thin 2x300x2", "thin 257x2x2"):
        assert (V, F) == (18, 16)
    if name == "big":
        assert (V, F) == (20100, 40196) and (nx * ny * nz + 255) // 256 > 1024
    if "level" in name or "sample" in name:                     # samples exactly on the level: not inside, t == 0 on the edges they own
        flat, d = e.tsdf.reshape(-1), np.array(mo.SLOT_DIRS)[ref.vertex_slot]
        t0 = flat[ref.vertex_owner] == np.float32(e.level)
        t1 = flat[ref.vertex_owner + d[:, 0] + d[:, 1] * nx + d[:, 2] * nx * ny] == np.float32(e.level)
        print("%s: %d samples equal the level, %d vertices with t == 0, %d with t == 1" % (name, (e.tsdf == np.float32(e.level)).sum(), t0.sum(), t1.sum()))
        assert {"plane on the level": t0.sum() >= 3, "plane under the level": t1.sum() >= 3, "torus on a sample": t0.sum() + t1.sum() >= 1}[name]
    if name.startswith("last corner"):
        assert nx * ny * nz % 4 == 3 and ref.face_cell.max() == ((nz - 2) * ny + ny - 2) * nx + nx - 2
    if name.startswith("min_weight"):
        assert sorted(np.unique(weight)) == [0.0, 0.5, 1.0, 3.0]
        ones = mo.marching_tetrahedra(e.tsdf, weight, None, e.origin, e.voxel, min_weight=1.0)
        full = mo.marching_tetrahedra(e.tsdf, np.ones_like(weight), None, e.origin, e.voxel)
        # the threshold is what decides: 0.75 separates the weights as 1 does, 0.5 lets the 0.5 voxels in
        assert F < full.faces.shape[0] and (F == ones.faces.shape[0] if e.min_weight == 0.75 else F > ones.faces.shape[0])
        ck, r = np.divmod(ref.face_cell, nx * ny)
        cj, ci = np.divmod(r, nx)
        corner = np.stack([weight[ck + ((c >> 2) & 1), cj + ((c >> 1) & 1), ci + (c & 1)] for c in range(8)])
        assert (corner >= e.min_weight).all() and (corner == 0.5).any() == (e.min_weight == 0.5)


def test_mesh_ply_round_trip(tmp_path, sphere):
    from envgs_amd import ckpt
    rng = np.random.default_rng(1)
    colors = rng.random((566, 3)).astype(np.float32) * 1.2 - 0.1                # some outside [0, 1]: clamped
    p = str(tmp_path / "m.ply")
    ckpt.save_mesh_ply(p, sphere.vertices, sphere.faces)
    v, f, c = ckpt.load_mesh_ply(p)
    assert c is None and v.dtype == np.float32 and f.dtype == np.int32
    assert np.array_equal(v, sphere.vertices) and np.array_equal(f, sphere.faces)
    import torch
    ckpt.save_mesh_ply(p, torch.from_numpy(sphere.vertices), torch.from_numpy(sphere.faces), torch.from_numpy(colors))
    v, f, c = ckpt.load_mesh_ply(p)
    assert np.array_equal(v, sphere.vertices) and np.array_equal(f, sphere.faces)
    assert c.dtype == np.uint8 and np.array_equal(c, np.rint(np.clip(colors.astype(np.float64), 0, 1) * 255).astype(np.uint8))
    head = open(p, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"] and "property list uchar int vertex_indices" in head
    assert [h for h in head if h.startswith("property") and "list" not in h] == ["property float x", "property float y", "property float z",
                                                                                  "property uchar red", "property uchar green", "property uchar blue"]
    ckpt.save_mesh_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v, f, c = ckpt.load_mesh_ply(p)
    assert v.shape == (0, 3) and f.shape == (0, 3)


@pytest.fixture(scope="module")
def lib():
    from envgs_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_bad_arguments_are_rejected_before_any_gpu_work(lib):
    from envgs_amd import _lib
    FAKE = 0x1000                                                               # never dereferenced on the host; rejected calls launch nothing

    def vol(nx=8, ny=8, nz=8, voxel=0.1, tsdf=FAKE, weight=FAKE):
        return _lib.TsdfVolume(nx, ny, nz, 0.0, 0.0, 0.0, voxel, tsdf, weight, None)

    def views(count=1, depth=FAKE, trunc=0.5):
        vs = _lib.TsdfViews()
        vs.count = count
        for q in range(min(count, 8)):
            v = vs.v[q]
            v.depth, v.H, v.W, v.fx, v.fy, v.trunc, v.depth_max = depth, 4, 4, 1.0, 1.0, trunc, float("inf")
        return vs

    bad_volumes = [vol(nx=1), vol(nz=1), vol(ny=2049), vol(voxel=0.0), vol(voxel=-1.0), vol(voxel=float("nan")), vol(nx=2048, ny=2048, nz=512),
                   vol(tsdf=None), vol(weight=None)]
    for v in bad_volumes:
        assert lib.envgs_tsdf_integrate(v, views(), 64.0, None) == -1
        assert lib.envgs_mesh_count(v, 0.0, 1.0, FAKE, 1 << 30, FAKE, None) == -1
        assert lib.envgs_mesh_extract(v, 0.0, FAKE, 1 << 30, 0, 0, None, None, None, None) == -1
    for vs in (views(count=9), views(count=0), views(depth=None), views(trunc=0.0)):
        assert lib.envgs_tsdf_integrate(vol(), vs, 64.0, None) == -1
    assert lib.envgs_tsdf_integrate(vol(), None, 64.0, None) == -1
    assert lib.envgs_tsdf_integrate(None, views(), 64.0, None) == -1
    assert lib.envgs_tsdf_integrate(vol(), views(), 0.0, None) == -1
    assert lib.envgs_mesh_temp_bytes(1, 8, 8) == 0 and lib.envgs_mesh_temp_bytes(2048, 2048, 512) == 0
    need = lib.envgs_mesh_temp_bytes(8, 8, 8)
    assert 4 * 512 <= need < 4 * 512 + 4096                                     # 4 B per voxel + the per-workgroup counters
    assert lib.envgs_mesh_count(vol(), 0.0, 1.0, FAKE, need - 1, FAKE, None) == -2
    assert lib.envgs_mesh_count(vol(), 0.0, 1.0, None, need, FAKE, None) == -1
    assert lib.envgs_mesh_extract(vol(), 0.0, FAKE, need, 1, 0, None, None, None, None) == -1          # vertices asked for, no buffer
    assert ctypes.sizeof(_lib.TsdfView) == 96 and ctypes.sizeof(_lib.TsdfViews) == 8 + 8 * 96 and ctypes.sizeof(_lib.TsdfVolume) == 56


def test_volume_on_cpu_tensors_raises():
    import torch
    from envgs_amd import mesh
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.TSDFVolume((-1, -1, -1), (1, 1, 1), 0.1, device="cpu")
    t = torch.ones(4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.TSDFVolume.from_tensors(t, t.clone(), None, (0, 0, 0), 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.fuse_surfels(None, [], dict(means3D=torch.zeros(4, 3)), 0)
