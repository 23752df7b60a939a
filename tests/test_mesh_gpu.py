"""GPU: the TSDF integration and marching-tetrahedra kernels (csrc/mesh.hip) against the independent NumPy oracle (tests/mesh_oracle.py).

PARITY UNPINNED (DESIGN.md "Mesh extraction"): there is no reference output to record, the oracle restates the semantics of include/envgs_mesh.h.
The integration is compared decision for decision: weights exactly, tsdf / rgb within 1e-6, on every voxel the float64 shadow does not call fragile;
a fragile voxel may differ only by the outcome of its fragile decisions, which are re-taken the other way and compared."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import mesh_oracle as mo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ---- 1. integration --------------------------------------------------------------------------------------------------------------------------------
DIMS = (40, 36, 32)
VOXEL, ORIGIN, TRUNC = 0.05, (-1.0131, -0.8873, -0.7919), 0.2
H, W = 48, 64
KMAT = [[70.0, 0.0, W / 2 + 0.37], [0.0, 72.1, H / 2 - 0.21], [0.0, 0.0, 1.0]]
SPHERE_C, SPHERE_R = (0.03, -0.02, 0.01), 0.6


def _sphere_depth(R, T):
    """Analytic z-depth of the sphere through the pixel centres (i + 0.5), 0 where the ray misses."""
    cc = np.asarray(R, np.float64) @ np.array(SPHERE_C) + np.asarray(T, np.float64).reshape(3)
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack([(px - KMAT[0][2]) / KMAT[0][0], (py - KMAT[1][2]) / KMAT[1][1], np.ones_like(px)], axis=-1)
    dd, dc = (d * d).sum(-1), d @ cc
    disc = dc * dc - dd * (cc @ cc - SPHERE_R ** 2)
    t = (dc - np.sqrt(np.maximum(disc, 0))) / dd
    return np.where(disc > 0, t, 0.0).astype(np.float32)


def _views(n):
    from envgs_amd import synth
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = []
    for v in range(n):
        cam = synth.orbit_camera(v, n_views=n, radius=3.0, H=H, W=W, fx=70.0)
        R, T = cam.R.numpy(), cam.T.numpy().reshape(3)
        rgb = np.stack([0.5 + 0.5 * np.sin(0.11 * px + 0.3 * v), 0.5 + 0.5 * np.cos(0.07 * py - 0.2 * v), (px + 2 * py) / (W + 2 * H)]).astype(np.float32)
        out.append(mo.make_view(_sphere_depth(R, T), KMAT, R, T, rgb=rgb, trunc=TRUNC))
    return out


def _stack(views, what):
    if what == "K":
        return torch.tensor(KMAT, dtype=torch.float32)
    return torch.from_numpy(np.stack([getattr(v, what) for v in views])).to(DEV if what in ("depth", "rgb") else "cpu")


def _fresh(color=True, dims=DIMS):
    from envgs_amd import mesh
    nx, ny, nz = dims
    t = torch.ones(nz, ny, nx, device=DEV)
    return mesh.TSDFVolume.from_tensors(t, torch.zeros_like(t), torch.zeros(3, nz, ny, nx, device=DEV) if color else None, ORIGIN, VOXEL, trunc=TRUNC)


def _integrate_all(vol, views, **kw):
    return vol.integrate(_stack(views, "depth"), _stack(views, "K"), _stack(views, "R"), _stack(views, "T"), rgb=_stack(views, "rgb"), **kw)


def check_fused(vol, views, label):
    """The rule of this file's docstring, for a volume fused from its initial state by `views` in order."""
    nx, ny, nz = vol.dims
    one = np.ones((nz, ny, nx), np.float32)
    c0 = None if vol.rgb is None else np.zeros((3, nz, ny, nx), np.float32)
    D32, W32, C32, _ = mo.integrate(one, 0 * one, c0, vol.origin, vol.voxel_size, views, vol.w_max, np.float32, trunc=vol.trunc)
    D64, W64, C64, frag = mo.integrate(one, 0 * one, c0, vol.origin, vol.voxel_size, views, vol.w_max, np.float64, trunc=vol.trunc)
    gD, gW = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    gC = None if vol.rgb is None else vol.rgb.cpu().numpy()
    keep = ~frag
    n_disagree = int((W32[keep] != W64[keep]).sum())
    eD = float(np.abs(gD - D32)[keep].max())
    eC = 0.0 if gC is None else float(np.abs(gC - C32)[:, keep].max())
    print("%s: fragile %d of %d voxels, oracle f32/f64 weight disagreements off them %d, observed voxels %d, max |tsdf - oracle| %.3g, max |rgb - oracle| %.3g, "
          "weights differing %d" % (label, frag.sum(), frag.size, n_disagree, (W32 > 0).sum(), eD, eC, (gW[keep] != W32[keep]).sum()))
    assert frag.mean() <= 0.01                                  # the condition under which the comparison means something
    assert (W32 > 0).sum() > 0.02 * frag.size and (W32 == 0).any()
    assert np.array_equal(gW[keep], W32[keep])
    assert eD <= 1e-6 and eC <= 1e-6
    n_alt = 0
    for k, j, i in zip(*np.nonzero(frag)):
        got = (gD[k, j, i], gW[k, j, i], None if gC is None else gC[:, k, j, i])
        close = lambda d, w, c: w == got[1] and abs(d - got[0]) <= 1e-6 and (c is None or got[2] is None or np.abs(np.array(c) - got[2]).max() <= 1e-6)
        if close(D32[k, j, i], W32[k, j, i], None if C32 is None else C32[:, k, j, i]):
            continue
        n_alt += 1                                              # differs: only by taking its fragile decisions the other way
        opts = mo.fragile_alternatives((i, j, k), vol.origin, vol.voxel_size, views, vol.trunc)
        start = (1.0, 0.0, None if gC is None else (0.0, 0.0, 0.0))
        assert any(close(*mo.integrate_voxel((i, j, k), start, vol.origin, vol.voxel_size, views, vol.w_max, vol.trunc, flips))
                   for flips in itertools.islice(itertools.product(*opts), 4096)), ("fragile voxel", (i, j, k), got)
    print("%s: fragile voxels that took another branch than the float32 oracle: %d" % (label, n_alt))
    return D32, W32, C32


@pytest.fixture(scope="module")
def six():
    views = _views(6)
    vol = _integrate_all(_fresh(), views)
    torch.cuda.synchronize()
    return views, vol


def test_integration_equals_the_oracle(six):
    views, vol = six
    check_fused(vol, views, "6 views")
    assert float(vol.weight.max()) >= 3.0 and float(vol.tsdf.min()) < -0.5       # several views overlap; the inside of the sphere is seen


def test_one_launch_equals_single_launches_to_the_bit(six):
    views, vol = six
    single = _fresh()
    for v in views:
        _integrate_all(single, [v])
    assert torch.equal(single.weight, vol.weight) and torch.equal(single.tsdf, vol.tsdf) and torch.equal(single.rgb, vol.rgb)


def test_eleven_views_go_in_chunks_of_eight_and_three():
    views = _views(11)
    vol = _integrate_all(_fresh(), views)
    check_fused(vol, views, "11 views")


def test_volume_without_colour_and_two_dimensional_depth(six):
    views, vol = six
    plain = _fresh(color=False)
    for v in views:                                             # (H,W) depth, (3,3) R, (3,) T: the unbatched form
        plain.integrate(torch.from_numpy(v.depth).to(DEV), torch.tensor(KMAT), torch.from_numpy(v.R), torch.from_numpy(v.T))
    assert plain.rgb is None and torch.equal(plain.tsdf, vol.tsdf) and torch.equal(plain.weight, vol.weight)
    plain.reset()
    assert float(plain.weight.abs().max()) == 0.0 and float((plain.tsdf - 1).abs().max()) == 0.0


def test_mask_equals_zeroed_depth():
    views = _views(6)
    rng = np.random.default_rng(5)
    masks = rng.random((6, H, W)) > 0.3
    zeroed = [mo.make_view(np.where(m, v.depth, 0), KMAT, v.R, v.T, rgb=v.rgb, trunc=TRUNC) for v, m in zip(views, masks)]
    a = _integrate_all(_fresh(), views, mask=torch.from_numpy(masks).to(DEV))
    b = _integrate_all(_fresh(), zeroed)
    assert torch.equal(a.tsdf, b.tsdf) and torch.equal(a.weight, b.weight) and torch.equal(a.rgb, b.rgb)
    check_fused(a, zeroed, "masked")


def test_depth_max_cuts(six):
    views, full = six
    cut = 2.55                                                  # the sphere's depths run from 2.4 to about 3
    assert any(((v.depth > 0) & (v.depth <= cut)).any() and (v.depth > cut).any() for v in views)
    vol = _integrate_all(_fresh(), views, depth_max=cut)
    limited = [mo.make_view(v.depth, KMAT, v.R, v.T, rgb=v.rgb, depth_max=cut, trunc=TRUNC) for v in views]
    check_fused(vol, limited, "depth_max")
    assert not torch.equal(vol.weight, full.weight)
    # and it is the same as removing those measurements
    removed = [mo.make_view(np.where(v.depth <= cut, v.depth, 0), KMAT, v.R, v.T, rgb=v.rgb, trunc=TRUNC) for v in views]
    other = _integrate_all(_fresh(), removed)
    assert torch.equal(other.tsdf, vol.tsdf) and torch.equal(other.weight, vol.weight)


def test_weight_saturates_at_w_max():
    from envgs_amd import mesh
    views = _views(6)
    vol = _fresh()
    vol.w_max = 2.0
    _integrate_all(vol, views)
    check_fused(vol, views, "w_max 2")
    assert float(vol.weight.max()) == 2.0


# ---- 2 / 3. extraction on analytic volumes, with colours ---------------------------------------------------------------------------------------------
def _analytic(name):
    """-> (tsdf (Nz,Ny,Nx), weight, origin, voxel, level, closed genus or None)"""
    c = (6.37, 5.61, 4.83)
    if name == "sphere":
        return mo.sphere_volume((14, 12, 10), c, 3.217), None, (0.0, 0.0, 0.0), 1.0, 0.0, 2
    if name == "torus":
        return mo.torus_volume((14, 12, 10), c, 3.1, 1.27), None, (0.0, 0.0, 0.0), 1.0, 0.0, 0
    if name == "open":                                          # the level set leaves through the border
        return mo.sphere_volume((33, 17, 9), (16.3, 8.2, 4.4), 6.3), None, (0.0, 0.0, 0.0), 1.0, 0.0, None
    if name == "hole":                                          # a block never observed
        w = np.ones((10, 12, 14), np.float32)
        w[3:6, 4:7, 5:9] = 0
        return mo.sphere_volume((14, 12, 10), c, 3.217), w, (0.0, 0.0, 0.0), 1.0, 0.0, None
    if name == "level":
        return mo.torus_volume((14, 12, 10), c, 3.1, 1.27), None, (0.0, 0.0, 0.0), 1.0, 0.35, 0
    if name == "large":                                         # several workgroups along every axis, world coordinates off the origin
        return 0.05 * mo.sphere_volume((48, 40, 36), (23.4, 19.7, 17.2), 13.3), None, (-1.17, 0.43, 2.01), 0.05, 0.0, 2
    raise KeyError(name)


def check_extraction(name, tsdf, weight, rgb, origin, voxel, level, euler, min_weight=1.0, vol=None):
    """A volume (NumPy planes; `vol` when they are on the device already) extracted twice on the device, against the oracle's extraction:
    counts, vertices within 1e-5 voxel, colours within 1e-6, faces equal canonically and in the oracle's cell order, two runs byte for byte,
    the topology the case names, nothing in a cell with an unobserved corner.  -> (mesh, oracle mesh, vertices, faces as NumPy)"""
    from envgs_amd import mesh
    nz, ny, nx = tsdf.shape
    ref = mo.marching_tetrahedra(tsdf, weight, rgb, origin, voxel, level=level, min_weight=min_weight)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if vol is None:
        vol = mesh.TSDFVolume.from_tensors(t(tsdf), t(weight), t(rgb), origin, voxel)
    m = vol.extract(level=level, min_weight=min_weight)
    again = vol.extract(level=level, min_weight=min_weight)
    V, F = m.vertices.shape[0], m.faces.shape[0]
    print("%s: V %d F %d (oracle %d %d)" % (name, V, F, ref.vertices.shape[0], ref.faces.shape[0]))
    assert V == ref.vertices.shape[0] and F == ref.faces.shape[0] and V > 0 and F > 0
    assert m.faces.dtype == torch.int32 and m.vertices.dtype == torch.float32
    gv, gf, gc = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.colors.cpu().numpy()
    ev, ec = float(np.abs(gv - ref.vertices).max()) / voxel, float(np.abs(gc - ref.colors).max())
    print("%s: max vertex error %.3g voxel, max colour error %.3g" % (name, ev, ec))
    assert ev <= 1e-5
    assert ec <= 1e-6
    assert np.array_equal(mo.canonical_faces(gf), mo.canonical_faces(ref.faces))
    cells = mo.face_cells(gf, ref.vertex_owner, ref.vertex_slot, (nx, ny, nz))
    assert (np.diff(cells) >= 0).all() and np.array_equal(cells, ref.face_cell)
    # two runs, byte for byte
    assert torch.equal(m.vertices, again.vertices) and torch.equal(m.faces, again.faces) and torch.equal(m.colors, again.colors)
    top = mo.mesh_topology(gf, V)
    assert top.all_referenced
    if euler is not None:
        assert top.closed_oriented and top.euler == euler
    else:
        assert not top.closed_oriented
    # nothing in a cell with a corner that was never observed
    ck, r = np.divmod(cells, nx * ny)
    cj, ci = np.divmod(r, nx)
    for c in range(8):
        assert (weight[ck + ((c >> 2) & 1), cj + ((c >> 1) & 1), ci + (c & 1)] >= min_weight).all()
    return m, ref, gv, gf


def _colours(dims):
    nx, ny, nz = dims
    X, Y, Z = mo.grid_points((nx, ny, nz))
    return np.stack([0.5 + 0.5 * np.sin(0.4 * X + 0.2 * Y), 0.5 + 0.5 * np.cos(0.3 * Y - 0.5 * Z), (X + Y + Z) / (nx + ny + nz)]).astype(np.float32)


@pytest.mark.parametrize("name", ["sphere", "torus", "open", "hole", "level", "large"])
def test_extraction_equals_the_oracle(name):
    tsdf, weight, origin, voxel, level, euler = _analytic(name)
    weight = np.ones_like(tsdf) if weight is None else weight
    nz, ny, nx = tsdf.shape
    m, ref, gv, gf = check_extraction(name, tsdf, weight, _colours((nx, ny, nz)), origin, voxel, level, euler)
    if name == "sphere":
        p = gv.astype(np.float64)[gf]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert (np.einsum("ij,ij->i", n, p.mean(axis=1) - np.array((6.37, 5.61, 4.83))) > 0).all()
    if name == "hole":
        full = mo.marching_tetrahedra(tsdf, np.ones_like(tsdf), None, origin, voxel)
        assert m.faces.shape[0] < full.faces.shape[0]


def test_extraction_without_colour_and_of_an_empty_volume():
    from envgs_amd import mesh
    tsdf = torch.from_numpy(mo.sphere_volume((14, 12, 10), (6.37, 5.61, 4.83), 3.217)).to(DEV)
    m = mesh.TSDFVolume.from_tensors(tsdf, torch.ones_like(tsdf), None, (0, 0, 0), 1.0).extract()
    assert m.colors is None and m.vertices.shape == (566, 3) and m.faces.shape == (1128, 3)
    m = mesh.TSDFVolume.from_tensors(tsdf, torch.zeros_like(tsdf), None, (0, 0, 0), 1.0).extract()          # nothing observed
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)
    m = mesh.TSDFVolume((-1, -1, -1), (1, 1, 1), 0.25, device=DEV).extract(min_weight=0.0)                   # observed, but no crossing
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------------
def _sphere_surfels(P=4096, radius=0.6):
    """Opaque surfels tangent to a sphere: Fibonacci points, the surfel normal (the rotation's z axis) along the radius."""
    i = np.arange(P) + 0.5
    z = 1 - 2 * i / P
    phi = i * math.pi * (3 - math.sqrt(5))
    n = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    q = np.stack([1 + n[:, 2], -n[:, 1], n[:, 0], np.zeros(P)], axis=1)              # (r, x, y, z): the rotation taking +z to n
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV).contiguous()
    return dict(means3D=f(radius * n), scales=f(np.full((P, 2), 0.03)), rotations=f(q), opacities=f(np.full((P, 1), 0.99)),
                shs=f((0.5 * n + 0.2)[:, None, :]))


def _render(cam, base):
    import diff_surfel_rasterization_wet as pkg
    st = pkg.GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=DEV),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=0, campos=cam.camera_center,
        prefiltered=False, debug=False)
    with torch.no_grad():
        return pkg.GaussianRasterizer(raster_settings=st)(
            means3D=base["means3D"], means2D=torch.zeros_like(base["means3D"]), shs=base["shs"], colors_precomp=None, opacities=base["opacities"],
            scales=base["scales"], rotations=base["rotations"], cov3D_precomp=None)


def test_fuse_surfels_end_to_end():
    from envgs_amd import mesh, synth
    base = _sphere_surfels()
    cams = [synth.orbit_camera(v, n_views=8, radius=3.0, H=96, W=96, fx=120.0, n=0.5, f=6.0, device=DEV) for v in range(8)]
    before = _render(cams[3], base)
    # an origin off the cameras' symmetry planes: with (-0.8, -0.8, -0.8) the voxels i == j lie in the plane through the optical axes of the views at
    # 45 and 225 degrees, project onto the pixel boundary u = 48 and make 2.3 % of the grid fragile (the oracle alone, on the CPU); so 0.22 %
    lo = (-0.8131, -0.7873, -0.8019)
    vol = mesh.TSDFVolume(lo, (0.8, 0.8, 0.8), 0.0345, device=DEV)
    assert vol.dims == (48, 48, 48) and abs(vol.trunc - 5 * 0.0345) < 1e-12
    maps = mesh.fuse_surfels(vol, cams, base, sh_degree=0, alpha_min=0.5)
    after = _render(cams[3], base)
    # the rasterizer is untouched by the volume: image, radii and allmap bit for bit.  Its fourth output, the per-surfel `weight`, is summed with float
    # atomics (raster_render.hip: the wavefronts' partial sums in LDS, the tiles' in HBM), so two forwards of the SAME call differ in its last bits
    # whatever lies between them: a surfel of 3 sigma = 3.6 px covers at most 2 x 2 tiles x 4 wavefronts = 16 non-negative terms, and two summation orders
    # of n terms differ by at most 2 (n - 1) 2^-24 of the sum
    for a, b in zip(before[:3], after[:3]):
        assert torch.equal(a, b)
    dw = float(((before[3] - after[3]).abs() / before[3].abs().clamp_min(1e-30)).max())
    print("end to end: rasterizer weight output, max relative difference between two forwards %.3g" % dw)
    assert dw <= 30 * 2.0 ** -24
    assert torch.equal(maps[3].rgb, before[0][:3]) and torch.equal(maps[3].alpha, before[2][1])
    # link 1: the fused volume is the oracle's integration of the maps the GPU rendered
    views = []
    for cam, mp in zip(cams, maps):
        alpha = mp.alpha.cpu().numpy()
        assert (alpha > 0.5).mean() > 0.05
        depth = np.where(alpha > 0.5, mp.depth.cpu().numpy(), 0).astype(np.float32)
        views.append(mo.make_view(depth, cam.K.cpu().numpy(), cam.R.cpu().numpy(), cam.T.cpu().numpy(), rgb=mp.rgb.cpu().numpy(), trunc=vol.trunc))
    check_fused(vol, views, "fuse_surfels")
    # link 2: the mesh is the oracle's extraction of the GPU's volume
    m = vol.extract()
    ref = mo.marching_tetrahedra(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.rgb.cpu().numpy(), vol.origin, vol.voxel_size)
    V = m.vertices.shape[0]
    print("end to end: V %d F %d" % (V, m.faces.shape[0]))
    assert V > 0 and V == ref.vertices.shape[0] and m.faces.shape[0] == ref.faces.shape[0]
    gv = m.vertices.cpu().numpy()
    assert np.abs(gv - ref.vertices).max() <= 1e-5 * vol.voxel_size and np.abs(m.colors.cpu().numpy() - ref.colors).max() <= 1e-6
    assert np.array_equal(mo.canonical_faces(m.faces.cpu().numpy()), mo.canonical_faces(ref.faces))
    assert (gv >= np.array(lo)).all() and (gv <= np.array(vol.origin) + (np.array(vol.dims) - 1) * vol.voxel_size + 1e-6).all()
    # and it is the sphere that was rendered: every vertex of the outer sheet lies near radius 0.6
    rad = np.linalg.norm(gv, axis=1)
    assert np.median(np.abs(rad - 0.6)) < 0.5 * vol.voxel_size
