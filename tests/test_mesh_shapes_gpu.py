"""GPU: csrc/mesh.hip at the shapes where it takes another path than on the volumes of tests/test_mesh_gpu.py -- ragged dimensions (quads of 4
voxels that wrap rows and slices, a tail lane, a partial workgroup), planes off 16 B (the scalar load / store paths), tiny and thin volumes,
cameras inside the volume, depth pixels that are NaN / inf / negative, views of different kinds in one launch, more workgroups than one scan
block holds, output rows capped below the counted totals.  The configurations are the table of tests/mesh_cases.py (checked on the oracle alone
in tests/test_mesh_cpu.py); the rules and tolerances are those of test_mesh_gpu.py, through its `check_fused` and `check_extraction`."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mesh_cases as mc
from tests import mesh_oracle as mo
from tests import test_mesh_gpu as base

pytestmark = pytest.mark.gpu
DEV = base.DEV
CANARY = -12345.5
ALL = ("tsdf", "weight", "rgb")


def _plane(shape, init, off):
    """A fresh contiguous plane; with `off`, a view one float into a canary-filled flat buffer, so 4 B past a 16 B boundary.
    -> (plane, the flat buffer or None)"""
    if not off:
        t = torch.full(shape, init, dtype=torch.float32, device=DEV)
        assert t.data_ptr() % 16 == 0
        return t, None
    count = int(np.prod(shape))
    buf = torch.full((count + 2,), CANARY, dtype=torch.float32, device=DEV)
    t = buf[1:1 + count].view(shape)
    t.fill_(init)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t, buf


def _volume(name, off=(), color=True):
    """The empty volume of a row of mc.INTEGRATION; the planes named in `off` are misaligned.  -> (volume, their flat buffers)"""
    from envgs_amd import mesh
    (nx, ny, nz), voxel, origin, _ = mc.INTEGRATION[name]
    tsdf, b0 = _plane((nz, ny, nx), 1.0, "tsdf" in off)
    weight, b1 = _plane((nz, ny, nx), 0.0, "weight" in off)
    rgb, b2 = _plane((3, nz, ny, nx), 0.0, "rgb" in off) if color else (None, None)
    vol = mesh.TSDFVolume.from_tensors(tsdf, weight, rgb, origin, voxel, trunc=mc.trunc_of(name))
    return vol, [b for b in (b0, b1, b2) if b is not None]


def _canaries_intact(bufs):
    return all(float(b[0]) == CANARY and float(b[-1]) == CANARY for b in bufs)


def _same(a, b):
    return torch.equal(a.tsdf, b.tsdf) and torch.equal(a.weight, b.weight) and (a.rgb is None or b.rgb is None or torch.equal(a.rgb, b.rgb))


# ---- 1. integration ----------------------------------------------------------------------------------------------------------------------------------
FRONT_END = [k for k, v in mc.INTEGRATION.items() if v[3] in ("orbit", "inside")]        # the view sets TSDFVolume.integrate can stack


@pytest.fixture(scope="module")
def fused():
    """name -> (views, the aligned colour volume fused from them in one launch): made once per row, read-only."""
    made = {}

    def get(name):
        if name not in made:
            views = mc.view_set(mc.INTEGRATION[name][3])
            vol, _ = _volume(name)
            base._integrate_all(vol, views)
            torch.cuda.synchronize()
            made[name] = (views, vol)
        return made[name]
    return get


@pytest.mark.parametrize("name", FRONT_END)
def test_integration_equals_the_oracle_at_every_shape(fused, name):
    views, vol = fused(name)
    assert vol.dims == mc.INTEGRATION[name][0]
    base.check_fused(vol, views, name)
    assert bool(torch.isfinite(vol.tsdf).all()) and bool(torch.isfinite(vol.weight).all()) and bool(torch.isfinite(vol.rgb).all())


@pytest.mark.parametrize("name", FRONT_END)
def test_one_launch_equals_single_launches_to_the_bit_at_every_shape(fused, name):
    views, vol = fused(name)
    single, _ = _volume(name)
    for v in views:
        base._integrate_all(single, [v])
    assert torch.equal(single.weight, vol.weight) and torch.equal(single.tsdf, vol.tsdf) and torch.equal(single.rgb, vol.rgb)


@pytest.mark.parametrize("off", [("tsdf",), ("weight",), ("rgb",), ALL], ids=lambda o: "+".join(o))
@pytest.mark.parametrize("name", ["37x35x33", "40x36x32"])
def test_misaligned_planes_take_the_scalar_paths_to_the_same_bits(fused, name, off):
    """The same arithmetic through another load / store path: tsdf or weight off 16 B turns the 16 B accesses of both off, rgb off 16 B those of
    the colour planes (which 37 x 35 x 33, n % 4 == 3, never has: its planes 1 and 2 start off a boundary anyway)."""
    views, aligned = fused(name)
    vol, bufs = _volume(name, off)
    assert len(bufs) == len(off)
    for p in off:
        assert getattr(vol, p).data_ptr() % 16 == 4
    for p in set(ALL) - set(off):
        assert getattr(vol, p).data_ptr() % 16 == 0
    base._integrate_all(vol, views)
    assert _same(vol, aligned) and vol.rgb is not None
    assert _canaries_intact(bufs)                               # the float before and the float behind every misaligned plane
    base.check_fused(vol, views, "%s, %s off 16 B" % (name, "+".join(off)))


@pytest.mark.parametrize("name", ["37x35x33", "40x36x32"])
def test_views_without_colour_leave_a_colour_volume_its_colours(name):
    """`each rgb channel likewise, when the volume and the view both carry colour`: here only the volume does."""
    orbit = mc.view_set("orbit")
    views = [mo.make_view(v.depth, base.KMAT, v.R, v.T, rgb=None, trunc=base.TRUNC) for v in orbit]
    args = (base._stack(views, "depth"), base._stack(views, "K"), base._stack(views, "R"), base._stack(views, "T"))
    plain, _ = _volume(name, color=False)
    plain.integrate(*args)
    coloured, _ = _volume(name)
    coloured.integrate(*args)
    assert torch.equal(coloured.tsdf, plain.tsdf) and torch.equal(coloured.weight, plain.weight)
    assert float(coloured.rgb.abs().max()) == 0.0
    base.check_fused(coloured, views, "%s, views without colour" % name)
    base.check_fused(plain, views, "%s, no colour anywhere" % name)
    # and colours that are not zero stay what they were, bit for bit
    painted, _ = _volume(name)
    before = torch.rand(painted.rgb.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    painted.rgb.copy_(before)
    painted.integrate(*args)
    assert torch.equal(painted.rgb, before) and torch.equal(painted.tsdf, plain.tsdf) and torch.equal(painted.weight, plain.weight)


def _launch(vol, views):
    """One envgs_tsdf_integrate over oracle views of any kind (the front end stacks its views, so they share H, W, trunc, depth_max and colour)."""
    from envgs_amd import _lib, mesh
    lib = _lib.load()
    vs, keep = _lib.TsdfViews(), []
    vs.count = len(views)
    for q, v in enumerate(views):
        depth = torch.from_numpy(v.depth).to(DEV).contiguous()
        rgb = None if v.rgb is None else torch.from_numpy(v.rgb).to(DEV).contiguous()
        keep += [depth, rgb]
        c = vs.v[q]
        c.depth, c.rgb = depth.data_ptr(), None if rgb is None else rgb.data_ptr()
        c.H, c.W = v.depth.shape
        c.fx, c.fy, c.cx, c.cy = float(v.fx), float(v.fy), float(v.cx), float(v.cy)
        c.R = (ctypes.c_float * 9)(*[float(x) for x in v.R.reshape(-1)])
        c.T = (ctypes.c_float * 3)(*[float(x) for x in v.T])
        c.depth_max, c.trunc = float(v.depth_max), float(v.trunc)
    _lib.check(lib.envgs_tsdf_integrate(vol._c_volume(), vs, vol.w_max, mesh._stream(vol.tsdf.device)), "envgs_tsdf_integrate")
    torch.cuda.synchronize()                                    # `keep` outlives the launch


def test_views_of_different_kinds_in_one_launch():
    views = mc.view_set("mixed")
    together, _ = _volume("mixed")
    _launch(together, views)
    single, _ = _volume("mixed")
    for v in views:
        _launch(single, [v])
    assert _same(together, single)
    base.check_fused(together, views, "mixed views, one launch")
    assert float(together.rgb.abs().max()) > 0.0


# ---- 2. extraction ---------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _extraction_volume(tsdf, weight, rgb, origin, voxel, off=()):
    from envgs_amd import mesh
    planes, bufs = {}, []
    for p, a in (("tsdf", tsdf), ("weight", weight), ("rgb", rgb)):
        t, b = _plane(a.shape, 0.0, p in off)
        t.copy_(_dev(a))
        planes[p] = t
        bufs += [] if b is None else [b]
    return mesh.TSDFVolume.from_tensors(planes["tsdf"], planes["weight"], planes["rgb"], origin, voxel), bufs


def _mesh_equal(a, b):
    return torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces) and torch.equal(a.colors, b.colors)


@pytest.mark.parametrize("name", mc.EXTRACTION)
def test_extraction_equals_the_oracle_at_every_shape(name):
    e = mc.extraction(name)
    nz, ny, nx = e.tsdf.shape
    weight = np.ones_like(e.tsdf) if e.weight is None else e.weight
    m, ref, gv, gf = base.check_extraction(name, e.tsdf, weight, base._colours((nx, ny, nz)), e.origin, e.voxel, e.level, e.euler, e.min_weight)
    assert np.isfinite(gv).all() and bool(torch.isfinite(m.colors).all())
    if name == "big":
        assert (nx * ny * nz + 255) // 256 > 1024               # the scan over the workgroups' counts runs in more than one block
    if name.startswith("thin"):
        assert min(nx, ny, nz) <= 3                             # every cell, or nearly every cell, lies on the border
    if "level" in name or "sample" in name:
        # a vertex whose owner's sample equals the level has t == 0 and sits on its voxel, bit for bit
        t0 = e.tsdf.reshape(-1)[ref.vertex_owner] == np.float32(e.level)
        k, r = np.divmod(ref.vertex_owner[t0], nx * ny)
        j, i = np.divmod(r, nx)
        at = np.stack([np.float32(e.origin[a]) + idx.astype(np.float32) * np.float32(e.voxel) for a, idx in enumerate((i, j, k))], axis=1)
        print("%s: %d vertices with t == 0" % (name, t0.sum()))
        assert np.array_equal(gv[t0], at)
        assert t0.sum() >= 3 or name != "plane on the level"
    if name == "min_weight 0.5":                                # a corner whose weight EQUALS min_weight counts as observed
        ck, r = np.divmod(ref.face_cell, nx * ny)
        cj, ci = np.divmod(r, nx)
        assert any((weight[ck + ((c >> 2) & 1), cj + ((c >> 1) & 1), ci + (c & 1)] == 0.5).any() for c in range(8))


@pytest.mark.parametrize("name", ["sphere", "open"])
def test_extraction_of_misaligned_planes_gives_the_same_bytes(name):
    tsdf, _, origin, voxel, level, _ = base._analytic(name)
    nz, ny, nx = tsdf.shape
    weight = mc.weights((nx, ny, nz), 7)                        # they differ inside every quad of 4 voxels: a load of the wrong element shows
    rgb = base._colours((nx, ny, nz))
    aligned = _extraction_volume(tsdf, weight, rgb, origin, voxel)[0].extract(level=level)
    ref = mo.marching_tetrahedra(tsdf, weight, rgb, origin, voxel, level=level)
    assert aligned.vertices.shape[0] == ref.vertices.shape[0] > 0 and aligned.faces.shape[0] == ref.faces.shape[0]
    for off in (("tsdf",), ("weight",), ("rgb",), ALL):
        vol, bufs = _extraction_volume(tsdf, weight, rgb, origin, voxel, off)
        for p in off:
            assert getattr(vol, p).data_ptr() % 16 == 4
        assert _mesh_equal(vol.extract(level=level), aligned), off
        assert _canaries_intact(bufs)


def test_garbage_in_unobserved_voxels_changes_nothing():
    tsdf, weight, origin, voxel, level, _ = base._analytic("hole")
    nz, ny, nx = tsdf.shape
    rgb = base._colours((nx, ny, nz))
    clean = _extraction_volume(tsdf, weight, rgb, origin, voxel)[0].extract(level=level)
    junk = np.array([np.nan, np.inf, -np.inf, -5.0], np.float32)
    hole = weight == 0
    assert hole.sum() == 36
    dirty_t, dirty_c = tsdf.copy(), rgb.copy()
    dirty_t[hole] = junk[np.arange(hole.sum()) % 4]
    for c in range(3):
        dirty_c[c][hole] = junk[(np.arange(hole.sum()) + c + 1) % 4]
    dirty = _extraction_volume(dirty_t, weight, dirty_c, origin, voxel)[0].extract(level=level)
    assert _mesh_equal(dirty, clean) and bool(torch.isfinite(dirty.vertices).all()) and bool(torch.isfinite(dirty.colors).all())
    base.check_extraction("hole with garbage", dirty_t, weight, dirty_c, origin, voxel, level, None)


def test_nothing_at_or_beyond_row_V_and_F_is_written():
    """envgs_mesh_extract with fewer rows than envgs_mesh_count counted: the rows asked for are those of the full run, the rest is untouched."""
    from envgs_amd import _lib, mesh
    lib, p = _lib.load(), _lib.ptr
    tsdf, _, origin, voxel, level, _ = base._analytic("sphere")
    nz, ny, nx = tsdf.shape
    vol, _ = _extraction_volume(tsdf, np.ones_like(tsdf), base._colours((nx, ny, nz)), origin, voxel)
    cv, stream = vol._c_volume(), mesh._stream(vol.tsdf.device)
    tb = lib.envgs_mesh_temp_bytes(nx, ny, nz)
    temp = torch.empty(tb, dtype=torch.uint8, device=DEV)
    totals = torch.empty(2, dtype=torch.int32, device=DEV)
    _lib.check(lib.envgs_mesh_count(cv, level, 1.0, p(temp), tb, p(totals), stream), "envgs_mesh_count")
    V, F = totals.tolist()
    assert (V, F) == (566, 1128)

    def run(Vc, Fc, vertices=True, faces=True):
        v = torch.full((V, 3), CANARY, dtype=torch.float32, device=DEV)
        c = torch.full((V, 3), CANARY, dtype=torch.float32, device=DEV)
        f = torch.full((F, 3), -7, dtype=torch.int32, device=DEV)
        rc = lib.envgs_mesh_extract(cv, level, p(temp), tb, Vc, Fc, p(v) if vertices else None, p(c), p(f) if faces else None, stream)
        torch.cuda.synchronize()
        return rc, v, c, f

    rc, fv, fc, ff = run(V, F)
    whole = vol.extract(level=level)
    assert rc == 0 and torch.equal(fv, whole.vertices) and torch.equal(fc, whole.colors) and torch.equal(ff, whole.faces)
    assert not bool((fv == CANARY).any()) and not bool((fc == CANARY).any()) and int(ff.min()) >= 0
    for Vc, Fc, with_v, with_f in ((V // 2, F // 3, True, True), (0, F, False, True), (V, 0, True, False), (1, 1, True, True), (V - 1, F - 1, True, True)):
        rc, v, c, f = run(Vc, Fc, with_v, with_f)
        assert rc == 0, (Vc, Fc)
        assert torch.equal(v[:Vc], fv[:Vc]) and torch.equal(c[:Vc], fc[:Vc]) and torch.equal(f[:Fc], ff[:Fc]), (Vc, Fc)
        assert bool((v[Vc:] == CANARY).all()) and bool((c[Vc:] == CANARY).all()) and bool((f[Fc:] == -7).all()), (Vc, Fc)
    # a null buffer only where its count is 0: rejected before any GPU work
    assert run(1, 0, vertices=False)[0] == -1 and run(0, 1, faces=False)[0] == -1


def test_extraction_on_a_side_stream_gives_the_same_bytes():
    tsdf, _, origin, voxel, level, _ = base._analytic("large")
    nz, ny, nx = tsdf.shape
    vol, _ = _extraction_volume(tsdf, np.ones_like(tsdf), base._colours((nx, ny, nz)), origin, voxel)
    here = vol.extract(level=level)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # count, the read-back of (V, F) and extract all run on `side`
        there = vol.extract(level=level)
    side.synchronize()
    assert here.vertices.shape[0] > 0 and _mesh_equal(here, there)


# ---- 3. end to end at ragged bounds ------------------------------------------------------------------------------------------------------------------
def test_fuse_surfels_end_to_end_at_ragged_bounds():
    """test_fuse_surfels_end_to_end with a voxel size that gives odd dimensions on all three axes (the fragile share of these bounds: the row
    "ragged e2e" of the case table, test_mesh_cpu.py), the same two oracle links."""
    from envgs_amd import mesh
    dims, voxel, lo, _ = mc.INTEGRATION["ragged e2e"]
    surfels = base._sphere_surfels()
    cams = mc.e2e_cameras(device=DEV)
    vol = mesh.TSDFVolume(lo, mc.E2E_HI, voxel, device=DEV)
    assert vol.dims == dims and all(d % 2 == 1 for d in vol.dims) and abs(vol.trunc - 5 * voxel) < 1e-12
    maps = mesh.fuse_surfels(vol, cams, surfels, sh_degree=0, alpha_min=0.5)
    # link 1: the fused volume is the oracle's integration of the maps the GPU rendered
    views = []
    for cam, mp in zip(cams, maps):
        alpha = mp.alpha.cpu().numpy()
        assert (alpha > 0.5).mean() > 0.05
        depth = np.where(alpha > 0.5, mp.depth.cpu().numpy(), 0).astype(np.float32)
        views.append(mo.make_view(depth, cam.K.cpu().numpy(), cam.R.cpu().numpy(), cam.T.cpu().numpy(), rgb=mp.rgb.cpu().numpy(), trunc=vol.trunc))
    base.check_fused(vol, views, "fuse_surfels, ragged")
    # link 2: the mesh is the oracle's extraction of the GPU's volume
    m = vol.extract()
    ref = mo.marching_tetrahedra(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.rgb.cpu().numpy(), vol.origin, vol.voxel_size)
    V = m.vertices.shape[0]
    print("end to end, ragged: V %d F %d" % (V, m.faces.shape[0]))
    assert V > 0 and V == ref.vertices.shape[0] and m.faces.shape[0] == ref.faces.shape[0]
    gv = m.vertices.cpu().numpy()
    assert np.abs(gv - ref.vertices).max() <= 1e-5 * vol.voxel_size and np.abs(m.colors.cpu().numpy() - ref.colors).max() <= 1e-6
    assert np.array_equal(mo.canonical_faces(m.faces.cpu().numpy()), mo.canonical_faces(ref.faces))
    assert (gv >= np.array(lo)).all() and (gv <= np.array(vol.origin) + (np.array(vol.dims) - 1) * vol.voxel_size + 1e-6).all()
    rad = np.linalg.norm(gv, axis=1)
    assert np.median(np.abs(rad - 0.6)) < 0.5 * vol.voxel_size
