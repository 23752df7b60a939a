"""GPU: the mesh rasteriser (csrc/mesh_raster.hip) through envgs_amd.mesh.render_mesh / visible_faces / cull_unseen and visualize.mesh_views, against
the independent oracle (tests/mesh_raster_oracle.py).  Every comparison is exact, as words -- NaN payloads and the sign of zero count -- and every
product call runs twice and must give identical bytes.  PARITY UNPINNED (DESIGN.md "Mesh rasterisation"): the semantics are this project's, stated
in include/envgs_mesh.h."""
import numpy as np
import pytest
import torch

from tests import mesh_raster_cases as rc
from tests import mesh_raster_oracle as ro
from tests import visualize_oracle as vo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("depth", "face", "bary", "normal", "color", "seen")


def _bits(a):
    """float arrays compared as words: NaN payloads and the sign of zero count."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _mesh(c, colors=True):
    from envgs_amd import mesh
    return mesh.Mesh(vertices=torch.from_numpy(c.vertices).to(DEV), faces=torch.from_numpy(c.faces).to(DEV),
                     colors=torch.from_numpy(c.colors).to(DEV) if colors and c.colors is not None else None)


_ORACLE = {}


def _oracle(c):
    """Computed once per case and shared; nobody changes it."""
    if c.name not in _ORACLE:
        _ORACLE[c.name] = ro.render(c.vertices, c.faces, c.cameras, c.H, c.W, c.near, c.colors)
    return _ORACLE[c.name]


def _render_twice(c, outputs=ALL, **kw):
    from envgs_amd import mesh
    m = _mesh(c)
    a = mesh.render_mesh(m, c.cameras, near=c.near, outputs=outputs, **kw)
    b = mesh.render_mesh(m, c.cameras, near=c.near, outputs=outputs, **kw)
    assert sorted(vars(a)) == sorted(vars(b))
    for name in vars(a):
        assert _same(getattr(a, name), getattr(b, name).cpu().numpy()), "two runs differ in " + name
    return a


def _check(c, outputs=ALL):
    got, want = _render_twice(c, outputs), _oracle(c)
    names = [o for o in outputs if o != "color" or c.colors is not None]
    assert sorted(vars(got)) == sorted(names)
    for name in names:
        g = getattr(got, name).cpu().numpy()
        assert _same(g, want[name]), "%s: %s differs in %d of %d words" % (c.name, name, (_bits(g) != _bits(want[name])).sum(), g.size)
    return got, want


@pytest.fixture(scope="module")
def small_max():
    from envgs_amd import _lib
    n = int(_lib.load().envgs_mesh_raster_small_max())
    assert 1 <= n <= 1024
    return n


@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: "%dx%d" % s)
def test_whole_image_triangle(size, extra):
    c = rc.whole_image(*size, extra=extra)
    _, want = _check(c)
    assert (want["face"] >= 0).all()
    if extra and size[0] >= 33:
        assert want["seen"][0] and want["seen"][1:13].any() and not want["seen"][13:].any()      # the small faces in front win, those behind never


def test_boxes_around_small_max(small_max):
    c = rc.boxed_faces(small_max)
    assert {rc.box_pixels(c, f) for f in range(len(c.faces))} == {small_max - 1, small_max, small_max + 1}
    _, want = _check(c)
    assert want["seen"].all()


def test_subpixel_faces():
    c = rc.subpixel_faces()
    _, want = _check(c)
    per_face = np.bincount(want["face"][want["face"] >= 0], minlength=len(c.faces))
    assert (per_face[:6] == 0).all() and (per_face[6:] == 1).all()
    assert np.array_equal(want["seen"], [0] * 6 + [1] * 6)


@pytest.mark.parametrize("reverse", [False, True])
def test_fans(reverse):
    for H, W, seed in ((33, 17, 21), (64, 48, 22), (5, 3, 23), (1, 1, 24)):
        c = rc.fan(H, W, seed, reverse=reverse, flat=seed % 2 == 0)
        _, want = _check(c)
        assert (want["face"] >= 0).all()


def test_quad():
    got, _ = _check(rc.quad())
    covered = (got.face[0] >= 0).cpu().numpy()
    assert covered.sum() == 48 and covered[3:9, 4:12].all()


def test_duplicate_faces():
    got, _ = _check(rc.duplicates())
    assert set(np.unique(got.face.cpu().numpy())) == {-1, 0}
    assert got.seen.cpu().tolist() == [1, 0, 0, 0, 0]


def test_interpenetrating_triangles():
    c = rc.interpenetrating()
    got, want = _check(c)
    cam = c.cameras[0]
    proj = ro.project(cam, c.vertices, c.near)
    k0, k1 = (ro.face_keys(f, c.vertices, c.faces, cam, c.H, c.W, c.near, proj) for f in (0, 1))
    both = (k0 != ro.EMPTY) & (k1 != ro.EMPTY)
    face = got.face[0].cpu().numpy()
    assert both.sum() > 100 and 0 < (face[both] == 0).sum() < both.sum()                        # each is in front somewhere
    assert np.array_equal(face[both], np.where(k0[both] < k1[both], 0, 1))                       # the per-pixel depth order


def test_extreme_coordinates():
    """Corners at the 2^21-pixel limit: the largest int64 edge functions, and the clamp of a box of 2^22 pixels a side."""
    c = rc.extreme_faces()
    _, want = _check(c)
    assert (want["face"] == 0).all() and want["seen"].tolist() == [1, 0, 0, 0]


def test_dropped_faces():
    c = rc.dropped()
    got, want = _check(c)
    seen = got.seen.cpu().numpy().astype(bool)
    assert not seen[c.bad].any() and seen[~c.bad][:-1].all()
    keep = np.flatnonzero(~c.bad)
    alone = ro.render(c.vertices, c.faces[keep], c.cameras, c.H, c.W, c.near)                    # the neighbours are unaffected
    assert np.array_equal(np.where(alone["face"] >= 0, keep[alone["face"]], -1), got.face.cpu().numpy())


@pytest.mark.parametrize("size", [(33, 17), (64, 48)], ids=lambda s: "%dx%d" % s)
def test_random_soup(size):
    c = rc.soup(*size)
    assert len(c.cameras) == 9 and len(c.faces) == 3000
    got, want = _check(c)
    assert 0 < want["seen"].sum() < len(c.faces)
    union = np.zeros(len(c.faces), np.uint8)
    union[np.unique(want["face"][want["face"] >= 0])] = 1                                        # over all 9 views: both launches
    assert _same(got.seen, union)


def test_requested_outputs():
    from envgs_amd import mesh
    c = rc.soup(33, 17)
    want = _oracle(c)
    m = _mesh(c)
    for outputs in (("face",), ("depth",), ("seen",), ("bary", "normal"), ("color",)):
        got = _render_twice(c, outputs)
        assert sorted(vars(got)) == sorted(outputs)
        for name in outputs:
            assert _same(getattr(got, name), want[name]), name
    for _ in range(2):
        vis = mesh.visible_faces(m, c.cameras, near=c.near)
        assert vis.dtype == torch.bool and _same(vis.view(torch.uint8), want["seen"])
    plain = mesh.render_mesh(_mesh(c, colors=False), c.cameras, near=c.near)                     # "color" is ignored for a mesh without colours
    assert sorted(vars(plain)) == ["depth", "face", "normal"] and _same(plain.depth, want["depth"])
    sized = mesh.render_mesh(m, c.cameras, size=(c.H, c.W), near=c.near, outputs=("face",))
    assert _same(sized.face, want["face"])


def test_empty_inputs():
    from envgs_amd import mesh
    c = rc.quad()
    m = _mesh(c)
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=DEV)
    no_faces = mesh.Mesh(vertices=m.vertices, faces=z(0, 3, dtype=torch.int32), colors=m.colors)
    nothing = mesh.Mesh(vertices=z(0, 3), faces=z(0, 3, dtype=torch.int32), colors=z(0, 3))
    no_vertices = mesh.Mesh(vertices=z(0, 3), faces=m.faces, colors=None)                        # every index is outside [0, 0)
    for mm, F in ((no_faces, 0), (nothing, 0), (no_vertices, 2)):
        for _ in range(2):
            r = mesh.render_mesh(mm, c.cameras, outputs=ALL)
            assert _same(r.depth, np.zeros((1, 24, 32), np.float32)) and _same(r.face, np.full((1, 24, 32), -1, np.int32))
            assert _same(r.bary, np.zeros((1, 24, 32, 3), np.float32)) and _same(r.normal, np.zeros((1, 24, 32, 3), np.float32))
            assert _same(r.seen, np.zeros(F, np.uint8))
            assert ("color" in vars(r)) == (mm.colors is not None)
        assert mesh.visible_faces(mm, c.cameras).shape == (F,)
    for _ in range(2):
        r = mesh.render_mesh(m, [], size=(24, 32), outputs=ALL)
        assert r.depth.shape == (0, 24, 32) and r.face.shape == (0, 24, 32) and r.color.shape == (0, 24, 32, 3)
        assert _same(r.seen, np.zeros(2, np.uint8))
    assert not mesh.visible_faces(m, [], size=(24, 32)).any()
    out = mesh.cull_unseen(m, [], size=(24, 32))
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3)
    torch.cuda.synchronize()


def test_cull_unseen():
    from envgs_amd import mesh
    c = rc.nested_boxes()
    want = _oracle(c)
    assert want["seen"][~c.inner].all() and not want["seen"][c.inner].any()
    m = _mesh(c)
    for _ in range(2):
        ref, ref_index = mesh.select_faces(m, torch.from_numpy(want["seen"]).to(DEV), return_index=True)
        got, index = mesh.cull_unseen(m, c.cameras, near=c.near, return_index=True)
        assert got.faces.shape == (12, 3) and got.vertices.shape == (8, 3)
        for name in ("vertices", "faces", "colors"):
            assert _same(getattr(got, name), getattr(ref, name).cpu().numpy()), name
        assert _same(index, ref_index.cpu().numpy()) and index.cpu().tolist() == list(range(8))
        assert _same(got.vertices, c.vertices[:8]) and _same(got.colors, c.colors[:8])
        assert _same(got.faces, c.faces[~c.inner])
        assert _same(mesh.cull_unseen(m, c.cameras, near=c.near).faces, c.faces[~c.inner])


def test_mesh_views_writes_the_oracles_pictures(tmp_path):
    from envgs_amd import visualize
    c = rc.soup(33, 17)
    cams = c.cameras[:3]
    want = _oracle(c)
    acc = (want["face"][:3] >= 0).astype(np.float32)[..., None]
    planes = [dict(kind="normal", img=want["normal"][:3], acc=acc, M=np.stack([cam.R for cam in cams]), opaque=True),
              dict(kind="depth", img=want["depth"][:3, ..., None], acc=acc, curve="normalize", opaque=True),
              dict(kind="color", img=want["color"][:3], acc=acc, opaque=True)]
    ref = vo.image_planes(planes)                                # (3 planes, 3 views, H, W, 4)
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        with visualize.ImageWriter(str(d), ext=".ppm") as w:
            paths = visualize.mesh_views(_mesh(c), cams, w, near=c.near)
        assert len(paths) == 9
        for t, name in enumerate(visualize.MESH_TYPES):
            for b in range(3):
                path = w.path(name, b, 0)
                assert path in paths
                assert open(path, "rb").read() == visualize.encode_ppm(ref[t, b]), (name, b)
