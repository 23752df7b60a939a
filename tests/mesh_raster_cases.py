"""Small meshes and cameras for the mesh rasteriser's tests (tests/test_mesh_raster_cpu.py, tests/test_mesh_raster_gpu.py).  Everything is generated;
nothing is read from disk.  A case is a namespace: name, vertices (V,3) f32, faces (F,3) i32, colors (V,3) f32 or None, cameras, H, W, near."""
import math
from types import SimpleNamespace

import numpy as np

from tests import mesh_raster_oracle as ro

F32 = np.float32
SIZES = ((1, 1), (5, 3), (33, 17), (64, 48))                    # H x W


def camera(H, W, fx=None, fy=None, cx=None, cy=None, R=None, T=None):
    fx = 0.9 * W if fx is None else fx
    fy = fx if fy is None else fy
    cx = 0.5 * W if cx is None else cx
    cy = 0.5 * H if cy is None else cy
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F32)
    return SimpleNamespace(K=K, R=np.eye(3, dtype=F32) if R is None else np.asarray(R, F32), T=np.zeros(3, F32) if T is None else np.asarray(T, F32),
                           image_height=int(H), image_width=int(W))


def look_at(eye, target, H, W, fx=None):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    return camera(H, W, fx=fx, R=R, T=-(R @ eye))


def unproject(cam, u, v, z):
    """The world point (of an R = I, T = 0 camera) that lands near pixel position (u, v) at depth z."""
    K = cam.K
    return [(u - float(K[0, 2])) * z / float(K[0, 0]), (v - float(K[1, 2])) * z / float(K[1, 1]), z]


def case(name, vertices, faces, cameras, H, W, colors=None, near=0.0):
    return SimpleNamespace(name=name, vertices=np.asarray(vertices, F32).reshape(-1, 3), faces=np.asarray(faces, np.int32).reshape(-1, 3),
                           colors=None if colors is None else np.asarray(colors, F32).reshape(-1, 3), cameras=list(cameras), H=int(H), W=int(W),
                           near=float(near))


def vertex_colors(V, seed=0):
    return np.random.default_rng(seed).random((V, 3)).astype(F32)


def _small_faces(cam, H, W, z, count, seed):
    """count little triangles of about a pixel, scattered over the image at depth z."""
    rng = np.random.default_rng(seed)
    v = []
    for _ in range(count):
        u0, v0 = rng.uniform(0, W), rng.uniform(0, H)
        for _k in range(3):
            v.append(unproject(cam, u0 + rng.uniform(-1.5, 1.5), v0 + rng.uniform(-1.5, 1.5), z * rng.uniform(0.98, 1.02)))
    return v


def whole_image(H, W, extra=False):
    """One triangle whose corners lie far outside the image and which covers all of it, at varying depth; with extra: small faces in front of it
    and behind it."""
    cam = camera(H, W)
    v = [unproject(cam, -20.0 * W - 7.3, -15.0 * H - 3.1, 2.0), unproject(cam, 40.0 * W + 5.7, -15.0 * H - 1.9, 3.5), unproject(cam, 0.4 * W, 45.0 * H + 2.2, 2.75)]
    if extra:
        v += _small_faces(cam, H, W, 1.0, 12, 1) + _small_faces(cam, H, W, 6.0, 12, 2)
    faces = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return case("whole_image_%dx%d%s" % (H, W, "_extra" if extra else ""), v, faces, [cam], H, W, colors=vertex_colors(len(v), 3))


def box_pixels(c, f=0, view=0):
    """Pixels in the clamped box of face f: those whose centre lies between the extreme sub-pixel coordinates, inside the image."""
    X, Y, _, usable = ro.project(c.cameras[view], c.vertices, c.near)
    idx = c.faces[f]
    assert usable[idx].all()
    xs, ys = X[idx], Y[idx]
    x0, x1 = max(0, -((128 - int(xs.min())) // 256)), min(c.W - 1, (int(xs.max()) - 128) // 256)
    y0, y1 = max(0, -((128 - int(ys.min())) // 256)), min(c.H - 1, (int(ys.max()) - 128) // 256)
    return max(0, x1 - x0 + 1) * max(0, y1 - y0 + 1)


def boxed_faces(small_max, H=33, W=17):
    """Faces whose boxes hold small_max - 1, small_max and small_max + 1 pixels, in several shapes (rows, columns, near-squares) and both windings."""
    cam = camera(H, W)
    v, want = [], []
    slot = 0
    for n in (small_max - 1, small_max, small_max + 1):
        shapes = {(n, 1), (1, n)} | {(w, n // w) for w in range(2, n) if n % w == 0}
        for w, h in sorted(shapes):
            if w > W - 1 or h > H - 1:
                continue
            px0, py0 = slot % max(1, W - w), (3 * slot) % max(1, H - h)
            slot += 1
            u0, u1, v0, v1 = px0 + 0.25, px0 + w - 0.25, py0 + 0.25, py0 + h - 0.25
            z = 1.5 + 0.01 * slot
            tri = [unproject(cam, u0, v0, z), unproject(cam, u1, v0 + 0.1, z * 1.1), unproject(cam, u0 + 0.1, v1, z * 0.9)]
            v += tri if slot % 2 else [tri[0], tri[2], tri[1]]
            want.append(n)
    faces = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    c = case("boxed_faces_%d" % small_max, v, faces, [cam], H, W, colors=vertex_colors(len(v), 4))
    got = [box_pixels(c, f) for f in range(len(faces))]
    assert got == want, (got, want)
    return c


def subpixel_faces(H=33, W=17):
    """Faces smaller than a pixel: some between the pixel centres (they cover none), some around exactly one centre."""
    cam = camera(H, W)
    v = []
    for k in range(6):                                           # between centres
        u, w = 2.0 + 2 * k + 0.02, 3.0 + 4 * k + 0.03
        v += [unproject(cam, u - 0.2, w - 0.2, 2.0), unproject(cam, u + 0.3, w - 0.1, 2.0), unproject(cam, u, w + 0.3, 2.0)]
    for k in range(6):                                           # around the centre of pixel (3 + 2k, 5 + 4k)
        u, w = 3.5 + 2 * k, 5.5 + 4 * k
        v += [unproject(cam, u - 0.3, w - 0.25, 2.0 + k), unproject(cam, u + 0.35, w - 0.2, 2.0 + k), unproject(cam, u - 0.05, w + 0.4, 2.0 + k)]
    faces = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return case("subpixel_faces", v, faces, [cam], H, W, colors=vertex_colors(len(v), 5))


def fan(H, W, seed, reverse=False, flat=False):
    """A closed fan around an apex inside the image whose spokes end far outside it: consecutive spokes less than 2 pi / 3 apart."""
    rng = np.random.default_rng(seed)
    cam = camera(H, W)
    n = int(rng.integers(5, 10))
    ang = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) * (2 * math.pi / n) + rng.uniform(0, 2 * math.pi)
    rad = 4.0 * (H + W) * rng.uniform(1.0, 1.5, n)
    au, av = rng.uniform(0, W), rng.uniform(0, H)
    depth = (lambda: 2.0) if flat else (lambda: float(rng.uniform(1.0, 4.0)))
    v = [unproject(cam, au, av, depth())] + [unproject(cam, au + r * math.cos(a), av + r * math.sin(a), depth()) for a, r in zip(ang, rad)]
    faces = [[0, 1 + k, 1 + (k + 1) % n] for k in range(n)]
    if reverse:
        faces = [[a, c, b] for a, b, c in faces]
    return case("fan_%dx%d_%d%s%s" % (H, W, seed, "_rev" if reverse else "", "_flat" if flat else ""), v, faces, [cam], H, W, colors=vertex_colors(n + 1, seed))


def quad():
    """The pixel-aligned quad u in [4, 12], v in [3, 9] at z = 2 as two triangles: 48 pixels, rows 3..8, columns 4..11."""
    cam = camera(24, 32, fx=50.0, fy=50.0, cx=16.0, cy=12.0)
    v = [unproject(cam, 4.0, 3.0, 2.0), unproject(cam, 12.0, 3.0, 2.0), unproject(cam, 12.0, 9.0, 2.0), unproject(cam, 4.0, 9.0, 2.0)]
    return case("quad", v, [[0, 1, 2], [0, 2, 3]], [cam], 24, 32, colors=vertex_colors(4, 6))


def duplicates(H=33, W=17):
    """The same face four times under different indices of the same vertices (and once through duplicated vertices): the lowest index wins."""
    cam = camera(H, W)
    tri = [unproject(cam, 1.2, 2.1, 2.0), unproject(cam, 15.3, 6.4, 3.0), unproject(cam, 6.6, 30.2, 2.5)]
    faces = [[3, 4, 5], [0, 1, 2], [1, 2, 0], [0, 2, 1], [0, 1, 2]]
    return case("duplicates", tri + tri, faces, [cam], H, W, colors=vertex_colors(6, 7))


def interpenetrating(H=64, W=48):
    """Two triangles that cross each other: each is in front over a part of their overlap."""
    cam = camera(H, W)
    a = [unproject(cam, 2.0, 3.0, 1.0), unproject(cam, 46.0, 10.0, 3.0), unproject(cam, 20.0, 60.0, 3.0)]
    b = [unproject(cam, 45.0, 58.0, 1.0), unproject(cam, 3.0, 50.0, 3.0), unproject(cam, 30.0, 2.0, 3.0)]
    return case("interpenetrating", a + b, [[0, 1, 2], [3, 4, 5]], [cam], H, W, colors=vertex_colors(6, 8))


def dropped(H=33, W=17, near=0.5):
    """Faces the rule drops, each between two ordinary neighbours: behind the camera, across the camera plane, a NaN and an inf corner, indices
    outside [0, V), zero screen area (a repeated corner; three collinear snapped positions), and a corner exactly at zc == near."""
    cam = camera(H, W)
    good = lambda k: [unproject(cam, 1.0 + k, 2.0 + 3 * k, 2.0 + k), unproject(cam, 9.0 + k, 4.0 + 3 * k, 2.5 + k), unproject(cam, 4.0 + k, 12.0 + 3 * k, 3.0 + k)]
    v, faces, bad = [], [], []
    def add(tri, is_bad):
        bad.append(is_bad)
        faces.append([len(v), len(v) + 1, len(v) + 2])
        v.extend(tri)
    add(good(0), False)
    add([[0.1, 0.1, -2.0], [0.5, 0.1, -2.0], [0.1, 0.5, -2.5]], True)                    # behind
    add(good(1), False)
    add([[-0.3, -0.2, 2.0], [0.4, -0.2, 2.0], [0.0, 0.3, -1.0]], True)                   # across the camera plane
    add(good(2), False)
    add([[float("nan"), 0.0, 2.0], [0.4, -0.2, 2.0], [0.0, 0.3, 2.0]], True)
    add([[-0.3, -0.2, 2.0], [float("inf"), -0.2, 2.0], [0.0, 0.3, 2.0]], True)
    add(good(3), False)
    add([unproject(cam, 3.0, 3.0, 2.0)] * 2 + [unproject(cam, 9.0, 9.0, 2.0)], True)    # zero area: a repeated corner
    add([unproject(cam, 2.0, 2.0, 2.0), unproject(cam, 4.0, 4.0, 2.0), unproject(cam, 8.0, 8.0, 2.0)], True)      # zero area: collinear (exact in f32)
    add(good(4), False)
    add([[-0.3, -0.2, near], [0.4, -0.2, 2.0], [0.0, 0.3, 2.0]], True)                   # zc == near exactly (R = I, T = 0)
    add(good(5), False)
    V = len(v)
    for idx in ([0, 1, V], [-1, 1, 2], [0, 2 ** 31 - 1, 2], [-2 ** 31, 1, 2]):          # would cover pixels if the bad index were read as a neighbour
        faces.append(idx)
        bad.append(True)
    faces.append(faces[0][::-1])                                                         # a last ordinary face, behind face 0 over the same pixels
    bad.append(False)
    c = case("dropped", v, faces, [cam], H, W, colors=vertex_colors(V, 9), near=near)
    c.bad = np.array(bad)
    return c


def extreme_faces(H=64, W=48):
    """Corners just inside and just outside the 2^21-pixel limit: the largest edge functions the int64 arithmetic has to hold.  The faces whose
    corners are all inside the limit cover the image; one corner outside drops the face."""
    cam = camera(H, W, fx=64.0, fy=64.0, cx=24.0, cy=32.0)
    big, over = 2.0 ** 21 - 4096.0, 2.0 ** 21 + 4096.0
    v, faces = [], []
    for k, (a, b) in enumerate(((big, big), (big, over), (over, big), (big, big))):
        z = 2.0 + k
        s = -1.0 if k == 3 else 1.0                             # the last one the other way round and mirrored
        v += [unproject(cam, -s * a, -s * b, z), unproject(cam, s * a, -s * b * 0.999, z), unproject(cam, s * 3.0, s * b, z)]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    return case("extreme_faces", v, faces, [cam], H, W, colors=vertex_colors(len(v), 13))


def ring_cameras(n, H, W, radius=3.0):
    cams = []
    for k in range(n):
        a = 2 * math.pi * k / n
        el = math.radians(15.0 + 12.0 * (k % 3))
        eye = [radius * math.cos(el) * math.cos(a), radius * math.cos(el) * math.sin(a), radius * math.sin(el)]
        cams.append(look_at(eye, [0.0, 0.0, 0.0], H, W, fx=0.8 * W))
    return cams


def soup(H, W, faces=3000, cameras=9, seed=11):
    """Random triangles of mixed sizes in the unit cube with colours, seen from a ring of cameras: two launches."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1, 1, (faces, 1, 3))
    scale = rng.choice([0.02, 0.1, 0.5, 2.0], (faces, 1, 1), p=[0.5, 0.3, 0.15, 0.05])
    v = (centre + scale * rng.uniform(-1, 1, (faces, 3, 3))).reshape(-1, 3)
    idx = np.arange(3 * faces, dtype=np.int32).reshape(-1, 3)
    idx[::7, 2] = idx[1::7, 0][:len(idx[::7])]                                           # some faces share vertices
    return case("soup_%dx%d" % (H, W), v, idx, ring_cameras(cameras, H, W), H, W, colors=vertex_colors(3 * faces, seed))


def _box(lo, hi):
    c = np.array([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], F32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    return c, np.array([t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))], np.int32)


def nested_boxes(H=33, W=17):
    """A closed box with a smaller one inside it, interleaved face by face, seen from six sides: no camera sees the inner box."""
    vo, fo = _box(-1.0, 1.0)
    vi, fi = _box(-0.4, 0.4)
    faces = np.empty((24, 3), np.int32)
    faces[0::2], faces[1::2] = fo, fi + 8
    eyes = [(4, 1, 0.5), (-4, 1, 0.5), (1, 4, 0.5), (1, -4, 0.5), (0.5, 1, 4), (0.5, 1, -4)]
    cams = [look_at(e, [0, 0, 0], H, W, fx=1.2 * W) for e in eyes]
    c = case("nested_boxes", np.concatenate([vo, vi]), faces, cams, H, W, colors=vertex_colors(16, 12))
    c.inner = np.arange(24) % 2 == 1
    return c


def all_cases(small_max=16):
    out = []
    for H, W in SIZES:
        out += [whole_image(H, W), whole_image(H, W, extra=True)]
    out += [boxed_faces(small_max), subpixel_faces(), quad(), duplicates(), interpenetrating(),
            dropped(), nested_boxes(), extreme_faces()]
    out += [fan(33, 17, 1), fan(33, 17, 2, reverse=True), fan(5, 3, 3, flat=True), fan(1, 1, 4), fan(64, 48, 5, reverse=True)]
    out += [soup(33, 17), soup(64, 48)]
    return out
