"""The rasterisation rule of include/envgs_mesh.h ("rasterisation") in NumPy and Python integers, face by face: the reference of
tests/test_mesh_raster_cpu.py (which holds the host build of csrc/mesh_raster.h to it bit for bit) and of tests/test_mesh_raster_gpu.py.  Written
from the rule's text, not from the header's code: projection in float32 operation by operation, edge functions in integers (int64 arrays over the
pixels of a box; the bounds of the rule keep them below 2^63), depth in float64, one 64-bit key per pixel, smallest wins.

A camera is anything with K (3,3), R (3,3) world -> camera and T (3,) or (3,1); a mesh is vertices (V,3) float32, faces (F,3) int32 and optional
colors (V,3) float32."""
import numpy as np

F32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LIMIT = F32(2.0 ** 21)


def _cam(cam):
    K = np.asarray(cam.K, F32).reshape(3, 3)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.asarray(cam.R, F32).reshape(3, 3), np.asarray(cam.T, F32).reshape(3)


def project(cam, vertices, near=0.0):
    """-> X, Y (V,) int64 sub-pixel positions (0 where not usable), zc (V,) float32, usable (V,) bool."""
    fx, fy, cx, cy, R, T = _cam(cam)
    v = np.asarray(vertices, F32).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        xc = R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + T[0]
        yc = R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + T[1]
        zc = R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + T[2]
        u = fx * (xc / zc) + cx
        w = fy * (yc / zc) + cy
        usable = np.isfinite(u) & np.isfinite(w) & (zc > F32(near)) & (np.abs(u) < LIMIT) & (np.abs(w) < LIMIT)
        X = np.where(usable, np.rint(u * F32(256.0)), F32(0.0)).astype(np.int64)
        Y = np.where(usable, np.rint(w * F32(256.0)), F32(0.0)).astype(np.int64)
    assert xc.dtype == F32 and u.dtype == F32
    return X, Y, zc, usable


def _drawn(f, faces, V, X, Y, usable):
    """-> (corner order as drawn, A > 0, exchanged) or None if the face is dropped."""
    idx = [int(i) for i in faces[f]]
    if any(i < 0 or i >= V for i in idx) or not all(usable[i] for i in idx):
        return None
    (x0, x1, x2), (y0, y1, y2) = [int(X[i]) for i in idx], [int(Y[i]) for i in idx]
    A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    if A == 0:
        return None
    return (idx, A, False) if A > 0 else ([idx[0], idx[2], idx[1]], -A, True)


def _edge_functions(order, X, Y, px, py):
    """px, py: int64 arrays of pixel indices.  -> [E_0, E_1, E_2] int64 arrays, covered bool array."""
    Px, Py = 256 * px + 128, 256 * py + 128
    E, inside = [], np.ones(px.shape, bool)
    for k in range(3):
        i, j = order[(k + 1) % 3], order[(k + 2) % 3]
        dx, dy = int(X[j]) - int(X[i]), int(Y[j]) - int(Y[i])
        e = dx * (Py - int(Y[i])) - dy * (Px - int(X[i]))
        top_left = dy < 0 or (dy == 0 and dx > 0)
        inside &= (e > 0) | ((e == 0) & top_left)
        E.append(e)
    return E, inside


def _terms(order, A, zc, E):
    """-> [l_k iz_k], s: float64 arrays."""
    t = [(e.astype(np.float64) / np.float64(A)) * (np.float64(1.0) / np.float64(zc[order[k]])) for k, e in enumerate(E)]
    return t, (t[0] + t[1]) + t[2]


def face_keys(f, vertices, faces, cam, H, W, near=0.0, projected=None):
    """The fragments of ONE face over all H x W pixels: (H, W) uint64 keys, EMPTY where it does not cover."""
    X, Y, zc, usable = projected if projected is not None else project(cam, vertices, near)
    keys = np.full((H, W), EMPTY, np.uint64)
    d = _drawn(f, faces, len(X), X, Y, usable)
    if d is None:
        return keys
    order, A, _ = d
    py, px = np.mgrid[0:H, 0:W].astype(np.int64)
    E, inside = _edge_functions(order, X, Y, px, py)
    with np.errstate(all="ignore"):
        _, s = _terms(order, A, zc, E)
        z = (np.float64(1.0) / s).astype(F32)
    k = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
    keys[inside] = k[inside]
    return keys


def key_image(vertices, faces, cam, H, W, near=0.0):
    """(H, W) uint64: the smallest key per pixel over all faces.  Faces are visited one by one; a box that provably contains every covered pixel
    (pixel centres between the extreme sub-pixel coordinates) limits the work."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    X, Y, zc, usable = project(cam, vertices, near)
    keys = np.full((H, W), EMPTY, np.uint64)
    for f in range(len(faces)):
        d = _drawn(f, faces, len(X), X, Y, usable)
        if d is None:
            continue
        order, A, _ = d
        xs, ys = [int(X[i]) for i in order], [int(Y[i]) for i in order]
        # centre 256 p + 128 in [lo, hi]  <=>  ceil((lo - 128) / 256) <= p <= floor((hi - 128) / 256); Python's // floors
        x0, x1 = max(0, -((128 - min(xs)) // 256)), min(W - 1, (max(xs) - 128) // 256)
        y0, y1 = max(0, -((128 - min(ys)) // 256)), min(H - 1, (max(ys) - 128) // 256)
        if x0 > x1 or y0 > y1:
            continue
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
        E, inside = _edge_functions(order, X, Y, px, py)
        if not inside.any():
            continue
        with np.errstate(all="ignore"):
            _, s = _terms(order, A, zc, E)
            z = (np.float64(1.0) / s).astype(F32)
        k = np.where(inside, (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f), EMPTY)
        keys[y0:y1 + 1, x0:x1 + 1] = np.minimum(keys[y0:y1 + 1, x0:x1 + 1], k)
    return keys


def _normal(p, exchanged):
    with np.errstate(all="ignore"):
        e1, e2 = p[1] - p[0], p[2] - p[0]
        c = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], F32)
        length = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        if length == 0:
            return np.zeros(3, F32)
        n = c / length
    return n if exchanged else -n                      # A > 0 before the exchange: the product points away from the camera


def resolve(keys, vertices, faces, cam, near=0.0, colors=None):
    """The maps of one view from its key image -> dict(depth, face, bary, normal[, color])."""
    H, W = keys.shape
    vertices = np.asarray(vertices, F32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    hit = keys != EMPTY
    face = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(0.0)).astype(F32)
    out = dict(depth=depth, face=face, bary=np.zeros((H, W, 3), F32), normal=np.zeros((H, W, 3), F32))
    if colors is not None:
        colors = np.asarray(colors, F32).reshape(-1, 3)
        out["color"] = np.zeros((H, W, 3), F32)
    X, Y, zc, usable = project(cam, vertices, near)
    for f in np.unique(face[hit]):
        order, A, exchanged = _drawn(int(f), faces, len(X), X, Y, usable)
        py, px = [a.astype(np.int64) for a in np.nonzero(face == f)]
        E, inside = _edge_functions(order, X, Y, px, py)
        assert inside.all()
        with np.errstate(all="ignore"):
            t, s = _terms(order, A, zc, E)
            b = [(tk / s).astype(F32) for tk in t]
        if exchanged:
            b = [b[0], b[2], b[1]]                      # back to the face's original corners
        idx = [int(i) for i in faces[f]]
        out["bary"][py, px] = np.stack(b, -1)
        out["normal"][py, px] = _normal(vertices[idx], exchanged)
        if colors is not None:
            with np.errstate(all="ignore"):
                c = [(b[0] * colors[idx[0], a] + b[1] * colors[idx[1], a]) + b[2] * colors[idx[2], a] for a in range(3)]
            out["color"][py, px] = np.stack(c, -1)
    return out


def render(vertices, faces, cameras, H, W, near=0.0, colors=None):
    """All views -> dict of stacked maps (n, H, W[, 3]), `key` (n, H, W) uint64 and `seen` (F,) uint8, the union over the views."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    names = ["depth", "face", "bary", "normal"] + (["color"] if colors is not None else [])
    shapes = dict(depth=(H, W), face=(H, W), bary=(H, W, 3), normal=(H, W, 3), color=(H, W, 3))
    maps = {n: [] for n in names}
    keys, seen = [], np.zeros(len(faces), np.uint8)
    for cam in cameras:
        k = key_image(vertices, faces, cam, H, W, near)
        keys.append(k)
        r = resolve(k, vertices, faces, cam, near, colors)
        for n in names:
            maps[n].append(r[n])
        seen[r["face"][r["face"] >= 0]] = 1
    out = {n: np.stack(v) if v else np.zeros((0,) + shapes[n], np.int32 if n == "face" else F32) for n, v in maps.items()}
    out["key"] = np.stack(keys) if keys else np.zeros((0, H, W), np.uint64)
    out["seen"] = seen
    return out
