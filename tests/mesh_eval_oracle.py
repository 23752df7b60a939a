"""NumPy oracle of the mesh evaluation (include/envgs_mesh.h, "evaluation"): the counter hash, the per-face sample counts, the samples, the
brute-force nearest point within a radius, and the metrics.  Written from the header, not from the kernels; the kernels of csrc/mesh_eval.hip and
the host build of csrc/mesh_rng.h are checked against it.  Nothing here is imported from the product."""
from types import SimpleNamespace

import numpy as np

F32, U32 = np.float32, np.uint32
COUNT_STREAM = 0xFFFFFFFF
TWO_M24 = F32(2.0 ** -24)


# ---- the hash -----------------------------------------------------------------------------------------------------------------------------------------
def mix(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)          # uint32 arithmetic carried in uint64, masked after every product
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x


def hash3(seed, f, j):
    """h(seed, f, j) -> uint32 array (broadcast)."""
    m = np.uint64(0xFFFFFFFF)
    f = np.asarray(f, np.uint64) & m
    j = np.asarray(j, np.uint64) & m
    return mix(mix(mix(np.asarray(seed, np.uint64)) ^ f) ^ j).astype(U32)


def bits24(h):
    return (np.asarray(h, U32) >> U32(8)).astype(np.int64)


def uniform(h):
    return bits24(h).astype(F32) * TWO_M24                        # < 2^24: the conversion and the product are exact


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------------------
def face_counts(vertices, faces, density, seed):
    """-> namespace(count (F,) int64, over: bool, area (F,) float32 with 0 for the excluded faces, valid (F,) bool)"""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = v.shape[0], f.shape[0]
    inrange = ((f >= 0) & (f < V)).all(axis=1)
    safe = np.where(inrange[:, None], f, 0)
    if V == 0:
        return SimpleNamespace(count=np.zeros(F, np.int64), over=False, area=np.zeros(F, F32), valid=np.zeros(F, bool))
    a, b, c = v[safe[:, 0]], v[safe[:, 1]], v[safe[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = F32(0.5) * np.sqrt((nx * nx + ny * ny) + nz * nz)
        assert area.dtype == F32
        finite = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
        valid = inrange & finite & np.isfinite(area) & (area != 0)
        t = area * F32(density) + uniform(hash3(seed, np.arange(F), COUNT_STREAM))
        assert t.dtype == F32
        over = valid & ~(t < F32(2.0 ** 24))
        count = np.where(valid & ~over, np.floor(np.where(valid & ~over, t, 0)), 0).astype(np.int64)
    return SimpleNamespace(count=count, over=bool(over.any()), area=np.where(valid, area, F32(0)), valid=valid)


def sample_uv(seed, face, k):
    """-> (u, v) float32 of sample k of each face, folded."""
    hu, hv = hash3(seed, face, 2 * np.asarray(k, np.int64)), hash3(seed, face, 2 * np.asarray(k, np.int64) + 1)
    u, v = uniform(hu), uniform(hv)
    fold = bits24(hu) + bits24(hv) > 2 ** 24
    return np.where(fold, F32(1) - u, u).astype(F32), np.where(fold, F32(1) - v, v).astype(F32)


def sample_surface(vertices, faces, colors, density, seed):
    """-> namespace(points (S,3) f32, colors (S,3) f32 or None, face (S,) i32, k (S,), u, v (S,) f32, count (F,), over)"""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fc = face_counts(v, f, density, seed)
    assert not fc.over and fc.count.sum() < 2 ** 31
    face = np.repeat(np.arange(f.shape[0]), fc.count)
    start = np.cumsum(fc.count) - fc.count
    k = np.arange(face.shape[0]) - start[face]
    u, w = sample_uv(seed, face, k)

    def interp(attr):
        a, b, c = attr[f[face, 0]], attr[f[face, 1]], attr[f[face, 2]]
        with np.errstate(all="ignore"):
            out = (a + u[:, None] * (b - a)) + w[:, None] * (c - a)
        assert out.dtype == F32
        return out

    points = interp(v) if face.shape[0] else np.zeros((0, 3), F32)
    cols = None if colors is None else (interp(np.asarray(colors, F32).reshape(-1, 3)) if face.shape[0] else np.zeros((0, 3), F32))
    return SimpleNamespace(points=points, colors=cols, face=face.astype(np.int32), k=k, u=u, v=w, count=fc.count, over=fc.over)


# ---- nearest ------------------------------------------------------------------------------------------------------------------------------------------
def nearest(queries, points, max_distance, chunk=256):
    """Brute force, literally the header's definition.  -> (dist2 (Q,) float32, index (Q,) int32)"""
    q = np.asarray(queries, F32).reshape(-1, 3)
    p = np.asarray(points, F32).reshape(-1, 3)
    r2 = F32(max_distance) * F32(max_distance)
    Q, N = q.shape[0], p.shape[0]
    dist2 = np.full(Q, np.inf, F32)
    index = np.full(Q, -1, np.int32)
    pf = np.isfinite(p).all(axis=1)
    if N == 0:
        return dist2, index
    for s in range(0, Q, chunk):
        qq = q[s:s + chunk]
        with np.errstate(all="ignore"):
            d = qq[:, None, :] - p[None, :, :]
            d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
            assert d2.dtype == F32
            cand = pf[None, :] & (d2 <= r2) & np.isfinite(qq).all(axis=1)[:, None]
        d2 = np.where(cand, d2, F32(np.inf))
        best = d2.argmin(axis=1)                                  # the first of equal minima: the lowest index
        got = cand[np.arange(qq.shape[0]), best]
        dist2[s:s + chunk] = np.where(got, d2[np.arange(qq.shape[0]), best], F32(np.inf))
        index[s:s + chunk] = np.where(got, best, -1)
    return dist2, index


# ---- metrics ------------------------------------------------------------------------------------------------------------------------------------------
def evaluate(pred, ref, max_distance, threshold):
    out = {}
    d = {}
    for name, a, b in (("pred", pred, ref), ("ref", ref, pred)):
        d2, _ = nearest(a, b, max_distance)
        with np.errstate(all="ignore"):
            dist = np.sqrt(d2.astype(np.float64))
        found = np.isfinite(dist)
        d[name] = dist
        out["n_" + name] = int(dist.shape[0])
        out["found_" + name] = int(found.sum())
        out["within_" + name] = int((dist <= float(threshold)).sum())
        out["mean_" + name] = float(dist[found].sum() / found.sum()) if found.any() else float("nan")
    P = out["within_pred"] / out["n_pred"] if out["n_pred"] else 0.0
    R = out["within_ref"] / out["n_ref"] if out["n_ref"] else 0.0
    return SimpleNamespace(accuracy=out["mean_pred"], completeness=out["mean_ref"], chamfer=0.5 * (out["mean_pred"] + out["mean_ref"]), precision=P, recall=R,
                           fscore=2 * P * R / (P + R) if P + R > 0 else 0.0, n_pred=out["n_pred"], n_ref=out["n_ref"], found_pred=out["found_pred"],
                           found_ref=out["found_ref"], within_pred=out["within_pred"], within_ref=out["within_ref"], d_pred=d["pred"], d_ref=d["ref"])
