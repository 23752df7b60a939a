"""NumPy oracle of the registration and of the Tanks-and-Temples protocol (include/envgs_mesh.h, "registration"): the fp32 transformation, the
brute-force nearest point, the 18 sums of an ICP iteration with math.fsum (exact sums of the double terms), a Kabsch / Umeyama solver of its own, the
literal ICP loop, the key and the mean rule of the voxel down-sampling and the crossing-number test of the crop volume.  Written from the header, not
from the kernels; csrc/mesh_register.hip and envgs_amd.mesh are checked against it.  Nothing here is imported from the product.

The registration cases of the GPU tests live here too (cases()), so that tests/test_mesh_register_cpu.py can show, on the oracle alone, that each is
one the oracle can judge."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from tests import mesh_eval_oracle as eo
from tests import mesh_simplify_oracle as so

F32, F64 = np.float32, np.float64
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


# ---- rule 1: the transformation ---------------------------------------------------------------------------------------------------------------------------
def rows_f32(T):
    """The upper 3x4 of T, every entry rounded once to fp32."""
    return np.asarray(T, F64)[:3, :4].astype(F32)


def transform(points, T):
    """x' = ((M00 x + M01 y) + M02 z) + M03 ..., every product and sum a separate fp32 operation."""
    p = np.asarray(points, F32).reshape(-1, 3)
    M = rows_f32(T)
    out = np.zeros(p.shape, F32)
    with np.errstate(all="ignore"):
        for r in range(3):
            s = M[r, 0] * p[:, 0]
            s = s + M[r, 1] * p[:, 1]
            s = s + M[r, 2] * p[:, 2]
            out[:, r] = s + M[r, 3]
    assert out.dtype == F32
    return out


def transform_terms(points, T):
    """sum over the four terms |M_r0 x| + |M_r1 y| + |M_r2 z| + |M_r3| per row and coordinate, in double: what the fp32 roundings are relative to."""
    p = np.abs(np.asarray(points, F32).reshape(-1, 3).astype(F64))
    M = np.abs(rows_f32(T).astype(F64))
    return p @ M[:, :3].T + M[:, 3][None, :]


# ---- rule 2: the sums -------------------------------------------------------------------------------------------------------------------------------------
def center(target):
    """c of the header: the centre of the box of the finite target rows, (lo + hi) / 2 per axis in double; the origin when there is none."""
    t = np.asarray(target, F32).reshape(-1, 3)
    fin = t[np.isfinite(t).all(axis=1)].astype(F64)
    return 0.5 * (fin.min(axis=0) + fin.max(axis=0)) if fin.shape[0] else np.zeros(3)


def sums(source, target, T, max_distance, c):
    """-> namespace(sums (18,) the exact sums of the double terms, rounded once (math.fsum); abs (18,) the sums of their magnitudes; n; moved (Q,3);
    dist2 (Q,), index (Q,): the brute-force matches of the moved rows)."""
    moved = transform(source, T)
    dist2, index = eo.nearest(moved, target, max_distance)
    hit = index >= 0
    t = np.asarray(target, F32).reshape(-1, 3)
    ah = moved[hit].astype(F64) - c[None, :]
    bh = t[index[hit]].astype(F64) - c[None, :]
    terms = np.zeros((int(hit.sum()), 18), F64)
    terms[:, 0] = 1.0
    terms[:, 1] = dist2[hit].astype(F64)
    terms[:, 2:5], terms[:, 5:8] = ah, bh
    for r in range(3):
        for k in range(3):
            terms[:, 8 + 3 * r + k] = ah[:, r] * bh[:, k]
    terms[:, 17] = ((ah[:, 0] * ah[:, 0]) + (ah[:, 1] * ah[:, 1])) + (ah[:, 2] * ah[:, 2])
    exact = np.array([math.fsum(terms[:, k]) for k in range(18)], F64)
    mag = np.array([math.fsum(np.abs(terms[:, k])) for k in range(18)], F64)
    return SimpleNamespace(sums=exact, abs=mag, n=int(hit.sum()), moved=moved, dist2=dist2, index=index)


def sums_bound(Q, mag):
    """Q 2^-52 sum |term|: any order of adding Q doubles stays within (Q - 1) 2^-53 (1 + small) of the exact sum relative to the magnitudes, and fsum
    itself rounds once."""
    return Q * 2.0 ** -52 * mag


# ---- rule 3: the solver -----------------------------------------------------------------------------------------------------------------------------------
def solve(s, with_scale=False, c=None):
    """Umeyama's closed form from the 18 sums, written on the covariance of the pairs.  -> (4,4) float64, or None where the header stops the loop
    (n < 3, or with_scale a variance that is not positive)."""
    s = np.asarray(s, F64)
    n = s[0]
    if n < 3:
        return None
    c = np.zeros(3) if c is None else np.asarray(c, F64)
    mu_a, mu_b = s[2:5] / n, s[5:8] / n
    cov = (s[8:17].reshape(3, 3).T - n * np.outer(mu_b, mu_a)) / n          # E[(b - mu_b)(a - mu_a)^T]
    var_a = s[17] / n - mu_a @ mu_a
    W, sig, Zt = np.linalg.svd(cov)
    flip = np.ones(3)
    if np.linalg.det(W) * np.linalg.det(Zt) < 0:
        flip[2] = -1.0
    R = (W * flip[None, :]) @ Zt
    scale = 1.0
    if with_scale:
        if not var_a > 0:
            return None
        scale = float((sig * flip).sum() / var_a)
    out = np.eye(4)
    out[:3, :3] = scale * R
    out[:3, 3] = c + (mu_b - scale * R @ mu_a) - scale * R @ c
    return out


def icp(source, target, max_distance, c, init=None, with_scale=False, max_iterations=20, rel_fitness=1e-6, rel_rmse=1e-6):
    """The loop of the header, literally.  -> namespace(transformation, fitness, inlier_rmse, iterations, converged, history [(T_k, sums_k)])"""
    T = np.eye(4) if init is None else np.array(init, F64)
    N = np.asarray(source).reshape(-1, 3).shape[0]
    history, prev, converged, updates = [], None, False, 0
    while True:
        e = sums(source, target, T, max_distance, c)
        fitness = e.n / N if N else 0.0
        rmse = math.sqrt(e.sums[1] / e.n) if e.n else 0.0
        history.append((T.copy(), e.sums))
        if prev is not None and abs(fitness - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
            converged = True
            break
        prev = (fitness, rmse)
        if e.n < 3 or updates >= max_iterations:
            break
        delta = solve(e.sums, with_scale, c)
        if delta is None:
            break
        T = delta @ T
        updates += 1
    return SimpleNamespace(transformation=T, fitness=fitness, inlier_rmse=rmse, iterations=updates, converged=converged, history=history, last=e)


def rmse_bound(source, T, index):
    """The fp32 floor of inlier_rmse at a transformation that maps the source onto its matches exactly: per matched row and coordinate
    2^-24 |M_rj| |p_j| for each stored source coordinate plus 4 2^-24 sum |terms| for the product and the three sums every term passes through;
    the root of the mean of the squared row bounds."""
    p = np.abs(np.asarray(source, F32).reshape(-1, 3).astype(F64))
    M = np.abs(rows_f32(T).astype(F64))
    e = EPS32 * (p @ M[:, :3].T) + 4.0 * EPS32 * transform_terms(source, T)
    hit = np.asarray(index) >= 0
    return math.sqrt(float((e[hit] ** 2).sum(axis=1).mean())) if hit.any() else 0.0


# ---- rule 4: the voxel mean ---------------------------------------------------------------------------------------------------------------------------------
def voxel_downsample(points, voxel, origin=None):
    """-> namespace(points (C,3) f32, cluster (N,) i32, keys (N,) int64 with 2^63 - 1 for a row that is not finite, origin, dims)"""
    p = np.asarray(points, F32).reshape(-1, 3)
    origin, dims = so.grid_of(p, voxel, origin)
    assert max(dims) <= 2 ** 21
    ijk, lin, u = so.vertex_cells(p, origin, voxel, dims)
    has = np.isfinite(p).all(axis=1)
    keys = np.where(has, ijk[:, 0] | (ijk[:, 1] << 21) | (ijk[:, 2] << 42), np.int64(2 ** 63 - 1))
    occupied = np.unique(keys[has])
    C = occupied.size
    cluster = np.full(p.shape[0], -1, np.int64)
    cluster[has] = np.searchsorted(occupied, keys[has])
    with np.errstate(all="ignore"):
        frac = (u - ijk.astype(F32)).astype(F32)
    frac = np.where(frac > 0, np.where(frac > 1, F32(1), frac), F32(0)).astype(F32)
    q = so._fixed(np.where(has[:, None], frac, F32(0)), 2 ** so.POS_BITS)
    members = np.bincount(cluster[has], minlength=C).astype(np.int64)
    total = np.zeros((C, 3), np.int64)
    np.add.at(total, cluster[has], q[has])
    qm = so._rounded_mean(total, np.maximum(members, 1)[:, None])
    cell_ijk = np.stack([occupied & 0x1FFFFF, (occupied >> 21) & 0x1FFFFF, (occupied >> 42) & 0x1FFFFF], axis=1)
    inside = (cell_ijk.astype(F32) + (qm.astype(F32) * F32(2.0 ** -so.POS_BITS)).astype(F32)).astype(F32)
    out = (np.asarray(origin, F32)[None, :] + (inside * F32(voxel)).astype(F32)).astype(F32)
    first = np.full(C, p.shape[0], np.int64)
    np.minimum.at(first, cluster[has], np.nonzero(has)[0])
    single = members == 1
    out[single] = p[first[single]]
    return SimpleNamespace(points=out, cluster=cluster.astype(np.int32), keys=keys, origin=origin, dims=dims)


# ---- rule 5: the crop volume --------------------------------------------------------------------------------------------------------------------------------
UV = {"X": (0, 1, 2), "Y": (1, 0, 2), "Z": (2, 0, 1)}              # axis -> (w, u, v)


def in_polygon(points, axis, axis_min, axis_max, polygon):
    p32 = np.asarray(points, F32).reshape(-1, 3)
    p = p32.astype(F64)
    poly = np.asarray(polygon, F64).reshape(-1, 3)
    w, u, v = UV[axis]
    M = poly.shape[0]
    crossings = np.zeros(p.shape[0], np.int64)
    with np.errstate(all="ignore"):
        for j in range(M):
            k = (j + 1) % M
            uj, vj, uk, vk = poly[j, u], poly[j, v], poly[k, u], poly[k, v]
            straddle = (vj > p[:, v]) != (vk > p[:, v])
            x = (uk - uj) * (p[:, v] - vj) / (vk - vj) + uj
            crossings += straddle & (p[:, u] < x)
        band = (F64(axis_min) <= p[:, w]) & (p[:, w] <= F64(axis_max))
    return np.isfinite(p32).all(axis=1) & band & (crossings % 2 == 1)


# ---- the registration cases ---------------------------------------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(degrees)
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def similarity(axis, degrees, translation, scale=1.0):
    T = np.eye(4)
    T[:3, :3] = scale * rotation(axis, degrees)
    T[:3, 3] = translation
    return T


def bumpy_surface(n, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (n, 2))
    z = 0.3 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]) + 0.1 * np.sin(7.0 * xy[:, 0] + 5.0 * xy[:, 1])
    return np.concatenate([xy, z[:, None]], axis=1).astype(F32)


MAX_DISTANCE = 0.3


@functools.lru_cache(maxsize=None)
def cases():
    """name -> namespace(source, target (f32), truth (4,4): the transformation that maps the source onto its partners, with_scale, fitness: the
    fraction of source rows that have a partner, max_distance).  The source is the inverse of `truth` applied, in double, to every `step`-th target
    point and rounded to fp32; the outlier case appends 300 rows far from everything."""
    rng = np.random.default_rng(20)
    cube = rng.uniform(-1, 1, (2000, 3)).astype(F32)
    surface = bumpy_surface(3000, 21)
    out = {}
    for name, target, step, truth, with_scale, outliers in (
            ("cube", cube, 2, similarity((1, 2, 3), 2.0, (0.02, -0.03, 0.01)), False, 0),
            ("cube+scale", cube, 2, similarity((3, -1, 2), 1.5, (-0.03, 0.01, 0.02), 1.03), True, 0),
            ("surface", surface, 3, similarity((1, 1, 4), 3.0, (0.03, 0.02, -0.02)), False, 0),
            ("outliers", cube, 2, similarity((-2, 1, 1), 2.5, (0.01, 0.03, -0.03)), False, 300)):
        part = target[::step].astype(F64)
        inv = np.linalg.inv(truth)
        source = (part @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
        if outliers:
            far = np.random.default_rng(22).uniform(-1, 1, (outliers, 3)) + np.array([6.0, -5.0, 7.0])
            source = np.concatenate([source, far.astype(F32)])
        out[name] = SimpleNamespace(source=source, target=target, truth=truth, with_scale=with_scale, fitness=part.shape[0] / source.shape[0],
                                    max_distance=MAX_DISTANCE)
    return out
