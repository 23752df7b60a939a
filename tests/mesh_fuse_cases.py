"""The rigs and synthetic depth maps of the depth-fusion tests (csrc/mesh_fuse.hip), in one place: tests/golden/make_fuse_golden.py records the
reference's outputs on the golden cases, tests/test_mesh_fuse_cpu.py judges the oracle on them and tests/test_mesh_fuse_gpu.py the device.  NumPy only.

Every scene is the unit sphere at the origin seen from cameras on an arc, the depth being the analytic z-depth of the near intersection through the
pixel centres (0 where the ray misses: the reference's "no depth")."""
import functools
import os
from types import SimpleNamespace

import numpy as np

SPHERE_R = 1.0


def look_at(c, target=(0.0, 0.0, 0.0)):
    """R (world -> camera, rows = camera axes) and T of a camera at c looking at target, z up."""
    c = np.asarray(c, np.float64)
    fwd = np.asarray(target, np.float64) - c
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, (0.0, 0.0, 1.0))
    right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(fwd, right), fwd])
    return R, -R @ c


def intrinsics(H, W, f):
    """A focal length in pixels and a principal point slightly off the middle, so that no pixel centre sits on an axis of symmetry."""
    return np.array([[f, 0.0, W / 2 - 0.29], [0.0, f * 1.03, H / 2 + 0.17], [0.0, 0.0, 1.0]])


def sphere_depth(K, R, T, H, W, radius=SPHERE_R):
    """z-depth of the sphere |x| = radius through the pixel centres: the near intersection, 0 where the ray misses."""
    cc = np.asarray(T, np.float64).reshape(3)                   # the sphere's centre in camera coordinates
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack([(px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1], np.ones_like(px)], axis=-1)
    dd, dc = (d * d).sum(-1), d @ cc
    disc = dc * dc - dd * (cc @ cc - radius ** 2)
    t = (dc - np.sqrt(np.maximum(disc, 0))) / dd
    return np.where(disc > 0, t, 0.0).astype(np.float32)


def arc_rig(V, H, W, f=None, distance=3.2, step_deg=9.0, targets=None):
    """V cameras on an arc around the sphere, a few degrees apart, at slightly different heights and distances (distinct centres, no ties).
    targets: per-camera look-at points (default: the origin).  -> namespace(K, R, T (V,...) float32-exact float64 arrays, H, W, depth (V,H,W) f32)."""
    f = f if f is not None else 0.95 * min(H, W) * distance / 2.2
    K, R, T = [], [], []
    for v in range(V):
        az = np.radians(step_deg * (v - 0.5 * (V - 1)) + 0.7 * (v % 2))
        el = np.radians(12.0 + 4.0 * (v % 3))
        rad = distance * (1.0 + 0.013 * v)
        c = rad * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        r, t = look_at(c, (0.0, 0.0, 0.0) if targets is None else targets[v])
        K.append(intrinsics(H, W, f))
        R.append(r)
        T.append(t)
    q = lambda a: np.stack(a).astype(np.float32).astype(np.float64)      # what a float32 camera holds
    K, R, T = q(K), q(R), q(T)
    depth = np.stack([sphere_depth(K[v], R[v], T[v], H, W) for v in range(V)])
    return SimpleNamespace(K=K, R=R, T=T, H=H, W=W, depth=depth)


def centres(R, T):
    return -np.einsum("vji,vj->vi", R, T)


def nearest(R, T, n):
    """The n nearest other cameras by centre distance, ties to the lowest index: the sources of the golden cases (the CPU test compares
    mesh.nearest_views and the reference's compute_camera_similarity with it)."""
    C = centres(R, T)
    d = np.linalg.norm(C[:, None] - C[None], axis=-1)
    V = len(C)
    return np.array([[j for j in np.argsort(d[v], kind="stable") if j != v][:min(n, V - 1)] for v in range(V)], np.int64).reshape(V, min(n, V - 1))


DEFAULTS = dict(geo_abs_thresh=1.0, geo_rel_thresh=0.01, geo_sum_thresh=0.75, pho_abs_thresh=0.0)      # scripts/fusion/depth_fusion.py


def _case(rig, sources, **thresholds):
    return SimpleNamespace(K=rig.K, R=rig.R, T=rig.T, H=rig.H, W=rig.W, depth=rig.depth, sources=np.asarray(sources, np.int64),
                           thresholds=dict(DEFAULTS, **thresholds))


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """The inputs of a golden case, built once: treat as read-only."""
    if name == "sphere":                                        # six views at 48 x 64, the four nearest as sources
        rig = arc_rig(6, 48, 64)
        return _case(rig, nearest(rig.R, rig.T, 4))
    if name == "holes":                                         # zero depth punched into maps that serve as sources (1, 4) and as reference (2)
        rig = arc_rig(6, 48, 64)
        rig.depth = rig.depth.copy()
        rig.depth[1, 14:23, 20:31] = 0.0
        rig.depth[4, 25:37, 33:40] = 0.0
        rig.depth[2, 18:26, 26:41] = 0.0
        return _case(rig, nearest(rig.R, rig.T, 4))
    if name == "border":                                        # every camera looks past the sphere: its image cuts the surface its neighbours see
        tg = [(0.0, 0.9 * (-1) ** v, 0.5 * ((v % 3) - 1)) for v in range(5)]
        rig = arc_rig(5, 30, 40, targets=tg)
        return _case(rig, nearest(rig.R, rig.T, 3))
    if name == "s3":                                            # S = 3 under geo_sum_thresh 0.75: min_count 3 from 2.25
        rig = arc_rig(4, 24, 32)
        return _case(rig, nearest(rig.R, rig.T, 3))
    raise KeyError(name)


GOLDEN = ["sphere", "holes", "border", "s3"]
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuse_golden.npz")


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/fuse_golden.npz (make_fuse_golden.py): -> namespace(band, rays_origin, rays_direction, cases = {name: namespace of its arrays,
    plus `thresholds` as the keyword arguments}).  Loaded once: treat as read-only."""
    z = np.load(GOLDEN_PATH)
    out = {}
    for name in GOLDEN:
        c = SimpleNamespace(**{k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")})
        c.thresholds = dict(zip(("geo_abs_thresh", "geo_rel_thresh", "geo_sum_thresh", "pho_abs_thresh"), (float(t) for t in c.thresholds)))
        c.H, c.W = c.depth.shape[1:]
        out[name] = c
    return SimpleNamespace(band=float(z["band"]), rays_origin=z["rays/origin"], rays_direction=z["rays/direction"], cases=out)


# ---- the device shapes: (H, W) around one workgroup of 256 pixels and one scan block --------------------------------------------------------------------
SHAPES = [(1, 1), (1, 65), (3, 85), (16, 16), (1, 257), (17, 31)]


@functools.lru_cache(maxsize=None)
def shape_case(H, W, V=3, S=2):
    """V views of H x W with S sources each (cyclic: view v takes v+1, v+2, ..: more sources than other views repeat them).
    geo_rel_thresh is 0.03 here, not the script's 0.01: at 16 pixels across, the bilinear interpolation error of the sphere's depth is itself
    about 1 %, so 0.01 cuts through the bulk of the pixels and the measured band leaves up to 1.8 % of them on the threshold (the oracle alone,
    on the CPU).  These cases are about indexing; at 0.03 at most one pixel of a case is fragile.  The golden cases keep the defaults."""
    rig = arc_rig(V, H, W, f=0.8 * max(H, W, 8) * 3.2 / 2.2, step_deg=4.0)
    src = [[(v + 1 + k % max(V - 1, 1)) % V for k in range(S)] for v in range(V)] if V > 1 else [[] for _ in range(V)]
    return _case(rig, np.array(src, np.int64).reshape(V, S if V > 1 else 0), geo_rel_thresh=0.03)


@functools.lru_cache(maxsize=None)
def bad_values_case():
    """Zero, NaN, +inf and negative depths in maps that are references and sources at once."""
    rig = arc_rig(4, 24, 40)
    d = rig.depth = rig.depth.copy()
    d[0, 3::7, 2::5] = np.nan
    d[0, 5::7, 0::5] = np.inf
    d[1, 1::6, 4::5] = -1.0
    d[1, 2::6, 1::7] = 0.0
    d[2, 4::5, 3::6] = np.nan
    d[3, 0::6, 2::4] = -np.inf
    return _case(rig, nearest(rig.R, rig.T, 3))


@functools.lru_cache(maxsize=None)
def far_border_case():
    """Sources that see most of the reference's surface outside their image, and one BEHIND the surface: camera 3 sits inside the sphere's far side
    looking away, so the reference's points have negative z there."""
    tg = [(0.0, 1.6 * (-1) ** v, 0.0) for v in range(3)] + [(9.0, 0.0, 0.0)]
    rig = arc_rig(4, 24, 40, targets=tg)
    r, t = look_at((-3.0, 0.1, 0.2), (-9.0, 0.0, 0.0))          # behind the sphere, looking away from it
    rig.R[3], rig.T[3] = r.astype(np.float32), t.astype(np.float32)
    rig.depth[3] = np.float32(2.5)                              # it claims a depth everywhere, so only the geometry can reject it
    return _case(rig, [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], geo_sum_thresh=0.5)      # two of three: the one behind never agrees
