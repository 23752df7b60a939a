"""The shapes at which the mesh kernels (csrc/mesh.hip) take another path, in one table: tests/test_mesh_cpu.py checks on the oracle alone that
every integration configuration is one `check_fused` can judge, tests/test_mesh_shapes_gpu.py runs them on the device.

A lane of tsdf_integrate / mesh_classify owns 4 consecutive voxels of the x-fastest planes, a workgroup 1024 (integration, classify) or 256
(count, emit), 16 B accesses need 16 B alignment of every plane: so `n % 4`, `nx % 4`, `n % 1024` and the alignment of tsdf / weight / rgb select
the paths, and nothing else about a shape does."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import mesh_oracle as mo
from tests import test_mesh_gpu as base                         # its six-view orbit, sphere and intrinsics are the scene of every row

# ---- integration: name -> (dims (nx,ny,nz), voxel, origin, view set); "reaches" says why the row is there ------------------------------------------------
INTEGRATION = {
    # n % 4 == 3: the last lane owns 3 voxels; nx % 4 == 1: quads wrap rows and slices; a partial last workgroup; rgb planes 1, 2 off 16 B
    "37x35x33": ((37, 35, 33), 0.05, (-0.9131, -0.8873, -0.7919), "orbit"),
    "41x37x33": ((41, 37, 33), 0.05, (-1.0131, -0.8873, -0.7919), "orbit"),                    # n % 4 == 1
    "3x3x3": ((3, 3, 3), 0.45, (-0.4431, -0.4573, -0.4619), "orbit"),                          # every quad crosses a row; nx ny = 9 crosses slices
    "2x2x2": ((2, 2, 2), 0.7, (-0.3431, -0.3573, -0.3619), "orbit"),                           # the minimum volume
    "5x3x2": ((5, 3, 2), 0.4, (-0.8131, -0.4373, -0.2119), "orbit"),                           # n % 4 == 2, one workgroup with a tail
    "7x5x3": ((7, 5, 3), 0.3, (-0.9131, -0.6373, -0.3119), "orbit"),                           # n % 4 == 1, one workgroup with a tail
    "2x3x171": ((2, 3, 171), 0.0125, (0.5531, -0.0173, -1.0619), "orbit"),                     # n = 1026: a second workgroup of two voxels
    # nx > 1024: a row longer than a workgroup's 1024 voxels.  (voxel 0.002 from (-1.0131, 0.0127, 0.5781) lies in front of the sphere in every
    # image and is observed everywhere; this row runs from x = -1.54 to 1.54 through the sphere, off its axes, and leaves the silhouettes)
    "1027x2x2": ((1027, 2, 2), 0.003, (-1.5431, 0.4127, 0.3081), "orbit"),
    "inside": ((37, 35, 33), 0.05, (-0.9131, -0.8873, -0.7919), "inside"),                     # zc <= 0 for part of the volume; NaN / inf / < 0 depth
    "mixed": ((37, 35, 33), 0.05, (-0.9131, -0.8873, -0.7919), "mixed"),                       # views of two sizes, +- colour, own trunc / depth_max
    "40x36x32": ((40, 36, 32), 0.05, (-1.0131, -0.8873, -0.7919), "orbit"),                    # the aligned n % 1024 == 0 shape: the 16 B paths
    # the ragged end-to-end bounds of test_mesh_shapes_gpu.py, on analytic depth maps of the surfel sphere through the cameras it renders
    "ragged e2e": ((43, 41, 39), 0.0391, (-0.8131, -0.7873, -0.8019), "e2e"),
}
E2E_HI = (0.8, 0.75, 0.68)                                      # with the voxel and origin above: TSDFVolume rounds to (43, 41, 39)


def trunc_of(name):
    return 5 * INTEGRATION[name][1] if INTEGRATION[name][3] == "e2e" else base.TRUNC


def sphere_depth(R, T, H, W, K, far=False, centre=base.SPHERE_C):
    """z-depth of the sphere of test_mesh_gpu.py through the pixel centres of any image: the near intersection, or the far one (the only one a
    camera inside the sphere sees), 0 where the ray misses."""
    cc = np.asarray(R, np.float64) @ np.array(centre) + np.asarray(T, np.float64).reshape(3)
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack([(px - K[0][2]) / K[0][0], (py - K[1][2]) / K[1][1], np.ones_like(px)], axis=-1)
    dd, dc = (d * d).sum(-1), d @ cc
    disc = dc * dc - dd * (cc @ cc - base.SPHERE_R ** 2)
    root = np.sqrt(np.maximum(disc, 0))
    t = (dc + root) / dd if far else (dc - root) / dd
    return np.where(disc > 0, t, 0.0).astype(np.float32)


def _look(c, fwd):
    """R, T of a camera at c looking along fwd, z up (the construction of synth.orbit_camera)."""
    fwd = np.asarray(fwd, np.float64) / np.linalg.norm(fwd)
    right = np.cross(fwd, (0.0, 0.0, 1.0))
    right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(fwd, right), fwd])
    return R.astype(np.float32), (-R @ np.asarray(c, np.float64)).astype(np.float32)


def _inside_views():
    """Five cameras INSIDE the sphere at different yaws: part of the volume is behind each (zc <= 0), the depth is the far intersection, and a
    lattice of pixels holds what a rendered map can hold where nothing was hit: NaN, +inf, a negative number.  Random colour."""
    rng = np.random.default_rng(11)
    out = []
    for v in range(5):
        yaw = 0.4 + 2.0 * np.pi * v / 5
        c = np.array(base.SPHERE_C) + 0.22 * np.array([np.cos(yaw + 2.1), np.sin(yaw + 2.1), 0.3 * np.sin(1.7 * v)])
        R, T = _look(c, (np.cos(yaw), np.sin(yaw), 0.25 * np.cos(1.3 * v)))
        depth = sphere_depth(R, T, base.H, base.W, base.KMAT, far=True)
        assert (depth > 0).all()                                # from inside every ray hits
        depth[1::7, 2::5] = np.nan
        depth[3::7, 0::5] = np.inf
        depth[5::7, 4::5] = -1.0
        out.append(mo.make_view(depth, base.KMAT, R, T, rgb=rng.random((3, base.H, base.W), dtype=np.float32), trunc=base.TRUNC))
    return out


H2, W2 = 30, 40
KMAT2 = [[44.0, 0.0, W2 / 2 - 0.29], [0.0, 45.3, H2 / 2 + 0.17], [0.0, 0.0, 1.0]]


def _mixed_views():
    """What the C-ABI allows in ONE launch and the Python front end never builds: two image sizes, views with and without colour, each with its
    own trunc and depth_max (the sphere's depths run from 2.4 to about 3)."""
    from envgs_amd import synth
    orbit = base._views(6)
    rng = np.random.default_rng(12)
    small = []
    for v in (1, 3):
        cam = synth.orbit_camera(v, n_views=5, radius=3.0, H=H2, W=W2, fx=44.0)
        R, T = cam.R.numpy(), cam.T.numpy().reshape(3)
        small.append((sphere_depth(R, T, H2, W2, KMAT2), R, T))
    mk = mo.make_view
    return [mk(orbit[0].depth, base.KMAT, orbit[0].R, orbit[0].T, rgb=orbit[0].rgb, trunc=0.2),
            mk(small[0][0], KMAT2, small[0][1], small[0][2], rgb=None, trunc=0.15, depth_max=2.7),
            mk(orbit[2].depth, base.KMAT, orbit[2].R, orbit[2].T, rgb=None, trunc=0.25),
            mk(small[1][0], KMAT2, small[1][1], small[1][2], rgb=rng.random((3, H2, W2), dtype=np.float32), trunc=0.2, depth_max=2.55),
            mk(orbit[4].depth, base.KMAT, orbit[4].R, orbit[4].T, rgb=orbit[4].rgb, trunc=0.1, depth_max=2.6)]


def e2e_cameras(device="cpu"):
    from envgs_amd import synth
    return [synth.orbit_camera(v, n_views=8, radius=3.0, H=96, W=96, fx=120.0, n=0.5, f=6.0, device=device) for v in range(8)]


def _e2e_views():
    """The eight cameras of the end-to-end test with the analytic depth of the sphere its surfels lie on: the fragile share is decided by where
    the voxels project, which the rendered maps share."""
    out = []
    for cam in e2e_cameras():
        K, R, T = cam.K.numpy(), cam.R.numpy(), cam.T.numpy().reshape(3)
        depth = sphere_depth(R, T, 96, 96, K, centre=(0.0, 0.0, 0.0))      # the surfel sphere is centred on the origin
        out.append(mo.make_view(depth, K, R, T, rgb=np.zeros((3, 96, 96), np.float32), trunc=trunc_of("ragged e2e")))
    return out


@functools.lru_cache(maxsize=None)
def view_set(kind):
    """The views of a row, built once and shared: treat as read-only."""
    return {"orbit": lambda: base._views(6), "inside": _inside_views, "mixed": _mixed_views, "e2e": _e2e_views}[kind]()


def oracle_conditions(name):
    """What `check_fused` needs of a configuration, from the oracle alone (no GPU)."""
    dims, voxel, origin, kind = INTEGRATION[name]
    nx, ny, nz = dims
    views = view_set(kind)
    one = np.ones((nz, ny, nx), np.float32)
    c0 = np.zeros((3, nz, ny, nx), np.float32)
    D32, W32, C32, _ = mo.integrate(one, 0 * one, c0, origin, voxel, views, 64.0, np.float32, trunc=trunc_of(name))
    D64, W64, C64, frag = mo.integrate(one, 0 * one, c0, origin, voxel, views, 64.0, np.float64, trunc=trunc_of(name))
    keep = ~frag
    return SimpleNamespace(n=frag.size, fragile=int(frag.sum()), share=float(frag.mean()), observed=int((W32 > 0).sum()),
                           unobserved=int((W32 == 0).sum()), disagree=int((W32[keep] != W64[keep]).sum()),
                           finite=bool(np.isfinite(D32).all() and np.isfinite(W32).all() and np.isfinite(C32).all()),
                           max_weight=float(W32.max()), min_tsdf=float(D32.min()))


# ---- extraction: name -> (tsdf (Nz,Ny,Nx), weight or None, origin, voxel, level, min_weight, euler or None) -------------------------------------------------
THIN = [(2, 2, 2), (3, 3, 3), (2, 2, 300), (300, 2, 2), (2, 300, 2), (257, 2, 2), (5, 51, 3)]
BIG = (81, 65, 51)                                              # 268 515 voxels: 1 049 workgroups of 256, past the 1 024 counters of one scan block
OFF_ORIGIN = (-1.17, 0.43, 2.01)


def _thin(dims):
    c = tuple(0.5 * (n - 1) + o for n, o in zip(dims, (-0.2, -0.25, -0.15)))     # off the middle: one corner of (2, 2, 2) lies inside
    return mo.sphere_volume(dims, c, 0.3 * max(dims))


def weights(dims, seed):
    """Weights in {0, 0.5, 1, 3}, mostly observed."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    return rng.choice(np.array([0.0, 0.5, 1.0, 3.0], np.float32), size=(nz, ny, nx), p=[0.04, 0.16, 0.4, 0.4])


@functools.lru_cache(maxsize=None)
def extraction(name):
    c = (6.37, 5.61, 4.83)
    E = lambda tsdf, weight=None, origin=(0.0, 0.0, 0.0), voxel=1.0, level=0.0, min_weight=1.0, euler=None: \
        SimpleNamespace(tsdf=tsdf, weight=weight, origin=origin, voxel=voxel, level=level, min_weight=min_weight, euler=euler)
    if name.startswith("thin "):
        return E(_thin(tuple(int(s) for s in name[5:].split("x"))))
    if name == "big":
        nx, ny, nz = BIG
        return E(0.05 * mo.sphere_volume(BIG, (0.49 * nx, 0.47 * ny, 0.52 * nz), 0.37 * min(BIG)), origin=OFF_ORIGIN, voxel=0.05, euler=2)
    if name == "plane on the level":                            # integer samples: every voxel of the plane i + j + k == 10 sits exactly on the level,
        X, Y, Z = mo.grid_points((9, 8, 7))                     # outside (the comparison is strict), the lower corner of 7 crossed edges: t == 0
        return E((10.0 - X - Y - Z).astype(np.float32), origin=OFF_ORIGIN, voxel=0.05)
    if name == "plane under the level":                         # the same plane from the other side: its voxels are the UPPER corners, t == 1
        X, Y, Z = mo.grid_points((9, 8, 7))
        return E((X + Y + Z - 10.0).astype(np.float32), origin=OFF_ORIGIN, voxel=0.05)
    if name == "torus on a sample":                             # the level is one of the field's own values, next to the surface of "level"
        t = mo.torus_volume((14, 12, 10), c, 3.1, 1.27)
        return E(t, origin=OFF_ORIGIN, voxel=0.05, level=float(t.reshape(-1)[np.argmin(np.abs(t - 0.35))]), euler=0)
    if name == "min_weight 0.75":
        return E(mo.sphere_volume((14, 12, 10), c, 3.217), weights((14, 12, 10), 3), min_weight=0.75)
    if name == "min_weight 0.5":                                # a weight exactly equal to min_weight counts as observed
        return E(mo.sphere_volume((14, 12, 10), c, 3.217), weights((14, 12, 10), 3), min_weight=0.5)
    if name == "last corner 13x11x9":                           # n % 4 == 3: the surface cuts the last cell, whose corners the tail lane of mesh_classify owns
        return E(mo.sphere_volume((13, 11, 9), (12.2, 10.1, 8.3), 1.9))
    raise KeyError(name)


EXTRACTION = ["thin %dx%dx%d" % d for d in THIN] + ["big", "plane on the level", "plane under the level", "torus on a sample", "min_weight 0.75", "min_weight 0.5", "last corner 13x11x9"]

