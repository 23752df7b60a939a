"""The inputs of the thinning tests in one place: tests/test_mesh_thin_cpu.py checks the oracle and its round model on them, tests/test_mesh_thin_gpu.py
runs the device on them.  Built once and shared: treat as read-only."""
import functools
import math

import numpy as np

F32 = np.float32


def cube_radius(n, neighbours):
    """The radius at which n uniform points of the unit cube have about `neighbours` others within it."""
    return float((neighbours / (n * 4.0 / 3.0 * math.pi)) ** (1.0 / 3.0))


def sheet_radius(n, neighbours):
    return float(math.sqrt(neighbours / (n * math.pi)))


@functools.lru_cache(maxsize=None)
def cube(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=F32)


@functools.lru_cache(maxsize=None)
def sheet(n, seed):
    p = np.random.default_rng(seed).random((n, 3), dtype=F32)
    p[:, 2] = F32(0.25) + F32(0.1) * p[:, 0]                     # a tilted plane
    return p


COLLINEAR_N, COLLINEAR_RADIUS = 600, 1.0


@functools.lru_cache(maxsize=None)
def collinear():
    """600 points spaced 0.59 radii along x: each has one neighbour on either side, so index order decides one point per round."""
    p = np.zeros((COLLINEAR_N, 3), F32)
    p[:, 0] = (np.arange(COLLINEAR_N) * 0.59).astype(F32)
    return p


# name -> (points, radius): the prototype inputs of the round scheme
PROTOTYPE = {
    "cube, 6 neighbours": lambda: (cube(4000, 61), cube_radius(4000, 6)),
    "cube, 50 neighbours": lambda: (cube(4000, 62), cube_radius(4000, 50)),
    "sheet, 5 neighbours": lambda: (sheet(4000, 63), sheet_radius(4000, 5)),
    "sheet, 30 neighbours": lambda: (sheet(4000, 64), sheet_radius(4000, 30)),
    "collinear": lambda: (collinear(), COLLINEAR_RADIUS),
}

LATTICE_L = 12


@functools.lru_cache(maxsize=None)
def lattice():
    """12^3 points at whole coordinates: every d2 is exact, and with cell 1 every point lies on a cell wall."""
    g = np.arange(LATTICE_L, dtype=F32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1].copy()


@functools.lru_cache(maxsize=None)
def duplicates():
    """50 positions x 20 exact copies in shuffled order, with 9 rows that are not finite mixed in.  -> (points, position of each row or -1)"""
    rng = np.random.default_rng(71)
    pos = rng.random((50, 3), dtype=F32)
    which = np.repeat(np.arange(50), 20)
    specials = np.array([[np.nan, 0.5, 0.5], [0.5, np.nan, 0.5], [0.5, 0.5, np.nan], [np.inf, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, np.inf],
                         [-np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], [0.5, 0.5, -np.inf]], F32)
    points = np.concatenate([pos[which], specials])
    which = np.concatenate([which, np.full(9, -1)])
    order = rng.permutation(points.shape[0])
    return points[order], which[order]


@functools.lru_cache(maxsize=None)
def cluster():
    """3 000 points within radius / 2 of one centre, radius 0.1: every pair is within the radius."""
    rng = np.random.default_rng(72)
    d = rng.normal(size=(3000, 3))
    d *= (0.049 * rng.random((3000, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray([0.3, -0.2, 1.1]) + d).astype(F32)


@functools.lru_cache(maxsize=None)
def offset_cloud():
    """Coordinates near 1 000, radius 0.01: the spacing of fp32 there is 6e-5."""
    return (1000 + 0.2 * np.random.default_rng(73).random((3000, 3))).astype(F32)


@functools.lru_cache(maxsize=None)
def torus(n, seed=74):
    """About n area-uniform points on a torus (ring 1, tube 0.4) and their mean spacing sqrt(area / n)."""
    rng = np.random.default_rng(seed)
    out = []
    while sum(len(o) for o in out) < n:                          # rejection: the area element is proportional to ring + tube cos(phi)
        theta, phi, u = rng.random(n) * 2 * math.pi, rng.random(n) * 2 * math.pi, rng.random(n)
        ok = u * 1.4 <= 1.0 + 0.4 * np.cos(phi)
        theta, phi = theta[ok], phi[ok]
        out.append(np.stack([(1.0 + 0.4 * np.cos(phi)) * np.cos(theta), (1.0 + 0.4 * np.cos(phi)) * np.sin(theta), 0.4 * np.sin(phi)], axis=1))
    p = np.concatenate(out)[:n].astype(F32)
    return p, float(math.sqrt(4 * math.pi ** 2 * 1.0 * 0.4 / n))
