"""The inputs of the mesh evaluation tests in one table: tests/test_mesh_eval_cpu.py checks on the oracle alone that every seeded sampling case
is one the oracle itself passes (its total is near the expected one, its samples lie in their faces), tests/test_mesh_eval_gpu.py runs them on
the device.  Built once and shared: treat as read-only."""
import functools
from types import SimpleNamespace

import numpy as np

F32 = np.float32
SEED = 0


def _case(vertices, faces, density, colors=None, seed=SEED):
    return SimpleNamespace(vertices=np.asarray(vertices, F32).reshape(-1, 3), faces=np.asarray(faces, np.int32).reshape(-1, 3), density=float(density),
                           colors=None if colors is None else np.asarray(colors, F32).reshape(-1, 3), seed=seed)


_TRI = [[0, 0, 0], [2, 0, 0], [0, 2, 0]]                          # area 2
# name -> (case, the counts per face at SEED, written out).  area * density is a whole number in every sampled face, so the rounding draw changes
# nothing unless it is within 2^-20 of 1; tests/test_mesh_eval_cpu.py confirms the written counts on the oracle.
HAND = {
    "one right triangle": (_case(_TRI, [[0, 1, 2]], 8.0, colors=[[1, 0, 0], [0, 1, 0], [0, 0, 1]]), [16]),
    "a quad": (_case([[0, 0, 1], [2, 0, 1], [2, 2, 1], [0, 2, 1]], [[0, 1, 2], [0, 2, 3]], 4.0), [8, 8]),
    "a zero-area face": (_case(_TRI + [[1, 0, 0]], [[0, 3, 1], [0, 1, 1], [0, 1, 2]], 8.0), [0, 0, 16]),
    "indices -1 and V": (_case(_TRI, [[0, 1, 2], [-1, 1, 2], [0, 3, 2], [2, 0, 1]], 8.0, colors=np.eye(3)), [16, 0, 0, 16]),
    "a NaN vertex": (_case(_TRI + [[np.nan, 1, 1], [np.inf, 0, 0]], [[0, 1, 3], [0, 1, 2], [4, 1, 2]], 8.0), [0, 16, 0]),
}


@functools.lru_cache(maxsize=None)
def giant():
    """One face of area 50 among 999 of area 2.5e-4, at density 2000: 100 000 samples against 0 or 1 each."""
    rng = np.random.default_rng(21)
    F = 1000
    base = rng.uniform(-3, 3, (F, 3))
    v = np.stack([base, base + [0.0223607, 0, 0], base + [0, 0.0223607, 0]], axis=1)      # legs sqrt(5e-4)
    v[500] = [[-5, -5, 0.5], [5, -5, 0.5], [-5, 5, 0.5]]
    faces = np.arange(3 * F).reshape(F, 3)
    return _case(v.reshape(-1, 3), faces, 2000.0, colors=rng.random((3 * F, 3)), seed=7)


MANY_F = 256 * 1049 + 3                                           # more than 1 024 workgroup totals, as the `big` row of tests/mesh_cases.py


@functools.lru_cache(maxsize=None)
def many():
    """MANY_F tiny faces with areas from 0 to 1.2e-3 at density 1000: 0, 1 or 2 samples each."""
    rng = np.random.default_rng(22)
    base = rng.uniform(-1, 1, (MANY_F, 3))
    leg = np.sqrt(2.4e-3 * rng.random((MANY_F, 1)))
    v = np.stack([base, base + leg * [1.0, 0, 0], base + leg * [0, 0.6, 0.8]], axis=1)
    return _case(v.reshape(-1, 3), np.arange(3 * MANY_F).reshape(MANY_F, 3), 1000.0, colors=rng.random((3 * MANY_F, 3)), seed=3)


@functools.lru_cache(maxsize=None)
def soup():
    """An indexed mesh with shared vertices, a few bad faces among good ones, random colours: 3 000 faces over 700 vertices."""
    rng = np.random.default_rng(23)
    v = rng.uniform(-1, 1, (700, 3))
    v[13] = np.nan
    f = rng.integers(0, 700, (3000, 3))
    f[5] = [-1, 3, 4]
    f[77] = [1, 700, 2]
    f[100] = [9, 9, 10]
    return _case(v, f, 3.0, colors=rng.random((700, 3)), seed=0xFFFFFFFF)


SEEDED = {"giant": giant, "many": many, "soup": soup}             # every case whose counts are not written out


# ---- nearest ------------------------------------------------------------------------------------------------------------------------------------------
L = 6                                                             # the lattice: L^3 points at whole coordinates 0 .. L-1, cell 1: points ON cell walls


@functools.lru_cache(maxsize=None)
def lattice():
    g = np.arange(L, dtype=F32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1].copy()      # x fastest


@functools.lru_cache(maxsize=None)
def lattice_queries():
    rng = np.random.default_rng(31)
    p = lattice()
    walls = p[rng.integers(0, p.shape[0], 60)] + rng.choice([0.0, 0.25, 0.5], (60, 3)).astype(F32) * [0, 1, 1]      # x on a wall, y and z anywhere
    mids = np.concatenate([p[rng.integers(0, p.shape[0], 40)] + np.asarray(o, F32) for o in ([0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0.5])])
    c = np.array([[x, y, z] for x in (0, L - 1) for y in (0, L - 1) for z in (0, L - 1)], F32)
    corners = np.concatenate([c, c + (c > 0) * 0.5 - (c == 0) * 0.5])
    far = np.array([[-1000, 2, 2], [1000 + L, 2.5, 2], [2, -1000, 3], [2, 1000 + L, 3.5], [1, 1, -1000], [1.5, 1, 1000 + L], [-1000, -1000, -1000],
                    [1000 + L, 1000 + L, 1000 + L]], F32)
    edge = np.array([[-1, 2, 2], [2, 2, -1], [L, 3, 3], [-3, -4, 2], [2, L + 2, L + 3], [-1, -1, 2]], F32)      # d2 exactly 1, 1, 1, 25, 25, 2
    return np.concatenate([walls, mids, corners, far, edge]).astype(F32)


@functools.lru_cache(maxsize=None)
def cloud():
    rng = np.random.default_rng(32)
    return SimpleNamespace(points=rng.random((5000, 3), dtype=F32), queries=rng.random((3000, 3), dtype=F32) * F32(1.1) - F32(0.05), max_distance=0.05)


@functools.lru_cache(maxsize=None)
def offset_cloud():
    rng = np.random.default_rng(33)
    return SimpleNamespace(points=(1000 + 0.5 * rng.random((2000, 3))).astype(F32), queries=(1000 + 0.5 * rng.random((500, 3))).astype(F32),
                           max_distance=0.05, cell_size=0.01)


def with_specials(a, seed):
    """A copy with NaN, +inf and -inf planted in a few rows."""
    rng = np.random.default_rng(seed)
    a = a.copy()
    rows = rng.choice(a.shape[0], 9, replace=False)
    for r, (col, val) in zip(rows, [(0, np.nan), (1, np.nan), (2, np.nan), (0, np.inf), (1, np.inf), (2, np.inf), (0, -np.inf), (1, -np.inf), (2, -np.inf)]):
        a[r, col] = val
    return a
