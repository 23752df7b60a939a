"""The meshes of tests/test_mesh_simplify_cpu.py and tests/test_mesh_simplify_gpu.py: hand-made ones with their answers typed in, and the generators
of the cases that aim at one kernel path each.  NumPy only; the expected values of the generated cases come from tests/mesh_simplify_oracle.py."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import mesh_oracle as mo

F32, I32 = np.float32, np.int32
NAN = float("nan")


def _mesh(vertices, faces, colors=None, origin=(0.0, 0.0, 0.0), cell=1.0, dims=(1, 1, 1)):
    return SimpleNamespace(vertices=np.asarray(vertices, F32).reshape(-1, 3), faces=np.asarray(faces, I32).reshape(-1, 3),
                           colors=None if colors is None else np.asarray(colors, F32).reshape(-1, 3), origin=tuple(origin), cell=float(cell),
                           dims=tuple(dims))


# ---- hand-made: name -> (mesh, vertices', faces', colours' or None, vertex_cluster), typed in -------------------------------------------------------------
# four vertices over a 2 x 2 x 1 grid of unit cells: 0 in cell (0,0), 1 and 3 in cell (1,0), 2 in cell (0,1); cells 0, 1, 2 are clusters 0, 1, 2
_QUAD_V = [[0.1, 0.2, 0.7], [1.5, 0.25, 0.5], [0.3, 1.9, 0.1], [1.75, 0.75, 0.5]]
_QUAD_C = [[0.1, 0.2, 0.3], [0.25, 0.5, 1.0], [0.7, 0.8, 0.9], [0.75, 0.5, 0.0]]
_QUAD_F = [[0, 1, 2], [2, 1, 3]]
_TRI_V = [[0.1, 0.2, 0.7], [1.3, 0.6, 0.2], [0.3, 1.9, 0.1]]      # one vertex in each of the cells 0, 1, 2

HAND = {
    # the second face has two corners in cluster 1 and goes; the cluster's position is the mean of (1.5, .25, .5) and (1.75, .75, .5), its colour too
    "shared edge, one face left": (_mesh(_QUAD_V, _QUAD_F, _QUAD_C, dims=(2, 2, 1)),
                                   [[0.1, 0.2, 0.7], [1.625, 0.5, 0.5], [0.3, 1.9, 0.1]], [[0, 1, 2]],
                                   [[0.1, 0.2, 0.3], [0.5, 0.5, 0.5], [0.7, 0.8, 0.9]], [0, 1, 2, 1]),
    # one cell of edge 2 holds everything: both faces collapse, no face names the cluster, nothing is left
    "shared edge, nothing left": (_mesh(_QUAD_V, _QUAD_F, _QUAD_C, cell=2.0, dims=(1, 1, 1)), [], [], [], [-1, -1, -1, -1]),
    # singletons keep their position bit for bit: 0.1, 0.7, 1.3 are no multiples of 2^-20
    "a face and its rotations": (_mesh(_TRI_V, [[1, 2, 0], [0, 1, 2], [2, 0, 1]], dims=(2, 2, 1)), _TRI_V, [[1, 2, 0]], None, [0, 1, 2]),
    "a face and its reverse": (_mesh(_TRI_V, [[0, 1, 2], [0, 2, 1]], dims=(2, 2, 1)), _TRI_V, [[0, 1, 2], [0, 2, 1]], None, [0, 1, 2]),
    # vertex 3 has no cell: the face that names it goes, and so does cluster 3 = cell (1,1) of vertex 4, which only that face named
    "a NaN vertex": (_mesh(_TRI_V + [[1.5, NAN, 0.5], [1.5, 1.5, 0.5]], [[0, 1, 2], [1, 3, 4]], dims=(2, 2, 1)), _TRI_V, [[0, 1, 2]], None,
                     [0, 1, 2, -1, -1]),
    "indices -1 and V": (_mesh(_TRI_V, [[0, 1, -1], [0, 3, 2], [2, 0, 1]], dims=(2, 2, 1)), _TRI_V, [[2, 0, 1]], None, [0, 1, 2]),
    # x = 1 exactly is the lower face of cell 1 (offset 0); x = 2 exactly, the grid's upper bound, is clamped into cell 1 with offset 1: mean 1.5.
    # y = -3 lies below the grid: clamped into row 0 with offset 0.  The other two vertices are alone in cells (0,0) and (0,1).
    "cell boundary and upper bound": (_mesh([[1.0, 0.25, 0.5], [2.0, -3.0, 0.5], [0.5, 0.5, 0.5], [0.5, 1.5, 0.5]], [[0, 2, 3], [1, 3, 2]], dims=(2, 2, 1)),
                                      [[0.5, 0.5, 0.5], [1.5, 0.125, 0.5], [0.5, 1.5, 0.5]], [[1, 0, 2], [1, 2, 0]], None, [1, 1, 0, 2]),
}


# ---- renumbering -----------------------------------------------------------------------------------------------------------------------------------
def renumber(m, perm):
    """The same mesh with vertex v called perm[v]: rows moved, faces re-indexed (indices out of range are left alone)."""
    perm = np.asarray(perm, np.int64)
    V = m.vertices.shape[0]
    v = np.empty_like(m.vertices)
    v[perm] = m.vertices
    c = None
    if m.colors is not None:
        c = np.empty_like(m.colors)
        c[perm] = m.colors
    f = m.faces.astype(np.int64)
    ok = (f >= 0) & (f < V)
    g = f.copy()
    g[ok] = perm[f[ok]]
    return SimpleNamespace(vertices=v, faces=g.astype(I32), colors=c, origin=m.origin, cell=m.cell, dims=m.dims)


def numbering(kind, n, seed=11):
    if kind == "identity":
        return np.arange(n, dtype=np.int64)
    if kind == "reversed":
        return np.arange(n, dtype=np.int64)[::-1].copy()
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


def _colours(V, seed):
    return (np.random.default_rng(seed).random((V, 3)) * 1.2 - 0.1).astype(F32)      # some below 0, some above 1


# ---- the generated cases ---------------------------------------------------------------------------------------------------------------------------
def row(n):
    """n vertices along x, one per cell of a n x 1 x 1 grid, joined by a triangle strip: every vertex is its own cluster, cluster k = cell k.
    The rank scan sees n consecutive occupied cells."""
    rng = np.random.default_rng(n)
    v = np.stack([np.arange(n) + rng.uniform(0.05, 0.95, n), rng.uniform(0.05, 0.95, n), rng.uniform(0.05, 0.95, n)], axis=1)
    i = np.arange(max(n - 2, 0))
    return _mesh(v, np.stack([i, i + 1, i + 2], axis=1), _colours(n, n), dims=(n, 1, 1))


SPARSE_DIMS = (65, 65, 63)                                       # 266 175 cells = 1 040 workgroups of 256: past the 1 024 totals of one scan block


def sparse_grid():
    """About one cell in 150 of the 65 x 65 x 63 grid holds one or two vertices, the last cell among them; random faces over them."""
    nx, ny, nz = SPARSE_DIMS
    cells = nx * ny * nz
    rng = np.random.default_rng(7)
    occ = np.unique(np.concatenate([rng.choice(cells, cells // 150, replace=False), [0, 255, 256, 262143, 262144, cells - 1]]))
    lin = np.concatenate([occ, occ[::3]])
    rng.shuffle(lin)
    ijk = np.stack([lin % nx, (lin // nx) % ny, lin // (nx * ny)], axis=1)
    origin, cell = (-1.3, 0.7, 2.1), 0.25
    v = (np.asarray(origin) + (ijk + rng.uniform(0.1, 0.9, ijk.shape)) * cell)
    V = v.shape[0]
    f = rng.integers(0, V, size=(4000, 3))
    f[-1] = [int(np.nonzero(lin == cells - 1)[0][0]), int(np.nonzero(lin == 0)[0][0]), int(np.nonzero(lin == 262144)[0][0])]
    return _mesh(v, f, _colours(V, 8), origin=origin, cell=cell, dims=SPARSE_DIMS)


def giant(n=70000, singletons=True):
    """n vertices inside cell (0,0,0); with singletons, three more, alone in their cells, that form the one surviving face."""
    rng = np.random.default_rng(n)
    v = rng.uniform(0.0, 1.0, (n, 3))
    f = rng.integers(0, n, size=(500, 3))                         # all collapse
    c = _colours(n + 3, 5)
    if not singletons:
        return _mesh(v, f, c[:n], dims=(1, 1, 1))
    v = np.concatenate([v, [[1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 0.5]]])
    f = np.concatenate([f[:250], [[n, n + 2, n + 1]], f[250:], [[0, n, n + 1]]])       # the last one keeps the giant cluster alive too
    return _mesh(v, f, c, dims=(2, 2, 1))


RUNS = (1, 2, 63, 64, 65, 300, 1, 64, 2)                         # members per cell, consecutive in the identity numbering


def runs():
    """Cells along x holding RUNS consecutive vertices each (the runs start at every lane offset and straddle wavefronts and workgroups), and a
    triangle strip over the first vertex of each run and random faces between runs."""
    rng = np.random.default_rng(12)
    cell_of = np.repeat(np.arange(len(RUNS)), RUNS)
    V = cell_of.size
    origin, cell = (0.37, -1.21, 5.3), 0.173
    v = np.asarray(origin) + np.stack([cell_of + rng.uniform(0, 1, V), rng.uniform(0, 1, V), rng.uniform(0, 1, V)], axis=1) * cell
    first = np.concatenate([[0], np.cumsum(RUNS)[:-1]])
    i = np.arange(len(RUNS) - 2)
    f = np.concatenate([np.stack([first[i], first[i + 1], first[i + 2]], axis=1), rng.integers(0, V, size=(600, 3))])
    return _mesh(v, f, _colours(V, 13) * 200.0, origin=origin, cell=cell, dims=(len(RUNS), 1, 1))


def spread(n=500):
    """n vertices at least 0.02 apart on a jittered lattice; a cell of 0.01 holds at most one: every vertex is a singleton."""
    rng = np.random.default_rng(21)
    side = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    v = (g * 0.03 + rng.uniform(0, 0.01, (n, 3))).astype(F32)
    v = v[rng.permutation(n)]
    f = rng.integers(0, n, size=(2 * n, 3))
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
    odd = np.array([0x7fc12345, 0x80000000, 0x00000001, 0xff800000], np.uint32).view(F32)      # a NaN payload, -0.0, a denormal, -inf: copied, not computed
    c = _colours(n, 22)
    c[:4, 0] = odd
    return _mesh(v, f, c, cell=0.01)


def colour_range():
    """Two vertices per cell; the colours of each pair come from 0, 1, 255, 300, -1, NaN, +inf and ordinary values.  The last pair sits on the
    grid's upper bound and beyond it."""
    special = np.array([0.0, 1.0, 255.0, 300.0, -1.0, NAN, np.inf, 0.3, 254.99999, 1e-6, 0.5 - 2.0 ** -18], F32)
    n = special.size
    v = np.stack([np.repeat(np.arange(n), 2) + np.tile([0.25, 0.5], n), np.full(2 * n, 0.5), np.full(2 * n, 0.5)], axis=1)
    v[-2] = [float(n), 1.0, 1.0]                                  # exactly the upper bound on every axis
    v[-1] = [n + 7.5, 3.0, 1e30]                                  # beyond it
    c = np.stack([np.repeat(special, 2), np.tile(special, 2), np.roll(np.repeat(special, 2), 3)], axis=1)
    i = np.arange(n - 2)
    f = np.stack([2 * i, 2 * i + 3, 2 * i + 4], axis=1)
    return _mesh(v, f, c, dims=(n, 1, 1))


def face_rules(V=40):
    """V singletons along x and two extra vertices (one shares cell 0, one is NaN); faces: good ones, ones that collapse after mapping, ones with
    the indices -1, V and 2^31 - 1, and ones that name the NaN vertex."""
    v = np.stack([np.arange(V) + 0.5, np.full(V, 0.5), np.full(V, 0.5)], axis=1)
    v = np.concatenate([v, [[0.25, 0.25, 0.25], [3.5, NAN, 0.5]]])
    twin, nan = V, V + 1
    W = V + 2
    f = [[0, 1, 2], [twin, 0, 5], [0, twin, twin], [3, 4, -1], [W, 4, 5], [2 ** 31 - 1, 1, 2], [nan, 6, 7], [6, 7, 8], [8, 6, 7], [twin, 1, 2], [7, 6, 8],
         [9, 9, 10], [-2 ** 31, 3, 4], [10, 11, nan], [5, 6, 7]]
    return _mesh(v, f, _colours(W, 31), dims=(V, 1, 1))


def rotations(copies=4096):
    """`copies` times one triangle over three singletons, in its three rotations, and its reverse likewise: two faces survive, those of index 0
    and of the first reversed one."""
    rng = np.random.default_rng(41)
    base = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]])
    f = base[rng.integers(0, 6, copies)]
    return _mesh(_TRI_V, f, dims=(2, 2, 1))


def duplicates(unique=75000, side=48, seed=43):
    """4 x `unique` faces over side^3 singleton vertices: every face occurs four times (in random rotations), scattered through the array."""
    rng = np.random.default_rng(seed)
    V = side ** 3
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    v = g + rng.uniform(0.1, 0.9, g.shape)
    a = rng.integers(0, V, unique)
    f = np.stack([a, (a + rng.integers(1, 50, unique)) % V, (a + rng.integers(50, 99, unique)) % V], axis=1)
    f = np.concatenate([np.roll(f, int(k), axis=1) if k else f for k in (0, 1, 2, 1)])
    rot = rng.integers(0, 3, f.shape[0])
    f = np.stack([f[np.arange(f.shape[0]), (rot + e) % 3] for e in range(3)], axis=1)
    return _mesh(v, f[rng.permutation(f.shape[0])], dims=(side, side, side))


# ---- the analytic sphere ---------------------------------------------------------------------------------------------------------------------------
# the shapes and grids of tests/mesh_cases.py INTEGRATION "40x36x32" and "37x35x33", here with an analytic distance field: centre and radius in voxels
SPHERES = {
    "40x36x32": ((40, 36, 32), 0.05, (-1.0131, -0.8873, -0.7919), (19.37, 17.61, 15.83), 11.217),
    "37x35x33": ((37, 35, 33), 0.05, (-0.9131, -0.8873, -0.7919), (18.21, 17.33, 16.47), 12.613),
}


def _sphere_colours(dims):
    X, Y, Z = mo.grid_points(dims)
    return np.stack([0.5 + 0.5 * np.sin(0.4 * X + 0.2 * Y), 0.5 + 0.5 * np.cos(0.3 * Y - 0.5 * Z), (X + Y + Z) / sum(dims)]).astype(F32)


@functools.lru_cache(maxsize=None)
def sphere(name):
    """-> namespace(tsdf, rgb, origin, voxel, centre, radius (world), mesh: the oracle's extraction).  Computed once; do not modify."""
    dims, voxel, origin, c, r = SPHERES[name]
    tsdf = mo.sphere_volume(dims, c, r)
    rgb = _sphere_colours(dims)
    m = mo.marching_tetrahedra(tsdf, np.ones_like(tsdf), rgb, origin, voxel)
    centre = tuple(o + voxel * x for o, x in zip(origin, c))
    return SimpleNamespace(tsdf=tsdf, rgb=rgb, origin=origin, voxel=voxel, dims=dims, centre=centre, radius=voxel * r, mesh=m)
