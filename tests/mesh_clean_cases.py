"""The meshes of tests/test_mesh_clean_cpu.py and tests/test_mesh_clean_gpu.py: hand-made ones with their answers written out, strips, crumbs and the
multi-object volume.  NumPy only; the expected values of the generated cases come from tests/mesh_clean_oracle.py."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import mesh_oracle as mo

I32 = np.int32


def _faces(rows):
    return np.asarray(rows, I32).reshape(-1, 3)


# name -> (V, faces, vertex_label, face_label, faces per component, vertices per component), typed in
HAND = {
    "one triangle": (3, _faces([[0, 1, 2]]), [0, 0, 0], [0], [1], [3]),
    "two triangles sharing one vertex": (5, _faces([[0, 1, 2], [2, 3, 4]]), [0, 0, 0, 0, 0], [0, 0], [2], [5]),
    # vertices 0 and 4 are named by nobody; the faces are listed against the component order
    "two disjoint triangles": (8, _faces([[5, 7, 6], [1, 2, 3]]), [-1, 0, 0, 0, -1, 1, 1, 1], [1, 0], [1, 1], [3, 3]),
    # (0,0,2) joins 0 and 2; (3,3,3) is a component of one vertex and one face
    "degenerate faces": (4, _faces([[0, 0, 2], [3, 3, 3]]), [0, -1, 0, 1], [0, 1], [1, 1], [2, 1]),
    # an index -1 and an index V: both faces ignored, so vertex 0 stays unreferenced and 1 is reached only through the third face
    "out of range": (4, _faces([[0, 1, -1], [1, 2, 4], [2, 3, 1]]), [-1, 0, 0, 0], [-1, -1, 0], [1], [3]),
    "no faces": (3, _faces([]), [-1, -1, -1], [], [], []),
}


def numbering(kind, n, seed=11):
    if kind == "identity":
        return np.arange(n, dtype=np.int64)
    if kind == "reversed":
        return np.arange(n, dtype=np.int64)[::-1].copy()
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


def strip(F, kind):
    """F triangles, face i = vertices (i, i+1, i+2) renamed by the numbering: one component.  Reversed is the adversarial numbering for the
    hooking: face i brings a vertex below every root so far, so every hook re-roots."""
    V = F + 2
    perm = numbering(kind, V)
    i = np.arange(F, dtype=np.int64)
    return V, perm[np.stack([i, i + 1, i + 2], axis=1)].astype(I32)


def crumbs(N):
    """N disjoint triangles (4i, 4i+1, 4i+3); vertex 4i+2 is named by nobody."""
    i = 4 * np.arange(N, dtype=np.int64)
    return 4 * N, np.stack([i, i + 1, i + 3], axis=1).astype(I32)


def random_mesh(V, F, seed):
    """Random triples over a sparse subset of the vertices: many components of many sizes, unreferenced vertices, some degenerate faces."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, V, size=(F, 3))
    near = rng.random(F) < 0.8                                  # most faces stay local, so that components do not all merge into one
    f[near, 1] = np.clip(f[near, 0] + rng.integers(-2, 3, size=near.sum()), 0, V - 1)
    f[near, 2] = np.clip(f[near, 0] + rng.integers(-2, 3, size=near.sum()), 0, V - 1)
    return f.astype(I32)


# ---- the multi-object volume ------------------------------------------------------------------------------------------------------------------------
# CONDITION: the objects are far enough apart that no cell crossed by one surface sees another object's distance (in the min over the objects,
# every corner of such a cell takes its value from that one object).  test_mesh_clean_cpu.test_multi_object_* checks it: if the shapes are
# changed, the equality of the cleaned mesh with the extraction of the kept-only volume is the check that they still are.
MULTI_DIMS = (48, 40, 36)
MULTI_SPHERES = [((9.37, 8.61, 8.83), 5.217), ((30.4, 9.3, 9.1), 3.31), ((41.2, 30.7, 9.6), 2.13), ((9.6, 30.2, 26.4), 1.37), ((42.3, 8.4, 28.7), 0.71)]
MULTI_TORUS = ((28.3, 27.6, 24.8), 6.1, 2.27)
MULTI_FACES = [3032, 1192, 496, 4928, 164, 24]                  # in label order
MULTI_SMALLEST = [0, 260, 786, 2366, 3724, 4914]
MULTI_EULER = [2, 2, 2, 0, 2, 2]                                # label 3 is the torus
# keep_largest -> the objects that stay: ("torus",) and indices into MULTI_SPHERES
MULTI_KEPT = {1: ("torus",), 2: ("torus", 0), 3: ("torus", 0, 1)}


def _object_volume(obj):
    if obj == "torus":
        return mo.torus_volume(MULTI_DIMS, *MULTI_TORUS)
    return mo.sphere_volume(MULTI_DIMS, *MULTI_SPHERES[obj])


@functools.lru_cache(maxsize=None)
def multi_colours():
    X, Y, Z = mo.grid_points(MULTI_DIMS)
    return np.stack([0.5 + 0.5 * np.sin(0.4 * X), 0.5 + 0.5 * np.cos(0.3 * Y), (X + Y + Z) / 124.0]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def multi_volume(objects=None):
    """-> namespace(tsdf, mesh: the oracle's extraction) of the min over `objects` (None: all six).  Computed once per object set; do not modify."""
    objs = ["torus"] + list(range(len(MULTI_SPHERES))) if objects is None else list(objects)
    tsdf = np.minimum.reduce([_object_volume(o) for o in objs])
    mesh = mo.marching_tetrahedra(tsdf, np.ones_like(tsdf), multi_colours(), (0.0, 0.0, 0.0), 1.0)
    return SimpleNamespace(tsdf=tsdf, mesh=mesh)
