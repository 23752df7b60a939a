"""Independent NumPy restatement of the mesh simplification semantics (include/envgs_mesh.h, "simplification of an indexed triangle mesh"; DESIGN.md
"Mesh simplification").  PARITY UNPINNED like the rest of the module: this file, written from the header's text and not from the kernels, is what
csrc/mesh_simplify.hip and the host build of csrc/mesh_facehash.h are checked against.  Nothing here is imported from the product.

  grid_of(vertices, cell, origin)        the grid the Python wrapper documents: origin and dims
  vertex_cells(vertices, origin, cell, dims)     rule 1: (i, j, k), linear cell index (-1: no cell), u
  dedup_faces(mapped, candidate)         rule 4, last clause: the lowest face index of every oriented triple up to rotation
  simplify(...)                          rules 1-5
"""
import math
from types import SimpleNamespace

import numpy as np

F32 = np.float32
POS_BITS, COL_BITS = 20, 16


def grid_of(vertices, cell, origin=None):
    """-> (origin, dims): origin None = per-axis minimum of the finite vertices; dims = floor((max - origin) / cell) + 1 >= 1, in double."""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    fin = v[np.isfinite(v).all(axis=1)].astype(np.float64)
    lo = fin.min(axis=0) if fin.shape[0] else np.zeros(3)
    hi = fin.max(axis=0) if fin.shape[0] else np.zeros(3)
    if origin is not None:
        lo = np.asarray(origin, np.float64)
    dims = tuple(max(1, int(math.floor((h - l) / float(cell))) + 1) if h > l else 1 for l, h in zip(lo, hi))
    return tuple(float(x) for x in lo), dims


def vertex_cells(vertices, origin, cell, dims):
    """Rule 1.  -> ijk (V,3) int64, lin (V,) int64 with -1 for a vertex that has a non-finite coordinate, u (V,3) float32."""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    o = np.asarray(origin, F32)
    with np.errstate(all="ignore"):
        u = ((v - o[None, :]) / F32(cell)).astype(F32)            # fp32 subtract, fp32 IEEE divide
        fl = np.floor(u)
    ijk = np.zeros(v.shape, np.int64)
    for a in range(3):
        n = int(dims[a])
        col = fl[:, a]
        small = ~(col >= 1.0)                                     # decided on the float: NaN lands here too, but such a vertex has no cell anyway
        huge = col >= 2147483648.0
        mid = ~small & ~huge
        ijk[huge, a] = n - 1
        ijk[mid, a] = np.minimum(col[mid].astype(np.int64), n - 1)
    lin = ijk[:, 0] + dims[0] * (ijk[:, 1] + dims[1] * ijk[:, 2])
    lin[~np.isfinite(v).all(axis=1)] = -1
    return ijk, lin, u


def _fixed(values, one):
    """q = (uint32) floor(value * one + 0.5), in fp32."""
    return np.floor((values.astype(F32) * F32(one)).astype(F32) + F32(0.5)).astype(np.int64)


def _rounded_mean(total, n):
    return (2 * total + n) // (2 * n)


def dedup_faces(mapped, candidate):
    """(F,) bool: candidate and no candidate of lower index has the same oriented triple up to cyclic rotation.  A plain walk in face order."""
    seen = set()
    out = np.zeros(len(mapped), bool)
    for f, (a, b, c) in enumerate(np.asarray(mapped, np.int64).reshape(-1, 3).tolist()):
        if not candidate[f]:
            continue
        key = min((a, b, c), (b, c, a), (c, a, b))
        if key not in seen:
            seen.add(key)
            out[f] = True
    return out


def simplify(vertices, faces, colors, origin, cell, dims):
    """-> namespace(vertices (V',3) f32, faces (F',3) i32, colors (V',3) f32 or None, vertex_cluster (V,) i32: new index of each input vertex or
    -1, cluster (V,) i32: cluster number before the selection, mapped (F,3) i32, keep (F,) bool, count: C, cl_vertices, cl_colors: (C,3))"""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    V = v.shape[0]
    col = None if colors is None else np.asarray(colors, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ijk, lin, u = vertex_cells(v, origin, cell, dims)
    has = lin >= 0

    # 2. clusters = occupied cells by ascending linear index
    occupied = np.unique(lin[has])
    C = occupied.size
    cluster = np.full(V, -1, np.int64)
    cluster[has] = np.searchsorted(occupied, lin[has])

    # 3. representatives
    cl_v = np.zeros((C, 3), F32)
    cl_c = None if col is None else np.zeros((C, 3), F32)
    with np.errstate(all="ignore"):
        frac = (u - ijk.astype(F32)).astype(F32)
    frac = np.where(frac > 0, np.where(frac > 1, F32(1), frac), F32(0)).astype(F32)
    qpos = _fixed(np.where(has[:, None], frac, F32(0)), 2 ** POS_BITS)
    if col is not None:
        cc = np.where(col > 0, np.where(col > 255, F32(255), col), F32(0)).astype(F32)
        qcol = _fixed(cc, 2 ** COL_BITS)
    members = np.bincount(cluster[has], minlength=C).astype(np.int64)
    n3 = members[:, None]
    o32, cell32 = np.asarray(origin, F32), F32(cell)
    cell_ijk = np.stack([occupied % dims[0], (occupied // dims[0]) % dims[1], occupied // (dims[0] * dims[1])], axis=1)
    total = np.zeros((C, 3), np.int64)
    np.add.at(total, cluster[has], qpos[has])                    # integer sums: the order of the adds cannot matter
    qm = _rounded_mean(total, n3)
    inside = (cell_ijk.astype(F32) + (qm.astype(F32) * F32(2.0 ** -POS_BITS)).astype(F32)).astype(F32)
    cl_v[:] = (o32[None, :] + (inside * cell32).astype(F32)).astype(F32)
    if col is not None:
        total = np.zeros((C, 3), np.int64)
        np.add.at(total, cluster[has], qcol[has])
        cl_c[:] = (_rounded_mean(total, n3).astype(F32) * F32(2.0 ** -COL_BITS)).astype(F32)
    first = np.full(C, V, np.int64)
    np.minimum.at(first, cluster[has], np.nonzero(has)[0])
    single = members == 1                                         # a cell of one vertex keeps it bit for bit
    cl_v[single] = v[first[single]]
    if col is not None:
        cl_c[single] = col[first[single]]

    # 4. faces
    in_range = ((f >= 0) & (f < V)).all(axis=1)
    corner_ok = (f >= 0) & (f < V)
    mapped = np.full(f.shape, -1, np.int64)
    mapped[corner_ok] = cluster[f[corner_ok]]
    cand = in_range & (mapped >= 0).all(axis=1)
    cand &= (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 2] != mapped[:, 0])
    keep = dedup_faces(mapped, cand)

    # 5. the clusters a surviving face names, ascending; faces re-indexed
    g = mapped[keep]
    used = np.zeros(C, bool)
    used[g.reshape(-1)] = True
    new = np.cumsum(used) - 1
    new_of_cluster = np.where(used, new, -1)
    vertex_cluster = np.full(V, -1, np.int64)
    vertex_cluster[has] = new_of_cluster[cluster[has]]
    return SimpleNamespace(vertices=cl_v[used], faces=new[g].astype(np.int32).reshape(-1, 3), colors=None if cl_c is None else cl_c[used],
                           vertex_cluster=vertex_cluster.astype(np.int32), cluster=cluster.astype(np.int32), mapped=mapped.astype(np.int32),
                           keep=keep, count=C, cl_vertices=cl_v, cl_colors=cl_c)
