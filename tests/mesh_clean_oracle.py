"""Independent NumPy / SciPy restatement of the mesh clean-up semantics (include/envgs_mesh.h, "clean-up of an indexed triangle mesh"; DESIGN.md
"Mesh extraction").  PARITY UNPINNED like the rest of the module: this file, not a recorded fixture, is what csrc/mesh_clean.hip and the host build of
csrc/mesh_unionfind.h are checked against.  Nothing here is imported from the product.

  components(V, faces)        labels and per-component counts
  select_faces(...)           the surviving vertices / colours / faces, in their old relative order
  clean_keep(counts, ...)     which components the clean() rule keeps
"""
from types import SimpleNamespace

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def valid_faces(V, faces):
    """(F,) bool: all three indices in [0, V).  Every other face is ignored throughout."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def components(V, faces):
    """Faces are connected iff they share a vertex index.  -> namespace(count, vertex_label (V,), face_label (F,), faces (C,), vertices (C,),
    smallest (C,): the smallest vertex index of each component); components numbered by ascending smallest vertex; -1 = unreferenced / ignored."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(V, f)
    g = f[ok]
    vertex_label = np.full(V, -1, np.int64)
    face_label = np.full(f.shape[0], -1, np.int64)
    if g.shape[0]:
        rows = np.concatenate([g[:, 0], g[:, 1]])
        cols = np.concatenate([g[:, 1], g[:, 2]])
        graph = coo_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(V, V))
        _, raw = connected_components(graph, directed=False)    # gives every unreferenced vertex a label of its own
        referenced = np.zeros(V, bool)
        referenced[g.reshape(-1)] = True
        ref_idx = np.nonzero(referenced)[0]                      # ascending vertex index
        # renumber by smallest vertex: the first time a raw label appears while walking the referenced vertices upwards
        uniq, first = np.unique(raw[ref_idx], return_index=True)
        order = np.argsort(first, kind="stable")
        new_of_uniq = np.empty(uniq.size, np.int64)
        new_of_uniq[order] = np.arange(uniq.size)
        vertex_label[ref_idx] = new_of_uniq[np.searchsorted(uniq, raw[ref_idx])]
        face_label[ok] = vertex_label[g[:, 0]]
    C = int(vertex_label.max()) + 1 if V else 0
    lab_v = vertex_label[vertex_label >= 0]
    lab_f = face_label[face_label >= 0]
    smallest = np.full(C, V, np.int64)
    np.minimum.at(smallest, lab_v, np.nonzero(vertex_label >= 0)[0])
    return SimpleNamespace(count=C, vertex_label=vertex_label.astype(np.int32), face_label=face_label.astype(np.int32),
                           faces=np.bincount(lab_f, minlength=C).astype(np.int32), vertices=np.bincount(lab_v, minlength=C).astype(np.int32),
                           smallest=smallest)


def components_plain(V, faces):
    """The same labelling by a plain sequential union-find (no SciPy): the oracle's own cross-check."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(V, f)
    used = [False] * V
    for a, b, c in f[ok].tolist():
        used[a] = used[b] = used[c] = True
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    label_of_root, vertex_label = {}, np.full(V, -1, np.int32)
    for v in range(V):
        if used[v]:
            vertex_label[v] = label_of_root.setdefault(find(v), len(label_of_root))
    face_label = np.full(f.shape[0], -1, np.int32)
    face_label[ok] = vertex_label[f[ok][:, 0]]
    return vertex_label, face_label


def select_faces(vertices, faces, colors, keep):
    """A face survives iff keep != 0 and its indices are in range; a vertex iff a surviving face names it; both keep their order.
    -> namespace(vertices, faces (int32, re-indexed), colors or None, vertex_index (V',): old index of each new vertex)"""
    vertices = np.asarray(vertices)
    V = vertices.shape[0]
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    sel = (np.asarray(keep).reshape(-1) != 0) & valid_faces(V, f)
    g = f[sel]
    used = np.zeros(V, bool)
    used[g.reshape(-1)] = True
    new = np.cumsum(used) - 1
    idx = np.nonzero(used)[0]
    return SimpleNamespace(vertices=vertices[idx], faces=new[g].astype(np.int32).reshape(-1, 3), colors=None if colors is None else np.asarray(colors)[idx],
                           vertex_index=idx.astype(np.int32))


def clean_keep(comp_faces, keep_largest=50, min_faces=50):
    """(C,) bool: kept iff face count >= max(min_faces, count of the keep_largest-th largest component); the second term is 0 when keep_largest
    is None, 0 or >= C.  Ties at the threshold are all kept."""
    n = np.asarray(comp_faces, np.int64)
    nth = 0
    if keep_largest is not None and 0 < keep_largest < n.size:
        nth = int(np.sort(n)[::-1][keep_largest - 1])
    return n >= max(int(min_faces), nth)


def clean(vertices, faces, colors, keep_largest=50, min_faces=50):
    comp = components(np.asarray(vertices).shape[0], faces)
    kept = np.concatenate([clean_keep(comp.faces, keep_largest, min_faces), [False]])
    return select_faces(vertices, faces, colors, kept[comp.face_label])
