"""Independent NumPy restatement of the mesh-extraction semantics (include/envgs_mesh.h; DESIGN.md "Mesh extraction").  PARITY UNPINNED: the
reference's fuser cannot run and its marching step lives in libraries outside it, so this file -- not a recorded fixture -- is what the HIP kernels are
checked against.  Nothing here is imported from the product: the marching-tetrahedra case table is derived below from the geometry of the unit cell.

  integrate(...)            TSDF fusion in the canonical order, in float32 (the statement the kernel must equal) or float64 (the shadow that lists
                            the voxels whose decisions are fragile)
  integrate_voxel(...)      the same for ONE voxel with chosen decisions flipped: what a fragile voxel may legitimately be instead
  marching_tetrahedra(...)  vertices / colours / faces in the canonical order
  mesh_topology(...)        closedness, orientation and Euler characteristic of a face list
"""
import itertools
from types import SimpleNamespace

import numpy as np

SLOT_DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


def make_view(depth, K, R, T, rgb=None, depth_max=np.inf, trunc=None):
    return SimpleNamespace(depth=np.asarray(depth, np.float32), rgb=None if rgb is None else np.asarray(rgb, np.float32),
                           fx=np.float32(K[0][0]), fy=np.float32(K[1][1]), cx=np.float32(K[0][2]), cy=np.float32(K[1][2]),
                           R=np.asarray(R, np.float32).reshape(3, 3), T=np.asarray(T, np.float32).reshape(3), depth_max=np.float32(depth_max),
                           trunc=None if trunc is None else np.float32(trunc))


def voxel_positions(dims, origin, voxel, dt):
    nx, ny, nz = dims
    f = lambda n, o: dt(o) + np.arange(n).astype(dt) * dt(voxel)
    x, y, z = f(nx, origin[0]), f(ny, origin[1]), f(nz, origin[2])
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return X, Y, Z


def _project(view, X, Y, Z, dt):
    R, T = view.R.astype(dt), view.T.astype(dt)
    xc = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z + T[0]
    yc = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z + T[1]
    zc = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + T[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = dt(view.fx) * (xc / zc) + dt(view.cx)
        v = dt(view.fy) * (yc / zc) + dt(view.cy)
    return u, v, zc


def integrate(tsdf, weight, rgb, origin, voxel, views, w_max=64.0, dtype=np.float32, trunc=None):
    """tsdf, weight (Nz,Ny,Nx), rgb (3,Nz,Ny,Nx) or None: NOT modified.  Returns (tsdf, weight, rgb, fragile): the fused planes in `dtype` and
    the boolean plane of voxels for which some view has u or v within 1e-4 of an integer, or sdf within 1e-5 trunc of -trunc (meaningful from the
    float64 run)."""
    dt = dtype
    D, Wt = tsdf.astype(dt), weight.astype(dt)
    C = None if rgb is None else rgb.astype(dt)
    nz, ny, nx = D.shape
    X, Y, Z = voxel_positions((nx, ny, nz), origin, voxel, dt)
    fragile = np.zeros(D.shape, bool)
    for view in views:
        tr = dt(view.trunc if view.trunc is not None else trunc)
        H, W = view.depth.shape
        u, v, zc = _project(view, X, Y, Z, dt)
        front = zc > 0
        with np.errstate(invalid="ignore"):
            fu, fv = np.floor(u), np.floor(v)
            inside = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            near_image = front & (u > -1) & (u < W + 1) & (v > -1) & (v < H + 1)
            fragile |= near_image & ((np.abs(u - np.rint(u)) < 1e-4) | (np.abs(v - np.rint(v)) < 1e-4))
        px = np.where(inside, fu, 0).astype(np.int64)
        py = np.where(inside, fv, 0).astype(np.int64)
        d = view.depth[py, px].astype(dt)
        ok = inside & (d > 0) & (d <= dt(view.depth_max))
        sdf = d - zc
        fragile |= ok & (np.abs(sdf + tr) < 1e-5 * float(tr))
        ok = ok & ~(sdf < -tr)
        with np.errstate(invalid="ignore"):
            val = np.minimum(dt(1), sdf / tr)
        w1 = Wt + dt(1)
        with np.errstate(invalid="ignore"):
            D = np.where(ok, (Wt * D + val) / w1, D)
            if C is not None and view.rgb is not None:
                for c in range(3):
                    C[c] = np.where(ok, (Wt * C[c] + view.rgb[c][py, px].astype(dt)) / w1, C[c])
        Wt = np.where(ok, np.minimum(w1, dt(w_max)), Wt)
    return D, Wt, C, fragile


def integrate_voxel(ijk, start, origin, voxel, views, w_max, trunc, flips):
    """One voxel in float32, scalar by scalar.  start = (D, W, (r, g, b) or None).  flips[view] = (dpx, dpy, flip_sdf): the pixel column / row
    moved by that much and the sdf < -trunc decision inverted.  Returns (D, W, rgb)."""
    f = np.float32
    D, Wt, C = f(start[0]), f(start[1]), None if start[2] is None else [f(c) for c in start[2]]
    x, y, z = (f(origin[a]) + f(ijk[a]) * f(voxel) for a in range(3))
    for view, (dpx, dpy, flip) in zip(views, flips):
        tr = f(view.trunc if view.trunc is not None else trunc)
        H, W = view.depth.shape
        R, T = view.R, view.T
        xc = R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + T[0]
        yc = R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + T[1]
        zc = R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + T[2]
        if not zc > 0:
            continue
        u = view.fx * (xc / zc) + view.cx
        v = view.fy * (yc / zc) + view.cy
        px, py = int(np.floor(u)) + dpx, int(np.floor(v)) + dpy
        if not (0 <= px < W and 0 <= py < H):
            continue
        d = view.depth[py, px]
        if not (d > 0 and d <= view.depth_max):
            continue
        sdf = f(d - zc)
        if (sdf < -tr) != flip:
            continue
        val = min(f(1), f(sdf / tr))
        w1 = f(Wt + f(1))
        D = f(f(Wt * D + val) / w1)
        if C is not None and view.rgb is not None:
            C = [f(f(Wt * C[c] + view.rgb[c][py, px]) / w1) for c in range(3)]
        Wt = min(w1, f(w_max))
    return D, Wt, C


def fragile_alternatives(ijk, origin, voxel, views, trunc):
    """Per view, the decisions a float64 look at this voxel calls fragile: [(dpx, dpy, flip_sdf), ...] including the plain (0, 0, False)."""
    out = []
    x, y, z = (float(np.float32(origin[a])) + float(ijk[a]) * float(np.float32(voxel)) for a in range(3))
    for view in views:
        tr = float(view.trunc if view.trunc is not None else trunc)
        R, T = view.R.astype(np.float64), view.T.astype(np.float64)
        xc, yc, zc = (R[r, 0] * x + R[r, 1] * y + R[r, 2] * z + T[r] for r in range(3))
        opts_x, opts_y, opts_s = [0], [0], [False]
        if zc > 0:
            u = float(view.fx) * (xc / zc) + float(view.cx)
            v = float(view.fy) * (yc / zc) + float(view.cy)
            if abs(u - round(u)) < 1e-4:
                opts_x = [0, -1, 1]
            if abs(v - round(v)) < 1e-4:
                opts_y = [0, -1, 1]
            H, W = view.depth.shape
            for dpx in opts_x:
                for dpy in opts_y:
                    px, py = int(np.floor(u)) + dpx, int(np.floor(v)) + dpy
                    if 0 <= px < W and 0 <= py < H and abs(float(view.depth[py, px]) - zc + tr) < 1e-5 * tr:
                        opts_s = [False, True]
        out.append(list(itertools.product(opts_x, opts_y, opts_s)))
    return out


# ---- marching tetrahedra over the Kuhn split ------------------------------------------------------------------------------------------------------
def _corner(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def kuhn_tetrahedra():
    """The six corner paths 0 -> 7 of the unit cell, one per order in which the axes are added."""
    tets = []
    for perm in itertools.permutations(range(3)):
        c, path = 0, [0]
        for axis in perm:
            c |= 1 << axis
            path.append(c)
        tets.append(tuple(path))
    return tets


def case_table():
    """table[t][m] = triangles of tetrahedron t under sign case m (bit q = path corner q inside): each triangle three edges (q_lo, q_hi) of path
    positions, wound so that the normal points from the inside corners to the outside corners.  Derived, not typed: a triangle cuts a lone corner
    off; two against two give a quad, split along the diagonal from edge (first inside, first outside) to edge (last inside, last outside)."""
    table = []
    for path in kuhn_tetrahedra():
        pos = [_corner(c) for c in path]
        row = []
        for m in range(16):
            ins = [q for q in range(4) if (m >> q) & 1]
            outs = [q for q in range(4) if not (m >> q) & 1]
            if len(ins) in (0, 4):
                row.append([])
                continue
            if len(ins) == 1:
                tris = [[(ins[0], o) for o in outs]]
            elif len(ins) == 3:
                tris = [[(outs[0], i) for i in ins]]
            else:
                (a, b), (c, d) = ins, outs
                tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
            direction = np.mean([pos[q] for q in outs], axis=0) - np.mean([pos[q] for q in ins], axis=0)
            fixed = []
            for tri in tris:
                p = [0.5 * (pos[e[0]] + pos[e[1]]) for e in tri]
                normal = np.cross(p[1] - p[0], p[2] - p[0])
                s = float(normal @ direction)
                assert abs(s) > 1e-9
                if s < 0:
                    tri = [tri[0], tri[2], tri[1]]
                fixed.append([(min(e), max(e)) for e in tri])
            row.append(fixed)
        table.append(row)
    return table


def marching_tetrahedra(tsdf, weight, rgb, origin, voxel, level=0.0, min_weight=1.0):
    """-> namespace(vertices (V,3) f32, colors (V,3) f32 or None, faces (F,3) i32, face_cell (F,), vertex_owner (V,), vertex_slot (V,))."""
    f32 = np.float32
    tsdf = np.asarray(tsdf, f32)
    nz, ny, nx = tsdf.shape
    inside = tsdf < f32(level)
    seen = np.asarray(weight, f32) >= f32(min_weight)
    sub = lambda a, c: a[(c >> 2) & 1:nz - 1 + ((c >> 2) & 1), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        valid &= sub(seen, c)
    ck, cj, ci = np.nonzero(valid)                                  # ascending cell order
    cell_lin = (ck * ny + cj) * nx + ci
    corner_in = [sub(inside, c)[valid] for c in range(8)]
    lin_off = lambda c: (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny
    slot_of = {dx | (dy << 1) | (dz << 2): s for s, (dx, dy, dz) in enumerate(SLOT_DIRS)}
    # every crossed edge of an emitted cell owns a vertex, kept by its lower corner
    used = np.zeros((nx * ny * nz, 7), bool)
    for p in range(8):
        for q in range(8):
            if p != q and (p & q) == p:
                crossed = corner_in[p] != corner_in[q]
                used[cell_lin[crossed] + lin_off(p), slot_of[p ^ q]] = True
    vid = (np.cumsum(used.reshape(-1)) - 1).reshape(used.shape)
    owner, slot = np.nonzero(used)                                  # ascending (owner, slot)
    k, r = np.divmod(owner, nx * ny)
    j, i = np.divmod(r, nx)
    d = np.array(SLOT_DIRS)[slot]
    flat = tsdf.reshape(-1)
    other = owner + d[:, 0] + d[:, 1] * nx + d[:, 2] * nx * ny
    da, db = flat[owner], flat[other]
    t = (f32(level) - da) / (db - da)
    o, h = [f32(v) for v in origin], f32(voxel)
    verts = np.empty((owner.size, 3), f32)
    for axis, idx in enumerate((i, j, k)):
        a = o[axis] + idx.astype(f32) * h
        b = o[axis] + (idx + d[:, axis]).astype(f32) * h
        verts[:, axis] = a + t * (b - a)
    colors = None
    if rgb is not None:
        cf = np.asarray(rgb, f32).reshape(3, -1)
        colors = np.stack([cf[c][owner] + t * (cf[c][other] - cf[c][owner]) for c in range(3)], axis=1).astype(f32)
    faces, fcell = [], []
    table = case_table()
    for ti, path in enumerate(kuhn_tetrahedra()):
        case = sum(corner_in[path[q]].astype(np.int64) << q for q in range(4))
        for m in range(1, 15):
            sel = np.nonzero(case == m)[0]
            if not sel.size:
                continue
            for tri in table[ti][m]:
                idx = [vid[cell_lin[sel] + lin_off(path[q0]), slot_of[path[q0] ^ path[q1]]] for q0, q1 in tri]
                faces.append(np.stack(idx, axis=1))
                fcell.append(cell_lin[sel])
    if faces:
        faces, fcell = np.concatenate(faces), np.concatenate(fcell)
        order = np.argsort(fcell, kind="stable")
        faces, fcell = faces[order], fcell[order]
    else:
        faces, fcell = np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    return SimpleNamespace(vertices=verts, colors=colors, faces=faces.astype(np.int32), face_cell=fcell, vertex_owner=owner, vertex_slot=slot)


def face_cells(faces, vertex_owner, vertex_slot, dims):
    """The cell of each face, from its three crossed edges alone: their six end points span the cell's tetrahedron, whose first corner is the
    cell's corner 0."""
    nx, ny, nz = dims
    k, r = np.divmod(np.asarray(vertex_owner), nx * ny)
    j, i = np.divmod(r, nx)
    lo = np.stack([i, j, k], axis=1)[np.asarray(faces, np.int64)]          # (F,3,3): the lower end of each edge
    c = lo.min(axis=1)
    return (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]


def canonical_faces(faces):
    """Each triple rotated to start with its smallest index, rows sorted: equal iff the two face lists are equal as multisets of oriented triangles."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not f.size:
        return f
    s = np.argmin(f, axis=1)
    rot = np.stack([f[np.arange(len(f)), (s + q) % 3] for q in range(3)], axis=1)
    return rot[np.lexsort((rot[:, 2], rot[:, 1], rot[:, 0]))]


def mesh_topology(faces, n_vertices):
    """-> namespace(closed_oriented: every directed edge occurs once and its reverse once; euler = V - E + F; all vertices referenced)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = de[:, 0] * (n_vertices + 1) + de[:, 1]
    rkey = de[:, 1] * (n_vertices + 1) + de[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    closed = bool((cnt == 1).all() and np.array_equal(uniq, np.unique(rkey)) and not (de[:, 0] == de[:, 1]).any())
    und = np.unique(np.minimum(key, rkey))
    return SimpleNamespace(closed_oriented=closed, euler=int(n_vertices - und.size + f.shape[0]),
                           all_referenced=bool(np.unique(f).size == n_vertices))


# ---- analytic volumes of the tests ----------------------------------------------------------------------------------------------------------------
def grid_points(dims):
    nx, ny, nz = dims
    Z, Y, X = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return X, Y, Z


def sphere_volume(dims, c, r):
    X, Y, Z = grid_points(dims)
    return (np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r).astype(np.float32)


def torus_volume(dims, c, R, r):
    X, Y, Z = grid_points(dims)
    ring = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2) - R
    return (np.sqrt(ring ** 2 + (Z - c[2]) ** 2) - r).astype(np.float32)
