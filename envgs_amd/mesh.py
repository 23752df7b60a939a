"""Mesh extraction (include/envgs_mesh.h, csrc/mesh.hip, csrc/mesh_clean.hip, csrc/mesh_simplify.hip, csrc/mesh_eval.hip): TSDF fusion of rendered
depth into a dense volume, marching tetrahedra over it, the clean-up of the mesh (connected components, order-preserving face selection, removal
of small components), its simplification by vertex clustering, and its evaluation against a ground-truth cloud (surface samples, exact nearest
points, Chamfer and F-score; the DTU protocol; rigid registration and the Tanks-and-Temples protocol: csrc/mesh_register.hip).

PARITY UNPINNED: the reference ships a fuser (easyvolcap/utils/tsdf_utils.py, fusion_utils.py, runners/visualizers/geometry_visualizer.py) that
cannot run as it stands and leaves the marching step to libraries outside it, so the semantics are this project's ("Mesh extraction");
tests/mesh_oracle.py restates them independently.  There is no CPU path: CPU tensors raise.

    vol = TSDFVolume((-1, -1, -1), (1, 1, 1), voxel_size=0.01)
    fuse_surfels(vol, cameras, base, sh_degree=3)
    mesh = clean(vol.extract())                 # csrc/mesh_clean.hip: components(), select_faces() and the 2DGS rule built on them
    mesh = simplify(clean(vol.extract()), 2 * voxel_size, origin=vol.origin)      # csrc/mesh_simplify.hip: vertex clustering on a uniform grid
    ckpt.save_mesh_ply("scene.ply", mesh.vertices, mesh.faces, mesh.colors)
    score = evaluate(mesh, scan_points, max_distance=0.2, threshold=0.01, density=1e4)      # csrc/mesh_eval.hip: .chamfer, .fscore, ...
    dtu = evaluate_dtu(cull_to_masks(mesh, cameras, masks), scan_points, radius=0.2, max_distance=20.0, density=25.0,
                       observed=(obs_mask, origin, voxel), box=(lo, hi), plane=plane)       # the DTU protocol: thin_points() and the filters
    tnt = evaluate_tnt(mesh, scan_points, tau=0.003, init=T_colmap_to_scan, crop=load_crop_volume("Barn.json"), density=4e5)
                                                                                            # Tanks and Temples: register(), voxel_downsample(), the crop
    maps = render_mesh(mesh, cameras)                               # csrc/mesh_raster.hip: exact depth, face, normal and colour maps of the mesh through
    mesh = cull_unseen(mesh, cameras)                               # cameras (a triangle z-buffer, no clipping), and the cull of what no camera sees
    cloud, maps = fuse_surfel_points(cameras, base, sh_degree=3)     # csrc/mesh_fuse.hip: depth-map fusion, the route without a volume -- PARITY
                                                                     # PINNED by tests/golden/fuse_golden.npz (the section "depth fusion" below)
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

MAX_VIEWS = 8                 # ENVGS_TSDF_MAX_VIEWS


def _stream(dev):
    return _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _need_gpu(t, what):
    if t.device.type != "cuda":
        raise RuntimeError("%s needs tensors on the GPU; there is no CPU path" % what)


def _host(t, shape):
    """Camera parameters travel by value: a small host copy."""
    return torch.as_tensor(t, dtype=torch.float32).detach().cpu().reshape(shape)


class Mesh(SimpleNamespace):
    """vertices (V,3) f32 world coordinates, faces (F,3) i32, colors (V,3) f32 or None: device tensors."""


class TSDFVolume:
    """A dense truncated-signed-distance volume over [bounds_min, bounds_max]: `tsdf` (Nz,Ny,Nx) in units of the truncation distance, initialised
    to 1; `weight` (Nz,Ny,Nx), initialised to 0; `rgb` (3,Nz,Ny,Nx) when color=True.  Voxel (i,j,k) sits at origin + (i,j,k) voxel_size; the
    dimensions are rounded up so that the grid covers the bounds.  trunc defaults to 5 voxel_size (the convention of the 2DGS mesh extraction,
    adopted here as this project's choice)."""

    def __init__(self, bounds_min, bounds_max, voxel_size, trunc=None, color=True, w_max=64.0, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("TSDFVolume needs a GPU device; there is no CPU path")
        lo = [float(v) for v in bounds_min]
        hi = [float(v) for v in bounds_max]
        voxel_size = float(voxel_size)
        if not voxel_size > 0.0 or any(not h > l for l, h in zip(lo, hi)):
            raise ValueError("TSDFVolume: voxel_size must be positive and bounds_max above bounds_min")
        dims = [max(2, int(math.ceil((h - l) / voxel_size - 1e-9)) + 1) for l, h in zip(lo, hi)]
        self._setup(dims, lo, voxel_size, trunc, w_max)
        nx, ny, nz = dims
        self.tsdf = torch.ones(nz, ny, nx, dtype=torch.float32, device=device)
        self.weight = torch.zeros(nz, ny, nx, dtype=torch.float32, device=device)
        self.rgb = torch.zeros(3, nz, ny, nx, dtype=torch.float32, device=device) if color else None

    def _setup(self, dims, origin, voxel_size, trunc, w_max):
        nx, ny, nz = dims
        if min(dims) < 2 or max(dims) > 2048 or nx * ny * nz >= 2 ** 31:
            raise ValueError("TSDFVolume: dimensions %s are outside 2..2048 per axis / 2^31 voxels" % (dims,))
        self.dims = (nx, ny, nz)
        self.origin = tuple(float(o) for o in origin)
        self.voxel_size = float(voxel_size)
        self.trunc = 5.0 * self.voxel_size if trunc is None else float(trunc)
        self.w_max = float(w_max)

    @classmethod
    def from_tensors(cls, tsdf, weight, rgb, origin, voxel_size, trunc=None, w_max=64.0):
        """A volume made elsewhere: tsdf, weight (Nz,Ny,Nx) and rgb (3,Nz,Ny,Nx) or None, contiguous float32 device tensors, used in place."""
        _need_gpu(tsdf, "TSDFVolume.from_tensors")
        for t, shape in ((tsdf, tuple(tsdf.shape)), (weight, tuple(tsdf.shape)), (rgb, (3,) + tuple(tsdf.shape))):
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != tsdf.device or tsdf.dim() != 3:
                raise ValueError("TSDFVolume.from_tensors: tensors must be contiguous float32, (Nz,Ny,Nx) / (3,Nz,Ny,Nx), on one device")
        self = cls.__new__(cls)
        nz, ny, nx = tsdf.shape
        self._setup([nx, ny, nz], origin, voxel_size, trunc, w_max)
        self.tsdf, self.weight, self.rgb = tsdf, weight, rgb
        return self

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.rgb is not None:
            self.rgb.zero_()

    def _c_volume(self):
        nx, ny, nz = self.dims
        return _lib.TsdfVolume(nx, ny, nz, self.origin[0], self.origin[1], self.origin[2], self.voxel_size, self.tsdf.data_ptr(),
                               self.weight.data_ptr(), None if self.rgb is None else self.rgb.data_ptr())

    def integrate(self, depth, K, R, T, rgb=None, mask=None, depth_max=float("inf")):
        """Fuses z-depth maps (H,W) or (B,H,W) (0 or negative = no measurement) seen through K (3,3), R (3,3) world -> camera and T (3,) --
        each alone or one per view -- with optional colour maps (3,H,W) / (B,3,H,W).  mask: boolean, False = no measurement.  Views go to the
        device 8 per launch, in the order given."""
        lib = _lib.load()
        _need_gpu(depth, "TSDFVolume.integrate")
        dev = self.tsdf.device
        if depth.dim() == 2:
            depth = depth[None]
            rgb = None if rgb is None else rgb[None]
            mask = None if mask is None else mask.reshape((1,) + tuple(depth.shape[1:]))
        B, H, W = depth.shape
        depth = depth.to(device=dev, dtype=torch.float32)
        if mask is not None:                                    # the one masked copy
            depth = torch.where(mask.to(dev).reshape(B, H, W), depth, torch.zeros((), dtype=torch.float32, device=dev))
        depth = depth.contiguous()
        if rgb is not None:
            rgb = rgb.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(rgb.shape) != (B, 3, H, W):
                raise ValueError("TSDFVolume.integrate: rgb must be (B,3,H,W) for depth (B,H,W)")
        K = _host(K, (-1, 3, 3)); R = _host(R, (-1, 3, 3)); T = _host(T, (-1, 3))
        per_view = lambda a, b: a[b if a.shape[0] > 1 else 0]
        vol = self._c_volume()
        for b0 in range(0, B, MAX_VIEWS):
            views = _lib.TsdfViews()
            views.count = min(MAX_VIEWS, B - b0)
            for q in range(views.count):
                b = b0 + q
                k, r, t = per_view(K, b), per_view(R, b), per_view(T, b)
                v = views.v[q]
                v.depth = depth[b].data_ptr()
                v.rgb = None if rgb is None else rgb[b].data_ptr()
                v.H, v.W = H, W
                v.fx, v.fy, v.cx, v.cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
                v.R = (_lib.ctypes.c_float * 9)(*[float(x) for x in r.reshape(-1)])
                v.T = (_lib.ctypes.c_float * 3)(*[float(x) for x in t])
                v.depth_max = float(depth_max)
                v.trunc = self.trunc
            _lib.check(lib.envgs_tsdf_integrate(vol, views, self.w_max, _stream(dev)), "envgs_tsdf_integrate")
        return self

    def extract(self, level=0.0, min_weight=1.0):
        """Marching tetrahedra over the cells whose 8 corners all have weight >= min_weight -> Mesh.  One host sync: the read-back of (V, F)."""
        lib = _lib.load()
        dev = self.tsdf.device
        nx, ny, nz = self.dims
        tb = lib.envgs_mesh_temp_bytes(nx, ny, nz)
        temp = torch.empty(tb, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int32, device=dev)
        vol = self._c_volume()
        p = _lib.ptr
        _lib.check(lib.envgs_mesh_count(vol, float(level), float(min_weight), p(temp), tb, p(totals), _stream(dev)), "envgs_mesh_count")
        V, F = [int(x) & 0xFFFFFFFF for x in totals.tolist()]
        if V >= 2 ** 31 or F >= 2 ** 31:
            raise RuntimeError("TSDFVolume.extract: %d vertices / %d faces do not fit int32 indices" % (V, F))
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        colors = torch.empty(V, 3, dtype=torch.float32, device=dev) if self.rgb is not None else None
        _lib.check(lib.envgs_mesh_extract(vol, float(level), p(temp), tb, V, F, p(vertices), p(colors), p(faces), _stream(dev)), "envgs_mesh_extract")
        return Mesh(vertices=vertices, faces=faces, colors=colors)


# ---- clean-up (csrc/mesh_clean.hip) ---------------------------------------------------------------------------------------------------------------
def _mesh_tensors(mesh, what):
    """-> (vertices, faces, colors) of a Mesh-like namespace, checked: contiguous device tensors of the documented dtypes and shapes."""
    v, f, c = mesh.vertices, mesh.faces, getattr(mesh, "colors", None)
    _need_gpu(v, what)
    _need_gpu(f, what)
    if v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3 or not v.is_contiguous():
        raise ValueError("%s: vertices must be a contiguous (V,3) float32 tensor" % what)
    if f.dtype != torch.int32 or f.dim() != 2 or f.shape[1] != 3 or not f.is_contiguous():
        raise ValueError("%s: faces must be a contiguous (F,3) int32 tensor" % what)
    if c is not None:
        _need_gpu(c, what)
        if c.dtype != torch.float32 or tuple(c.shape) != tuple(v.shape) or not c.is_contiguous():
            raise ValueError("%s: colors must be a contiguous (V,3) float32 tensor" % what)
    if f.device != v.device or (c is not None and c.device != v.device):
        raise ValueError("%s: vertices, faces and colors must be on one device" % what)
    if v.shape[0] >= 2 ** 31 or f.shape[0] >= 2 ** 31:
        raise ValueError("%s: %d vertices / %d faces do not fit int32 indices" % (what, v.shape[0], f.shape[0]))
    return v, f, c


def components(mesh):
    """Connected components of the mesh: faces are connected iff they share a vertex index (include/envgs_mesh.h).  Components are numbered by
    ascending smallest vertex index; a face with an index outside [0, V) is ignored (label -1), as is an unreferenced vertex.
    -> namespace(count: int, vertex_label (V,) i32, face_label (F,) i32, faces (C,) i32, vertices (C,) i32: per-component counts), device
    tensors.  One host sync: the read-back of the count."""
    v, f, _ = _mesh_tensors(mesh, "components")
    lib = _lib.load()
    dev = v.device
    V, F = v.shape[0], f.shape[0]
    tb = lib.envgs_mesh_components_temp_bytes(V, F)
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    vertex_label = torch.empty(V, dtype=torch.int32, device=dev)
    face_label = torch.empty(F, dtype=torch.int32, device=dev)
    comp_faces = torch.empty(min(V, F), dtype=torch.int32, device=dev)
    comp_vertices = torch.empty(min(V, F), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.check(lib.envgs_mesh_components(V, F, p(f), p(temp), tb, p(vertex_label), p(face_label), p(comp_faces), p(comp_vertices), p(count), _stream(dev)),
               "envgs_mesh_components")
    C = int(count.item())
    return SimpleNamespace(count=C, vertex_label=vertex_label, face_label=face_label, faces=comp_faces[:C], vertices=comp_vertices[:C])


def select_faces(mesh, keep, return_index=False):
    """The mesh of the faces with keep != 0 (`keep`: (F,) bool or uint8 device tensor) and of the vertices they name, both in their old relative
    order, faces re-indexed, vertices and colours copied bit for bit.  Faces with an index outside [0, V) are never selected.
    -> Mesh, or (Mesh, vertex_index (V',) i32: the old index of each new vertex) with return_index.  One host sync: the read-back of (V', F')."""
    v, f, c = _mesh_tensors(mesh, "select_faces")
    _need_gpu(keep, "select_faces")
    if keep.dtype == torch.bool and keep.is_contiguous():
        keep = keep.view(torch.uint8)                           # a bool tensor stores 0 / 1 bytes
    if keep.dtype != torch.uint8 or keep.dim() != 1 or keep.shape[0] != f.shape[0] or not keep.is_contiguous() or keep.device != v.device:
        raise ValueError("select_faces: keep must be a contiguous (F,) bool or uint8 tensor on the mesh's device")
    lib = _lib.load()
    dev = v.device
    V, F = v.shape[0], f.shape[0]
    tb = lib.envgs_mesh_select_temp_bytes(V, F)
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.check(lib.envgs_mesh_select_count(V, F, p(f), p(keep), p(temp), tb, p(totals), _stream(dev)), "envgs_mesh_select_count")
    Vo, Fo = [int(x) for x in totals.tolist()]
    vertices = torch.empty(Vo, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(Fo, 3, dtype=torch.int32, device=dev)
    colors = torch.empty(Vo, 3, dtype=torch.float32, device=dev) if c is not None else None
    index = torch.empty(Vo, dtype=torch.int32, device=dev) if return_index else None
    _lib.check(lib.envgs_mesh_select_emit(V, F, p(v), p(c), p(f), p(keep), p(temp), tb, Vo, Fo, p(vertices), p(colors), p(faces), p(index), _stream(dev)),
               "envgs_mesh_select_emit")
    out = Mesh(vertices=vertices, faces=faces, colors=colors)
    return (out, index) if return_index else out


def clean(mesh, keep_largest=50, min_faces=50):
    """Drops the debris of a fused mesh, by the rule of the 2DGS mesh post-processing (adopted here as this project's choice): a component is
    kept iff its face count >= max(min_faces, face count of the keep_largest-th largest component); the second term is 0 when keep_largest is
    None, 0 or at least the number of components.  Ties at the threshold are all kept.  The choice is made on the (C,) tables on the device;
    two host syncs in all: the one of components() and the one of select_faces()."""
    comp = components(mesh)
    threshold = torch.full((), int(min_faces), dtype=torch.int32, device=comp.faces.device)
    if keep_largest is not None and 0 < int(keep_largest) < comp.count:
        threshold = torch.maximum(threshold, torch.sort(comp.faces, descending=True).values[int(keep_largest) - 1])
    kept = torch.cat([comp.faces >= threshold, torch.zeros(1, dtype=torch.bool, device=comp.faces.device)])      # row -1: the ignored faces
    return select_faces(mesh, kept[comp.face_label.long()])


# ---- simplification (csrc/mesh_simplify.hip) --------------------------------------------------------------------------------------------------------
def _grid_dims(extent, cell_size):
    """Cells per axis that cover [0, extent]: floor(extent / cell_size) + 1, at least 1 (Python ints, so they may exceed any machine range)."""
    dims = []
    for e in extent:
        r = e / cell_size if e > 0.0 else 0.0
        dims.append(max(1, int(math.floor(r)) + 1) if math.isfinite(r) else 2 ** 62)
    return dims


def _finite_extent(vertices):
    """-> (lo, hi): the per-axis extrema of the rows of (V,3) whose three coordinates are finite; zeros when there is none.  One host sync, a
    second one when some row is not finite."""
    lo, hi = [0.0] * 3, [0.0] * 3
    if vertices.shape[0]:
        # column by column: a full reduction of a strided column is 15 x faster here than amin(dim=0) over (V,3) (0.08 against 1.2 ms at V = 1.6 M)
        columns = lambda t: [torch.aminmax(t[:, a]) for a in range(3)]
        read = lambda lows, highs: torch.stack([torch.stack(lows), torch.stack(highs)]).tolist()
        cols = columns(vertices)
        ext = read([c.min for c in cols], [c.max for c in cols])
        if not all(math.isfinite(x) for x in ext[0] + ext[1]):    # a NaN or an infinity somewhere: again, over the finite vertices alone
            finite = torch.isfinite(vertices).all(dim=1, keepdim=True)
            ext = read([c.min for c in columns(torch.where(finite, vertices, float("inf")))],
                       [c.max for c in columns(torch.where(finite, vertices, float("-inf")))])
        if all(math.isfinite(x) for x in ext[0] + ext[1]):        # else: no finite vertex, any grid will do
            lo, hi = ext
    return lo, hi


def simplify_grid(vertices, cell_size, origin=None, dims=None):
    """The clustering grid simplify() uses: -> (origin (ox, oy, oz), dims (nx, ny, nz)).  origin None: the per-axis minimum of the vertices whose
    three coordinates are finite; dims[a] = floor((max[a] - origin[a]) / cell_size) + 1 over the same vertices, at least 1 (in double; positions
    outside the grid are clamped into its border cells, so the rounding of this formula never loses a vertex).  One host sync: the read-back of
    the six extrema (a second one when some vertex is not finite); none when origin and dims are both given (dims: (nx, ny, nz) cells, used as they are).  Raises ValueError for a grid of
    2^31 cells or more, naming the smallest admissible cell_size."""
    _need_gpu(vertices, "simplify")
    cell_size = float(cell_size)
    if not (cell_size > 0.0 and math.isfinite(cell_size)) or not float(torch.tensor(cell_size, dtype=torch.float32)) > 0.0:
        raise ValueError("simplify: cell_size must be positive and finite")
    if origin is not None:
        origin = [float(o) for o in origin]
        if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
            raise ValueError("simplify: origin must be three finite numbers")
    if dims is not None:
        dims = tuple(int(n) for n in dims)
        if len(dims) != 3 or min(dims) < 1 or math.prod(dims) >= 2 ** 31:
            raise ValueError("simplify: dims %s must be three counts of at least 1 whose product is below 2^31" % (dims,))
        if origin is not None:
            return tuple(origin), dims
    lo, hi = _finite_extent(vertices)
    if origin is not None:
        lo = origin
    if dims is not None:
        return tuple(lo), dims
    extent = [h - l for l, h in zip(lo, hi)]
    cells = lambda c: math.prod(_grid_dims(extent, c))
    if cells(cell_size) >= 2 ** 31:
        bad, good = cell_size, 2.0 * cell_size
        while cells(good) >= 2 ** 31:
            bad, good = good, 2.0 * good
        for _ in range(60):
            mid = 0.5 * (bad + good)
            bad, good = (bad, mid) if cells(mid) < 2 ** 31 else (mid, good)
        raise ValueError("simplify: cell_size %g gives a grid of %d cells, 2^31 or more; the smallest admissible cell_size here is %r"
                         % (cell_size, cells(cell_size), good))
    return tuple(lo), tuple(_grid_dims(extent, cell_size))


def simplify(mesh, cell_size, origin=None, return_index=False, dims=None):
    """Vertex clustering on a uniform grid of edge cell_size (include/envgs_mesh.h, "simplification"): the vertices of one cell become one vertex,
    at the integer-accumulated mean of their positions and colours (a cell of one vertex keeps it bit for bit); faces are re-mapped, and those
    that collapse, name a vertex without a cell, or repeat an earlier face up to rotation are dropped.  Clusters are numbered by ascending cell
    index and faces keep their order, so the result does not depend on scheduling or on the numbering of the input vertices: two runs give
    identical bytes.  origin: the grid's corner (e.g. the volume's origin, cell_size = k voxel_size); None = the minimum of the finite vertices.
    dims: the grid's (nx, ny, nz) cells; None = as many as cover the finite vertices.  Vertices outside the grid are clamped into its border cells.
    -> Mesh, or (Mesh, vertex_cluster (V,) i32: the new index of each input vertex, -1 if none) with return_index.
    Two host syncs: the read-back of the vertex extrema that size the grid (simplify_grid; none when origin and dims are both given), and the
    read-back of (V', F') of the selection; the cluster count stays on the device."""
    v, f, c = _mesh_tensors(mesh, "simplify")
    (ox, oy, oz), (nx, ny, nz) = simplify_grid(v, cell_size, origin, dims)
    lib = _lib.load()
    dev = v.device
    V, F = v.shape[0], f.shape[0]
    R = min(V, nx * ny * nz)
    tb = lib.envgs_mesh_simplify_temp_bytes(V, F, nx, ny, nz)
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    cl_vertices = torch.empty(R, 3, dtype=torch.float32, device=dev)
    cl_colors = torch.empty(R, 3, dtype=torch.float32, device=dev) if c is not None else None
    cl_faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    keep = torch.empty(F, dtype=torch.uint8, device=dev)
    vertex_cluster = torch.empty(V, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.check(lib.envgs_mesh_simplify_cluster(V, F, p(v), p(c), p(f), ox, oy, oz, float(cell_size), nx, ny, nz, p(temp), tb, p(cl_vertices), p(cl_colors),
                                               p(cl_faces), p(keep), p(vertex_cluster), p(count), _stream(dev)), "envgs_mesh_simplify_cluster")
    clustered = Mesh(vertices=cl_vertices, faces=cl_faces, colors=cl_colors)
    if not return_index:
        return select_faces(clustered, keep)
    out, index = select_faces(clustered, keep, return_index=True)
    new_of_cluster = torch.full((R + 1,), -1, dtype=torch.int32, device=dev)                 # row -1: the vertices without a cluster
    new_of_cluster[index.long()] = torch.arange(index.shape[0], dtype=torch.int32, device=dev)
    return out, new_of_cluster[vertex_cluster.long()]


def surface_depth(allmap, depth_ratio=0.0):
    """surf_depth of the reference's render() (gaussian2d_utils.py:1125-1131): the expected depth allmap[0] / alpha mixed with the median depth
    allmap[5] by depth_ratio, non-finite values zeroed -- the expression of envgs_step.base_pass and of the surface_normal kernel."""
    expected = torch.nan_to_num(allmap[0] / allmap[1], 0, 0)
    median = torch.nan_to_num(allmap[5], 0, 0)
    return expected * (1.0 - depth_ratio) + median * depth_ratio


def fuse_surfels(volume, cameras, base, sh_degree, depth_ratio=0.0, alpha_min=0.5, scale_modifier=1.0):
    """Renders `base` (means3D, shs, opacities, scales, rotations) from every camera (synth.make_camera namespaces) through
    diff_surfel_rasterization_wet under no_grad, and integrates the surface depth and the rendered colour of the pixels with alpha > alpha_min.
    Returns the per-view maps it integrated: [namespace(depth (H,W), alpha (H,W), rgb (3,H,W))]."""
    import diff_surfel_rasterization_wet as pkg
    _need_gpu(base["means3D"], "fuse_surfels")
    dev = base["means3D"].device
    maps = []
    with torch.no_grad():
        bg = torch.zeros(3, dtype=torch.float32, device=dev)
        for cam in cameras:
            st = pkg.GaussianRasterizationSettings(
                image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg,
                scale_modifier=scale_modifier, viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
                sh_degree=sh_degree, campos=cam.camera_center.to(dev), prefiltered=False, debug=False)
            color, _, allmap, _ = pkg.GaussianRasterizer(raster_settings=st)(
                means3D=base["means3D"], means2D=torch.zeros_like(base["means3D"]), shs=base["shs"], colors_precomp=None,
                opacities=base["opacities"], scales=base["scales"], rotations=base["rotations"], cov3D_precomp=None)
            maps.append(SimpleNamespace(depth=surface_depth(allmap, depth_ratio), alpha=allmap[1], rgb=color[:3].contiguous()))
        for b0 in range(0, len(maps), MAX_VIEWS):
            chunk, cams = maps[b0:b0 + MAX_VIEWS], cameras[b0:b0 + MAX_VIEWS]
            if len({tuple(m.depth.shape) for m in chunk}) == 1:
                groups = [(chunk, cams)]
            else:                                               # views of different sizes cannot share a (B,H,W) stack
                groups = [([m], [c]) for m, c in zip(chunk, cams)]
            for ms, cs in groups:
                volume.integrate(torch.stack([m.depth for m in ms]), torch.stack([c.K.cpu() for c in cs]), torch.stack([c.R.cpu() for c in cs]),
                                 torch.stack([c.T.cpu().reshape(3) for c in cs]), rgb=torch.stack([m.rgb for m in ms]),
                                 mask=torch.stack([m.alpha > alpha_min for m in ms]))
    return maps


# ---- evaluation (csrc/mesh_eval.hip) ------------------------------------------------------------------------------------------------------------------
POINTS_MAX_DIM, POINTS_MAX_CELLS = 1024, 2 ** 27                 # ENVGS_POINTS_MAX_DIM, ENVGS_POINTS_MAX_CELLS


def sample_surface(mesh, density, seed=0, return_face=False):
    """Area-proportional surface samples with canonical bytes (include/envgs_mesh.h, "evaluation"): face f gets floor(area density + u_f) samples,
    u_f and the samples themselves coming from a counter hash of (seed, f, k), ordered by ascending (face, k).  Faces with an index outside
    [0, V), a corner or an area that is not finite, or no area get none.  density: samples per unit area, positive and finite; seed: 0 .. 2^32-1.
    -> (points (S,3) f32, colors (S,3) f32 or None), plus face (S,) i32 with return_face.  One host sync: the read-back of S.  Raises ValueError
    when a face would get 2^24 samples or more, or the mesh 2^31 or more."""
    v, f, c = _mesh_tensors(mesh, "sample_surface")
    density, seed = float(density), int(seed)
    if not (density > 0.0 and math.isfinite(density)) or not 0.0 < float(torch.tensor(density, dtype=torch.float32)) < float("inf"):
        raise ValueError("sample_surface: density must be positive and finite")
    if not 0 <= seed < 2 ** 32:
        raise ValueError("sample_surface: seed must be in 0 .. 2^32 - 1")
    lib = _lib.load()
    dev = v.device
    V, F = v.shape[0], f.shape[0]
    tb = lib.envgs_mesh_sample_temp_bytes(V, F)
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    p = _lib.ptr
    _lib.check(lib.envgs_mesh_sample_count(V, F, p(v), p(f), density, seed, p(temp), tb, p(totals), _stream(dev)), "envgs_mesh_sample_count")
    S, over = totals.tolist()
    if over:
        raise ValueError("sample_surface: density %g gives one face 2^24 samples or more" % density)
    if not 0 <= S < 2 ** 31:
        raise ValueError("sample_surface: density %g gives %d samples, 2^31 or more" % (density, S & (2 ** 64 - 1)))
    points = torch.empty(S, 3, dtype=torch.float32, device=dev)
    colors = torch.empty(S, 3, dtype=torch.float32, device=dev) if c is not None else None
    face = torch.empty(S, dtype=torch.int32, device=dev) if return_face else None
    _lib.check(lib.envgs_mesh_sample_emit(V, F, p(v), p(c), p(f), seed, p(temp), tb, S, p(points), p(colors), p(face), _stream(dev)),
               "envgs_mesh_sample_emit")
    return (points, colors, face) if return_face else (points, colors)


def _points_tensor(t, what):
    _need_gpu(t, what)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous() or t.shape[0] >= 2 ** 31:
        raise ValueError("%s: points must be a contiguous (N,3) float32 tensor of fewer than 2^31 rows" % what)
    return t


def _f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


class PointGrid:
    """A uniform grid over the finite rows of points (N,3), for exact nearest-point queries within max_distance (include/envgs_mesh.h).  The grid
    is sized as simplify_grid sizes its own: the origin is the per-axis minimum of the finite points, dims[a] = floor(extent[a] / cell_size) + 1;
    at most 1024 cells per axis and 2^27 in all.  cell_size None: max(max_distance / 16, the edge at which the bounding box holds about 4 cells
    per point), raised until the limits hold -- a guess that nobody has tuned ("Mesh evaluation"); an explicit cell_size outside the
    limits raises ValueError, naming the smallest admissible value.  The result of nearest() does not depend on cell_size.
    One host sync: the read-back of the extrema (a second one when some point is not finite).  `points` itself is not kept."""

    def __init__(self, points, max_distance, cell_size=None, _default_cell=None):
        """_default_cell: the first guess thin_points() puts in place of the heuristic when cell_size is None; raised by the same rule."""
        points = _points_tensor(points, "PointGrid")
        max_distance = float(max_distance)
        if not (max_distance >= 0.0 and math.isfinite(max_distance) and math.isfinite(_f32(max_distance))):
            raise ValueError("PointGrid: max_distance must be finite and not negative")
        lo, hi = _finite_extent(points)
        extent = [h - l for l, h in zip(lo, hi)]
        N = points.shape[0]

        def admissible(c):
            d = _grid_dims(extent, c)
            return max(d) <= POINTS_MAX_DIM and math.prod(d) <= POINTS_MAX_CELLS

        if cell_size is None:
            spans = [e for e in extent if e > 0.0]
            per_point = (math.prod(spans) / (4.0 * max(N, 1))) ** (1.0 / len(spans)) if spans else 0.0
            cell_size = max(max_distance / 16.0, per_point) if _default_cell is None else float(_default_cell)
            if not (cell_size > 0.0 and math.isfinite(cell_size) and _f32(cell_size) > 0.0):
                cell_size = 1.0
            while not admissible(cell_size):
                cell_size *= 1.125
        else:
            cell_size = float(cell_size)
            if not (cell_size > 0.0 and math.isfinite(cell_size)) or not 0.0 < _f32(cell_size) < float("inf"):
                raise ValueError("PointGrid: cell_size must be positive and finite")
            if not admissible(cell_size):
                bad, good = cell_size, 2.0 * cell_size
                while not admissible(good):
                    bad, good = good, 2.0 * good
                for _ in range(60):
                    mid = 0.5 * (bad + good)
                    bad, good = (bad, mid) if admissible(mid) else (mid, good)
                raise ValueError("PointGrid: cell_size %g gives a grid of %s cells, beyond 1024 per axis or 2^27 in all; the smallest admissible "
                                 "cell_size here is %r" % (cell_size, _grid_dims(extent, cell_size), good))
        self.origin, self.dims = tuple(lo), tuple(_grid_dims(extent, cell_size))
        self.cell_size, self.max_distance, self.count, self.device = cell_size, max_distance, N, points.device
        self.center = tuple(0.5 * (l + h) for l, h in zip(lo, hi))      # of the box of the finite points, in double: the c of register_sums()
        lib = _lib.load()
        nx, ny, nz = self.dims
        tb = lib.envgs_points_grid_temp_bytes(N, nx, ny, nz)
        temp = torch.empty(tb, dtype=torch.uint8, device=points.device)
        self.cell_end = torch.empty(nx * ny * nz, dtype=torch.int32, device=points.device)
        self.records = torch.empty(N, 4, dtype=torch.float32, device=points.device)
        p = _lib.ptr
        _lib.check(lib.envgs_points_grid_build(N, p(points), lo[0], lo[1], lo[2], cell_size, nx, ny, nz, p(temp), tb, p(self.cell_end), p(self.records),
                                               _stream(points.device)), "envgs_points_grid_build")

    def nearest(self, queries):
        """-> (dist2 (Q,) f32, index (Q,) i32): per query the finite point of least squared distance among those within max_distance, of equal ones
        the lowest index; +inf and -1 when there is none or the query is not finite.  No host sync."""
        queries = _points_tensor(queries, "PointGrid.nearest")
        if queries.device != self.device:
            raise ValueError("PointGrid.nearest: the queries must be on the grid's device")
        Q = queries.shape[0]
        dist2 = torch.empty(Q, dtype=torch.float32, device=self.device)
        index = torch.empty(Q, dtype=torch.int32, device=self.device)
        nx, ny, nz = self.dims
        p = _lib.ptr
        _lib.check(_lib.load().envgs_points_nearest(Q, p(queries), self.max_distance, self.origin[0], self.origin[1], self.origin[2], self.cell_size, nx, ny, nz,
                                                    p(self.cell_end), p(self.records), p(dist2), p(index), _stream(self.device)), "envgs_points_nearest")
        return dist2, index


def nearest_points(queries, points, max_distance, cell_size=None):
    """PointGrid(points, max_distance, cell_size).nearest(queries) -> (dist2 (Q,) f32, index (Q,) i32)."""
    return PointGrid(points, max_distance, cell_size).nearest(queries)


def _eval_points(x, density, seed, what):
    if isinstance(x, torch.Tensor):
        return _points_tensor(x, what)
    if density is None:
        raise ValueError("%s: a mesh needs a sampling density" % what)
    return sample_surface(x, density, seed)[0]


def evaluate(mesh_or_points, reference_points, max_distance, threshold, density=None, seed=0):
    """A prediction -- a Mesh, sampled at `density` with `seed`, or a (N,3) point tensor -- against a ground-truth cloud (M,3), by the conventions
    of the DTU and Tanks-and-Temples evaluations (adopted here as this project's choice).  With d = sqrt(dist2) in float64 of the nearest point
    within max_distance:
      accuracy      mean d over the prediction samples that found a neighbour (the DTU rule: what lies beyond max_distance is left out)
      completeness  the same from the reference to the prediction;     chamfer  (accuracy + completeness) / 2
      precision     share of ALL prediction samples with d <= threshold (no neighbour is a miss);   recall  the same the other way
      fscore        2 P R / (P + R), 0 when both are 0
    plus the counts n_pred, n_ref, found_pred, found_ref, within_pred, within_ref and the per-point distances d_pred (N,), d_ref (M,) (float64
    device tensors, +inf = no neighbour).  A mean over no sample is nan, a share of no sample 0.  threshold <= max_distance is required.
    Two grids, two searches; the reductions are torch in float64 with one read-back."""
    max_distance, threshold = float(max_distance), float(threshold)
    if not 0.0 <= threshold <= max_distance:
        raise ValueError("evaluate: 0 <= threshold <= max_distance is required")
    pred = _eval_points(mesh_or_points, density, seed, "evaluate")
    ref = _points_tensor(reference_points, "evaluate")
    if pred.device != ref.device:
        raise ValueError("evaluate: the prediction and the reference must be on one device")
    d_pred = torch.sqrt(PointGrid(ref, max_distance).nearest(pred)[0].double())
    d_ref = torch.sqrt(PointGrid(pred, max_distance).nearest(ref)[0].double())
    rows = []
    for d in (d_pred, d_ref):
        found = torch.isfinite(d)
        rows += [torch.where(found, d, torch.zeros((), dtype=torch.float64, device=d.device)).sum(), found.sum().double(), (d <= threshold).sum().double()]
    sum_p, found_p, within_p, sum_r, found_r, within_r = torch.stack(rows).tolist()
    n_pred, n_ref = pred.shape[0], ref.shape[0]
    accuracy = sum_p / found_p if found_p else float("nan")
    completeness = sum_r / found_r if found_r else float("nan")
    precision = within_p / n_pred if n_pred else 0.0
    recall = within_r / n_ref if n_ref else 0.0
    fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0
    return SimpleNamespace(accuracy=accuracy, completeness=completeness, chamfer=0.5 * (accuracy + completeness), precision=precision, recall=recall,
                           fscore=fscore, n_pred=n_pred, n_ref=n_ref, found_pred=int(found_p), found_ref=int(found_r), within_pred=int(within_p),
                           within_ref=int(within_r), d_pred=d_pred, d_ref=d_ref)


def compare_meshes(a, b, max_distance, threshold, density, seed=0):
    """evaluate() of the surface samples of mesh `a` against those of mesh `b`, both at `density` with `seed`: what simplify() or clean() cost."""
    return evaluate(a, sample_surface(b, density, seed)[0], max_distance, threshold, density=density, seed=seed)


# ---- the DTU protocol (csrc/mesh_eval.hip: thinning and culling; the filters are torch) -----------------------------------------------------------------
THIN_GROUP = 4                # rounds per read-back of the undecided count ("DTU protocol")


def _thin_shells(radius, cell_size, dims):
    """R of include/envgs_mesh.h ("thinning"): the smallest integer with ((float)R * cell) * (1 - 2^-10) >= radius in fp32, clipped to the grid."""
    radius, cell, last = _f32(radius), _f32(cell_size), max(dims) - 1
    reach = lambda r: _f32(_f32(float(r) * cell) * 0.9990234375) >= radius       # a product of two fp32 numbers in double, rounded once, is the fp32 product
    R = min(last, max(0, int(radius / cell) - 2))
    while R < last and not reach(R):
        R += 1
    return R


def _thin(points, radius, seed, cell_size, group, history):
    points = _points_tensor(points, "thin_points")
    radius = float(radius)
    if not (radius >= 0.0 and math.isfinite(radius) and math.isfinite(_f32(radius))):
        raise ValueError("thin_points: radius must be finite and not negative")
    if seed is not None:
        seed = int(seed)
        if not 0 <= seed < 2 ** 32:
            raise ValueError("thin_points: seed must be in 0 .. 2^32 - 1, or None for the given order")
    grid = PointGrid(points, radius, cell_size, _default_cell=radius * 1.002 if radius > 0.0 else None)
    lib = _lib.load()
    dev, N = points.device, points.shape[0]
    (ox, oy, oz), (nx, ny, nz) = grid.origin, grid.dims
    shells = _thin_shells(radius, grid.cell_size, grid.dims)
    tb = lib.envgs_points_thin_temp_bytes(N)
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    keep = torch.empty(N, dtype=torch.bool, device=dev)
    p, s = _lib.ptr, _stream(dev)
    _lib.check(lib.envgs_points_thin_begin(N, p(points), p(temp), tb, p(count), s), "envgs_points_thin_begin")
    undecided, rounds, launched = N, 0, 0                         # N: the bound that needs no read-back
    while undecided and launched < N + group:                     # every round decides a point: N rounds suffice, whatever the floats are
        _lib.check(lib.envgs_points_thin_round(N, p(points), radius, int(seed is not None), seed or 0, ox, oy, oz, grid.cell_size, nx, ny, nz, shells,
                                               p(grid.cell_end), p(grid.records), p(temp), tb, launched, group, undecided, p(count), s),
                   "envgs_points_thin_round")
        launched += group
        undecided, rounds = count.tolist()
        if history is not None:
            history.append(undecided)
    if undecided:
        raise RuntimeError("thin_points: %d points undecided after %d rounds" % (undecided, launched))
    _lib.check(lib.envgs_points_thin_keep(N, p(temp), tb, p(keep), s), "envgs_points_thin_keep")
    return keep, rounds


def thin_points(points, radius, seed=0, cell_size=None, return_rounds=False):
    """The thinning step of the DTU evaluation (include/envgs_mesh.h, "thinning"): keep (N,) bool such that no two kept points are within `radius`
    of each other (d2 <= radius^2 in fp32, inclusive) and every dropped finite point has a kept one within it -- exactly the set the DTU loop keeps
    when it visits the points by ascending key: key(i) = hash(seed, i) for seed in 0 .. 2^32-1 (a strict order, the stand-in for the script's
    shuffle), or the given order with seed=None.  Rows that are not finite are never kept.  radius: finite, >= 0 (0 removes exact duplicates); N
    below 2^31.  points[keep] keeps the ascending original index: the canonical order.
    The result depends on the points, the radius and the seed alone, never on cell_size (None: just above the radius, so that one shell of cells
    around a point holds its neighbours; raised as PointGrid raises its own until the grid limits hold; an explicit value outside the limits raises
    PointGrid's ValueError) and never on scheduling: two runs give identical bytes.
    The device decides in rounds; a point waits for its lower-keyed neighbours.  The hash order needs about log N rounds.  Index order on spatially
    sorted input (a scan line, a lattice) can need up to N rounds, one launch each: shuffle such input or give a seed.
    -> keep, or (keep, rounds: the rounds that found work) with return_rounds.  Host syncs: the extrema read-back of the grid, plus one count
    read-back per group of THIN_GROUP = 4 rounds."""
    keep, rounds = _thin(points, radius, seed, cell_size, THIN_GROUP, None)
    return (keep, rounds) if return_rounds else keep


def cull_to_masks(mesh, cameras, masks, return_index=False):
    """The cull_scan step of the 2DGS DTU evaluation: drops every vertex that some camera sees outside its object mask, and the faces that lose a
    corner.  cameras: namespaces with K (3,3), R (3,3) world -> camera and T (3,) (synth.make_camera); masks: (n,H,W) bool or uint8 device tensor,
    0 = outside.  A vertex is projected by the pixel rule of TSDFVolume.integrate, verbatim (include/envgs_mesh.h, "culling"); it passes a view iff
    it is behind the camera (zc <= 0), or its pixel is outside the image, or the mask is set there; a vertex that is not finite fails.  The faces
    whose three corners pass every view go through select_faces(), so the order is preserved and the vertices are compacted as clean() does.
    To dilate the masks first, as the 2DGS script does: torch.nn.functional.max_pool2d(masks[:, None].float(), 2 * k + 1, 1, k)[:, 0] > 0.
    -> Mesh, or (Mesh, vertex_index) with return_index.  Views go to the device 8 per launch.  One host sync: that of select_faces()."""
    v, f, _ = _mesh_tensors(mesh, "cull_to_masks")
    _need_gpu(masks, "cull_to_masks")
    cameras = list(cameras)
    if masks.dtype == torch.bool:
        masks = masks.contiguous().view(torch.uint8)
    if masks.dtype != torch.uint8 or masks.dim() != 3 or masks.shape[0] != len(cameras) or masks.device != v.device or (len(cameras) and masks[0].numel() == 0):
        raise ValueError("cull_to_masks: masks must be a (n,H,W) bool or uint8 tensor on the mesh's device, one per camera")
    masks = masks.contiguous()
    lib = _lib.load()
    dev, V, F = v.device, v.shape[0], f.shape[0]
    vertex_keep = torch.empty(V, dtype=torch.uint8, device=dev)
    face_keep = torch.empty(F, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    for b0 in range(0, max(len(cameras), 1), MAX_VIEWS):
        views = _lib.CullViews()
        views.count = min(MAX_VIEWS, len(cameras) - b0)
        for q in range(views.count):
            cam, c = cameras[b0 + q], views.v[q]
            k, r, t = _host(cam.K, (3, 3)), _host(cam.R, (3, 3)), _host(cam.T, (3,))
            c.mask = masks[b0 + q].data_ptr()
            c.H, c.W = masks.shape[1], masks.shape[2]
            c.fx, c.fy, c.cx, c.cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
            c.R = (_lib.ctypes.c_float * 9)(*[float(x) for x in r.reshape(-1)])
            c.T = (_lib.ctypes.c_float * 3)(*[float(x) for x in t])
        _lib.check(lib.envgs_mesh_cull_vertices(V, p(v), views, int(b0 > 0), p(vertex_keep), _stream(dev)), "envgs_mesh_cull_vertices")
    _lib.check(lib.envgs_mesh_cull_faces(V, F, p(f), p(vertex_keep), p(face_keep), _stream(dev)), "envgs_mesh_cull_faces")
    return select_faces(mesh, face_keep, return_index=return_index)


# ---- rasterisation (csrc/mesh_raster.hip, csrc/mesh_raster.h) -----------------------------------------------------------------------------------------
RASTER_OUTPUTS = ("depth", "face", "bary", "normal", "color", "seen")
_RASTER_MAPS = {"depth": ((), torch.float32), "face": ((), torch.int32), "bary": ((3,), torch.float32), "normal": ((3,), torch.float32),
                "color": ((3,), torch.float32)}


def _raster_size(cameras, size, what):
    if size is not None:
        H, W = (int(s) for s in size)
    else:
        sizes = {(int(getattr(c, "image_height", getattr(c, "H", -1))), int(getattr(c, "image_width", getattr(c, "W", -1)))) for c in cameras}
        if len(sizes) != 1:
            raise ValueError("%s: the cameras must share one size (got %s); pass size=(H, W)" % (what, sorted(sizes) if sizes else "no cameras"))
        H, W = sizes.pop()
    if H < 1 or W < 1 or H * W >= 2 ** 28:
        raise ValueError("%s: the image size %d x %d is outside 1 .. 2^28 pixels" % (what, H, W))
    return H, W


def _raster(mesh, cameras, size, near, outputs, what, stats=None):
    cameras = list(cameras)
    outputs = tuple(outputs)
    for o in outputs:
        if o not in RASTER_OUTPUTS:
            raise ValueError("%s: unknown output %r: one of %s" % (what, o, ", ".join(RASTER_OUTPUTS)))
    H, W = _raster_size(cameras, size, what)
    near = float(near)
    if math.isnan(near):
        raise ValueError("%s: near must not be NaN" % what)
    for t, dtype, name in ((mesh.vertices, torch.float32, "vertices"), (mesh.faces, torch.int32, "faces")):
        if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("%s: %s must be a (N,3) %s tensor" % (what, name, dtype))
    v, f, c = _mesh_tensors(mesh, what)
    lib = _lib.load()
    dev, V, F, n = v.device, v.shape[0], f.shape[0], len(cameras)
    maps = {o: torch.empty((n, H, W) + _RASTER_MAPS[o][0], dtype=_RASTER_MAPS[o][1], device=dev) for o in outputs
            if o in _RASTER_MAPS and (o != "color" or c is not None)}
    seen = torch.empty(F, dtype=torch.uint8, device=dev) if "seen" in outputs else None
    if seen is not None and n == 0:
        seen.zero_()
    tb = lib.envgs_mesh_raster_temp_bytes(H, W, min(n, MAX_VIEWS))
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    row = lambda name, b0: _lib.c_void_p(maps[name][b0].data_ptr()) if name in maps else None
    for b0 in range(0, n, MAX_VIEWS):
        views = _lib.MeshRasterViews()
        views.count = min(MAX_VIEWS, n - b0)
        for q in range(views.count):
            cam, cv = cameras[b0 + q], views.v[q]
            k, r, t = _host(cam.K, (3, 3)), _host(cam.R, (3, 3)), _host(cam.T, (3,))
            cv.fx, cv.fy, cv.cx, cv.cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
            cv.R = (_lib.ctypes.c_float * 9)(*[float(x) for x in r.reshape(-1)])
            cv.T = (_lib.ctypes.c_float * 3)(*[float(x) for x in t])
        _lib.check(lib.envgs_mesh_raster(V, F, p(v), p(c) if "color" in maps else None, p(f), views, H, W, near, int(b0 == 0), p(temp), tb,
                                         row("depth", b0), row("face", b0), row("bary", b0), row("normal", b0), row("color", b0), p(seen), p(stats),
                                         _stream(dev)), "envgs_mesh_raster")
    if seen is not None:
        maps["seen"] = seen
    return SimpleNamespace(**maps)


def render_mesh(mesh, cameras, size=None, near=0.0, outputs=("depth", "face", "normal", "color")):
    """The mesh through cameras: a triangle z-buffer, exact to the bit (include/envgs_mesh.h, "rasterisation"; tests/mesh_raster_oracle.py restates
    the rule).  cameras: namespaces with K (3,3), R (3,3) world -> camera and T (3,), as cull_to_masks() takes them; size: (H, W), default the
    cameras' image_height / image_width, which must agree; near: a corner is usable only with zc > near.  outputs, any of:
        depth  (n,H,W) f32    the z of the nearest face under the pixel's centre, 0 where none
        face   (n,H,W) i32    its index (of equal depths the lowest), -1 where none
        bary   (n,H,W,3) f32  perspective-correct barycentric coordinates, in the order of the face's corners
        normal (n,H,W,3) f32  the face's unit normal in WORLD space, oriented towards the camera whatever the winding
        color  (n,H,W,3) f32  the vertex colours interpolated with bary; ignored for a mesh without colours
        seen   (F,) u8        1 iff the face wins a pixel of some view
    What is not asked for is neither computed nor written.  Both windings are drawn; a face with an index outside [0, V), a corner that is not
    finite or not beyond `near`, or zero area on the screen is dropped whole.  DEVIATION from a graphics pipeline: there is NO CLIPPING -- a face
    that crosses the camera plane is not drawn at all (its visible part is missing), so keep `near` small and the mesh in front of the cameras.
    PARITY UNPINNED: the reference renders meshes only through its OpenGL viewer.
    -> namespace of device tensors.  Views go to the device 8 per launch; no host sync; two calls give identical bytes."""
    return _raster(mesh, cameras, size, near, outputs, "render_mesh")


def visible_faces(mesh, cameras, size=None, near=0.0):
    """(F,) bool device tensor: the faces that win at least one pixel of at least one camera under render_mesh()'s rule.  No maps are written; no
    host sync."""
    return _raster(mesh, cameras, size, near, ("seen",), "visible_faces").seen.view(torch.bool)


def cull_unseen(mesh, cameras, size=None, near=0.0, return_index=False):
    """Drops the faces no camera sees -- inner shells, back sides that were never observed -- and the vertices only they name:
    select_faces(mesh, visible_faces(...)), so the order is preserved and the vertices are compacted as clean() does.
    -> Mesh, or (Mesh, vertex_index) with return_index.  One host sync: that of select_faces()."""
    return select_faces(mesh, visible_faces(mesh, cameras, size, near), return_index=return_index)


def _triple(x, what):
    x = [_f32(v) for v in x]
    if len(x) != 3:
        raise ValueError("%s: three numbers are required" % what)
    return x


def in_box(points, lo, hi):
    """(N,) bool: lo <= p < hi on every axis (fp32 compares; a row that is not finite is False)."""
    points = _points_tensor(points, "in_box")
    lo = torch.tensor(_triple(lo, "in_box"), dtype=torch.float32, device=points.device)
    hi = torch.tensor(_triple(hi, "in_box"), dtype=torch.float32, device=points.device)
    return ((points >= lo) & (points < hi) & torch.isfinite(points)).all(dim=1)


def in_volume(points, volume, origin, voxel_size):
    """(N,) bool: the DTU observation mask.  volume: (nx,ny,nz) bool or uint8 device tensor indexed [gx, gy, gz]; g = rint((p - origin) / voxel_size)
    per axis in fp32, ties to even (what np.around and torch.round both do); inside iff 0 <= g < dims on every axis and volume[g] != 0.  A row
    that is not finite is False."""
    points = _points_tensor(points, "in_volume")
    _need_gpu(volume, "in_volume")
    if volume.dim() != 3 or volume.dtype not in (torch.bool, torch.uint8) or volume.device != points.device:
        raise ValueError("in_volume: volume must be a (nx,ny,nz) bool or uint8 tensor on the points' device")
    voxel = _f32(voxel_size)
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError("in_volume: voxel_size must be positive and finite")
    o = torch.tensor(_triple(origin, "in_volume"), dtype=torch.float32, device=points.device)
    dims = torch.tensor(list(volume.shape), dtype=torch.float32, device=points.device)
    # the divisor is a device tensor: torch turns a division by a host scalar into a product with its reciprocal, which rounds differently
    g = torch.round((points - o) / torch.full((1,), voxel, dtype=torch.float32, device=points.device))
    ok = ((g >= 0) & (g < dims) & torch.isfinite(points)).all(dim=1)          # decided on the floats, before any conversion
    gi = torch.where(ok[:, None], g, torch.zeros((), dtype=torch.float32, device=points.device)).long()
    return ok & (volume[gi[:, 0], gi[:, 1], gi[:, 2]] != 0)


def above_plane(points, plane):
    """(N,) bool: ((a x + b y) + c z) + d > 0 for plane = (a, b, c, d), every product and sum a separate fp32 operation.  A row that is not finite
    is False."""
    points = _points_tensor(points, "above_plane")
    plane = [_f32(v) for v in plane]
    if len(plane) != 4:
        raise ValueError("above_plane: plane must be (a, b, c, d)")
    a, b, c, d = plane
    s = points[:, 0] * a
    s = s + points[:, 1] * b
    s = s + points[:, 2] * c
    s = s + d
    return (s > 0) & torch.isfinite(points).all(dim=1)


def evaluate_dtu(mesh_or_points, scan_points, radius, max_distance, density=None, seed=0, observed=None, box=None, plane=None, threshold=None):
    """The DTU evaluation protocol on the device.  The prediction -- a Mesh sampled at `density`, or a (N,3) point tensor -- is thinned at `radius`
    with `seed` (thin_points), then filtered:
      data_in   the thinned points inside box = (lo, hi) (in_box);   data_obs  those of data_in inside observed = (volume, origin, voxel_size) (in_volume)
      accuracy      mean nearest distance from data_obs to ALL scan points, over the points found within max_distance
      completeness  the same from the scan points above plane = (a, b, c, d) (above_plane) to data_in;   chamfer  the mean of the two
    A filter that is None is skipped.  Also returned: the counts n_samples (before thinning), n_thinned, n_in, n_pred (data_obs), n_scan, n_ref (scan
    above the plane), found_pred, found_ref, thin_rounds, and the distances d_pred (n_pred,), d_ref (n_ref,) as evaluate() gives them.  With
    `threshold` (<= max_distance): within_pred, within_ref, precision, recall and fscore over the same two sets, by evaluate()'s rules.
    seed=None thins in the given order (a mesh is then sampled with seed 0).
    Stated deviations from the DTU script: random area-proportional surface samples in place of its per-triangle lattice plus the vertices;
    d <= max_distance where the script has <; a hash order in place of NumPy's shuffle.  The scan is taken as given (the DTU scans are thinned
    already); thin it with thin_points() if it is not."""
    max_distance = float(max_distance)
    if threshold is not None:
        threshold = float(threshold)
        if not 0.0 <= threshold <= max_distance:
            raise ValueError("evaluate_dtu: 0 <= threshold <= max_distance is required")
    pred = _eval_points(mesh_or_points, density, 0 if seed is None else seed, "evaluate_dtu")
    scan = _points_tensor(scan_points, "evaluate_dtu")
    if pred.device != scan.device:
        raise ValueError("evaluate_dtu: the prediction and the scan must be on one device")
    keep, rounds = _thin(pred, radius, seed, None, THIN_GROUP, None)
    thinned = pred[keep]
    data_in = thinned if box is None else thinned[in_box(thinned, box[0], box[1])]
    data_obs = data_in if observed is None else data_in[in_volume(data_in, observed[0], observed[1], observed[2])]
    ref = scan if plane is None else scan[above_plane(scan, plane)]
    d_pred = torch.sqrt(PointGrid(scan, max_distance).nearest(data_obs.contiguous())[0].double())
    d_ref = torch.sqrt(PointGrid(data_in.contiguous(), max_distance).nearest(ref.contiguous())[0].double())
    rows = []
    for d in (d_pred, d_ref):
        found = torch.isfinite(d)
        rows += [torch.where(found, d, torch.zeros((), dtype=torch.float64, device=d.device)).sum(), found.sum().double(),
                 (d <= (max_distance if threshold is None else threshold)).sum().double()]
    sum_p, found_p, within_p, sum_r, found_r, within_r = torch.stack(rows).tolist()
    accuracy = sum_p / found_p if found_p else float("nan")
    completeness = sum_r / found_r if found_r else float("nan")
    out = SimpleNamespace(accuracy=accuracy, completeness=completeness, chamfer=0.5 * (accuracy + completeness), n_samples=pred.shape[0],
                          n_thinned=thinned.shape[0], n_in=data_in.shape[0], n_pred=data_obs.shape[0], n_scan=scan.shape[0], n_ref=ref.shape[0],
                          found_pred=int(found_p), found_ref=int(found_r), thin_rounds=rounds, d_pred=d_pred, d_ref=d_ref)
    if threshold is not None:
        out.precision = within_p / out.n_pred if out.n_pred else 0.0
        out.recall = within_r / out.n_ref if out.n_ref else 0.0
        out.fscore = 2.0 * out.precision * out.recall / (out.precision + out.recall) if out.precision + out.recall > 0.0 else 0.0
        out.within_pred, out.within_ref = int(within_p), int(within_r)
    return out


# ---- registration and the Tanks-and-Temples protocol (csrc/mesh_register.hip; include/envgs_mesh.h, "registration") ------------------------------------
REGISTER_SUMS, VOXEL_MAX_DIM, POLYGON_MAX = 18, 2 ** 21, 256     # ENVGS_REGISTER_SUMS, ENVGS_VOXEL_MAX_DIM, ENVGS_POLYGON_MAX


def _transformation(T, what):
    """-> (4,4) float64 NumPy copy of a 4x4 or 3x4 transformation (the last row of a 3x4 is 0 0 0 1), checked finite."""
    if isinstance(T, torch.Tensor):
        T = T.detach().cpu().numpy()
    T = np.array(T, dtype=np.float64)
    if T.shape == (3, 4):
        T = np.vstack([T, [0.0, 0.0, 0.0, 1.0]])
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("%s: the transformation must be a finite 4x4 or 3x4 matrix" % what)
    return T


def _rigid_rows(T):
    """The upper 3x4 of T, each entry rounded once to fp32, as the host array the C-ABI takes (and the owner that keeps it alive)."""
    with np.errstate(over="ignore"):
        m = np.ascontiguousarray(T[:3, :4], dtype=np.float32).reshape(12)
    if not np.isfinite(m).all():
        raise ValueError("the transformation does not fit fp32")
    return m.ctypes.data_as(_lib.ctypes.POINTER(_lib.ctypes.c_float)), m


def transform_points(points, T):
    """(N,3) f32: x' = ((M00 x + M01 y) + M02 z) + M03 and likewise y', z' in fp32 without FMA, M the upper 3x4 of T (4x4 or 3x4, float64, on the
    host) with each entry rounded once to fp32.  A row that is not finite stays not finite.  The device function is the one register() calls.
    No host sync."""
    points = _points_tensor(points, "transform_points")
    m, owner = _rigid_rows(_transformation(T, "transform_points"))
    out = torch.empty(points.shape[0], 3, dtype=torch.float32, device=points.device)
    _lib.check(_lib.load().envgs_points_transform(points.shape[0], _lib.ptr(points), m, _lib.ptr(out), _stream(points.device)), "envgs_points_transform")
    del owner
    return out


def rigid_from_sums(sums, with_scale=False, center=None):
    """The least-squares rigid (or, with_scale, similarity) transformation of the matched pairs behind the 18 sums of one registration iteration
    (include/envgs_mesh.h, "registration", rules 2 and 3): n, sum d2, sum ah (3), sum bh (3), sum ah bh^T (9, row major), sum |ah|^2, with ah, bh
    the moved source point and its match less `center`.  A pure float64 function of its arguments: no GPU, no library.
      am = sum ah / n, bm = sum bh / n;   H = sum ah bh^T - n am bm^T;   U S V^T = svd(H)
      R = V diag(1, 1, d) U^T with d = +1 or -1, the sign of det(V U^T) (never a reflection);   s = tr(S diag(1, 1, d)) / (sum |ah|^2 - n |am|^2)
      or 1;   t = bm - s R am;   the result maps x to s R x + (c + t - s R c), c = center (None: the origin).
    -> (4,4) float64.  Raises ValueError for n < 3, for sums that are not finite, and with_scale for a denominator that is not positive.  A planar or
    collinear cloud is no error: the rotation is then the proper one of least angle among the minimisers the SVD offers."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1)
    if s.shape[0] != REGISTER_SUMS:
        raise ValueError("rigid_from_sums: 18 sums are required")
    if not np.isfinite(s).all():
        raise ValueError("rigid_from_sums: the sums are not finite")
    n = s[0]
    if not n >= 3:
        raise ValueError("rigid_from_sums: fewer than 3 pairs")
    c = np.zeros(3) if center is None else np.asarray(center, dtype=np.float64).reshape(3)
    am, bm = s[2:5] / n, s[5:8] / n
    H = s[8:17].reshape(3, 3) - n * np.outer(am, bm)
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) >= 0.0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    scale = 1.0
    if with_scale:
        den = s[17] - n * float(am @ am)
        if not den > 0.0:
            raise ValueError("rigid_from_sums: the source pairs have no extent, the scale is undefined")
        scale = (S[0] + S[1] + d * S[2]) / den
    sR = scale * R
    out = np.eye(4)
    out[:3, :3] = sR
    out[:3, 3] = c + (bm - sR @ am) - sR @ c
    return out


def register_sums(source, grid, T, return_rows=False):
    """One evaluation of a transformation T (4x4 or 3x4, float64, host) against a PointGrid: every source row is moved by transform_points' rule, its
    nearest target point within grid.max_distance found by PointGrid.nearest's rule, and the 18 sums of rigid_from_sums reduced in a fixed order
    (include/envgs_mesh.h), with c = grid.center, the centre of the box of the finite target points.  -> sums (18,) float64 NumPy, on the host: the
    one sync; with return_rows also (moved (Q,3) f32, dist2 (Q,) f32, index (Q,) i32) on the device -- what transform_points and
    grid.nearest(moved) give."""
    source = _points_tensor(source, "register_sums")
    if source.device != grid.device:
        raise ValueError("register_sums: the source must be on the grid's device")
    m, owner = _rigid_rows(_transformation(T, "register_sums"))
    lib = _lib.load()
    dev, Q = grid.device, source.shape[0]
    tb = lib.envgs_points_register_temp_bytes(Q)
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    sums = torch.empty(REGISTER_SUMS, dtype=torch.float64, device=dev)
    moved = torch.empty(Q, 3, dtype=torch.float32, device=dev) if return_rows else None
    dist2 = torch.empty(Q, dtype=torch.float32, device=dev) if return_rows else None
    index = torch.empty(Q, dtype=torch.int32, device=dev) if return_rows else None
    nx, ny, nz = grid.dims
    p = _lib.ptr
    center = (_lib.ctypes.c_double * 3)(*grid.center)
    _lib.check(lib.envgs_points_register_sums(Q, p(source), m, grid.max_distance, grid.origin[0], grid.origin[1], grid.origin[2], grid.cell_size, nx, ny, nz,
                                              p(grid.cell_end), p(grid.records), center, p(temp), tb, p(sums), p(moved), p(dist2), p(index), _stream(dev)),
               "envgs_points_register_sums")
    del owner
    host = sums.cpu().numpy()
    return (host, moved, dist2, index) if return_rows else host


def register(source, target_or_grid, max_distance, init=None, with_scale=False, max_iterations=20, rel_fitness=1e-6, rel_rmse=1e-6, cell_size=None):
    """Point-to-point ICP of source (N,3) onto a target -- a (M,3) point tensor, or a PointGrid built over one with this max_distance, so that several
    calls can share it.  T_0 = init (4x4 or 3x4; None: the identity).  Iteration k evaluates T_k (register_sums: ONE kernel over the source plus a
    fixed-order reduction, then one read-back of 18 doubles -- one host sync per iteration): fitness_k = n / N over ALL source rows, inlier_rmse_k =
    sqrt(sum d2 / n).  It stops as CONVERGED when |fitness_k - fitness_{k-1}| < rel_fitness and |rmse_k - rmse_{k-1}| < rel_rmse; as not converged
    when n < 3, when with_scale the source pairs have no extent, or after max_iterations updates; otherwise T_{k+1} = rigid_from_sums(sums_k) T_k in
    float64.  The source is always moved from its original coordinates by the total transformation, never incrementally.
    The search is exact and the sums are reduced in an order that depends on N alone, so the same inputs give the same transformation to the bit, from
    run to run and at every cell_size (None: PointGrid's default).
    -> namespace(transformation (4,4) float64 NumPy: the last T_k evaluated, fitness, inlier_rmse, iterations: the updates applied, converged,
    center: the c of the sums, history: [namespace(transformation T_k, sums (18,), fitness, inlier_rmse)] one per evaluation)."""
    source = _points_tensor(source, "register")
    if isinstance(target_or_grid, PointGrid):
        grid = target_or_grid
        if _f32(grid.max_distance) != _f32(max_distance):
            raise ValueError("register: the grid was built for max_distance %r, not %r" % (grid.max_distance, max_distance))
    else:
        grid = PointGrid(target_or_grid, max_distance, cell_size)
    T = np.eye(4) if init is None else _transformation(init, "register")
    max_iterations = int(max_iterations)
    N = source.shape[0]
    center = np.array(grid.center, dtype=np.float64)
    history, converged, updates = [], False, 0
    while True:
        sums = register_sums(source, grid, T)
        n = int(sums[0])
        fitness = n / N if N else 0.0
        rmse = math.sqrt(sums[1] / n) if n else 0.0
        history.append(SimpleNamespace(transformation=T.copy(), sums=sums, fitness=fitness, inlier_rmse=rmse))
        if len(history) > 1 and abs(fitness - history[-2].fitness) < rel_fitness and abs(rmse - history[-2].inlier_rmse) < rel_rmse:
            converged = True
            break
        if n < 3 or updates >= max_iterations:
            break
        try:
            delta = rigid_from_sums(sums, with_scale, center)
        except ValueError:
            break
        T = delta @ T
        updates += 1
    return SimpleNamespace(transformation=T, fitness=fitness, inlier_rmse=rmse, iterations=updates, converged=converged, center=center, history=history)


def voxel_grid(points, voxel_size, origin=None):
    """The grid voxel_downsample() uses: -> (origin, dims), as simplify_grid sizes its own (origin None: the per-axis minimum of the finite rows;
    dims[a] = floor(extent[a] / voxel_size) + 1), with up to 2^21 cells per axis and no bound on their product.  Raises ValueError beyond that,
    naming the smallest admissible voxel_size.  One host sync: the extrema (a second one when some row is not finite)."""
    points = _points_tensor(points, "voxel_downsample")
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and math.isfinite(voxel_size)) or not 0.0 < _f32(voxel_size) < float("inf"):
        raise ValueError("voxel_downsample: voxel_size must be positive and finite")
    lo, hi = _finite_extent(points)
    if origin is not None:
        lo = [float(o) for o in origin]
        if len(lo) != 3 or not all(math.isfinite(o) for o in lo):
            raise ValueError("voxel_downsample: origin must be three finite numbers")
    extent = [h - l for l, h in zip(lo, hi)]
    admissible = lambda c: max(_grid_dims(extent, c)) <= VOXEL_MAX_DIM
    if not admissible(voxel_size):
        bad, good = voxel_size, 2.0 * voxel_size
        while not admissible(good):
            bad, good = good, 2.0 * good
        for _ in range(60):
            mid = 0.5 * (bad + good)
            bad, good = (bad, mid) if admissible(mid) else (mid, good)
        raise ValueError("voxel_downsample: voxel_size %g gives %s cells, beyond 2^21 per axis; the smallest admissible voxel_size here is %r"
                         % (voxel_size, _grid_dims(extent, voxel_size), good))
    return tuple(lo), tuple(_grid_dims(extent, voxel_size))


def voxel_downsample(points, voxel_size, origin=None, return_index=False):
    """One point per occupied voxel: the sparse form of simplify()'s clustering (include/envgs_mesh.h, "registration", rule 4), for grids far beyond
    2^31 cells.  The cell of a point is rule 1 of the simplification on the grid of voxel_grid(); the clusters are the occupied cells by ascending key
    i | j << 21 | k << 42 (the simplification's own order, x fastest); the representative is its rule 3, word for word: a single member keeps its
    bits, otherwise the rounded mean of 64-bit integer sums in steps of 2^-20 of a cell.  The result depends on no order: two runs and two
    permutations of the input give identical bytes.  Rows that are not finite belong to no cluster.
    -> (C,3) f32, with return_index also cluster (N,) i32 (-1 = none).  The keys are sorted by torch.sort; everything else is HIP.  Host syncs: those
    of voxel_grid, and the read-back of C."""
    points = _points_tensor(points, "voxel_downsample")
    (ox, oy, oz), (nx, ny, nz) = voxel_grid(points, voxel_size, origin)
    lib = _lib.load()
    dev, N = points.device, points.shape[0]
    cell = float(voxel_size)
    p, s = _lib.ptr, _stream(dev)
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    _lib.check(lib.envgs_points_voxel_keys(N, p(points), ox, oy, oz, cell, nx, ny, nz, p(keys), s), "envgs_points_voxel_keys")
    sorted_keys, order = torch.sort(keys)
    tb = lib.envgs_points_voxel_temp_bytes(N)
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    cluster = torch.empty(N, dtype=torch.int32, device=dev) if return_index else None
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(lib.envgs_points_voxel_cluster(N, p(points), ox, oy, oz, cell, nx, ny, nz, p(sorted_keys), p(order), p(temp), tb, p(cluster), p(count), s),
               "envgs_points_voxel_cluster")
    C = int(count.item())
    out = torch.empty(C, 3, dtype=torch.float32, device=dev)
    _lib.check(lib.envgs_points_voxel_finish(N, p(points), ox, oy, oz, cell, nx, ny, nz, p(temp), tb, C, p(out), s), "envgs_points_voxel_finish")
    return (out, cluster) if return_index else out


_AXES = {"X": 0, "Y": 1, "Z": 2}


def in_polygon_volume(points, axis, axis_min, axis_max, polygon):
    """(N,) bool: the crop volume of the Tanks-and-Temples toolbox, Open3D's SelectionPolygonVolume.  axis "X", "Y" or "Z" is the orthogonal axis w;
    (u, v) = (1, 2), (0, 2), (0, 1); polygon (M,3), 3 <= M <= 256.  A finite point is inside iff axis_min <= p[w] <= axis_max and the number of
    edges (j, j+1 mod M) with (v_j > p_v) != (v_k > p_v) and p_u < (u_k - u_j) * (p_v - v_j) / (v_k - v_j) + u_j is odd, evaluated in double as
    written on the fp32 point and the float64 polygon.  A row that is not finite is False.  No host sync."""
    points = _points_tensor(points, "in_polygon_volume")
    if axis not in _AXES:
        raise ValueError("in_polygon_volume: axis must be 'X', 'Y' or 'Z'")
    poly = np.asarray(polygon.detach().cpu().numpy() if isinstance(polygon, torch.Tensor) else polygon, dtype=np.float64)
    if poly.ndim != 2 or poly.shape[1] != 3 or not 3 <= poly.shape[0] <= POLYGON_MAX or not np.isfinite(poly).all():
        raise ValueError("in_polygon_volume: polygon must be a finite (M,3) array, 3 <= M <= 256")
    axis_min, axis_max = float(axis_min), float(axis_max)
    if math.isnan(axis_min) or math.isnan(axis_max):
        raise ValueError("in_polygon_volume: axis_min and axis_max must be numbers")
    dev = points.device
    poly_dev = torch.from_numpy(np.ascontiguousarray(poly)).to(dev)
    inside = torch.empty(points.shape[0], dtype=torch.bool, device=dev)
    _lib.check(_lib.load().envgs_points_in_polygon(points.shape[0], _lib.ptr(points), _AXES[axis], axis_min, axis_max, poly.shape[0], _lib.ptr(poly_dev),
                                                   _lib.ptr(inside), _stream(dev)), "envgs_points_in_polygon")
    return inside


def load_crop_volume(path):
    """Reads an Open3D SelectionPolygonVolume JSON (the crop files of Tanks and Temples): -> namespace(axis "X" / "Y" / "Z", axis_min, axis_max,
    polygon (M,3) float64 NumPy), the arguments of in_polygon_volume()."""
    import json
    with open(path) as f:
        d = json.load(f)
    polygon = np.asarray(d["bounding_polygon"], dtype=np.float64).reshape(-1, 3)
    axis = str(d["orthogonal_axis"]).upper()
    if axis not in _AXES:
        raise ValueError("load_crop_volume: orthogonal_axis %r is not X, Y or Z" % d["orthogonal_axis"])
    return SimpleNamespace(axis=axis, axis_min=float(d["axis_min"]), axis_max=float(d["axis_max"]), polygon=polygon)


def _crop(points, crop):
    if crop is None:
        return points
    return points[in_polygon_volume(points, crop.axis, crop.axis_min, crop.axis_max, crop.polygon)].contiguous()


def evaluate_tnt(mesh_or_points, scan_points, tau, init=None, crop=None, density=None, seed=0, max_points=4_000_000):
    """The Tanks-and-Temples evaluation on the device, by the schedule of the toolbox's run.py.  The prediction -- a Mesh sampled at `density` with
    `seed`, or a (N,3) point tensor -- is brought into the scan's frame by `init` (4x4; None: the identity) and three ICP refinements, then scored at
    the distance tau.  crop: a namespace as load_crop_volume() gives (axis, axis_min, axis_max, polygon), or None for no crop.  With T = init:
      1. the prediction moved by T and cropped, the scan cropped, both down-sampled at voxel tau (voxel_downsample);  register() with
         max_distance 80 tau and 20 iterations from the identity gives D;  T = D T
      2. the same at voxel tau / 2 with max_distance 20 tau
      3. every k-th row of each cloud, k the smallest that leaves at most max_points rows, the prediction moved by T, both cropped;
         max_distance 2 tau
      4. the prediction moved by the final T and cropped, it and the cropped scan down-sampled at voxel tau / 2;
         evaluate(prediction, scan, max_distance=tau, threshold=tau)
    -> the namespace of evaluate() (precision, recall, fscore at tau; accuracy, completeness, ...) plus transformation (4,4) float64, the total T, and
    registrations: the three register() results.  Every step is deterministic, so two runs give identical numbers.
    Stated deviations from the toolbox: d <= tau and d <= max_distance where it has <; the canonical voxel means of voxel_downsample() in place of
    Open3D's hash-ordered float means; no RANSAC / trajectory alignment -- the caller supplies `init`; no histogram plots."""
    tau = float(tau)
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError("evaluate_tnt: tau must be positive and finite")
    max_points = int(max_points)
    if max_points < 1:
        raise ValueError("evaluate_tnt: max_points must be at least 1")
    pred = _eval_points(mesh_or_points, density, seed, "evaluate_tnt")
    scan = _points_tensor(scan_points, "evaluate_tnt")
    if pred.device != scan.device:
        raise ValueError("evaluate_tnt: the prediction and the scan must be on one device")
    T = np.eye(4) if init is None else _transformation(init, "evaluate_tnt")
    scan_cropped = _crop(scan, crop)
    registrations = []
    for voxel, reach in ((tau, 80.0 * tau), (0.5 * tau, 20.0 * tau)):
        source = voxel_downsample(_crop(transform_points(pred, T), crop), voxel)
        target = voxel_downsample(scan_cropped, voxel)
        registrations.append(register(source, target, reach, max_iterations=20))
        T = registrations[-1].transformation @ T
    every = lambda t: t[::max(1, -(-t.shape[0] // max_points))].contiguous()
    source = _crop(transform_points(every(pred), T), crop)
    registrations.append(register(source, _crop(every(scan), crop), 2.0 * tau, max_iterations=20))
    T = registrations[-1].transformation @ T
    moved = voxel_downsample(_crop(transform_points(pred, T), crop), 0.5 * tau)
    out = evaluate(moved, voxel_downsample(scan_cropped, 0.5 * tau), max_distance=tau, threshold=tau)
    out.transformation, out.registrations = T, registrations
    return out


# ---- depth fusion (csrc/mesh_fuse.hip; include/envgs_mesh.h, "depth fusion") ----------------------------------------------------------------------------
# PARITY PINNED by tests/golden/fuse_golden.npz: the second route from a trained scene to a point cloud, the reference's scripts/fusion/depth_fusion.py
# (fusion_utils.py: depth_reprojection, depth_geometry_consistency, compute_consistency).  No voxel size and no iso-surface: every view's depth is checked
# against its nearest views, the agreeing depths are averaged and the surviving pixels are back-projected.
FUSE_MAX_SOURCES = 255        # the count is a byte


def _fuse_cameras(cameras, what):
    """-> (K, R, T) float64 arrays (V,3,3), (V,3,3), (V,3) on the host."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("%s: at least one camera is needed" % what)
    host = lambda name, shape: torch.stack([torch.as_tensor(getattr(c, name)).reshape(shape) for c in cameras]).detach().cpu().double().numpy()
    K, R, T = host("K", (3, 3)), host("R", (3, 3)), host("T", (3,))                  # one copy per attribute, not per camera
    if not (np.isfinite(K).all() and np.isfinite(R).all() and np.isfinite(T).all()):
        raise ValueError("%s: camera parameters must be finite" % what)
    return K, R, T


def nearest_views(cameras, n):
    """For each camera the min(n, V - 1) OTHER cameras by ascending distance between the centres -R^T T, in float64 on the host; ties go to the
    lowest index.  -> (V, min(n, V-1)) int64 (host).  For rigs with distinct centres this is the reference's
    compute_camera_similarity(c2ws, c2ws)[1][:, 1:1+n].  Deviation: with coincident centres the reference's sort of 1 / distance sees several
    infinities and its [1:] may drop a camera other than the view itself; here the view itself is always the one left out."""
    _, R, T = _fuse_cameras(cameras, "nearest_views")
    V, n = R.shape[0], int(n)
    if n < 0:
        raise ValueError("nearest_views: n must not be negative")
    C = -np.einsum("vji,vj->vi", R, T)
    d = np.linalg.norm(C[:, None, :] - C[None, :, :], axis=-1)
    out = np.empty((V, min(n, V - 1)), np.int64)
    for v in range(V):
        order = [j for j in np.argsort(d[v], kind="stable") if j != v]
        out[v] = order[:out.shape[1]]
    return torch.from_numpy(out)


def fuse_min_count(geo_sum_thresh, S):
    """The smallest integer n with n >= geo_sum_thresh * S in Python float arithmetic: the reference's `geo_mask_sum >= geo_sum_thresh * S`."""
    return max(0, math.ceil(float(geo_sum_thresh) * S))         # math.ceil of a float is exact


def fuse_view_maps(K, R, T):
    """(V,12) float64: A_v = R_v^T K_v^-1 row major, then c_v = -R_v^T T_v (rule 5)."""
    Rt = np.swapaxes(R, -1, -2)
    return np.concatenate([(Rt @ np.linalg.inv(K)).reshape(-1, 9), -(Rt @ T[..., None])[..., 0]], axis=-1)


def fuse_pair_maps(K, R, T, sources):
    """The two affine maps of include/envgs_mesh.h ("depth fusion", rule 1) for every (view r, source s = sources[r, k]) of a (V,S) table, composed
    in float64: fwd carries a pixel and depth of r into the image of s, back the other way.  -> (fwd, back), (V,S,12) each: A row major, then b."""
    Kinv = np.linalg.inv(K)
    Ks, Ts, Kis, col = K[sources], T[sources], Kinv[sources], lambda a: a[..., None]         # (V,S,...)
    Rab = R[sources] @ np.swapaxes(R, -1, -2)[:, None]                                        # R_s R_r^T
    Rba = np.swapaxes(Rab, -1, -2)
    fwd_A = Ks @ Rab @ Kinv[:, None]
    fwd_b = (Ks @ col(Ts - (Rab @ col(T[:, None]))[..., 0]))[..., 0]
    back_A = K[:, None] @ Rba @ Kis
    back_b = (K[:, None] @ col(T[:, None] - (Rba @ col(Ts))[..., 0]))[..., 0]
    V, S = sources.shape
    return np.concatenate([fwd_A.reshape(V, S, 9), fwd_b], axis=-1), np.concatenate([back_A.reshape(V, S, 9), back_b], axis=-1)


_FUSE_SOURCE_DT = np.dtype([("depth", "<u8"), ("H", "<i4"), ("W", "<i4"), ("fwd", "<f4", (12,)), ("back", "<f4", (12,))])
_FUSE_SOURCES_DT = np.dtype([("count", "<i4"), ("reserved0", "<i4"), ("v", _FUSE_SOURCE_DT, (MAX_VIEWS,))])


def _fuse_packs(K, R, T, src, depth_ptr, H, W):
    """The envgs_fuse_sources structs of a call, filled at once: (V, launches per view) records that _lib.FuseSources reads in place."""
    assert _FUSE_SOURCES_DT.itemsize == _lib.ctypes.sizeof(_lib.FuseSources)
    V, S = src.shape
    packs = np.zeros((V, max(1, -(-S // MAX_VIEWS))), _FUSE_SOURCES_DT)
    if S:
        fwd, back = fuse_pair_maps(K, R, T, src)
        for q in range(packs.shape[1]):
            cols = slice(q * MAX_VIEWS, min(S, (q + 1) * MAX_VIEWS))
            n = cols.stop - cols.start
            packs["count"][:, q] = n
            v = packs["v"][:, q, :n]
            v["depth"] = depth_ptr + src[:, cols].astype(np.uint64) * np.uint64(4 * H * W)
            v["H"], v["W"] = H, W
            v["fwd"], v["back"] = fwd[:, cols], back[:, cols]
    return packs


def _fuse_thresholds(geo_abs_thresh, geo_rel_thresh, geo_sum_thresh, pho_abs_thresh, what):
    th = [float(geo_abs_thresh), float(geo_rel_thresh), float(geo_sum_thresh), float(pho_abs_thresh)]
    if not all(math.isfinite(t) and math.isfinite(_f32(t)) for t in th):
        raise ValueError("%s: the thresholds must be finite" % what)
    return th


def _fuse_depth(depth, n_cameras, what):
    """Shape, dtype and size first, the device last.  A list of (H,W) maps is stacked, if they share one size."""
    if isinstance(depth, (list, tuple)):
        if not depth or not all(isinstance(d, torch.Tensor) and d.dim() == 2 for d in depth):
            raise ValueError("%s: depth must be a (V,H,W) float32 tensor or a list of (H,W) maps" % what)
        if len({tuple(d.shape) for d in depth}) != 1:
            raise ValueError("%s: all views of a call must share one size" % what)
        depth = torch.stack(list(depth))
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or depth.dim() != 3:
        raise ValueError("%s: depth must be a (V,H,W) float32 tensor; all views of a call share one size" % what)
    V, H, W = depth.shape
    if V != n_cameras or H < 1 or W < 1:
        raise ValueError("%s: depth must hold one non-empty (H,W) map per camera" % what)
    if V * H * W >= 2 ** 31:
        raise ValueError("%s: V H W must be below 2^31" % what)
    return depth


def _fuse_sources(sources, V, what):
    src = np.asarray(sources.detach().cpu().numpy() if isinstance(sources, torch.Tensor) else sources)
    if src.size == 0:
        src = np.zeros((V, 0), np.int64)
    if src.ndim != 2 or src.shape[0] != V or src.dtype.kind not in "iu":
        raise ValueError("%s: sources must be a (V,S) table of view indices" % what)
    if src.shape[1] > FUSE_MAX_SOURCES:
        raise ValueError("%s: at most %d sources per view" % (what, FUSE_MAX_SOURCES))
    src = src.astype(np.int64)
    if ((src < 0) | (src >= V)).any():
        raise ValueError("%s: a source index is out of range" % what)
    if (src == np.arange(V)[:, None]).any():
        raise ValueError("%s: a view cannot be its own source" % what)
    return src


def _consistency(depth, cameras, sources, n_srcs, geo_abs_thresh, geo_rel_thresh, geo_sum_thresh, pho_abs_thresh, what):
    cameras = list(cameras)
    K, R, T = _fuse_cameras(cameras, what)
    depth = _fuse_depth(depth, len(cameras), what)
    V, H, W = depth.shape
    abs_t, rel_t, sum_t, pho_t = _fuse_thresholds(geo_abs_thresh, geo_rel_thresh, geo_sum_thresh, pho_abs_thresh, what)
    src = _fuse_sources(nearest_views(cameras, n_srcs) if sources is None else sources, V, what)
    S = src.shape[1]
    if depth.device.type != "cuda":
        raise ValueError("%s: depth must be on the GPU; there is no CPU path" % what)
    depth = depth.contiguous()
    lib = _lib.load()
    dev, p, s = depth.device, _lib.ptr, _stream(depth.device)
    count = torch.empty(V, H, W, dtype=torch.uint8, device=dev)
    total = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    packs = _fuse_packs(K, R, T, src, depth.data_ptr(), H, W)
    for r in range(V):
        for q in range(packs.shape[1]):
            pack = _lib.FuseSources.from_buffer(packs[r, q:q + 1])
            _lib.check(lib.envgs_fuse_consistency(H, W, p(depth[r]), pack, abs_t, rel_t, int(q > 0), p(count[r]), p(total[r]), s),
                       "envgs_fuse_consistency")
    min_count = fuse_min_count(sum_t, S)
    tb = lib.envgs_fuse_temp_bytes(V, H, W)
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    depth_avg = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    final = torch.empty(V, H, W, dtype=torch.bool, device=dev)
    n = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.check(lib.envgs_fuse_count(V, H, W, p(depth), p(count), p(total), min(min_count, 2 ** 32 - 1), pho_t, p(depth_avg), p(final), p(temp), tb, p(n), s),
               "envgs_fuse_count")
    out = SimpleNamespace(depth_avg=depth_avg, count=count, photo_mask=None, geo_mask=None, final_mask=final)
    return out, SimpleNamespace(depth=depth, K=K, R=R, T=T, temp=temp, tb=tb, n=n, min_count=min_count, pho=pho_t)


def depth_consistency(depth, cameras, sources=None, n_srcs=4, geo_abs_thresh=1.0, geo_rel_thresh=0.01, geo_sum_thresh=0.75, pho_abs_thresh=0.0):
    """The multi-view consistency check of the reference's depth fusion (include/envgs_mesh.h, "depth fusion"; the defaults are those of
    scripts/fusion/depth_fusion.py).  depth: (V,H,W) float32 device tensor of z-depths, <= 0 = no depth; cameras: V namespaces with K (3,3),
    R (3,3) world -> camera and T (synth.make_camera); sources: a (V,S) index tensor or list of lists, S <= 255, default nearest_views(cameras,
    n_srcs).  Each pixel of each view is projected into its sources with its depth, the source depth is sampled there as grid_sample does
    (bilinear, border) and brought back; a source agrees iff the pixel returns within geo_abs_thresh pixels, the returned depth is within
    geo_rel_thresh relative and the sample is positive.
    -> namespace(depth_avg (V,H,W) f32: the mean of the pixel's depth and the agreeing returned depths; count (V,H,W) u8: the agreeing sources;
       geo_mask: count >= geo_sum_thresh S; photo_mask: depth > pho_abs_thresh; final_mask: both), the masks bool.
    S = 0 gives depth_avg = depth and geo_mask all true, as the reference's expressions do.  All views share one size.  A pixel whose depth is not
    finite or not positive agrees with nothing.  No host sync: the camera parameters are read on the host, where synth.make_camera keeps them
    (a K, R or T that lives on the device is copied, which waits for it)."""
    out, ctx = _consistency(depth, cameras, sources, n_srcs, geo_abs_thresh, geo_rel_thresh, geo_sum_thresh, pho_abs_thresh, "depth_consistency")
    if 0 < ctx.min_count <= 255:
        out.geo_mask = out.count >= ctx.min_count
    else:                                                       # nothing to reach, or more than a byte can count
        out.geo_mask = torch.full_like(out.final_mask, ctx.min_count <= 0)
    out.photo_mask = ctx.depth > _f32(ctx.pho)
    return out


def _fuse_map(t, shape, like, name, what):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.device != like.device or t.dtype != torch.float32 or tuple(t.shape) != shape:
        raise ValueError("%s: %s must be a (V,3,H,W) float32 tensor on the depth's device" % (what, name))
    return t.contiguous()


def fuse_depth_points(depth, cameras, rgb=None, normal=None, return_index=False, **thresholds):
    """depth_consistency() followed by the back-projection of the pixels of final_mask, in ascending (view, row, column) order -- the order of the
    reference's torch.cat over views of final_mask.view(-1).nonzero():  point = c_v + depth_avg (R_v^T K_v^-1 (x + 0.5, y + 0.5, 1)).
    rgb, normal: (V,3,H,W) float32 maps gathered at the kept pixels, or None.  thresholds: the keyword arguments of depth_consistency().
    -> (points (N,3), colors (N,3) or None, normals (N,3) or None), plus index (N,) int64, the flat (view H + row) W + column, with return_index.
    One host sync per call: the read-back of N (the reference's loop makes one per view)."""
    known = dict(sources=None, n_srcs=4, geo_abs_thresh=1.0, geo_rel_thresh=0.01, geo_sum_thresh=0.75, pho_abs_thresh=0.0)
    if set(thresholds) - set(known):
        raise TypeError("fuse_depth_points: unknown arguments %s" % sorted(set(thresholds) - set(known)))
    out, ctx = _consistency(depth, cameras, what="fuse_depth_points", **dict(known, **thresholds))
    V, H, W = ctx.depth.shape
    rgb = _fuse_map(rgb, (V, 3, H, W), ctx.depth, "rgb", "fuse_depth_points")
    normal = _fuse_map(normal, (V, 3, H, W), ctx.depth, "normal", "fuse_depth_points")
    dev = ctx.depth.device
    view_maps = torch.from_numpy(fuse_view_maps(ctx.K, ctx.R, ctx.T).astype(np.float32)).to(dev)
    N = int(ctx.n.item())                                       # the one host sync
    new = lambda dt: torch.empty(N, 3, dtype=dt, device=dev)
    points = new(torch.float32)
    colors = new(torch.float32) if rgb is not None else None
    normals = new(torch.float32) if normal is not None else None
    index = torch.empty(N, dtype=torch.int64, device=dev) if return_index else None
    p = _lib.ptr
    _lib.check(_lib.load().envgs_fuse_emit(V, H, W, p(out.depth_avg), p(out.final_mask), p(ctx.temp), ctx.tb, p(view_maps), p(rgb), p(normal), N,
                                           p(points), p(colors), p(normals), p(index), _stream(dev)), "envgs_fuse_emit")
    return (points, colors, normals, index) if return_index else (points, colors, normals)


def render_surface_maps(cameras, base, sh_degree, depth_ratio=0.0, scale_modifier=1.0):
    """Renders `base` from every camera as fuse_surfels() does (the same rasterizer call under no_grad) and returns the per-view maps
    [namespace(depth (H,W), alpha (H,W), rgb (3,H,W), normal (3,H,W))]: normal is the rendered normal allmap[2:5] rotated from view to world space,
    the expression of envgs_step.base_pass."""
    import diff_surfel_rasterization_wet as pkg
    _need_gpu(base["means3D"], "render_surface_maps")
    dev = base["means3D"].device
    maps = []
    with torch.no_grad():
        bg = torch.zeros(3, dtype=torch.float32, device=dev)
        for cam in cameras:
            st = pkg.GaussianRasterizationSettings(
                image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg,
                scale_modifier=scale_modifier, viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
                sh_degree=sh_degree, campos=cam.camera_center.to(dev), prefiltered=False, debug=False)
            color, _, allmap, _ = pkg.GaussianRasterizer(raster_settings=st)(
                means3D=base["means3D"], means2D=torch.zeros_like(base["means3D"]), shs=base["shs"], colors_precomp=None,
                opacities=base["opacities"], scales=base["scales"], rotations=base["rotations"], cov3D_precomp=None)
            normal = (allmap[2:5].permute(1, 2, 0) @ (cam.world_view_transform.to(dev)[:3, :3].T)).permute(2, 0, 1).contiguous()
            maps.append(SimpleNamespace(depth=surface_depth(allmap, depth_ratio), alpha=allmap[1], rgb=color[:3].contiguous(), normal=normal))
    return maps


def fuse_surfel_points(cameras, base, sh_degree, alpha_min=0.5, depth_ratio=0.0, scale_modifier=1.0, **thresholds):
    """From surfels to a fused cloud: render_surface_maps(), the depth zeroed where alpha <= alpha_min (zero is the reference's "no depth" and
    fails the photometric mask), then fuse_depth_points() with the rendered colour and normal.  All cameras must share one image size.
    -> (namespace(points, colors, normals, index), maps): the cloud goes straight into evaluate_dtu(), evaluate_tnt(), thin_points() and
    voxel_downsample(); maps are the rendered maps, with the depth as it was fused."""
    cameras = list(cameras)
    maps = render_surface_maps(cameras, base, sh_degree, depth_ratio, scale_modifier)
    if len({tuple(m.depth.shape) for m in maps}) != 1:
        raise ValueError("fuse_surfel_points: all cameras must share one image size")
    for m in maps:
        m.depth = torch.where(m.alpha > alpha_min, m.depth, torch.zeros_like(m.depth))
    points, colors, normals, index = fuse_depth_points(torch.stack([m.depth for m in maps]), cameras, rgb=torch.stack([m.rgb for m in maps]),
                                                       normal=torch.stack([m.normal for m in maps]), return_index=True, **thresholds)
    return SimpleNamespace(points=points, colors=colors, normals=normals, index=index), maps
