"""Image output on the device: the visualizer's maps as finished 8-bit RGBA (include/envgs_visualize.h, csrc/visualize.hip), an asynchronous
writer of PNG / PPM files, a driver that renders cameras through the EnvGS forward and writes the eight pictures of configs/models/envgs.yaml, and
mesh_views(), which writes the shaded-normal, depth and colour pictures of a mesh from mesh.render_mesh()'s maps through the same planes.

Semantics: the reference's VolumetricVideoVisualizer (runners/visualizers/volumetric_video_visualizer.py, generate_type :84-268) and the byte rule
of data_utils.save_image (:1230), in float32, operation by operation; tests/visualize_oracle.py states them in NumPy and
tests/golden/visualize_golden.npz holds the reference's own bytes.  The reference copies float32 RGBA to the host and quantises there; here one
launch per view writes the bytes of every plane, a quarter of the traffic, and the depth range comes from one exact radix select per image whose
result never leaves the device.

Deviations, all stated in the header: a NaN gives the byte 0; the depth range uses n = max(int(N * 0.01), 1) (the reference raises under 100
pixels); far <= near gives 1 where d <= near and 0 elsewhere (the reference divides by zero); each image of a batch is normalised on its own (the
reference ravels the batch; with B = 1, its only real use, the two agree); depth with curve="linear" stands on three channels (the reference writes
a two-channel file).

Colour maps: "linear" (the reference's default) is built in.  The reference's named maps (turbo, virdis, jet) are NOT here: their tables are the
reference's program text.  A caller passes a table of their own: depth(..., table=t) with t a (K, 3) float32 device tensor of colours at K uniform
knots -- e.g. torch.tensor(matplotlib.colormaps["turbo"](numpy.linspace(0, 1, 256))[:, :3], dtype=torch.float32, device=dev); it is evaluated by the
reference's colormap_list rule (a value exactly on an inner knot is counted by both its segments).  The table must be finite.

No video: the reference assembles .mp4 files by calling ffmpeg, which is out of scope here; ImageWriter writes image files only.
GPU tensors only: there is no CPU path."""
import ctypes
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

COLOR, GRAY, DEPTH, NORMAL, GT, ERROR = range(6)                     # ENVGS_VIS_* kinds
WEIGHT_MODES = {None: 0, "one_minus": 1, "twice": 2}                  # ENVGS_VIS_WEIGHT_*
CURVES = {"linear": 0, "normalize": 1}                               # ENVGS_VIS_CURVE_*
OPAQUE, HAS_BG = 1, 2                                                # ENVGS_VIS_OPAQUE, ENVGS_VIS_BG
MAX_PLANES, MAX_TABLE = 16, 65536
TYPES = ("RENDER", "DEPTH", "ALPHA", "NORMAL", "SURFACE_NORMAL", "SPECULAR", "DIFFUSE", "REFLECTION")      # configs/models/envgs.yaml
P_DEPTH = 0.01                                                       # normalize_depth's p


class _Map:
    """A tensor with its layout: chw(t) / hwc(t) mark one map of a plane whose other maps are laid out differently."""

    def __init__(self, t, layout):
        self.t, self.layout = t, layout


def chw(t):
    """(C, H, W) / (B, C, H, W): e.g. the rasterizer's allmap[1:2]."""
    return _Map(t, "chw")


def hwc(t):
    """(H, W, C) / (B, H, W, C)."""
    return _Map(t, "hwc")


class Plane:
    """One output plane: what image_planes takes.  Built by color(), gray(), depth(), normal(), ground_truth() and error()."""

    def __init__(self, kind, layout, opaque=False, **fields):
        if layout not in ("hwc", "chw"):
            raise ValueError("layout must be 'hwc' or 'chw', got %r" % (layout,))
        self.kind, self.layout, self.opaque = kind, layout, bool(opaque)
        self.img = self.weight = self.acc = self.gt = self.msk = self.M = self.table = self.bg = None
        self.weight_mode, self.curve, self.dpt_mult = None, "normalize", 1.0
        self.__dict__.update(fields)


def _weight_mode(weight, weight_mode):
    if weight_mode not in WEIGHT_MODES:
        raise ValueError("weight_mode must be None, 'one_minus' or 'twice', got %r" % (weight_mode,))
    if (weight is None) != (weight_mode is None):
        raise ValueError("weight and weight_mode go together: got weight %s, weight_mode %r" % ("None" if weight is None else "given", weight_mode))
    return weight_mode


def color(img, acc=None, weight=None, weight_mode=None, layout="hwc", opaque=False):
    """Three channels of img (RENDER, SURFACE, a 3-channel SPECULAR); with a one-channel `weight`: weight_mode="one_minus" img * (1 - weight)
    (DIFFUSE), "twice" (img * weight) * 2 (REFLECTION).  acc: the alpha byte (None or opaque=True: 255)."""
    return Plane(COLOR, layout, opaque, img=img, acc=acc, weight=weight, weight_mode=_weight_mode(weight, weight_mode))


def gray(img, acc=None, layout="hwc", opaque=False):
    """One channel on three (ALPHA, a 1-channel SPECULAR, ROUGHNESS)."""
    return Plane(GRAY, layout, opaque, img=img, acc=acc)


def depth(dpt, acc=None, curve="normalize", table=None, dpt_mult=1.0, layout="hwc", opaque=False):
    """DEPTH.  curve="linear": the depth itself; "normalize": 1 - (d - near) / (far - near) between the 1 % and 99 % order statistics of each
    image, clipped, through the colour map (table=None: 'linear'; or a (K, 3) float32 device tensor, see the module's docstring); then * dpt_mult."""
    if curve not in CURVES:
        raise ValueError("curve must be 'linear' or 'normalize', got %r" % (curve,))
    if table is not None and curve != "normalize":
        raise ValueError("a colour table needs curve='normalize'")
    return Plane(DEPTH, layout, opaque, img=dpt, acc=acc, curve=curve, table=table, dpt_mult=float(dpt_mult))


def normal(n, acc=None, M=None, layout="hwc", opaque=False):
    """NORMAL / SURFACE_NORMAL: n normalised, rotated by M ((3, 3) or (B, 3, 3): `n @ M.mT`, the reference's world-to-view R; None: identity),
    y and z flipped, * 0.5 + 0.5, * acc."""
    return Plane(NORMAL, layout, opaque, img=n, acc=acc, M=M)


def ground_truth(gt, msk=None, bg=None, layout="hwc", opaque=False):
    """Ground truth: float, or uint8 read as k / 255; three channels, or one on three.  With msk and bg (three floats): gt + bg * (1 - msk).
    The alpha byte is msk."""
    return Plane(GT, layout, opaque, gt=gt, msk=msk, bg=bg)


def error(img, gt, msk=None, bg=None, acc=None, weight=None, weight_mode=None, layout="hwc", opaque=False):
    """The error map of a colour plane: clip(sum_c (img_c - gt_c)^2, 0, 1) on three channels, img as color() reads it, gt as ground_truth() fills it.
    The alpha byte is clip(msk + acc, 0, 1)."""
    return Plane(ERROR, layout, opaque, img=img, gt=gt, msk=msk, bg=bg, acc=acc, weight=weight, weight_mode=_weight_mode(weight, weight_mode))


def _map(plane, name, channels, size, keep_u8=False):
    """-> (tensor kept alive, VisMap, B) of map `name` of a plane, or (None, empty VisMap, None)."""
    v = getattr(plane, name)
    if v is None:
        return None, _lib.VisMap(), None
    t, layout = (v.t, v.layout) if isinstance(v, _Map) else (v, plane.layout)
    if not torch.is_tensor(t):
        raise TypeError("%s must be a tensor, got %s" % (name, type(t).__name__))
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise ValueError("%s must be one image (3-D) or a batch of images (4-D), got shape %s" % (name, tuple(t.shape)))
    B, (h, w, c) = t.shape[0], (t.shape[1:] if layout == "hwc" else (t.shape[2], t.shape[3], t.shape[1]))
    ok = c in channels if isinstance(channels, tuple) else c >= channels
    if (h, w) != tuple(size) or not ok:
        raise ValueError("%s must be %s images of %d x %d with %s channels, got shape %s" % (
            name, layout, size[0], size[1], " or ".join(map(str, channels)) if isinstance(channels, tuple) else "at least %d" % channels, tuple(t.shape)))
    if not (t.dtype.is_floating_point or (t.dtype == torch.uint8 and keep_u8)):
        raise ValueError("%s must be a float tensor%s, got %s" % (name, " or uint8" if keep_u8 else "", t.dtype))
    t = t.detach() if t.dtype == torch.uint8 else t.detach().to(torch.float32)
    s = t.stride()
    sb, sc, sy, sx = (s[0], s[3], s[1], s[2]) if layout == "hwc" else s
    if c == 1:
        sc = 0                                              # one channel on three
    m = _lib.VisMap(ctypes.c_void_p(t.data_ptr()), (ctypes.c_int64 * 4)(sb, sc, sy, sx))
    return t, m, B


def depth_ranks(N, p=P_DEPTH):
    """normalize_depth's n = int(N * p), at least 1 -> the 0-based ranks of near and far."""
    n = max(int(N * p), 1)
    return n - 1, N - n


def image_planes(planes, size, canvas=None, origin=(0, 0), out=None):
    """planes: a list of at most 16 Plane records; size: (H, W) of their maps; canvas: (Ho, Wo) of the output, origin: (x0, y0) of the maps inside
    it (the reference's uncrop_output_images; every byte outside is 0) -- default: the maps' own size.
    Maps are "hwc" (H, W, C) / (B, H, W, C) or "chw" (C, H, W) / (B, C, H, W) by the plane's `layout`, or one by one through chw() / hwc(); a 3-D
    input is a batch of one; any strides: a [..., :3] slice, allmap[1:2], a permuted view are read in place.  Float maps other than float32 are
    converted first; a uint8 ground truth stays 8-bit.
    -> (T, B, Ho, Wo, 4) uint8 device tensor, RGBA, or `out` (such a tensor, contiguous) filled and returned.  One launch, plus one radix select per
    image for every depth plane with curve="normalize"; no host synchronisation; the same bytes on every call."""
    planes = list(planes)
    if not 1 <= len(planes) <= MAX_PLANES:
        raise ValueError("planes must hold 1 to %d planes, got %d" % (MAX_PLANES, len(planes)))
    H, W = (int(v) for v in size)
    Ho, Wo = (H, W) if canvas is None else (int(v) for v in canvas)
    x0, y0 = (int(v) for v in origin)
    if min(H, W) < 1:
        raise ValueError("empty images: size %s" % ((H, W),))
    if x0 < 0 or y0 < 0 or x0 + W > Wo or y0 + H > Ho:
        raise ValueError("a %d x %d crop at origin (x0, y0) = %s leaves the %d x %d canvas" % (H, W, (x0, y0), Ho, Wo))
    descs = (_lib.VisPlane * len(planes))()
    keep, B, dev = [], None, None
    pending_ranges = []
    for i, p in enumerate(planes):
        if not isinstance(p, Plane):
            raise TypeError("planes[%d] must be a Plane (color(), gray(), depth(), normal(), ground_truth(), error()), got %s" % (i, type(p).__name__))
        d = descs[i]
        d.kind, d.weight_mode, d.curve, d.dpt_mult = p.kind, WEIGHT_MODES[p.weight_mode], CURVES[p.curve], p.dpt_mult
        d.flags = OPAQUE if p.opaque else 0
        need = {COLOR: ("img",), GRAY: ("img",), DEPTH: ("img",), NORMAL: ("img",), GT: ("gt",), ERROR: ("img", "gt")}[p.kind]
        for name in need:
            if getattr(p, name) is None:
                raise ValueError("planes[%d]: %s is missing" % (i, name))
        specs = dict(img=1 if p.kind in (GRAY, DEPTH) else 3, weight=(1,), acc=(1,), gt=(1, 3, 4), msk=(1,))
        for name, channels in specs.items():
            t, m, b = _map(p, name, channels, (H, W), keep_u8=name == "gt")
            if t is None:
                continue
            if name == "img" and p.kind in (GRAY, DEPTH):
                m.stride[1] = 0
            if B is None:
                B, dev = b, t.device
            elif b != B or t.device != dev:
                raise ValueError("planes[%d]: %s has batch %d on %s, the maps before it batch %d on %s" % (i, name, b, t.device, B, dev))
            setattr(d, name, m)
            keep.append(t)
            if name == "gt":
                d.gt_dtype = 1 if t.dtype == torch.uint8 else 0
            if name == "img" and p.kind == DEPTH and p.curve == "normalize":
                pending_ranges.append((d, t, m))
        if p.bg is not None:
            bg = [float(v) for v in p.bg]
            if len(bg) != 3:
                raise ValueError("planes[%d]: bg must be three floats, got %d" % (i, len(bg)))
            d.bg = (ctypes.c_float * 3)(*bg)
            d.flags |= HAS_BG
        for name in ("M", "table"):
            t = getattr(p, name)
            if t is None:
                continue
            if not torch.is_tensor(t) or t.device.type != "cuda":
                raise RuntimeError("planes[%d]: %s must be a GPU tensor; there is no CPU path" % (i, name))
            t = t.detach().to(torch.float32).contiguous()
            if name == "M":
                if tuple(t.shape) == (3, 3):
                    t = t.expand(B, 3, 3).contiguous()
                if tuple(t.shape) != (B, 3, 3):
                    raise ValueError("planes[%d]: M must be (3, 3) or (%d, 3, 3), got %s" % (i, B, tuple(t.shape)))
            else:
                if t.dim() != 2 or t.shape[1] != 3 or not 2 <= t.shape[0] <= MAX_TABLE:
                    raise ValueError("planes[%d]: table must be (K, 3) with 2 <= K <= %d, got %s" % (i, MAX_TABLE, tuple(t.shape)))
                d.table_k = t.shape[0]
            setattr(d, name, t.data_ptr())
            keep.append(t)
    for i, p in enumerate(planes):
        for name in ("M", "table"):
            t = getattr(p, name)
            if t is not None and t.device != dev:
                raise ValueError("planes[%d]: %s is on %s, the maps on %s" % (i, name, t.device, dev))
    if dev.type != "cuda":
        raise RuntimeError("image_planes needs GPU tensors; there is no CPU path (the maps are on %s)" % (dev,))
    T = len(planes)
    if out is None:
        out = torch.empty(T, B, Ho, Wo, 4, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != (T, B, Ho, Wo, 4) or not out.is_contiguous()
          or out.data_ptr() % 4):
        raise ValueError("out must be a contiguous (%d, %d, %d, %d, 4) uint8 tensor on %s" % (T, B, Ho, Wo, dev))
    if B == 0:
        return out
    lib = _lib.load()
    stream = _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if pending_ranges:
        r0, r1 = depth_ranks(H * W)
        tb = lib.envgs_visualize_depth_range_temp_bytes()
        temp = torch.empty(tb, dtype=torch.uint8, device=dev)
        done = {}
        for d, t, m in pending_ranges:
            key = (t.data_ptr(), tuple(m.stride))
            if key not in done:                                  # the same depth map under two colour maps: one select
                nf = torch.empty(B, 2, dtype=torch.float32, device=dev)
                _lib.check(lib.envgs_visualize_depth_range(B, H, W, _lib.ptr(t), (ctypes.c_int64 * 3)(m.stride[0], m.stride[2], m.stride[3]), r0, r1,
                                                           _lib.ptr(nf), _lib.ptr(temp), tb, stream), "envgs_visualize_depth_range")
                done[key] = nf
            d.near_far = done[key].data_ptr()
        keep += [temp] + list(done.values())
    _lib.check(lib.envgs_visualize_planes(T, descs, B, H, W, Ho, Wo, x0, y0, _lib.ptr(out), stream), "envgs_visualize_planes")
    return out


def to_bytes(img, alpha=None, layout="hwc"):
    """The save_image rule alone, for a user's own tensor: img three channels (or one, on three), alpha one channel or None (255).
    -> (B, H, W, 4) uint8 device tensor; b = rint(clip(v * 255, 0, 255)) in float32, ties to even, NaN -> 0."""
    if not torch.is_tensor(img):
        raise TypeError("img must be a tensor, got %s" % type(img).__name__)
    if img.dim() not in (3, 4):
        raise ValueError("img must be one image (3-D) or a batch of images (4-D), got shape %s" % (tuple(img.shape),))
    if layout not in ("hwc", "chw"):
        raise ValueError("layout must be 'hwc' or 'chw', got %r" % (layout,))
    shape = img.shape[-3:]
    (H, W, C) = shape if layout == "hwc" else (shape[1], shape[2], shape[0])
    plane = gray(img, acc=alpha, layout=layout) if C == 1 else color(img, acc=alpha, layout=layout)
    return image_planes([plane], (H, W))[0]


# ---- files --------------------------------------------------------------------------------------------------------------------------------------
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(a, compression=6):
    """a: (H, W, 3) or (H, W, 4) uint8 -> the bytes of an 8-bit RGB / RGBA PNG; filter 0 on every row, one IDAT chunk.  Standard library only."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or min(a.shape[:2]) < 1:
        raise ValueError("encode_png takes a non-empty (H, W, 3) or (H, W, 4) uint8 array, got %s %s" % (a.dtype, a.shape))
    H, W, C = a.shape
    rows = np.zeros((H, 1 + W * C), np.uint8)                   # the filter byte 0 in front of every row
    rows[:, 1:] = a.reshape(H, W * C)
    head = struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 6, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", head) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), int(compression))) + _chunk(b"IEND", b"")


def encode_ppm(a):
    """a: (H, W, 3) or (H, W, 4) uint8 -> a binary PPM (P6) of its first three channels."""
    a = np.ascontiguousarray(np.asarray(a)[..., :3])
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("encode_ppm takes an (H, W, 3) or (H, W, 4) uint8 array, got %s %s" % (a.dtype, a.shape))
    return b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a.tobytes()


class ImageWriter:
    """The visualizer's I/O half: add() starts an asynchronous device -> pinned-host copy of finished bytes on a side stream, behind an event on
    the caller's stream, and returns at once; flush() / close() wait for the copies' events and hand the arrays to at most `workers` threads
    (never processes) that encode and write them.  More than `max_pending` copies in flight: the oldest is drained first, so pinned memory stays
    bounded (the reference's stream_delay).

    Files: result_dir / pattern.format(type=, frame=, camera=) + suffix + ext, the reference's img_pattern; suffix "_gt" / "_error" for the ground
    truth and the error map.  ext ".png": 8-bit RGBA, or RGB with store_alpha_channel=False, zlib level `compression`, filter 0, written with the
    standard library alone; ".ppm": binary P6, RGB only.  No video (ffmpeg is out of scope)."""

    def __init__(self, result_dir, pattern="{type}/frame{frame:04d}_camera{camera:04d}", ext=".png", store_alpha_channel=True, workers=3, compression=6,
                 max_pending=4):
        if ext not in (".png", ".ppm"):
            raise ValueError("ext must be '.png' or '.ppm', got %r" % (ext,))
        if int(workers) < 1:
            raise ValueError("workers must be at least 1, got %r" % (workers,))
        if not 0 <= int(compression) <= 9:
            raise ValueError("compression must be a zlib level 0..9, got %r" % (compression,))
        if int(max_pending) < 1:
            raise ValueError("max_pending must be at least 1, got %r" % (max_pending,))
        try:
            pattern.format(type="RENDER", frame=0, camera=0)
        except (KeyError, IndexError, ValueError) as e:
            raise ValueError("pattern must format with type, frame and camera alone: %r (%s)" % (pattern, e))
        self.result_dir, self.pattern, self.ext = str(result_dir), pattern, ext
        self.store_alpha_channel = bool(store_alpha_channel) and ext == ".png"
        self.workers, self.compression, self.max_pending = int(workers), int(compression), int(max_pending)
        self._pool = None
        self._streams = {}
        self._pending = []               # (event, pinned host tensor, paths per (plane, image))
        self._futures = []
        self.written = []                # every path handed to the pool, in order
        self._closed = False

    def path(self, type, camera, frame, suffix=""):
        return os.path.join(self.result_dir, self.pattern.format(type=type, frame=frame, camera=camera) + suffix + self.ext)

    def add(self, bytes, types, camera, frame, suffix=""):
        """bytes: (T, B, Ho, Wo, 4) uint8 device tensor (image_planes' result); types: T names, each a string or a (name, suffix) pair;
        camera / frame: one label, or one per image of the batch.  No synchronisation of the caller's stream.  -> the paths that will be written."""
        if self._closed:
            raise RuntimeError("the writer is closed")
        if not torch.is_tensor(bytes) or bytes.dtype != torch.uint8 or bytes.dim() != 5 or bytes.shape[-1] != 4:
            raise ValueError("bytes must be a (T, B, Ho, Wo, 4) uint8 tensor, got %s" % (tuple(bytes.shape) if torch.is_tensor(bytes) else type(bytes).__name__,))
        if bytes.device.type != "cuda":
            raise RuntimeError("ImageWriter.add needs a GPU tensor; there is no CPU path")
        T, B = bytes.shape[:2]
        types = [(t, suffix) if isinstance(t, str) else (t[0], t[1]) for t in types]
        if len(types) != T:
            raise ValueError("%d types for %d planes" % (len(types), T))
        labels = []
        for name, v in (("camera", camera), ("frame", frame)):
            v = list(v) if isinstance(v, (list, tuple)) else [v] * B
            if len(v) != B:
                raise ValueError("%s has %d labels for %d images" % (name, len(v), B))
            labels.append(v)
        paths = [[self.path(t, labels[0][b], labels[1][b], s) for b in range(B)] for t, s in types]
        if T == 0 or B == 0:
            return []
        dev = bytes.device
        side = self._streams.get(dev)
        if side is None:
            side = self._streams[dev] = torch.cuda.Stream(dev)
        bytes = bytes.detach().contiguous()
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        host = torch.empty(bytes.shape, dtype=torch.uint8, pin_memory=True)
        side.wait_event(ready)
        with torch.cuda.stream(side):
            host.copy_(bytes, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(side)
        bytes.record_stream(side)                           # the allocator hands the block out again only behind the copy
        self._pending.append((copied, host, paths))
        while len(self._pending) > self.max_pending:
            self._drain_one()
        return [p for row in paths for p in row]

    def _write(self, path, a):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        data = encode_ppm(a) if self.ext == ".ppm" else encode_png(a if self.store_alpha_channel else a[..., :3], self.compression)
        with open(path, "wb") as f:
            f.write(data)
        return path

    def _drain_one(self):
        copied, host, paths = self._pending.pop(0)
        copied.synchronize()                                # the copy's own event: neither the device nor the caller's stream
        a = host.numpy()
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.workers)
        for t, row in enumerate(paths):
            for b, path in enumerate(row):
                self._futures.append(self._pool.submit(self._write, path, a[t, b]))
                self.written.append(path)

    def flush(self):
        """Waits for every copy and every file.  -> the paths written so far."""
        while self._pending:
            self._drain_one()
        futures, self._futures = self._futures, []
        for f in futures:
            f.result()                                      # an I/O error surfaces here
        return list(self.written)

    def close(self):
        if not self._closed:
            try:
                self.flush()
            finally:
                self._closed = True
                if self._pool is not None:
                    self._pool.shutdown(wait=True)
                    self._pool = None
        return list(self.written)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------
def view_planes(out, cam, types=TYPES, image=None, mask=None, gt_bg=None, store_alpha_channel=True, dpt_curve="normalize", dpt_mult=1.0, dpt_table=None,
                depth_ratio=0.0):
    """The planes of one view: out = envgs_step.envgs_forward's result, cam its camera.  -> (planes, names) for image_planes / ImageWriter.add;
    names[i] is (type, suffix).  With `image` ((H, W, C >= 3) float or uint8) RENDER also gets its "_gt" and "_error" planes."""
    from . import fused
    b = out["base"]
    allmap, img = b["allmap"], b["img"]
    S = img.shape[0] - 4
    acc, spec = chw(allmap[1:2]), chw(img[3:3 + S])
    H, W = cam.image_height, cam.image_width
    opaque = not store_alpha_channel
    planes, names = [], []
    surf = None
    for t in types:
        if t == "RENDER":
            planes.append(color(out["rgb"], acc=acc, opaque=opaque)); names.append((t, ""))
            if image is not None:
                gt = image[..., :3]
                planes.append(ground_truth(gt, msk=mask, bg=gt_bg, opaque=opaque)); names.append((t, "_gt"))
                planes.append(error(out["rgb"], gt, msk=mask, bg=gt_bg, acc=acc, opaque=opaque)); names.append((t, "_error"))
        elif t in ("DEPTH", "SURFACE_NORMAL"):
            if surf is None:
                surf = fused.surface_normal(allmap, cam, depth_ratio)                   # surf_depth (1, H, W), surf_normal (3, H, W) in world space
            if t == "DEPTH":
                planes.append(depth(chw(surf[0]), acc=acc, curve=dpt_curve, table=dpt_table, dpt_mult=dpt_mult, opaque=opaque))
            else:
                planes.append(normal(chw(surf[1]), acc=acc, M=cam.world_view_transform[:3, :3].t(), opaque=opaque))      # world -> view: the reference's R
            names.append((t, ""))
        elif t == "ALPHA":
            planes.append(gray(acc, acc=acc, opaque=opaque)); names.append((t, ""))
        elif t == "NORMAL":
            # the rasterizer's normal is in VIEW space already: M = None.  The reference rotates it to world space (gaussian2d_utils.py:1123) and
            # back (`norm @ batch.R.mT`): two float32 rotations that cancel up to rounding -- a deviation of at most one byte step
            planes.append(normal(chw(allmap[2:5]), acc=acc, opaque=opaque)); names.append((t, ""))
        elif t == "SPECULAR":
            planes.append(gray(spec, acc=acc, opaque=opaque) if S == 1 else color(spec, acc=acc, opaque=opaque)); names.append((t, ""))
        elif t in ("DIFFUSE", "REFLECTION"):
            if S != 1:
                raise ValueError("%s needs a one-channel specular map, the rasterizer package gives %d" % (t, S))
            if t == "DIFFUSE":
                planes.append(color(chw(img[:3]), acc=acc, weight=spec, weight_mode="one_minus", opaque=opaque))
            elif "ref_rgb" in out:                                                      # a filtered pass: rgb_env * spec * 2 scattered already
                planes.append(color(out["ref_rgb"].reshape(H, W, 3), acc=acc, opaque=opaque))
            else:
                planes.append(color(out["rgb_env"].reshape(H, W, 3), acc=acc, weight=spec, weight_mode="twice", opaque=opaque))
            names.append((t, ""))
        else:
            raise ValueError("unknown visualization type %r: one of %s" % (t, ", ".join(TYPES)))
    return planes, names


MESH_TYPES = ("MESH_NORMAL", "MESH_DEPTH", "MESH_RENDER")
MESH_GROUP = 8                                                       # cameras per render_mesh / image_planes call: one launch group of the rasteriser


def mesh_views(mesh, cameras, writer, types=MESH_TYPES, size=None, near=0.0, labels=None, dpt_curve="normalize", dpt_mult=1.0, dpt_table=None):
    """Pictures of a mesh (mesh.Mesh: vertices, faces, colors) through cameras with K, R, T: mesh.render_mesh()'s maps fed to the planes above, no
    kernel of its own.  types, out of MESH_TYPES:
        MESH_NORMAL  the shaded-normal picture: normal() of the face normals (world space, towards the camera) with M = the camera's R
        MESH_DEPTH   depth() of the z-buffer, background included at depth 0, as DEPTH treats the surfel depth
        MESH_RENDER  color() of the interpolated vertex colours; a mesh without colours raises
    The alpha map of every plane is face >= 0.  Per group of 8 cameras: ONE render_mesh, ONE image_planes and ONE writer.add call; files follow
    the writer's pattern with camera, frame = (i, 0) or labels[i].  No host synchronisation beyond the writer's waits for its own copies.
    -> the paths in the order they were enqueued; they exist after writer.flush() / close().  The rasteriser does not clip (mesh.render_mesh)."""
    from . import mesh as mesh_ops
    cameras = list(cameras)
    types = list(types)
    for t in types:
        if t not in MESH_TYPES:
            raise ValueError("unknown mesh visualization type %r: one of %s" % (t, ", ".join(MESH_TYPES)))
    if labels is not None and len(labels) != len(cameras):
        raise ValueError("%d cameras for %d labels" % (len(cameras), len(labels)))
    if "MESH_RENDER" in types and getattr(mesh, "colors", None) is None:
        raise ValueError("MESH_RENDER needs a mesh with colours")
    wanted = ("face",) + tuple(o for o, t in (("normal", "MESH_NORMAL"), ("depth", "MESH_DEPTH"), ("color", "MESH_RENDER")) if t in types)
    opaque = not writer.store_alpha_channel
    paths = []
    for b0 in range(0, len(cameras) if types else 0, MESH_GROUP):
        group = cameras[b0:b0 + MESH_GROUP]
        r = mesh_ops.render_mesh(mesh, group, size=size, near=near, outputs=wanted)
        acc = (r.face >= 0).to(torch.float32).unsqueeze(-1)
        planes = []
        for t in types:
            if t == "MESH_NORMAL":
                M = torch.stack([torch.as_tensor(c.R, dtype=torch.float32).reshape(3, 3) for c in group]).to(r.face.device)
                planes.append(normal(r.normal, acc=acc, M=M, opaque=opaque))
            elif t == "MESH_DEPTH":
                planes.append(depth(r.depth.unsqueeze(-1), acc=acc, curve=dpt_curve, table=dpt_table, dpt_mult=dpt_mult, opaque=opaque))
            else:
                planes.append(color(r.color, acc=acc, opaque=opaque))
        idx = range(b0, b0 + len(group))
        camera, frame = ([i for i in idx], [0] * len(group)) if labels is None else ([labels[i][0] for i in idx], [labels[i][1] for i in idx])
        paths += writer.add(image_planes(planes, tuple(r.face.shape[1:])), types, camera, frame)
    return paths


def visualize_views(cameras, base, env, sh_degree, bg, env_bg, writer, types=TYPES, images=None, masks=None, labels=None, gt_bg=None, dpt_curve="normalize",
                    dpt_mult=1.0, dpt_table=None, pkg=None, tpkg=None, tracer=None):
    """Renders every camera through envgs_step.envgs_forward under torch.no_grad() and writes its pictures: per view ONE image_planes call and ONE
    writer.add.  The arguments mirror metrics.evaluate_views; writer: an ImageWriter (the caller closes it); types: names out of TYPES, the eight
    of configs/models/envgs.yaml by default; images[i]: (H, W, C >= 3) float or uint8 on the device -- RENDER then gets its "_gt" and "_error"
    files; masks[i]: (H, W, 1) float, gt_bg: three floats (the sampler's bg_brightness) to fill the ground truth with.
    -> the paths in the order they were enqueued; they exist after writer.flush() / close().

    DEPTH shows fused.surface_normal's surf_depth, SURFACE_NORMAL its world-space normal with M = the camera's world-to-view rotation, NORMAL the
    rasterizer's view-space allmap[2:5] with M = None (the reference rotates to world space and back: at most one byte step apart).
    Host synchronisation: none beyond the forward's own (metrics.evaluate_views lists them) and the writer's waits for its own copies."""
    from . import envgs_step, synth
    for name, v in (("images", images), ("masks", masks), ("labels", labels)):
        if v is not None and len(v) != len(cameras):
            raise ValueError("%d cameras for %d %s" % (len(cameras), len(v), name))
    if pkg is None:
        import diff_surfel_rasterization_wet_ch05 as pkg
    if tpkg is None:
        import diff_surfel_tracing as tpkg
    if tracer is None:
        tracer = tpkg.SurfelTracer()
    paths = []
    with torch.no_grad():
        for i, cam in enumerate(cameras):
            out = envgs_step.envgs_forward(pkg, tpkg, tracer, cam, synth.get_rays(cam), base, env, bg, env_bg, sh_degree)
            planes, names = view_planes(out, cam, types, None if images is None else images[i], None if masks is None else masks[i], gt_bg,
                                        writer.store_alpha_channel, dpt_curve, dpt_mult, dpt_table)
            camera, frame = (i, 0) if labels is None else labels[i]
            paths += writer.add(image_planes(planes, (cam.image_height, cam.image_width)), names, camera, frame)
    return paths
