"""Fused caller-side glue (include/envgs_glue.h): drop-in replacements for the torch expressions the
reference evaluates between its two extension calls.  Optional -- the extensions do not need them.

    sh_colors(means3D, shs, campos, sh_degree, specular, roughness) -> (P, 3+S+1)
        == cat([clamp_min(eval_sh(deg, shs^T, normalize(xyz - campos)) + 0.5, 0), specular, roughness], -1)     gaussian2d_utils.py:1071-1084
    reflect(allmap, ray_o, ray_d, viewmatrix, depth_ratio=0.0) -> normal_world (3,H,W), depth (1,H,W), ref_o (H,W,3), ref_d (H,W,3)
        == gaussian2d_utils.py:1119-1136 + envgs_sampler.py:420-431
    select_pixels / reflect_filtered / blend_filtered: the same two stages when only the pixels of a mask are traced
        == envgs_sampler.py:433-455 (ref_msk, ref_o[ref_msk][None]) and :461-476 (the masked blend, ref_rgb_map)
"""
import torch

from . import _lib
from .raster import sh_degree_of


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _stream(dev):
    return _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- argument checks of the entries that hand raw pointers to a one-lane-per-element kernel (reflect, blend, the bounce trio, surfel_quads).
# Shapes, index dtypes and devices first (ValueError), then the device kind (RuntimeError: no CPU path); all of it before the library is touched.
# The VALUES of sel / idx (unique, inside [0, R)) are not checked: that would read them back to the host.  They stay the caller's promise.
def _need_gpu(t):
    if t.device.type != "cuda":
        raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")


def _check_devices(fn, first, **others):
    for name, t in others.items():
        if t.device != first.device:
            raise ValueError("%s: %s is on %s, the call is on %s" % (fn, name, t.device, first.device))


def _check_image(fn, name, t, channels):
    if t.dim() != 3 or t.shape[0] not in channels or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError("%s: %s must be (%s,H,W), got %s" % (fn, name, "|".join(str(c) for c in channels), tuple(t.shape)))
    return int(t.shape[1]), int(t.shape[2])


def _check_numel(fn, n, what, **ts):
    for name, t in ts.items():
        if t.numel() != n:
            raise ValueError("%s: %s must hold %s = %d elements, got %s" % (fn, name, what, n, tuple(t.shape)))


def _check_rows(fn, widths, **ts):
    """Per-ray tensors (R, width): 2-D, the stated widths, one row count.  -> R"""
    R = None
    for (name, t), w in zip(ts.items(), widths):
        if t.dim() != 2 or t.shape[1] != w:
            raise ValueError("%s: %s must be (R,%d), got %s" % (fn, name, w, tuple(t.shape)))
        if R is None:
            R = int(t.shape[0])
        elif t.shape[0] != R:
            raise ValueError("%s: %s has %d rows, %s has %d" % (fn, name, t.shape[0], next(iter(ts)), R))
    return R


def _check_index(fn, name, t, dev):
    if t.dtype != torch.int64 or t.dim() != 1:
        raise ValueError("%s: %s must be a 1-D int64 tensor of row indices, got %s %s" % (fn, name, t.dtype, tuple(t.shape)))
    if t.device != dev:
        raise ValueError("%s: %s is on %s, the call is on %s" % (fn, name, t.device, dev))


class _ShColors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, shs, campos, deg, specular, roughness):
        lib = _lib.load()
        if means3D.device.type != "cuda":
            raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")
        means3D, shs, specular, roughness = _f32c(means3D), _f32c(shs), _f32c(specular), _f32c(roughness)
        campos = _f32c(campos).reshape(-1)
        P, M, S = means3D.shape[0], shs.shape[1], specular.shape[1]
        colors = torch.empty(P, 3 + S + 1, dtype=torch.float32, device=means3D.device)
        clamped = torch.empty(P, 3, dtype=torch.uint8, device=means3D.device)
        p = _lib.ptr
        _lib.check(lib.envgs_sh_colors_forward(P, deg, M, S, p(means3D), p(shs), p(campos), p(specular), p(roughness), p(colors), p(clamped),
                                               _stream(means3D.device)), "envgs_sh_colors_forward")
        ctx.save_for_backward(means3D, shs, campos, clamped)
        ctx.meta = (P, deg, M, S)
        return colors

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        means3D, shs, campos, clamped = ctx.saved_tensors
        P, deg, M, S = ctx.meta
        g = _f32c(g)
        dm = torch.empty_like(means3D); dsh = torch.empty_like(shs)
        dsp = torch.empty(P, S, dtype=torch.float32, device=g.device); dr = torch.empty(P, 1, dtype=torch.float32, device=g.device)
        p = _lib.ptr
        _lib.check(lib.envgs_sh_colors_backward(P, deg, M, S, p(means3D), p(shs), p(campos), p(clamped), p(g), p(dm), p(dsh), p(dsp), p(dr),
                                                _stream(g.device)), "envgs_sh_colors_backward")
        return dm, dsh, None, None, dsp, dr


def sh_colors(means3D, shs, campos, sh_degree, specular, roughness):
    return _ShColors.apply(means3D, shs, campos, sh_degree_of(sh_degree), specular, roughness)


class _Reflect(torch.autograd.Function):
    @staticmethod
    def forward(ctx, allmap, ray_o, ray_d, viewmatrix, depth_ratio):
        ctx.set_materialize_grads(False)          # outputs the loss does not use arrive as None (= NULL upstream pointer), not as buffers of zeros
        lib = _lib.load()
        if allmap.device.type != "cuda":
            raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")
        allmap, ray_o, ray_d, viewmatrix = _f32c(allmap), _f32c(ray_o), _f32c(ray_d), _f32c(viewmatrix)
        _, H, W = allmap.shape
        f32 = dict(dtype=torch.float32, device=allmap.device)
        nw = torch.empty(3, H, W, **f32); dep = torch.empty(1, H, W, **f32)
        ref_o = torch.empty(H, W, 3, **f32); ref_d = torch.empty(H, W, 3, **f32)
        p = _lib.ptr
        _lib.check(lib.envgs_reflect_forward(H, W, float(depth_ratio), p(allmap), p(ray_o), p(ray_d), p(viewmatrix), p(nw), p(dep), p(ref_o),
                                             p(ref_d), _stream(allmap.device)), "envgs_reflect_forward")
        ctx.save_for_backward(allmap, ray_o, ray_d, viewmatrix)
        ctx.ratio = float(depth_ratio)
        ctx.need = (ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return nw, dep, ref_o, ref_d

    @staticmethod
    def backward(ctx, g_nw, g_dep, g_ro, g_rd):
        lib = _lib.load()
        allmap, ray_o, ray_d, viewmatrix = ctx.saved_tensors
        _, H, W = allmap.shape
        c = lambda g: None if g is None else _f32c(g)
        g_nw, g_dep, g_ro, g_rd = c(g_nw), c(g_dep), c(g_ro), c(g_rd)
        dall = torch.empty_like(allmap)
        dro = torch.empty_like(ray_o) if ctx.need[0] else None
        drd = torch.empty_like(ray_d) if ctx.need[1] else None
        p = _lib.ptr
        _lib.check(lib.envgs_reflect_backward(H, W, ctx.ratio, p(allmap), p(ray_o), p(ray_d), p(viewmatrix), p(g_nw), p(g_dep), p(g_ro), p(g_rd),
                                              p(dall), p(dro), p(drd), _stream(allmap.device)), "envgs_reflect_backward")
        return dall, dro, drd, None, None


def reflect(allmap, ray_o, ray_d, viewmatrix, depth_ratio=0.0):
    """normal_world (3,H,W), depth (1,H,W), ref_o (H,W,3), ref_d (H,W,3) from allmap (7,H,W), rays of 3 H W elements each and the (4,4) view
    matrix; one launch each way.  Inputs of another dtype or layout are converted to contiguous float32; gradients come back in the input's dtype
    and shape.  Non-finite depths: a NaN, +inf or -inf expected depth (allmap[0] / allmap[1]) or median (allmap[5]) becomes 0 and passes no
    gradient.  The reference's nan_to_num(x, 0, 0) sends -inf to the lowest finite float (-3.4e38) instead; the rasterizer cannot produce one
    (depths are >= 0.2), so that value is not reproduced (the same rule as surface_normal; include/envgs_glue.h).
    ValueError: allmap not (7,H,W), a ray tensor not of 3 H W elements, a view matrix not of 16, tensors on different devices."""
    H, W = _check_image("reflect", "allmap", allmap, (7,))
    _check_numel("reflect", 3 * H * W, "3 H W", ray_o=ray_o, ray_d=ray_d)
    _check_numel("reflect", 16, "4 x 4", viewmatrix=viewmatrix)
    _check_devices("reflect", allmap, ray_o=ray_o, ray_d=ray_d, viewmatrix=viewmatrix)
    _need_gpu(allmap)
    return _Reflect.apply(allmap, ray_o, ray_d, viewmatrix, depth_ratio)


class _SurfaceNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, allmap, viewmatrix, fx, fy, depth_ratio):
        ctx.set_materialize_grads(False)          # outputs the loss does not use arrive as None (= NULL upstream pointer), not as buffers of zeros
        lib = _lib.load()
        if allmap.device.type != "cuda":
            raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")
        allmap, viewmatrix = _f32c(allmap), _f32c(viewmatrix)
        _, H, W = allmap.shape
        f32 = dict(dtype=torch.float32, device=allmap.device)
        sd = torch.empty(1, H, W, **f32); sn = torch.empty(3, H, W, **f32)
        p = _lib.ptr
        _lib.check(lib.envgs_surface_normal_forward(H, W, float(depth_ratio), float(fx), float(fy), p(allmap), p(viewmatrix), p(sd), p(sn),
                                                    _stream(allmap.device)), "envgs_surface_normal_forward")
        ctx.save_for_backward(allmap, viewmatrix)
        ctx.cfg = (float(depth_ratio), float(fx), float(fy))
        return sd, sn

    @staticmethod
    def backward(ctx, g_sd, g_sn):
        lib = _lib.load()
        allmap, viewmatrix = ctx.saved_tensors
        _, H, W = allmap.shape
        ratio, fx, fy = ctx.cfg
        c = lambda g: None if g is None else _f32c(g)
        g_sd, g_sn = c(g_sd), c(g_sn)
        dall = torch.empty_like(allmap)
        p = _lib.ptr
        _lib.check(lib.envgs_surface_normal_backward(H, W, ratio, fx, fy, p(allmap), p(viewmatrix), p(g_sd), p(g_sn), p(dall),
                                                     _stream(allmap.device)), "envgs_surface_normal_backward")
        return dall, None, None, None, None


def surface_normal(allmap, cam, depth_ratio=0.0):
    """surf_depth (1,H,W), surf_normal (3,H,W) of render()'s tail (gaussian2d_utils.py:1125-1142, dpt2norm :1190-1206) in one kernel each way;
    cam: the prepare_gaussian_camera namespace (image size, FoVx / FoVy, world_view_transform)."""
    import math
    fx = cam.image_width / (2.0 * math.tan(cam.FoVx / 2.0))
    fy = cam.image_height / (2.0 * math.tan(cam.FoVy / 2.0))
    return _SurfaceNormal.apply(allmap, cam.world_view_transform, fx, fy, depth_ratio)


_FACES = {}


def surfel_quads(means3D, scales, rotations):
    """get_disks (optix_utils.py:39-69) in one launch: v (4P,3) f32, f (2P,3) i32.  No gradient flows through the quads (they only seed the
    acceleration structure); the face table depends on P alone and is cached (the last 8 sizes; a table a caller still holds stays valid).
    ValueError: means3D / scales / rotations not (P,3) / (P,2) / (P,4) with one P, or on different devices."""
    P = _check_rows("surfel_quads", (3, 2, 4), means3D=means3D, scales=scales, rotations=rotations)
    _check_devices("surfel_quads", means3D, scales=scales, rotations=rotations)
    _need_gpu(means3D)
    lib = _lib.load()
    dev = means3D.device
    m, s, q = _f32c(means3D.detach()), _f32c(scales.detach()), _f32c(rotations.detach())
    v = torch.empty(4 * P, 3, dtype=torch.float32, device=dev)
    f = _FACES.get((dev.index, P))
    fresh = f is None
    if fresh:
        f = torch.empty(2 * P, 3, dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.check(lib.envgs_surfel_quads(P, p(m), p(s), p(q), p(v), p(f) if fresh else None, _stream(dev)), "envgs_surfel_quads")
    if fresh:                                             # (cached only once its launch was accepted: a refused call leaves no unwritten table behind)
        _FACES[(dev.index, P)] = f
        if len(_FACES) > 8:
            _FACES.pop(next(iter(_FACES)))
    return v, f


class _Blend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, rgb_env):
        lib = _lib.load()
        if img.device.type != "cuda":
            raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")
        img, rgb_env = _f32c(img), _f32c(rgb_env)
        C, H, W = img.shape
        rgb = torch.empty(H, W, 3, dtype=torch.float32, device=img.device)
        p = _lib.ptr
        _lib.check(lib.envgs_blend_forward(H, W, C, p(img), p(rgb_env), p(rgb), _stream(img.device)), "envgs_blend_forward")
        ctx.save_for_backward(img, rgb_env)
        return rgb

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        img, rgb_env = ctx.saved_tensors
        C, H, W = img.shape
        g = _f32c(g)
        dimg = torch.empty_like(img)
        denv = torch.empty_like(rgb_env) if ctx.needs_input_grad[1] else None
        p = _lib.ptr
        _lib.check(lib.envgs_blend_backward(H, W, C, p(img), p(rgb_env), p(g), p(dimg), p(denv), _stream(img.device)), "envgs_blend_backward")
        return dimg, denv


def blend(img, rgb_env):
    """(1 - s) * img[:3] + s * rgb_env  (H,W,3) from the -ch05 / -ch07 rasterizer output img (C,H,W) = [rgb | specular C-4 | roughness] and the
    traced colour rgb_env (H,W,3): envgs_sampler.py:474, one launch each way instead of ~20 (include/envgs_glue.h).
    ValueError: img not (5|7,H,W), rgb_env not of 3 H W elements (any shape of that size, e.g. (1,HW,3), is taken row-major), different devices."""
    H, W = _check_image("blend", "img", img, (5, 7))
    _check_numel("blend", 3 * H * W, "3 H W", rgb_env=rgb_env)
    _check_devices("blend", img, rgb_env=rgb_env)
    _need_gpu(img)
    return _Blend.apply(img, rgb_env)


class PixelSelection:
    """The pixels whose reflection rays are traced (select_pixels).  mask (H,W) bool: the reference's ref_msk; count: S, a host int; keep (H*W)
    uint8 and positions (H*W) int32 on the device: kept pixel p owns compact row positions[p], its rank in row-major order (= x[mask] order)."""
    __slots__ = ("mask", "count", "keep", "positions", "H", "W")

    def __init__(self, mask, count, keep, positions):
        self.mask, self.count, self.keep, self.positions = mask, count, keep, positions
        self.H, self.W = mask.shape


def select_pixels(mask=None, allmap=None, acc_threshold=0.75):
    """The pixel selection of a filtered reflection pass.  Exactly one of
        mask   (H,W) bool / uint8 on the GPU: any selection the caller computed (the reference's specular filter, envgs_sampler.py:441), or
        allmap (7,H,W): the acc filter, mask = allmap[1] > acc_threshold (:443), evaluated by one kernel.
    One prefix scan (envgs_compact_scan) gives every kept pixel its compact row and the kept count; reading that count is the ONE host
    synchronisation of the filtered path (the tracer launches by ray count; the reference's boolean indexing synchronises at the same place)."""
    if (mask is None) == (allmap is None):
        raise ValueError("select_pixels: give exactly one of mask and allmap")
    lib = _lib.load()
    src = mask if mask is not None else allmap
    dev = src.device
    if dev.type != "cuda":
        raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")
    p = _lib.ptr
    if mask is not None:
        if mask.dim() != 2:
            raise ValueError("select_pixels: mask must be (H,W), got %s" % (tuple(mask.shape),))
        H, W = mask.shape
        mask = (mask if mask.dtype == torch.bool else mask != 0).contiguous()
        keep = mask.view(torch.uint8).reshape(-1)                           # (bool storage is one 0 / 1 byte per element)
    else:
        if allmap.dim() != 3 or allmap.shape[0] < 2:
            raise ValueError("select_pixels: allmap must be (7,H,W), got %s" % (tuple(allmap.shape),))
        a = _f32c(allmap.detach())
        _, H, W = a.shape
        keep = torch.empty(H * W, dtype=torch.uint8, device=dev)
        _lib.check(lib.envgs_select_acc(H, W, float(acc_threshold), p(a), p(keep), _stream(dev)), "envgs_select_acc")
        mask = keep.view(torch.bool).view(H, W)
    P = H * W
    pos = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    nk = torch.empty(1, dtype=torch.int32, device=dev)
    tb = lib.envgs_compact_temp_bytes(P)
    temp = torch.empty(max(tb, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.envgs_compact_scan(P, p(keep), p(pos), p(nk), p(temp), tb, _stream(dev)), "envgs_compact_scan")
    return PixelSelection(mask, int(nk.item()) & 0xFFFFFFFF, keep, pos)


def _check_selection(sel, H, W, dev):
    if (sel.H, sel.W) != (H, W) or sel.keep.device != dev:
        raise RuntimeError("pixel selection is for a %dx%d image on %s, the call is %dx%d on %s" % (sel.H, sel.W, sel.keep.device, H, W, dev))


class _ReflectFiltered(torch.autograd.Function):
    @staticmethod
    def forward(ctx, allmap, ray_o, ray_d, viewmatrix, depth_ratio, sel):
        ctx.set_materialize_grads(False)          # outputs the loss does not use arrive as None (= NULL upstream pointer), not as buffers of zeros
        lib = _lib.load()
        if allmap.device.type != "cuda":
            raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")
        allmap, ray_o, ray_d, viewmatrix = _f32c(allmap), _f32c(ray_o), _f32c(ray_d), _f32c(viewmatrix)
        _, H, W = allmap.shape
        _check_selection(sel, H, W, allmap.device)
        S = sel.count
        f32 = dict(dtype=torch.float32, device=allmap.device)
        nw = torch.empty(3, H, W, **f32); dep = torch.empty(1, H, W, **f32)
        ref_o = torch.empty(1, S, 3, **f32); ref_d = torch.empty(1, S, 3, **f32)
        p = _lib.ptr
        _lib.check(lib.envgs_reflect_filtered_forward(H, W, float(depth_ratio), S, p(allmap), p(ray_o), p(ray_d), p(viewmatrix), p(sel.keep),
                                                      p(sel.positions), p(nw), p(dep), p(ref_o), p(ref_d), _stream(allmap.device)),
                   "envgs_reflect_filtered_forward")
        ctx.save_for_backward(allmap, ray_o, ray_d, viewmatrix, sel.keep, sel.positions)
        ctx.ratio, ctx.count = float(depth_ratio), S
        ctx.need = (ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return nw, dep, ref_o, ref_d

    @staticmethod
    def backward(ctx, g_nw, g_dep, g_ro, g_rd):
        lib = _lib.load()
        allmap, ray_o, ray_d, viewmatrix, keep, pos = ctx.saved_tensors
        _, H, W = allmap.shape
        c = lambda g: None if (g is None or g.numel() == 0) else _f32c(g)
        g_nw, g_dep, g_ro, g_rd = c(g_nw), c(g_dep), c(g_ro), c(g_rd)
        dall = torch.empty_like(allmap)
        dro = torch.empty_like(ray_o) if ctx.need[0] else None
        drd = torch.empty_like(ray_d) if ctx.need[1] else None
        p = _lib.ptr
        _lib.check(lib.envgs_reflect_filtered_backward(H, W, ctx.ratio, ctx.count, p(allmap), p(ray_o), p(ray_d), p(viewmatrix), p(keep), p(pos),
                                                       p(g_nw), p(g_dep), p(g_ro), p(g_rd), p(dall), p(dro), p(drd), _stream(allmap.device)),
                   "envgs_reflect_filtered_backward")
        return dall, dro, drd, None, None, None


def reflect_filtered(allmap, ray_o, ray_d, viewmatrix, sel, depth_ratio=0.0):
    """reflect() for a filtered pass: normal_world (3,H,W) and depth (1,H,W) for every pixel, ref_o / ref_d (1,S,3) for the S pixels of `sel`
    (select_pixels) in x[mask] order -- envgs_sampler.py:420-455 without the dense ray tensors, the two boolean-mask gathers and their scatter-add
    backward: one launch each way."""
    return _ReflectFiltered.apply(allmap, ray_o, ray_d, viewmatrix, depth_ratio, sel)


class _BlendFiltered(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, rgb_env, sel):
        lib = _lib.load()
        if img.device.type != "cuda":
            raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")
        img, rgb_env = _f32c(img), _f32c(rgb_env)
        C, H, W = img.shape
        _check_selection(sel, H, W, img.device)
        if rgb_env.shape not in ((1, sel.count, 3), (sel.count, 3)):
            raise RuntimeError("blend_filtered: rgb_env must be (1,%d,3) or (%d,3), got %s" % (sel.count, sel.count, tuple(rgb_env.shape)))
        rgb = torch.empty(H, W, 3, dtype=torch.float32, device=img.device); ref_rgb = torch.empty_like(rgb)
        p = _lib.ptr
        _lib.check(lib.envgs_blend_filtered_forward(H, W, C, sel.count, p(img), p(rgb_env), p(sel.keep), p(sel.positions), p(rgb), p(ref_rgb),
                                                    _stream(img.device)), "envgs_blend_filtered_forward")
        ctx.save_for_backward(img, rgb_env, sel.keep, sel.positions)
        ctx.count = sel.count
        ctx.mark_non_differentiable(ref_rgb)
        return rgb, ref_rgb

    @staticmethod
    def backward(ctx, g, _g_ref):
        lib = _lib.load()
        img, rgb_env, keep, pos = ctx.saved_tensors
        C, H, W = img.shape
        g = _f32c(g)
        dimg = torch.empty_like(img)
        denv = torch.empty_like(rgb_env) if ctx.needs_input_grad[1] else None
        p = _lib.ptr
        _lib.check(lib.envgs_blend_filtered_backward(H, W, C, ctx.count, p(img), p(rgb_env), p(keep), p(pos), p(g), p(dimg), p(denv),
                                                     _stream(img.device)), "envgs_blend_filtered_backward")
        return dimg, denv, None


def blend_filtered(img, rgb_env, sel):
    """blend() for a filtered pass (envgs_sampler.py:465-476): rgb (H,W,3) = the blend at the pixels of `sel`, img[:3] elsewhere; ref_rgb (H,W,3)
    = rgb_env * s * 2 scattered to the kept pixels, zero elsewhere (a visualisation output: not differentiable).  rgb_env: the traced colour
    (1,S,3) or (S,3).  One launch each way instead of the masked assignment, the zero image + scatter and their scatter-add backward."""
    return _BlendFiltered.apply(img, rgb_env, sel)


class _BounceRays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ray_o, ray_d, dpt, acc, norm, sel):
        lib = _lib.load()
        if ray_o.device.type != "cuda":
            raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")
        ray_o, ray_d, dpt, acc, norm = (_f32c(t) for t in (ray_o, ray_d, dpt, acc, norm))
        sel = sel.contiguous()
        n = int(sel.numel())
        o2 = torch.empty(n, 3, dtype=torch.float32, device=ray_o.device); d2 = torch.empty_like(o2)
        p = _lib.ptr
        _lib.check(lib.envgs_bounce_rays_forward(n, p(sel), p(ray_o), p(ray_d), p(dpt), p(acc), p(norm), p(o2), p(d2), _stream(ray_o.device)),
                   "envgs_bounce_rays_forward")
        ctx.save_for_backward(ray_o, ray_d, dpt, acc, norm, sel)
        return o2, d2

    @staticmethod
    def backward(ctx, g_o2, g_d2):
        lib = _lib.load()
        ray_o, ray_d, dpt, acc, norm, sel = ctx.saved_tensors
        n = int(sel.numel())
        need = ctx.needs_input_grad
        outs = [torch.zeros_like(t) if need[i] else None for i, t in enumerate((ray_o, ray_d, dpt, acc, norm))]
        p = _lib.ptr
        # held in names: a converted copy made inside the call is freed as soon as its address is taken, and the second copy then takes the
        # first one's block -- both upstream pointers would show g_d2 (any upstream that is not contiguous float32, e.g. the expanded scalar of a sum)
        g_o2, g_d2 = _f32c(g_o2), _f32c(g_d2)
        _lib.check(lib.envgs_bounce_rays_backward(n, p(sel), p(ray_o), p(ray_d), p(dpt), p(acc), p(norm), p(g_o2), p(g_d2),
                                                  *[p(t) for t in outs], _stream(ray_o.device)), "envgs_bounce_rays_backward")
        return (*outs, None)


def bounce_rays(ray_o, ray_d, dpt, acc, norm, sel):
    """Rays of the next bounce stage from the rows `sel` (unique int64 indices) of a stage's rays (R,3) and outputs dpt / acc (R,1), norm (R,3):
    o2 = o + d dpt/acc, d2 = d - 2 (d.n) n with n = norm/|norm| -- (n,3) each; differentiable in everything but `sel`; one launch each way
    (include/envgs_glue.h: envgs_bounce_rays_forward).  The VALUES of `sel` (unique, inside [0, R)) are the caller's promise: checking them
    would read them back to the host.  ValueError: per-ray tensors that are not (R,3) (R,3) (R,1) (R,1) (R,3) with one R; a `sel` that is not a
    1-D int64 tensor on the same device."""
    _check_rows("bounce_rays", (3, 3, 1, 1, 3), ray_o=ray_o, ray_d=ray_d, dpt=dpt, acc=acc, norm=norm)
    _check_devices("bounce_rays", ray_o, ray_d=ray_d, dpt=dpt, acc=acc, norm=norm)
    _check_index("bounce_rays", "sel", sel, ray_o.device)
    _need_gpu(ray_o)
    return _BounceRays.apply(ray_o, ray_d, dpt, acc, norm, sel)


class _BounceBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, aux, col_next, sel):
        lib = _lib.load()
        if rgb.device.type != "cuda":
            raise RuntimeError("envgs_amd.fused needs tensors on the GPU; there is no CPU path")
        rgb, aux, col_next = _f32c(rgb), _f32c(aux), _f32c(col_next)
        sel = sel.contiguous()
        col = rgb.clone()
        p = _lib.ptr
        _lib.check(lib.envgs_bounce_blend_forward(int(sel.numel()), p(sel), p(rgb), p(aux), p(col_next), p(col), _stream(rgb.device)),
                   "envgs_bounce_blend_forward")
        ctx.save_for_backward(rgb, aux, col_next, sel)
        return col

    @staticmethod
    def backward(ctx, g_col):
        lib = _lib.load()
        rgb, aux, col_next, sel = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_col = _f32c(g_col)
        g_rgb = g_col.clone() if need[0] else None
        g_aux = torch.zeros_like(aux) if need[1] else None
        g_next = torch.empty_like(col_next) if need[2] else None
        p = _lib.ptr
        _lib.check(lib.envgs_bounce_blend_backward(int(sel.numel()), p(sel), p(rgb), p(aux), p(col_next), p(g_col), p(g_rgb), p(g_aux), p(g_next),
                                                   _stream(rgb.device)), "envgs_bounce_blend_backward")
        return g_rgb, g_aux, g_next, None


def bounce_blend(rgb, aux, col_next, sel):
    """A stage's colour with the next stage blended in at the rows that bounced: rgb (R,3) with rows sel replaced by
    (1 - s) rgb[sel] + s col_next, s = aux[sel, 0]; differentiable in rgb, aux, col_next (include/envgs_glue.h: envgs_bounce_blend_forward).
    The VALUES of `sel` (unique, inside [0, R)) are the caller's promise, as for bounce_rays.  ValueError: rgb / aux not (R,3) / (R,2) with one
    R; col_next not (sel.numel(), 3); a `sel` that is not a 1-D int64 tensor on the same device."""
    _check_rows("bounce_blend", (3, 2), rgb=rgb, aux=aux)
    _check_index("bounce_blend", "sel", sel, rgb.device)
    if col_next.dim() != 2 or tuple(col_next.shape) != (sel.numel(), 3):
        raise ValueError("bounce_blend: col_next must be (%d,3), one row per index of sel, got %s" % (sel.numel(), tuple(col_next.shape)))
    _check_devices("bounce_blend", rgb, aux=aux, col_next=col_next)
    _need_gpu(rgb)
    return _BounceBlend.apply(rgb, aux, col_next, sel)


def bounce_pack_mid(mid, k, stages, idx, ray_o, ray_d, dpt, acc, norm, aux, rgb):
    """Write stage k's 16 `mid` channels [o | d | dpt | acc | norm | aux | rgb] into mid (R, 16 * stages) at rows idx (None: row i).  No gradient.
    The kernel stores 16-byte vectors through mid + idx[i] * 16 stages + 16 k, so `mid` must be the float32 contiguous (R, 16 stages) tensor itself
    (16-byte aligned), not a column slice or a copy; the VALUES of idx (unique, inside [0, R)) are the caller's promise.  ValueError: such a
    `mid`; k outside [0, stages); stage tensors that are not (n,3) (n,3) (n,1) (n,1) (n,3) (n,2) (n,3) with one n; an idx that is not a 1-D
    int64 tensor of n indices on the same device; idx = None with n > R."""
    stages, k = int(stages), int(k)
    if stages < 1 or not 0 <= k < stages:
        raise ValueError("bounce_pack_mid: stage k = %d outside [0, stages = %d)" % (k, stages))
    if mid.dtype != torch.float32 or mid.dim() != 2 or mid.shape[1] != 16 * stages or not mid.is_contiguous() or mid.data_ptr() % 16:
        raise ValueError("bounce_pack_mid: mid must be a contiguous, 16-byte aligned float32 (R,%d) tensor, got %s %s with strides %s"
                         % (16 * stages, mid.dtype, tuple(mid.shape), tuple(mid.stride())))
    n = _check_rows("bounce_pack_mid", (3, 3, 1, 1, 3, 2, 3), ray_o=ray_o, ray_d=ray_d, dpt=dpt, acc=acc, norm=norm, aux=aux, rgb=rgb)
    _check_devices("bounce_pack_mid", mid, ray_o=ray_o, ray_d=ray_d, dpt=dpt, acc=acc, norm=norm, aux=aux, rgb=rgb)
    if idx is not None:
        _check_index("bounce_pack_mid", "idx", idx, mid.device)
        if idx.numel() != n:
            raise ValueError("bounce_pack_mid: idx holds %d indices for %d rows" % (idx.numel(), n))
    elif n > mid.shape[0]:
        raise ValueError("bounce_pack_mid: %d rows do not fit a mid of %d" % (n, mid.shape[0]))
    _need_gpu(mid)
    lib = _lib.load()
    p = _lib.ptr
    ts = [_f32c(t.detach()) for t in (ray_o, ray_d, dpt, acc, norm, aux, rgb)]
    idx = None if idx is None else idx.contiguous()       # (held in a name: a copy made inside the call would be freed before the launch)
    _lib.check(lib.envgs_bounce_pack_mid(n, p(idx), stages, k, *[p(t) for t in ts], p(mid), _stream(mid.device)), "envgs_bounce_pack_mid")
