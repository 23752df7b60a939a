"""Fused losses.  (1) Image loss  w_l1 * mean|x - y| + w_ssim * (1 - ssim(x, y))  (include/envgs_loss.h).

`l1_ssim_loss(x, y)` with the default weights is the supervision EnvGS trains with (configs/models/envgs.yaml:70-72; L1 and SSIM branches of
easyvolcap/models/supervisors/volumetric_video_supervisor.py:40-66,112-144 -> loss_utils.l1 :319-333 and ssim_utils.ssim :107-167).
x, y: (C, H, W) -- any strides, any float dtype; the gradient flows to x only (y is the ground truth).
(2) `EnvGSGeometryLoss`: the geometry regularisers of the same training recipe (include/envgs_supervisor.h; configs/models/envgs.yaml:74-81)."""
import torch

from . import _lib


def _stream(dev):
    return _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _L1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, w_l1, w_ssim):
        lib = _lib.load()
        if x.device.type != "cuda":
            raise RuntimeError("l1_ssim_loss needs GPU tensors; there is no CPU path")
        if x.shape != y.shape or x.dim() != 3:
            raise ValueError("l1_ssim_loss expects two (C, H, W) images of the same shape")
        C, H, W = x.shape
        if H < 11 or W < 11:
            raise ValueError("SSIM needs H, W >= 11 (the reference skips it below that)")
        dev = x.device
        xc = x.detach().to(torch.float32).contiguous(); yc = y.detach().to(torch.float32).contiguous()
        need = ctx.needs_input_grad[0]
        nb = lib.envgs_l1_ssim_partial_count(C, H, W)
        partial = torch.empty(nb, 2, dtype=torch.float32, device=dev)
        maps = torch.empty(3, C, H, W, dtype=torch.float32, device=dev) if need else None
        p = _lib.ptr
        _lib.check(lib.envgs_l1_ssim_forward(C, H, W, p(xc), p(yc), p(maps), p(partial), _stream(dev)), "envgs_l1_ssim_forward")
        sums = partial.double().sum(0) / float(C * H * W)              # (mean ssim, mean |x - y|): tile sums added in double
        loss = (w_l1 * sums[1] + w_ssim * (1.0 - sums[0])).to(torch.float32)
        ctx.saved = (xc, yc, maps, float(w_l1), float(w_ssim), x.dtype)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        xc, yc, maps, w_l1, w_ssim, dt = ctx.saved
        C, H, W = xc.shape
        dx = torch.empty_like(xc)
        go = g.detach().to(torch.float32).reshape(1).contiguous()
        p = _lib.ptr
        _lib.check(lib.envgs_l1_ssim_backward(C, H, W, p(xc), p(yc), p(maps), p(go), w_l1, w_ssim, p(dx), _stream(xc.device)), "envgs_l1_ssim_backward")
        return dx.to(dt), None, None, None


def l1_ssim_loss(x, y, w_l1=0.8, w_ssim=0.2):
    return _L1SSIM.apply(x, y, w_l1, w_ssim)


# ---- geometry regularisers of the EnvGS supervisor (include/envgs_supervisor.h) ------------------------------------------------------------
_TERMS = ("norm_loss", "gs_norm_loss", "msk_loss", "gs_dist_loss", "env_opacity_loss")          # columns ENVGS_SUP_NORM .. ENVGS_SUP_ENV
_F_NORM, _F_GS_NORM, _F_MSK, _F_DIST, _F_ENV_SPARSE, _F_ENV_L1, _F_NORM_ACC, _F_NORM_DPT, _F_GS_NORM_ACC, _F_GS_NORM_DPT = (1 << i for i in range(10))

# constructor options of the reference's EnvGSSupervisor that its compute_loss never reads, or whose branch is not built here
# (max_dpt_scale_percet: the torch.quantile mask), with the reference's defaults: anything else is refused
_UNSUPPORTED = dict(
    norm_loss_weight_final=None, max_dpt_scale_percet=False, use_spec_scale_norm_loss=False, use_spec_scale_norm_loss_start_iter=7000,
    use_spec_scale_norm_loss_until_iter=None, gs_norm_loss_weight_final=None, use_spec_scale_gs_norm_loss=False,
    use_spec_scale_gs_norm_loss_start_iter=7000, use_spec_scale_gs_norm_loss_until_iter=None, norm_smooth_loss_weight=0.0,
    norm_smooth_loss_start_iter=7000, norm_smooth_loss_until_iter=None, use_edge_aware_smooth=True, use_dpt_scale_norm_smooth_loss=True,
    res_norm_loss_weight=0.001, specular_loss_weight=0.0, specular_loss_start_iter=7000, specular_loss_until_iter=9000, specular_target=0.8,
    min_specular_percent=0.5, ref_rgb_loss_weight=0.0, ref_rgb_loss_start_iter=7000, ref_rgb_loss_until_iter=9000)


class _Geometry(torch.autograd.Function):
    """inputs: flat float32 GPU tensors or None -- norm_map (N,3), surf_norm_map (N,3), acc_map (N), dist_map (N), env_opacity (P) [differentiable];
    dpt_map (N), prior (N,3), msk (N), R (9) [constants].  -> (loss, the five term means)."""

    @staticmethod
    def forward(ctx, flags, weights, norm_map, surf_norm_map, acc_map, dist_map, env_opacity, dpt_map, prior, msk, R):
        lib = _lib.load()
        maps = [t for t in (norm_map, surf_norm_map, acc_map, dist_map, dpt_map, prior, msk) if t is not None]
        dev = (maps[0] if maps else env_opacity).device
        N = maps[0].shape[0] if maps else 1          # only the opacity term: one pixel workgroup runs empty and writes a zero row
        P = env_opacity.shape[0] if flags & (_F_ENV_SPARSE | _F_ENV_L1) else 0
        st, p = _stream(dev), _lib.ptr
        a = _lib.SupervisorArgs()
        a.N, a.P, a.flags = N, P, flags
        a.weight[:] = weights
        near_far = None
        if flags & (_F_NORM_DPT | _F_GS_NORM_DPT):
            if N < 100:
                raise ValueError("the depth scale takes the int(0.01 N)-th smallest / largest depth: it needs N >= 100 pixels, got %d" % N)
            near_far = torch.empty(2, dtype=torch.float32, device=dev)
            nbytes = lib.envgs_depth_percentiles_temp_bytes()
            temp = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
            _lib.check(lib.envgs_depth_percentiles(N, p(dpt_map), dpt_map.stride(0), p(near_far), p(temp), nbytes, st), "envgs_depth_percentiles")
        # one allocation for every gradient map that is wanted and that a selected term feeds
        want = (("g_norm_map", 0, 3 * N, flags & (_F_NORM | _F_GS_NORM)), ("g_surf_norm_map", 1, 3 * N, flags & _F_GS_NORM), ("g_acc_map", 2, N, flags & _F_MSK),
                ("g_dist_map", 3, N, flags & _F_DIST), ("g_env_opacity", 4, P, flags & (_F_ENV_SPARSE | _F_ENV_L1)))
        layout, total = [], 0
        for name, slot, n, fed in want:
            if fed and ctx.needs_input_grad[2 + slot]:
                layout.append((name, slot, total, n))
                total += n
        gbuf = torch.empty(total, dtype=torch.float32, device=dev) if total else None
        for name, slot, off, n in layout:
            setattr(a, name, gbuf.data_ptr() + 4 * off)
        for name, t in (("norm_map", norm_map), ("surf_norm_map", surf_norm_map), ("acc_map", acc_map), ("dpt_map", dpt_map), ("dist_map", dist_map),
                        ("env_opacity", env_opacity), ("prior", prior), ("msk", msk)):
            if t is not None:
                setattr(a, name, t.data_ptr())
                setattr(a, name + "_row", t.stride(0))
                if t.dim() == 2:
                    setattr(a, name + "_ch", t.stride(1))
        if R is not None:
            a.R = R.data_ptr()
        if near_far is not None:
            a.near_far = near_far.data_ptr()
        partial = torch.empty(lib.envgs_supervisor_partial_count(N, P), 5, dtype=torch.float32, device=dev)
        a.partial = partial.data_ptr()
        out = torch.empty(6, dtype=torch.float32, device=dev)
        _lib.check(lib.envgs_supervisor_forward(a, st), "envgs_supervisor_forward")
        _lib.check(lib.envgs_supervisor_finish(a, p(out), st), "envgs_supervisor_finish")
        ctx.saved = (gbuf, layout, N, P)             # an internal buffer, neither input nor output of the node: kept on ctx as _L1SSIM does
        loss, stats = out[5], out[:5]
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g, _g_stats):
        gbuf, layout, N, P = ctx.saved
        grads = [None] * 5
        if gbuf is not None:
            lib = _lib.load()
            go = g.detach().to(torch.float32).reshape(1).contiguous()
            dst = torch.empty_like(gbuf)
            p = _lib.ptr
            _lib.check(lib.envgs_supervisor_backward(gbuf.numel(), p(gbuf), p(go), p(dst), _stream(gbuf.device)), "envgs_supervisor_backward")
            for name, slot, off, n in layout:
                v = dst[off:off + n]
                grads[slot] = v.view(N, 3) if slot < 2 else v
        return (None, None, *grads, None, None, None, None)


class EnvGSGeometryLoss:
    """The regularisers of the reference's EnvGSSupervisor.compute_loss (easyvolcap/models/supervisors/envgs_supervisor.py:139-235) as one fused
    HIP pass: `loss, scalar_stats = reg(output, batch, iter)`.

    Constructed with the reference's keyword names and defaults (note: its start iterations default to 7000 / 3000; configs/models/envgs.yaml sets
    them to 0).  `output` / `batch` are mappings: output.norm_map (1,N,3), surf_norm_map (1,N,3), acc_map (1,N,1), dpt_map (1,N,1),
    dist_map (1,N,1), env_opacity (P,1); batch.norm (1,N,3; stored as n/2 + 1/2), batch.R (1,3,3), batch.msk (1,N,1).  Any strides: (H,W,3) views of
    (3,H,W) planes are read in place.  A term whose keys are missing, whose weight is 0 or whose [start_iter, until_iter) window does not hold
    `iter` is skipped, as in the reference.  Returns the weighted sum as a device scalar and a dict of device scalars named like the reference's
    scalar_stats.  Gradients flow to norm_map, surf_norm_map, dist_map, env_opacity and (from msk_loss only) acc_map; dpt_map and acc_map as
    scales are constants.  One view per call; no host synchronisation anywhere.

    One deliberate deviation from the reference: when the two depth percentiles coincide (more than 99 % of dpt_map holds one value, far == near)
    the reference's normalize_depth divides 0 by 0 and its loss is NaN.  Here the depth scale is then 0 where d == near, 0 where d > near and 1
    where d < near, and the loss and every gradient stay finite (tests/test_supervisor_shapes_gpu.py pins it)."""

    def __init__(self, norm_loss_weight=0.0, norm_loss_start_iter=7000, norm_loss_until_iter=None, use_acc_scale_norm_loss=False,
                 use_dpt_scale_norm_loss=False, gs_norm_loss_weight=0.0, gs_dist_loss_weight=0.0, gs_norm_loss_start_iter=7000,
                 gs_norm_loss_until_iter=None, use_acc_scale_gs_norm_loss=False, use_dpt_scale_gs_norm_loss=False, gs_dist_loss_start_iter=3000,
                 gs_dist_loss_until_iter=None, env_opacity_loss_weight=0.0, env_opacity_loss_type="sparse", env_opacity_loss_start_iter=0,
                 msk_loss_weight=0.0, msk_loss_start_iter=7000, msk_loss_until_iter=None, **kwargs):
        for k, v in kwargs.items():
            if k not in _UNSUPPORTED:
                raise TypeError("EnvGSGeometryLoss: unknown option %r" % k)
            if v != _UNSUPPORTED[k]:
                raise NotImplementedError("EnvGSGeometryLoss: option %s=%r is outside the fused terms (only its default %r is accepted)" % (k, v, _UNSUPPORTED[k]))
        if env_opacity_loss_type not in ("sparse", "l1"):
            raise ValueError("env_opacity_loss_type must be 'sparse' or 'l1', got %r" % (env_opacity_loss_type,))
        self.norm_loss_weight, self.norm_loss_start_iter, self.norm_loss_until_iter = norm_loss_weight, norm_loss_start_iter, norm_loss_until_iter
        self.use_acc_scale_norm_loss, self.use_dpt_scale_norm_loss = bool(use_acc_scale_norm_loss), bool(use_dpt_scale_norm_loss)
        self.gs_norm_loss_weight, self.gs_norm_loss_start_iter, self.gs_norm_loss_until_iter = gs_norm_loss_weight, gs_norm_loss_start_iter, gs_norm_loss_until_iter
        self.use_acc_scale_gs_norm_loss, self.use_dpt_scale_gs_norm_loss = bool(use_acc_scale_gs_norm_loss), bool(use_dpt_scale_gs_norm_loss)
        self.gs_dist_loss_weight, self.gs_dist_loss_start_iter, self.gs_dist_loss_until_iter = gs_dist_loss_weight, gs_dist_loss_start_iter, gs_dist_loss_until_iter
        self.env_opacity_loss_weight, self.env_opacity_loss_type, self.env_opacity_loss_start_iter = env_opacity_loss_weight, env_opacity_loss_type, env_opacity_loss_start_iter
        self.msk_loss_weight, self.msk_loss_start_iter, self.msk_loss_until_iter = msk_loss_weight, msk_loss_start_iter, msk_loss_until_iter

    @staticmethod
    def _open(it, start, until):
        return it >= start and (until is None or it < until)

    def active_terms(self, output, batch, iter):
        """(flags, weights) of the terms the reference would evaluate for these keys at this iteration."""
        if torch.is_tensor(iter) and iter.device.type != "cpu":
            raise TypeError("iter must be a host integer (reading a device tensor would synchronise)")
        it = int(iter)
        flags, w = 0, [0.0] * 5
        if "env_opacity" in output and self.env_opacity_loss_weight > 0 and it >= self.env_opacity_loss_start_iter:
            flags |= _F_ENV_SPARSE if self.env_opacity_loss_type == "sparse" else _F_ENV_L1
            w[4] = float(self.env_opacity_loss_weight)
        if "norm_map" in output and "norm" in batch and self.norm_loss_weight > 0 and self._open(it, self.norm_loss_start_iter, self.norm_loss_until_iter):
            flags |= _F_NORM | (_F_NORM_ACC if self.use_acc_scale_norm_loss else 0) | (_F_NORM_DPT if self.use_dpt_scale_norm_loss else 0)
            w[0] = float(self.norm_loss_weight)
        if "norm_map" in output and "surf_norm_map" in output and self.gs_norm_loss_weight > 0 and \
                self._open(it, self.gs_norm_loss_start_iter, self.gs_norm_loss_until_iter):
            flags |= _F_GS_NORM | (_F_GS_NORM_ACC if self.use_acc_scale_gs_norm_loss else 0) | (_F_GS_NORM_DPT if self.use_dpt_scale_gs_norm_loss else 0)
            w[1] = float(self.gs_norm_loss_weight)
        if "acc_map" in output and self.msk_loss_weight > 0 and self._open(it, self.msk_loss_start_iter, self.msk_loss_until_iter):
            flags |= _F_MSK
            w[2] = float(self.msk_loss_weight)
        if "dist_map" in output and self.gs_dist_loss_weight > 0 and self._open(it, self.gs_dist_loss_start_iter, self.gs_dist_loss_until_iter):
            flags |= _F_DIST
            w[3] = float(self.gs_dist_loss_weight)
        return flags, w

    def __call__(self, output, batch, iter):
        flags, w = self.active_terms(output, batch, iter)
        some = next((v for v in list(output.values()) + list(batch.values()) if torch.is_tensor(v) and v.device.type == "cuda"), None)
        if some is None:
            raise RuntimeError("EnvGSGeometryLoss needs GPU tensors; there is no CPU path")
        if not flags:
            return torch.zeros((), dtype=torch.float32, device=some.device), {}
        need = dict(norm_map=flags & (_F_NORM | _F_GS_NORM), surf_norm_map=flags & _F_GS_NORM, acc_map=flags & (_F_MSK | _F_NORM_ACC | _F_GS_NORM_ACC),
                    dist_map=flags & _F_DIST, env_opacity=flags & (_F_ENV_SPARSE | _F_ENV_L1), dpt_map=flags & (_F_NORM_DPT | _F_GS_NORM_DPT),
                    norm=flags & (_F_NORM | _F_MSK), msk=flags & _F_MSK, R=flags & _F_NORM)
        flat, N = {}, None
        for key, used in need.items():
            if not used:
                flat[key] = None
                continue
            src = batch if key in ("norm", "msk", "R") else output
            if key not in src:
                raise KeyError("EnvGSGeometryLoss: the selected terms read %r, which is missing" % key)
            t = src[key]
            if t.device.type != "cuda":
                raise RuntimeError("EnvGSGeometryLoss needs GPU tensors; there is no CPU path (%s is on %s)" % (key, t.device))
            t = t.to(torch.float32)
            if key == "R":
                if t.numel() != 9:
                    raise ValueError("EnvGSGeometryLoss handles one view per call (B = 1): batch.R has shape %s" % (tuple(t.shape),))
                flat[key] = t.detach().reshape(9).contiguous()
                continue
            if key in ("norm_map", "surf_norm_map", "norm"):
                if t.dim() < 2 or t.shape[-1] != 3:
                    raise ValueError("%s must be channel-last (..., 3), got %s" % (key, tuple(t.shape)))
                t = t.reshape(-1, 3)
            else:
                t = t.reshape(-1)
            if key != "env_opacity":
                if N is None:
                    N = t.shape[0]
                elif t.shape[0] != N:
                    raise ValueError("EnvGSGeometryLoss: %s has %d pixels, other maps have %d" % (key, t.shape[0], N))
            elif t.shape[0] < 1:
                raise ValueError("env_opacity is empty")
            flat[key] = t.detach() if key in ("dpt_map", "norm", "msk") else t
        loss, vec = _Geometry.apply(flags, w, flat["norm_map"], flat["surf_norm_map"], flat["acc_map"], flat["dist_map"], flat["env_opacity"],
                                    flat["dpt_map"], flat["norm"], flat["msk"], flat["R"])
        on = dict(norm_loss=flags & _F_NORM, gs_norm_loss=flags & _F_GS_NORM, msk_loss=flags & _F_MSK, gs_dist_loss=flags & _F_DIST,
                  env_opacity_loss=flags & (_F_ENV_SPARSE | _F_ENV_L1))
        return loss, {name: vec[i] for i, name in enumerate(_TERMS) if on[name]}
