"""Fused front end (include/envgs_model.h): from the RAW surfel parameters -- the dict `SurfelSet.p`, `ckpt.load_model_pt` and `ckpt.PT_PARAMS`
use: _xyz, _features_dc, _features_rest, _scaling, _rotation, _opacity, and for a reflective set _specular, _roughness -- to what the two
extensions take, ONE launch each way, gradients flowing to the raw leaves.

    activate(raw)                          -> dict(means3D, shs, scales, rotations, opacities[, specular, roughness])          == ckpt.activate(raw)
    raster_inputs(raw, campos, sh_degree)  -> dict(means3D, colors_precomp (P,C), opacities, scales, rotations)
        what render() with pipe.convert_SHs_python hands the rasterizer (gaussian2d_utils.py:1066-1084); dc / rest are read in place
    tracer_inputs(raw, others=None, quads=True) -> dict(means3D, shs, opacities, scales, rotations[, others_precomp][, v, f])
        the arguments of optix_utils.py:129-185 and the get_disks quads of :39-69 (no gradient flows through v)

The activations are recomputed in the backward: no activated tensor is kept alive for it.  A surfel whose upstream gradient rows are all zero gets
raw gradients that compare == 0 (FusedAdam skips exactly those entries)."""
import torch

from . import _lib
from .raster import sh_degree_of

_RAW = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_specular", "_roughness")
_COLS = {"_xyz": (3,), "_features_dc": (1, 3), "_scaling": (2,), "_rotation": (4,), "_opacity": (1,), "_roughness": (1,)}
# forward outputs in the order of the struct; `vertices` carries no gradient
_OUTS = ("scales", "rotations", "opacities", "specular_act", "roughness_act", "shs", "colors", "others", "vertices")


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _stream(dev):
    return _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check(raw, what):
    """The shapes of the raw parameter dict (ValueError): -> (P, M, S)."""
    for k in _RAW[:6]:
        if k not in raw:
            raise ValueError("%s: the raw parameter dict lacks %s" % (what, k))
    if ("_specular" in raw) != ("_roughness" in raw):
        raise ValueError("%s: _specular and _roughness come together" % what)
    xyz = raw["_xyz"]
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("%s: _xyz must be (P,3), got %s" % (what, tuple(xyz.shape)))
    P = xyz.shape[0]
    for k in _RAW:
        if k in raw and raw[k].shape[0] != P:
            raise ValueError("%s: %s has %d rows, _xyz has %d" % (what, k, raw[k].shape[0], P))
    for k, cols in _COLS.items():
        if k in raw and tuple(raw[k].shape[1:]) != cols:
            raise ValueError("%s: %s must be (P,%s), got %s" % (what, k, ",".join(map(str, cols)), tuple(raw[k].shape)))
    rest = raw["_features_rest"]
    if rest.dim() != 3 or rest.shape[2] != 3 or not 1 <= rest.shape[1] + 1 <= 16:
        raise ValueError("%s: _features_rest must be (P,M-1,3) with 1 <= M <= 16, got %s" % (what, tuple(rest.shape)))
    S = 0
    if "_specular" in raw:
        sp = raw["_specular"]
        if sp.dim() != 2 or sp.shape[1] not in (1, 3):
            raise ValueError("%s: _specular must be (P,1) or (P,3), got %s" % (what, tuple(sp.shape)))
        S = sp.shape[1]
    return P, rest.shape[1] + 1, S


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("envgs_amd.model needs tensors on the GPU; there is no CPU path")


class _SurfelInputs(torch.autograd.Function):
    """want: the names of _OUTS to produce, returned in that order."""

    @staticmethod
    def forward(ctx, want, deg, campos, xyz, dc, rest, scaling, rotation, opacity, specular, roughness):
        ctx.set_materialize_grads(False)          # outputs the loss does not use arrive as None (= NULL upstream pointer), not as buffers of zeros
        lib = _lib.load()
        dev = xyz.device
        raws = [None if t is None else _f32c(t) for t in (xyz, dc, rest, scaling, rotation, opacity, specular, roughness)]
        xyz, dc, rest, scaling, rotation, opacity, specular, roughness = raws
        P, M, S = xyz.shape[0], rest.shape[1] + 1, (0 if specular is None else specular.shape[1])
        if "colors" in want:
            campos = _f32c(campos.detach()).reshape(-1)
        f32 = dict(dtype=torch.float32, device=dev)
        shapes = dict(scales=(P, 2), rotations=(P, 4), opacities=(P, 1), specular_act=(P, S), roughness_act=(P, 1), shs=(P, M, 3),
                      colors=(P, 3 + S + 1 if S else 3), others=(P, 2), vertices=(4 * P, 3))
        outs = {k: torch.empty(*shapes[k], **f32) for k in want}
        clamped = torch.empty(P, 3, dtype=torch.uint8, device=dev) if "colors" in want else None
        a = _lib.SurfelInputsArgs()
        a.P, a.sh_degree, a.sh_coeffs, a.spec_channels = P, deg, M, S
        p = lambda t: None if t is None else t.data_ptr()
        a.xyz, a.features_dc, a.features_rest, a.scaling, a.rotation, a.opacity = p(xyz), p(dc), p(rest) if M > 1 else None, p(scaling), p(rotation), p(opacity)
        a.specular, a.roughness, a.campos, a.clamped = p(specular), p(roughness), p(campos) if "colors" in want else None, p(clamped)
        for k in want:
            setattr(a, k, p(outs[k]))
        _lib.check(lib.envgs_surfel_inputs_forward(a, _stream(dev)), "envgs_surfel_inputs_forward")
        ctx.save_for_backward(*[t for t in raws if t is not None], *([campos, clamped] if clamped is not None else []))
        ctx.meta = (tuple(want), P, deg, M, S)
        if "vertices" in want:
            ctx.mark_non_differentiable(outs["vertices"])
        return tuple(outs[k] for k in want)

    @staticmethod
    def backward(ctx, *gs):
        lib = _lib.load()
        want, P, deg, M, S = ctx.meta
        saved = list(ctx.saved_tensors)
        xyz, dc, rest, scaling, rotation, opacity = saved[:6]
        specular, roughness = (saved[6], saved[7]) if S else (None, None)
        campos, clamped = (saved[-2], saved[-1]) if "colors" in want else (None, None)
        dev = xyz.device
        a = _lib.SurfelInputsArgs()
        a.P, a.sh_degree, a.sh_coeffs, a.spec_channels = P, deg, M, S
        p = lambda t: None if t is None else t.data_ptr()
        a.xyz, a.features_dc, a.features_rest, a.scaling, a.rotation, a.opacity = p(xyz), p(dc), p(rest) if M > 1 else None, p(scaling), p(rotation), p(opacity)
        a.specular, a.roughness, a.campos, a.clamped = p(specular), p(roughness), p(campos), p(clamped)
        keep = []                                                   # (the contiguous upstream copies stay alive until the launch)
        for k, g in zip(want, gs):
            if k != "vertices" and g is not None:
                g = _f32c(g); keep.append(g)
                setattr(a, "g_" + k, p(g))
        d_xyz = torch.empty_like(xyz) if "colors" in want else None
        d = [torch.empty_like(t) if t is not None else None for t in (dc, rest, scaling, rotation, opacity, specular, roughness)]
        a.d_xyz = p(d_xyz)
        a.d_features_dc, a.d_features_rest, a.d_scaling, a.d_rotation, a.d_opacity, a.d_specular, a.d_roughness = [p(t) if t is None or t.numel() else None for t in d]
        _lib.check(lib.envgs_surfel_inputs_backward(a, _stream(dev)), "envgs_surfel_inputs_backward")
        return (None, None, None, d_xyz, *d)


def _apply(raw, want, deg=0, campos=None):
    outs = _SurfelInputs.apply(tuple(want), int(deg), campos, raw["_xyz"], raw["_features_dc"], raw["_features_rest"], raw["_scaling"], raw["_rotation"],
                               raw["_opacity"], raw.get("_specular"), raw.get("_roughness"))
    return dict(zip(want, outs))


def activate(raw):
    """ckpt.activate(raw) in one launch each way: exp scaling, normalised rotation, sigmoid opacity / specular / roughness, shs = cat(dc, rest);
    means3D is the _xyz tensor itself."""
    P, M, S = _check(raw, "activate")
    _need_gpu(*[raw.get(k) for k in _RAW])
    o = _apply(raw, ["shs", "scales", "rotations", "opacities"] + (["specular_act", "roughness_act"] if S else []))
    out = dict(means3D=raw["_xyz"], shs=o["shs"], scales=o["scales"], rotations=o["rotations"], opacities=o["opacities"])
    if S:
        out["specular"], out["roughness"] = o["specular_act"], o["roughness_act"]
    return out


def raster_inputs(raw, campos, sh_degree):
    """What render() with convert_SHs_python hands the rasterizer: colors_precomp (P,C) = [clamp_min(eval_sh(D, features, normalize(xyz - campos))
    + 0.5, 0) | sigmoid(specular) | sigmoid(roughness)] (C = 3+S+1, or 3 for a set without reflection parameters), opacities, scales,
    rotations, and means3D = the _xyz tensor itself.  envgs_step.base_pass takes the dict as `base` (it uses the colors_precomp key)."""
    P, M, S = _check(raw, "raster_inputs")
    deg = sh_degree_of(sh_degree)
    if not 0 <= deg <= 3 or (deg + 1) ** 2 > M:
        raise ValueError("raster_inputs: SH degree %d needs %d coefficients, the set has %d" % (deg, (deg + 1) ** 2, M))
    _need_gpu(campos, *[raw.get(k) for k in _RAW])
    o = _apply(raw, ["colors", "opacities", "scales", "rotations"], deg, campos)
    return dict(means3D=raw["_xyz"], colors_precomp=o["colors"], opacities=o["opacities"], scales=o["scales"], rotations=o["rotations"])


def tracer_inputs(raw, others=None, quads=True):
    """The tracer's arguments: shs = cat(dc, rest), opacities, scales, rotations, means3D = the _xyz tensor itself;
    others_precomp (P,2) = [sigmoid(specular), sigmoid(roughness)] -- by default iff the set has a single-channel _specular, ValueError when asked
    for without one; with `quads` the get_disks vertices v (4P,3) (no gradient) and the cached face table f (2P,3) of fused.surfel_quads.
    envgs_step.env_prepare / env_pass take the dict as `env` (they use the v key)."""
    P, M, S = _check(raw, "tracer_inputs")
    if others is None:
        others = S == 1
    elif others and S != 1:
        raise ValueError("tracer_inputs: others_precomp needs a single-channel _specular, the set has %d channels" % S)
    _need_gpu(*[raw.get(k) for k in _RAW])
    o = _apply(raw, ["shs", "opacities", "scales", "rotations"] + (["others"] if others else []) + (["vertices"] if quads else []))
    out = dict(means3D=raw["_xyz"], shs=o["shs"], opacities=o["opacities"], scales=o["scales"], rotations=o["rotations"])
    if others:
        out["others_precomp"] = o["others"]
    if quads:
        from . import fused
        f = fused._FACES.get((raw["_xyz"].device.index, P))
        if f is None:                                               # first call for this P: fused.surfel_quads fills its face cache
            _, f = fused.surfel_quads(raw["_xyz"], o["scales"], o["rotations"])
        out["v"], out["f"] = o["vertices"], f
    return out
