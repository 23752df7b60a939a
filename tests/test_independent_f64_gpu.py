"""GPU: the HIP extensions DIRECTLY against float64 autograd of the torch-eager twins (oracle/eager.py, oracle/eager_trace.py) -- no C oracle in
between.  VERDICT r4 ("oracle independence shrank"): since round 4 the ill-conditioned core of the rasterizer has one canonical fp32 operation
order shared by the HIP kernels and the C oracle, so their tight agreement (1e-4 per element, the parity suite) no longer says much about that
order itself; the chain to ground truth ran HIP ~ C oracle (GPU) and C oracle ~ float64 autograd (CPU, tests/test_oracle_grad.py,
tests/test_oracle_trace.py).  This file closes the triangle with the third side: dense float64 evaluation (every pixel x every surfel, no tiles, no
lists, no atomics, true derivatives from autograd) against the HIP result.  Asserted: 5e-5 of the tensor's scale for values, 2e-4 for gradients
(measured: values <= 6.7e-6, gradients <= 4.0e-5 -- the CPU leg C oracle ~ float64 asserts 2e-4 / 2e-3; on the two saturated scenes of
tests/saturated_scenes.py: values <= 1.2e-5, gradients <= 4.1e-5, where the C oracle itself is 1.2e-5 / 4.0e-5 away from float64).

The SH cases run at every degree 0..3 over 16 stored coefficients whose inactive part is large (tests/test_sh_degree_ladder.py:ladder_shs): float64 autograd
never reads a coefficient beyond (D+1)^2 and gives it a zero gradient, so a leak in a kernel shows against ground truth, not only against the C oracle."""
import numpy as np
import pytest
import torch

from envgs_amd import synth
from oracle import eager, eager_trace
from tests.util import scene_for, small_fx, cam_args, rel_err, record
from tests.test_oracle_trace import trace_scene
from tests.test_sh_degree_ladder import ladder_shs

pytestmark = pytest.mark.gpu


def _sh_cases(lead, tail):
    """The degree-3 case keeps its id; degrees 0..2 are added behind it."""
    return [pytest.param(*lead, 3, id="-".join(str(x) for x in lead))] + [pytest.param(*lead, d, id="-".join(str(x) for x in lead) + "-D%d" % d) for d in (0, 1, 2)] + \
           [pytest.param(*t, 0, id="-".join(str(x) for x in t)) for t in tail]


def _with_axes(cases, extra):
    """The earlier cases keep their ids and get an empty `axes`; `extra` = (id, values, axes) are appended."""
    return [pytest.param(*c.values, {}, id=c.id) for c in cases] + [pytest.param(*v, ax, id=i) for i, v, ax in extra]


# cameras, scale modifiers and an image below one tile in each direction that the orbit camera at modifier 1 does not reach (tests/util.py: CAMERAS).
# in_cloud at P=600, seed 3 and the others at P=300, seed 3: the float64 twin's radii equal the fp32 ones (tests/test_oracle_grad.py runs the same inputs)
_RASTER_AXES = [("in_cloud", (True, 3, 3), dict(camera="in_cloud", P=600)), ("aniso", (True, 3, 3), dict(camera="aniso")),
                ("mod0.5", (False, 5, 0), dict(scale_modifier=0.5)), ("mod1.7", (True, 3, 3), dict(scale_modifier=1.7)),
                ("17x15", (True, 3, 2), dict(HW=(17, 15), fx=small_fx(15))),
                # surfels on a surface, 40 % at opacity 1.0f: capped blends and pixels that end after two or three hits (tests/saturated_scenes.py).  No pixel of
                # this scene is audited, and the C oracle's own distance from float64 on it is recorded by tests/test_saturated_scenes_cpu.py
                ("saturated_sphere300", (True, 3, 3), dict(saturated=True))]


def _upstream_raster(C, H, W):
    gen = torch.Generator().manual_seed(4)
    dcol = torch.randn(C, H, W, generator=gen) / (H * W)
    dall = torch.randn(7, H, W, generator=gen) / (H * W); dall[5:] = 0          # (median depth: a selection; distortion: an fp32 cancellation -- both compared as values only)
    return dcol, dall


def saturated_raster_leg_inputs():
    """(g, cam, case, bg, dcol, dall) of the saturated rasterizer case (also read by the CPU file that measures the C oracle on the same inputs)."""
    from tests.saturated_scenes import raster_scene
    g, cam, c = raster_scene("sphere300_f64")
    return (g, cam, c, torch.tensor([0.3, 0.6, 0.1])) + _upstream_raster(3, c["H"], c["W"])


def float64_raster(g, cam, sh, deg, bg, dcol, dall, sm=1.0):
    """Float64 ground truth: the leaves (with their gradients) and (color, radii, allmap, weight) of oracle/eager.py."""
    d = torch.float64
    ca = cam_args(cam)
    names = ("means3D", "opacities", "scales", "rotations", "shs" if sh else "colors_precomp")
    L64 = {k: g[k].to(d).requires_grad_(True) for k in names}
    c64, r64, a64, w64 = eager.rasterize(L64["means3D"], L64["opacities"], ca["viewmatrix"].to(d), ca["projmatrix"].to(d), ca["campos"].to(d), ca["W"], ca["H"],
                                         scales=L64["scales"], rotations=L64["rotations"], shs=L64.get("shs"), colors_precomp=L64.get("colors_precomp"), sh_degree=deg, bg=bg,
                                         scale_modifier=sm)
    ((c64 * dcol.to(d)).sum() + (a64 * dall.to(d)).sum()).backward()
    return L64, (c64, r64, a64, w64)


@pytest.mark.parametrize("sh,C,deg,axes", _with_axes(_sh_cases((True, 3), [(False, 5), (False, 7)]), _RASTER_AXES))
def test_rasterizer_vs_float64_autograd(sh, C, deg, axes, request):
    import importlib
    mod = importlib.import_module({3: "diff_surfel_rasterization_wet", 5: "diff_surfel_rasterization_wet_ch05", 7: "diff_surfel_rasterization_wet_ch07"}[C])
    dev = torch.device("cuda:0")
    sm = axes.get("scale_modifier", 1.0)
    H, W = axes.get("HW", (48, 64))
    if axes.get("saturated"):
        g, cam, _, bg, dcol, dall = saturated_raster_leg_inputs()
    else:
        g, cam = scene_for(axes.get("camera", "orbit"), P=axes.get("P", 300), H=H, W=W, seed=3, C=C, sh=sh, fx=axes.get("fx"))
        if sh:
            g["shs"] = ladder_shs(g["shs"], deg)
        bg = torch.tensor([0.3, 0.6, 0.1])
        dcol, dall = _upstream_raster(C, cam.image_height, cam.image_width)
    ca = cam_args(cam)
    W, H = ca["W"], ca["H"]
    # ---- float64 ground truth
    names = ("means3D", "opacities", "scales", "rotations", "shs" if sh else "colors_precomp")
    L64, (c64, r64, a64, w64) = float64_raster(g, cam, sh, deg, bg, dcol, dall, sm)
    # ---- HIP
    st = mod.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg.to(dev), scale_modifier=sm,
                                           viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev), sh_degree=torch.tensor([deg], device=dev),
                                           campos=cam.camera_center.to(dev), prefiltered=False, debug=False)
    Lh = {k: g[k].to(dev).requires_grad_(True) for k in names}
    m2 = torch.zeros_like(Lh["means3D"], requires_grad=True)
    color, radii, allmap, weight = mod.GaussianRasterizer(raster_settings=st)(means3D=Lh["means3D"], means2D=m2, shs=Lh.get("shs"), colors_precomp=Lh.get("colors_precomp"),
                                                                             opacities=Lh["opacities"], scales=Lh["scales"], rotations=Lh["rotations"], cov3D_precomp=None)
    ((color * dcol.to(dev)).sum() + (allmap * dall.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    n = lambda t: t.detach().cpu().double().numpy()
    test = "hip_vs_float64.raster_C%d" % C + ("_D%d" % deg if sh else "") + ("." + request.node.callspec.id if axes else "")
    np.testing.assert_array_equal(radii.cpu().numpy(), r64.numpy())
    errs = {"color": rel_err(n(color), n(c64)), "weight": rel_err(n(weight).reshape(-1), n(w64).reshape(-1))}
    for ch, nm in ((0, "depth"), (1, "alpha"), (2, "normal.x"), (3, "normal.y"), (4, "normal.z")):
        errs["allmap." + nm] = rel_err(n(allmap[ch]), n(a64[ch]))
    for k, e in errs.items():
        record(test, k, e, "(max|a-b|/max|b| against float64 eager)")
        assert e < 5e-5, (k, e)
    assert rel_err(n(allmap[6]), n(a64[6])) < 5e-3
    q = g["rotations"].double()
    proj = lambda v: v - (v * q).sum(-1, keepdim=True) * q              # the kernel returns dL/d(q/|q|); torch's normalize backward projects it
    for k in names:
        a, b = Lh[k].grad.cpu().double(), L64[k].grad
        if k == "rotations":
            a, b = proj(a), proj(b)
        e = rel_err(a.reshape(b.shape).numpy(), b.numpy())
        record(test, "d" + k, e, "(max|a-b|/max|b| against float64 autograd)")
        assert e < 2e-4, (k, e)
    if sh and deg < 3:
        assert float(Lh["shs"].grad[:, (deg + 1) ** 2:].abs().max()) == 0.0          # as in float64: exactly nothing beyond the active degree


def _upstream_tracer(R):
    gen = torch.Generator().manual_seed(9)
    return [torch.randn(R, c, generator=gen) / R for c in (3, 1, 1, 3, 2)]


def saturated_tracer_leg_inputs():
    """(g, ro, rd, case, bg, upstream gradients) of the saturated tracer case (also read by the CPU file that measures the C oracle on the same inputs)."""
    from tests.saturated_scenes import trace_scene_of
    g, ro, rd, c = trace_scene_of("room200")
    return g, ro, rd, c, torch.tensor([0.2, 0.5, 0.7]), _upstream_tracer(ro.shape[0])


def float64_tracer(g, ro, rd, use_sh, camera, deg, bg, ups, sm=1.0):
    """Float64 ground truth: the leaves and rays (with their gradients) and (rgb, dpt, acc, norm, aux, wet) of oracle/eager_trace.py."""
    d = torch.float64
    R = ro.shape[0]
    names = ["means3D", "scales", "rotations", "opacities", "others", "shs" if use_sh else "colors_precomp"]
    L64 = {k: g[k].to(d).requires_grad_(True) for k in names}
    o64, d64 = ro.to(d).requires_grad_(True), rd.to(d).requires_grad_(True)
    outs = eager_trace.trace(o64, d64, L64["means3D"], L64["scales"], L64["rotations"], L64["opacities"], shs=L64.get("shs"),
                             colors_precomp=L64.get("colors_precomp"), others=L64["others"], sh_degree=deg, bg=bg.to(d), start_from_first=camera,
                             scale_modifier=sm)
    sum((x.reshape(R, -1) * u.to(d)).sum() for x, u in zip(outs[:5], ups)).backward()
    return L64, o64, d64, outs


@pytest.mark.parametrize("use_sh,camera,deg,axes", _with_axes(_sh_cases((True, True), [(False, False)]),
                                                                [("True-True-mod1.7", (True, True, 3), dict(scale_modifier=1.7)),
                                                                 ("False-False-mod1.7", (False, False, 0), dict(scale_modifier=1.7)),
                                                                 # surfels on a wall, 40 % at opacity 1.0f, a third of the rays aimed into a cap zone (no audited ray)
                                                                 ("saturated_room200", (True, True, 3), dict(saturated=True))]))
def test_tracer_vs_float64_autograd(use_sh, camera, deg, axes):
    sm = axes.get("scale_modifier", 1.0)
    import diff_surfel_tracing as tpkg
    dev = torch.device("cuda:0")
    if axes.get("saturated"):
        g, ro, rd, _, bg, ups = saturated_tracer_leg_inputs()
    else:
        g, ro, rd = trace_scene(P=200, R=400, seed=7, camera=camera)
        if use_sh:
            g["shs"] = ladder_shs(g["shs"], deg)
        bg = torch.tensor([0.2, 0.5, 0.7])
        ups = _upstream_tracer(ro.shape[0])
    R = ro.shape[0]
    names = ["means3D", "scales", "rotations", "opacities", "others", "shs" if use_sh else "colors_precomp"]
    L64, o64, d64, (rgb, dpt, acc, norm, aux, wet) = float64_tracer(g, ro, rd, use_sh, camera, deg, bg, ups, sm)
    ts = tpkg.SurfelTracingSettings(image_height=1, image_width=1, tanfovx=1.0, tanfovy=1.0, bg=bg.to(dev), scale_modifier=sm, viewmatrix=torch.eye(4, device=dev),
                                    projmatrix=torch.eye(4, device=dev), sh_degree=torch.tensor([deg], device=dev), campos=torch.zeros(3, device=dev), prefiltered=False,
                                    debug=False, max_trace_depth=0, specular_threshold=0.0)
    Lh = {k: g[k].to(dev).requires_grad_(True) for k in names}
    o, dd = ro.to(dev).requires_grad_(True), rd.to(dev).requires_grad_(True)
    v, f = synth.get_disks(Lh["means3D"].detach(), Lh["scales"].detach() * sm, Lh["rotations"].detach())      # the 3-sigma quads of the MODIFIED surfels
    t = tpkg.SurfelTracer(); t.build_acceleration_structure(v, f, rebuild=True)
    outs = t(o, dd, v, means3D=Lh["means3D"], grads3D=None, shs=Lh.get("shs"), colors_precomp=Lh.get("colors_precomp"), others_precomp=Lh["others"], opacities=Lh["opacities"],
             scales=Lh["scales"], rotations=Lh["rotations"], cov3D_precomp=None, tracer_settings=ts, start_from_first=camera)
    sum((outs[i].reshape(R, -1) * u.to(dev)).sum() for i, u in zip((0, 1, 2, 3, 5), ups)).backward()
    torch.cuda.synchronize()
    n = lambda x: x.detach().cpu().double().numpy()
    test = "hip_vs_float64.tracer_%s" % ("sh_D%d" % deg if use_sh else "rgb") + (".saturated_room200" if axes.get("saturated") else ".mod%g" % sm if axes else "")
    for nm, a, b in (("rgb", outs[0], rgb), ("dpt", outs[1], dpt), ("acc", outs[2], acc), ("norm", outs[3], norm), ("aux", outs[5], aux), ("wet", outs[7], wet)):
        e = rel_err(n(a).reshape(n(b).shape), n(b))
        record(test, nm, e, "(against float64 eager)")
        assert e < 5e-5, (nm, e)
    q = g["rotations"].double()
    proj = lambda x: x - (x * q).sum(-1, keepdim=True) * q
    for k in names:
        a, b = Lh[k].grad.cpu().double(), L64[k].grad
        if k == "rotations":
            a, b = proj(a), proj(b)
        e = rel_err(a.reshape(b.shape).numpy(), b.numpy())
        record(test, "d" + k, e, "(against float64 autograd)")
        assert e < 2e-4, (k, e)
    if use_sh and deg < 3:
        assert float(Lh["shs"].grad[:, (deg + 1) ** 2:].abs().max()) == 0.0
    for nm, a, b in (("dray_o", o.grad, o64.grad), ("dray_d", dd.grad, d64.grad)):
        e = rel_err(n(a), n(b))
        record(test, nm, e, "(against float64 autograd)")
        assert e < 2e-4, (nm, e)
