"""Every SH colour path at each degree and coefficient count.

The reference starts training at active_sh_degree = 0 and raises it one step at a time up to 3 while the (P, 16, 3) coefficient block is stored
throughout (gaussian2d_utils.py:294, oneupSHdegree at :402): the first thousands of iterations of every run evaluate degrees 0, 1 and 2 over 16
stored coefficients, and the k >= (D+1)^2 coefficients sit in memory but must be inert -- never read by a forward, never given a gradient (FusedAdam
would start moving them).  The SH colour and its gradient are evaluated in about a dozen hand-written places, each with its own degree gating:

  rasterizer   project_surfels (raster_project.hip), sh_record_bwd_q16 (glue.hip: fp32, M = 16), the one-lane ladder of project_surfels_bwd
               (raster_project_bwd.hip: fp16 storage or M != 16, its k = nb..M zero fill, its culled-surfel branch)
  tracer       quad_sh_color over the permuted copy (trace_lists.hip), surfel_color / load_sh (trace_common.h: M = 16 fp16, M = 16 fp32, generic),
               the K-buffer kernels (trace_kbuffer.hip: the atomic flush of trace_common.h's sh_lane, bwd_hit), batch_surfel_bwd's staging,
               sparse_hits_bwd, reduce_store (trace_surfel_bwd.hip)
  fused glue   sh_colors_* (glue.hip; tests/test_fused_glue.py)

Inputs: `ladder_shs` gives every inactive coefficient a value of the order of 1e3 (finite, representable in fp16), so that a leak of one of them misses
the 1e-4 contract by orders of magnitude instead of by rounding; higher bands are scaled up so that they contribute visibly, and a sixth of the surfels
sit far below the colour clamp.  An M-coefficient variant is ladder_shs(...)[:, :M].

  CPU leg   the C oracles against float64 autograd of the eager twins at the new (D, M) points, and the two exact properties of the float64 result
            (identical for M = 16 and M = (D+1)^2; zero gradient beyond nb) -- no `gpu` mark
  GPU       tests/test_trace_parity.py:_parity through every form of the tracer, the stage-wise rasterizer comparison forward and backward, and two
            training steps through envgs_step + FusedAdam, each with the exact statements on top: no gradient beyond nb, none on culled surfels."""
import functools

import numpy as np
import pytest
import torch

from tests.test_oracle_trace import trace_scene
from tests.util import small_scene, cam_args, rel_err, check_close, record

DEGREES = (0, 1, 2, 3)
POINTS = [(0, 16), (0, 1), (1, 16), (1, 4), (2, 16), (2, 9), (3, 16)]          # (D, M): M in {16, (D+1)^2}
GENERIC = [(0, 1), (1, 4), (2, 9), (1, 9)]                                     # layouts other than 16 coefficients (the last: M between nb and 16)


def ladder_shs(shs, deg):
    """shs: (P, 16, 3) float32 from the scene builders."""
    s = shs.clone(); P = s.shape[0]; nb = (deg + 1) ** 2
    s[:, 1:] *= 3.0                                   # higher bands contribute visibly
    s[:P // 6, 0] = -3.0                              # a sixth of the surfels sit far below the clamp
    if nb < 16:                                       # inactive coefficients: large, finite, never to be read
        s[:, nb:] = 1.0e3 * torch.randn(P, 16 - nb, 3, generator=torch.Generator().manual_seed(99))
    return s


def _nb(deg):
    return (deg + 1) ** 2


def _tracer_inputs(deg, M=16, half=False):
    g, ro, rd = trace_scene(P=300, R=512, seed=7, camera=False)
    g["shs"] = ladder_shs(g["shs"], deg)[:, :M].contiguous()
    if half:
        g["shs"] = g["shs"].half().float()            # what fp16 storage holds: the comparison is with the oracle on these values
    return g, ro, rd


def _raster_inputs(deg, M=16, half=False):
    g, cam = small_scene(P=600, H=70, W=90, seed=1, C=3, sh=True)             # ragged image, 36 culled surfels
    g["shs"] = ladder_shs(g["shs"], deg)[:, :M].contiguous()
    if half:
        g["shs"] = g["shs"].half().float()
    return g, cam


TRACE_BG = torch.tensor([0.3, 0.1, 0.7])
RASTER_BG = torch.tensor([0.2, 0.5, 0.9])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. CPU leg: the references themselves at the new points
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _trace_upstream(R):
    gen = torch.Generator().manual_seed(9)
    return [torch.randn(R, 3, generator=gen), torch.randn(R, generator=gen), torch.randn(R, generator=gen), torch.randn(R, 3, generator=gen),
            torch.randn(R, 2, generator=gen)]


@functools.lru_cache(maxsize=None)
def _trace_f64(deg, M):
    """float64 autograd of the eager twin on the tracer ladder scene: (outputs, gradients), detached."""
    from oracle import eager_trace
    g, ro, rd = _tracer_inputs(deg, M)
    d = torch.float64
    L = {k: g[k].to(d).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "others", "shs")}
    L["ray_o"] = ro.to(d).requires_grad_(True); L["ray_d"] = rd.to(d).requires_grad_(True)
    outs = eager_trace.trace(L["ray_o"], L["ray_d"], L["means3D"], L["scales"], L["rotations"], L["opacities"], shs=L["shs"], others=L["others"],
                             sh_degree=deg, bg=TRACE_BG, start_from_first=False)
    sum((x * y.to(d)).sum() for x, y in zip(outs[:5], _trace_upstream(ro.shape[0]))).backward()
    return [x.detach() for x in outs], {k: v.grad for k, v in L.items()}


@pytest.mark.parametrize("deg,M", POINTS)
def test_trace_oracle_vs_float64_on_the_ladder(deg, M):
    """The brute-force C tracer against float64 autograd of oracle/eager_trace.py, with the bounds of tests/test_oracle_trace.py (2e-4 values, 2e-3
    gradients); and, exactly: the float64 result does not depend on whether the inactive coefficients are stored, and gives them no gradient."""
    from oracle import trace as otr
    nb = _nb(deg)
    g, ro, rd = _tracer_inputs(deg, M)
    n = lambda k: g[k].numpy()
    fwd = otr.trace_forward(ro.numpy(), rd.numpy(), n("means3D"), n("scales"), n("rotations"), n("opacities"), others=n("others"), bg=TRACE_BG.numpy(),
                            start_from_first=False, shs=n("shs"), sh_degree=deg)
    bwd = otr.trace_backward(fwd, *[x.numpy() for x in _trace_upstream(ro.shape[0])])
    assert fwd["nhits"].mean() > 10
    assert float(np.abs(fwd["rgb"]).max()) < 10.0                          # the 1e3 fill reaches no output
    outs, gr = _trace_f64(deg, M)
    test = "ladder_cpu.trace_D%d_M%d" % (deg, M)
    for nm, b in zip(("rgb", "dpt", "acc", "norm", "aux", "wet"), outs):
        e = rel_err(fwd[nm], b.numpy())
        record(test, nm, e, "(C oracle against float64 eager)")
        assert e < 2e-4, (nm, e)
    record(test, "rgb.abs", float(np.abs(fwd["rgb"] - outs[0].numpy()).max()), "(absolute)")
    q = g["rotations"].double()
    proj = lambda v: v - (v * q).sum(-1, keepdim=True) * q
    tol = 2e-3
    for k_o, k_e in (("dmeans3D", "means3D"), ("dscales", "scales"), ("dopacities", "opacities"), ("dothers", "others"), ("drots", "rotations"), ("dshs", "shs"),
                     ("dray_o", "ray_o"), ("dray_d", "ray_d")):
        a, b = torch.from_numpy(np.asarray(bwd[k_o], np.float64)), gr[k_e]
        a = a.reshape(b.shape)
        if k_o == "drots":
            a, b = proj(a), proj(b)
        e = rel_err(a.numpy(), b.numpy())
        record(test, k_o, e, "(C oracle against float64 autograd)")
        assert e < tol, (k_o, e)
    # exact: nothing beyond nb receives a gradient, in float64 and in the C oracle; the stored-but-inactive block changes no float64 result
    assert float(np.abs(gr["shs"][:, nb:].numpy()).max(initial=0.0)) == 0.0
    assert float(np.abs(bwd["dshs"][:, nb:]).max(initial=0.0)) == 0.0
    assert float(gr["shs"][:, :nb].abs().max()) > 0
    o16, g16 = _trace_f64(deg, 16)
    for a, b in zip(outs, o16):
        assert torch.equal(a, b)
    for k in gr:
        assert torch.equal(gr[k], g16[k][:, :M] if k == "shs" else g16[k]), k


def _raster_upstream(H, W):
    gen = torch.Generator().manual_seed(2)
    return torch.randn(3, H, W, generator=gen) / (H * W), torch.randn(7, H, W, generator=gen) / (H * W)


RASTER_LEAVES = ("means3D", "opacities", "scales", "rotations", "shs")


@functools.lru_cache(maxsize=None)
def _raster_f64(deg, M):
    from oracle import eager
    g, cam = _raster_inputs(deg, M)
    ca = cam_args(cam)
    d = torch.float64
    L = {k: g[k].to(d).requires_grad_(True) for k in RASTER_LEAVES}
    color, radii, allmap, weight = eager.rasterize(L["means3D"], L["opacities"], ca["viewmatrix"].to(d), ca["projmatrix"].to(d), ca["campos"].to(d), ca["W"], ca["H"],
                                                   scales=L["scales"], rotations=L["rotations"], shs=L["shs"], sh_degree=deg, bg=RASTER_BG)
    dcol, dall = _raster_upstream(ca["H"], ca["W"])
    ((color * dcol.to(d)).sum() + (allmap * dall.to(d)).sum()).backward()
    return (color.detach(), radii, allmap.detach(), weight.detach()), {k: v.grad for k, v in L.items()}


@pytest.mark.parametrize("deg,M", POINTS)
def test_raster_oracle_vs_float64_on_the_ladder(deg, M):
    """The C rasterizer oracle against float64 autograd of oracle/eager.py, with the bounds of tests/test_oracle_grad.py; the same two exact properties."""
    from oracle import raster as orc
    nb = _nb(deg)
    g, cam = _raster_inputs(deg, M)
    ca = cam_args(cam)
    W, H = ca["W"], ca["H"]
    fwd = orc.raster_forward(g["means3D"].numpy(), g["opacities"].numpy(), ca["viewmatrix"].numpy(), ca["projmatrix"].numpy(), ca["campos"].numpy(), W, H,
                             bg=RASTER_BG.numpy(), scales=g["scales"].numpy(), rotations=g["rotations"].numpy(), shs=g["shs"].numpy(), sh_degree=deg)
    dcol, dall = _raster_upstream(H, W)
    bwd = orc.raster_backward(fwd, dcol.numpy(), dall.numpy())
    (color, radii, allmap, weight), gr = _raster_f64(deg, M)
    culled = fwd["radii"] == 0
    assert (~culled).sum() > 300 and culled.sum() > 10 and fwd["N"] > 500
    assert float(np.abs(fwd["out_color"]).max()) < 10.0                     # the 1e3 fill reaches no output
    np.testing.assert_array_equal(fwd["radii"], radii.numpy())
    test = "ladder_cpu.raster_D%d_M%d" % (deg, M)
    e = rel_err(fwd["out_color"], color.numpy())
    record(test, "color", e, "(C oracle against float64 eager)")
    assert e < 2e-4, e
    for ch in (0, 1, 2, 3, 4):
        assert rel_err(fwd["allmap"][ch], allmap[ch].numpy()) < 2e-4, ch
    assert rel_err(fwd["allmap"][6], allmap[6].numpy()) < 5e-3              # the distortion map cancels catastrophically in fp32
    assert (np.abs(fwd["allmap"][5] - allmap[5].numpy()) > 1e-3).mean() < 2e-3          # the median depth is a selection
    assert rel_err(fwd["weight"], weight.numpy()) < 2e-4
    q = g["rotations"].double()
    proj = lambda v: v - (v * q).sum(-1, keepdim=True) * q
    tol = 2e-3
    for k_o, k_e in (("dopacities", "opacities"), ("dshs", "shs"), ("dmeans3D", "means3D"), ("dscales", "scales"), ("drots", "rotations")):
        a, b = torch.from_numpy(np.asarray(bwd[k_o], np.float64)), gr[k_e]
        a = a.reshape(b.shape)
        if k_o == "drots":
            a, b = proj(a), proj(b)
        e = rel_err(a.numpy(), b.numpy())
        record(test, k_o, e, "(C oracle against float64 autograd)")
        assert e < tol, (k_o, e)
    assert float(np.abs(gr["shs"][:, nb:].numpy()).max(initial=0.0)) == 0.0
    assert float(np.abs(bwd["dshs"][:, nb:]).max(initial=0.0)) == 0.0 and float(np.abs(bwd["dshs"][culled]).max()) == 0.0
    assert float(gr["shs"][:, :nb].abs().max()) > 0
    (c16, r16, a16, w16), g16 = _raster_f64(deg, 16)
    assert torch.equal(color, c16) and torch.equal(allmap, a16) and torch.equal(weight, w16) and torch.equal(radii, r16)
    for k in gr:
        assert torch.equal(gr[k], g16[k][:, :M] if k == "shs" else g16[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. Tracer ladder
# ---------------------------------------------------------------------------------------------------------------------------------------------
class _PerLaneGathers:
    """The list path's colours by per-lane gathers (load_sh) instead of the cooperative fetch of the permuted copy."""
    def __enter__(self):
        from envgs_amd import tracing
        self.old = tracing.QUAD_SH["on"]
        tracing.QUAD_SH["on"] = False
    def __exit__(self, *a):
        from envgs_amd import tracing
        tracing.QUAD_SH["on"] = self.old


def _check_inactive_gradient(res, deg, M):
    """Exact: no gradient beyond nb; where the oracle has one below nb, so does the kernel (the values themselves: _parity's 1e-4 contract)."""
    nb = _nb(deg)
    got = res["got"]["dcolor"].cpu().numpy()
    want = res["rb"]["dshs"]
    assert got.shape == want.shape == (got.shape[0], M, 3) and got.dtype == np.float32
    assert float(np.abs(got[:, nb:]).max(initial=0.0)) == 0.0, "a gradient was written into an inactive SH coefficient"
    hit = np.abs(want[:, :nb]).reshape(want.shape[0], -1).max(-1) > 0
    assert hit.sum() > got.shape[0] // 2, "the scene is meant to hit most surfels"
    assert (np.abs(got[:, :nb]).reshape(got.shape[0], -1).max(-1) > 0)[hit].all(), "a surfel that was hit has no gradient on its active coefficients"


TRACER_FORMS = ("default", "per_lane", "fp16", "sparse", "kbuffer")


def _tracer_case(test, form, deg, M=16):
    from envgs_amd import tracing
    from tests.test_trace_parity import _parity, _Switch, _check_sparse_list, SPARSE_POISON
    from tests.test_fp16_storage import _F16Storage
    g, ro, rd = _tracer_inputs(deg, M, half=(form == "fp16"))
    kw = {}
    if form == "per_lane":
        kw = dict(hip_ctx=_PerLaneGathers())
    elif form == "fp16":
        kw = dict(hip_ctx=_F16Storage())
    elif form == "sparse":
        kw = dict(hip_ctx=_Switch(sparse="on", sparse_poison=SPARSE_POISON), after_hip=lambda: _check_sparse_list(test))        # (asserts sparse_invalid == 0)
    elif form == "kbuffer":
        kw = dict(hip_ctx=_Switch(force_cap=8), require_lists=False)
    res = _parity(test, g, ro, rd, TRACE_BG, deg, True, False, others=True, **kw)
    assert res["ref"]["nhits"].mean() > 10
    if form == "sparse":
        filed, cap, hits = res["extra"]
        assert filed > 0 and res["cnt"]["sparse_hits"] == filed, "no hit took the sparse path"
    if form == "kbuffer":
        assert res["cnt"]["max_list"] > 8 and (res["ref"]["nhits"] > 8).any() and res["n_listed"] < res["R"], "no ray overflowed its list"
    _check_inactive_gradient(res, deg, M)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("deg", DEGREES)
@pytest.mark.parametrize("form", TRACER_FORMS)
def test_tracer_ladder(form, deg, request):
    """_parity (index parity, the 1e-4 contract on every output and all nine gradients) at every degree with 16 stored coefficients, through:
    default   quad_sh_color fp32, batch_surfel_bwd's M = 16 fp32 staging, reduce_store
    per_lane  load_sh M = 16 fp32 (its nq rounding at nb = 1 and 9)
    fp16      both fp16 loaders and the fp16 staging, against the oracle on the rounded values
    sparse    sparse_hits_bwd (sparse_invalid == 0, entries filed)
    kbuffer   trace_kbuffer.hip forward, bwd_hit and the atomic flush (trace_common.h: sh_lane) for the rays over an 8-entry list capacity"""
    _tracer_case(request.node.name, form, deg)


@pytest.mark.gpu
@pytest.mark.parametrize("deg,M", GENERIC)
def test_tracer_ladder_generic_layout(deg, M, request):
    """M != 16: the generic branches of load_sh and of the staging, the stride M * 3 of reduce_store."""
    _tracer_case(request.node.name, "default", deg, M)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. Rasterizer ladder
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _raster_module_run(mod, g, cam, deg, dcol, dall, dev):
    from tests.test_raster_parity import _settings
    st = _settings(mod, cam, RASTER_BG, deg, dev)
    leaves = {k: g[k].to(dev).requires_grad_(True) for k in RASTER_LEAVES}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True) + 0
    means2D.retain_grad()
    color, radii, allmap, weight = mod.GaussianRasterizer(raster_settings=st)(
        means3D=leaves["means3D"], means2D=means2D, shs=leaves["shs"], colors_precomp=None, opacities=leaves["opacities"], scales=leaves["scales"],
        rotations=leaves["rotations"], cov3D_precomp=None)
    ((color * dcol.to(dev)).sum() + (allmap * dall.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return color.detach(), allmap.detach(), radii, dict({k: v.grad for k, v in leaves.items()}, means2D=means2D.grad)


def _raster_case(test, deg, M, half):
    import diff_surfel_rasterization_wet as mod
    from envgs_amd import raster
    from oracle import raster as orc
    from tests.test_raster_parity import _settings, _oracle, _compare_forward, _masked_upstream, _sh_clamp_fragile, GRAD_NAMES
    from tests.test_fp16_storage import _F16Storage
    dev = torch.device("cuda:0")
    nb = _nb(deg)
    g, cam = _raster_inputs(deg, M, half)
    H, W = cam.image_height, cam.image_width
    ref = _oracle(g, cam, RASTER_BG, deg, 3, True)
    aud = orc.raster_audit(ref, want_contrib=True)
    culled = ref["radii"] == 0
    assert culled.sum() > 10 and (ref["clamped"][~culled] != 0).sum() > 100
    # forward, stage by stage (sh_rgb at 1e-5, bit-exact clamp flags on the visible surfels, the index work, the images)
    st = _settings(mod, cam, RASTER_BG, deg, dev)
    gd = {k: v.to(dev) for k, v in g.items()}
    outs, saved = raster.rasterize_forward(3, gd["means3D"], gd["shs"].half() if half else gd["shs"], None, gd["opacities"], gd["scales"], gd["rotations"], None, st,
                                           keep_binning=True)
    torch.cuda.synchronize()
    _compare_forward(test, outs, saved, ref, aud, True, check_sets=True)
    # backward, as tests/test_raster_parity.py:test_backward_vs_oracle
    dcol, dall = _masked_upstream(3, H, W, 101, aud["fragile"])
    if half:
        with _F16Storage():                                                 # half copies inside the node, fp32 gradients out
            color, allmap, radii, grads = _raster_module_run(mod, g, cam, deg, dcol, dall, dev)
    else:
        color, allmap, radii, grads = _raster_module_run(mod, g, cam, deg, dcol, dall, dev)
    assert torch.equal(color, outs[0]) and torch.equal(allmap, outs[2])
    rb = orc.raster_backward(ref, dcol.numpy(), dall.numpy(), want_cond=True)
    nfr = int(aud["fragile"].sum())
    clampfrag = _sh_clamp_fragile(ref)
    record(test, "sh_clamp_fragile_surfels", float(clampfrag.sum()))
    for k_hip, k_ref in GRAD_NAMES + (("shs", "dshs"),):
        check_close(test, k_ref, grads[k_hip].cpu().numpy().reshape(rb[k_ref].shape), rb[k_ref], excluded=nfr, cond=rb["cond"][k_ref], unc=rb["unc"][k_ref],
                    keep=(~clampfrag if k_ref == "dshs" else None))
    dshs = grads["shs"].cpu().numpy()
    assert dshs.shape == (g["shs"].shape[0], M, 3) and dshs.dtype == np.float32
    np.testing.assert_array_equal(radii.cpu().numpy(), ref["radii"])
    assert float(np.abs(dshs[culled]).max()) == 0.0, "a culled surfel received an SH gradient"
    assert float(np.abs(dshs[:, nb:]).max(initial=0.0)) == 0.0, "a gradient was written into an inactive SH coefficient"
    assert float(np.abs(dshs[~culled][:, :nb]).max()) > 0
    if half:
        # against the fp32 path on the same (rounded) values: the conversion is exact, so the forward is identical and the gradients agree to fp32
        # rounding (the bounds of tests/test_fp16_storage.py:test_raster_fp16_storage_keeps_fp32_gradients)
        c32, a32, _, g32 = _raster_module_run(mod, g, cam, deg, dcol, dall, dev)
        assert torch.equal(color, c32) and torch.equal(allmap, a32)
        for k in g32:
            check_close(test, "fp16_vs_fp32.d" + k, grads[k].cpu().numpy(), g32[k].cpu().numpy(), tol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("deg", DEGREES)
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_raster_ladder(storage, deg, request):
    """16 stored coefficients at every degree.  f32: project_surfels and sh_record_bwd_q16; f16 storage: the one-lane ladder of project_surfels_bwd,
    against the oracle on the rounded values and against the fp32 run on the rounded values."""
    _raster_case(request.node.name, deg, 16, storage == "f16")


@pytest.mark.gpu
@pytest.mark.parametrize("deg,M", GENERIC)
def test_raster_ladder_generic_layout(deg, M, request):
    """M != 16 in fp32: the one-lane ladder again, plus its k = nb..M zero fill and the stride M * 3."""
    _raster_case(request.node.name, deg, M, False)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. What training relies on: an inactive coefficient never moves
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("deg", [0, 1])
@pytest.mark.parametrize("fused_glue", [True, False])
def test_inactive_coefficients_do_not_train(fused_glue, deg):
    """Two steps of envgs_step.envgs_forward + backward + FusedAdam.step() below degree 3, both sets with 16 stored coefficients and non-zero inactive
    ones.  FusedAdam skips elements whose gradient is exactly zero, so after the steps shs[:, nb:] of both sets is bit-identical to its initial value and
    its moments are exactly zero -- no tolerance -- while shs[:, :nb] has moved."""
    import diff_surfel_rasterization_wet_ch05 as pkg
    import diff_surfel_tracing as tpkg
    from envgs_amd import envgs_step, synth
    from envgs_amd.loss import l1_ssim_loss
    from envgs_amd.optim import FusedAdam
    from tests.test_train_convergence import _raw, _act
    dev = torch.device("cuda:0")
    nb = _nb(deg)
    Hh = Ww = 64
    b = synth.base_gaussians(1500, seed=3)
    b["scales"] = b["scales"] * 5.0
    b["opacities"] = torch.sigmoid(torch.randn(1500, 1, generator=torch.Generator().manual_seed(1)) + 1.5)
    b["specular"] = torch.sigmoid(torch.randn(1500, 1, generator=torch.Generator().manual_seed(2)))
    e = synth.env_gaussians(800, seed=4, bound=12.0)
    b["shs"] = ladder_shs(b["shs"], deg); e["shs"] = ladder_shs(e["shs"], deg)
    base, env = _raw(b, dev), _raw(e, dev)
    first = {"base": base["shs"].clone(), "env": env["shs"].clone()}
    assert float(first["base"][:, nb:].abs().min()) > 0 and float(first["env"][:, nb:].abs().min()) > 0
    for d in (base, env):
        for t in d.values():
            t.requires_grad_(True)
    cam = synth.orbit_camera(1, n_views=4, H=Hh, W=Ww, fx=1111.1 * Ww / 800.0, device=dev)
    rays = synth.get_rays(cam)
    bg = torch.zeros(3, device=dev); env_bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    target = torch.rand(3, Hh, Ww, generator=torch.Generator().manual_seed(5)).to(dev)
    lr = dict(means3D=2e-4, shs=2e-2, opacities=3e-2, scales=5e-3, rotations=1e-3, specular=3e-2, roughness=1e-2)
    opt = FusedAdam([{"params": [t], "lr": lr[k], "name": k} for k, t in base.items()] + [{"params": [t], "lr": lr[k], "name": "env_" + k} for k, t in env.items()],
                    lr=0.0, eps=1e-15)
    tracer = tpkg.SurfelTracer()
    old = envgs_step.FUSED["on"]
    envgs_step.FUSED["on"] = fused_glue
    try:
        for it in range(2):
            out = envgs_step.envgs_forward(pkg, tpkg, tracer, cam, rays, _act(base), _act(env), bg, env_bg, torch.tensor([deg], device=dev))
            l1_ssim_loss(out["rgb"].permute(2, 0, 1), target).backward()
            for name, d in (("base", base), ("env", env)):
                gsh = d["shs"].grad
                assert float(gsh[:, nb:].abs().max()) == 0.0, "%s set: a gradient reached an inactive SH coefficient" % name
                assert float(gsh[:, :nb].abs().max()) > 0.0
            opt.step()
            opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
    finally:
        envgs_step.FUSED["on"] = old
    for name, d in (("base", base), ("env", env)):
        p = d["shs"].detach()
        st = opt.state[d["shs"]]
        assert torch.equal(p[:, nb:], first[name][:, nb:]), "%s set: an inactive SH coefficient moved" % name
        assert float(st["exp_avg"][:, nb:].abs().max()) == 0.0 and float(st["exp_avg_sq"][:, nb:].abs().max()) == 0.0
        assert float(st["exp_avg"][:, :nb].abs().max()) > 0.0
        assert not torch.equal(p[:, :nb], first[name][:, :nb]), "%s set: the active SH coefficients did not move" % name
