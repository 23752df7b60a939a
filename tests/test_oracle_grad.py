"""CPU: the C oracle's forward and hand-written backward (R6-R8) against float64 autograd of the
torch-eager restatement (oracle/eager.py).  This is what makes the C oracle trustworthy as the
parity target for the HIP kernels: every gradient is checked against a true derivative."""
import numpy as np
import pytest
import torch

from oracle import eager, raster as orc
from tests.util import scene_for, cam_args, rel_err, record, record_fragile, small_fx, SMALL_IMAGES, FRAGILE_PX_MAX


def _run(sh, C, precomp_T, seed, camera="orbit", scale_modifier=1.0, HW=(48, 64), P=300, fx=None, mask_fragile=False, saturated=False):
    """saturated: tests/saturated_scenes.py:surface_object instead of the random cloud (surfels on a sphere, 40 % of them at opacity 1.0f).  mask_fragile: zero the upstream gradient at the pixels the oracle's audit marks (a threshold inside fp32 noise flips a contributor between the
    fp32 oracle and float64), as the GPU parity tests do; the mask is returned so that the values are compared on the other pixels."""
    if saturated:
        from tests.saturated_scenes import raster_case
        g, cam = raster_case(P, HW[0], HW[1], seed, C=C, fx=fx)
    else:
        g, cam = scene_for(camera, P=P, H=HW[0], W=HW[1], seed=seed, C=C, sh=sh, fx=fx)
    ca = cam_args(cam)
    W, H = ca["W"], ca["H"]
    bg = torch.tensor([0.3, 0.6, 0.1])
    gen = torch.Generator().manual_seed(seed + 1)
    dcol = torch.randn(C, H, W, generator=gen) / (H * W)
    dall = torch.randn(7, H, W, generator=gen) / (H * W)

    kw_np = dict(scales=g["scales"].numpy(), rotations=g["rotations"].numpy())
    tm = None
    if precomp_T:
        from envgs_amd import synth
        tm = synth.transmat_python(cam, g["means3D"], g["scales"], g["rotations"], scale_modifier=scale_modifier)
        kw_np = dict(transmat_precomp=tm.numpy())
    col_kw = dict(shs=g["shs"].numpy(), sh_degree=3) if sh else dict(colors_precomp=g["colors_precomp"].numpy())
    fwd = orc.raster_forward(g["means3D"].numpy(), g["opacities"].numpy(), ca["viewmatrix"].numpy(), ca["projmatrix"].numpy(),
                             ca["campos"].numpy(), W, H, bg=bg.numpy(), scale_modifier=scale_modifier, **kw_np, **col_kw)
    frag, tainted = np.zeros((H, W), bool), np.zeros(P, bool)
    if mask_fragile:
        aud = orc.raster_audit(fwd)
        frag, tainted = aud["fragile"], aud["tainted"]              # tainted: the surfels that touch a fragile pixel
        m = torch.from_numpy(~frag)
        dcol, dall = dcol * m, dall * m
    bwd = orc.raster_backward(fwd, dcol.numpy(), dall.numpy())

    d = torch.float64
    leaves = {k: g[k].to(d).requires_grad_(True) for k in ("means3D", "opacities")}
    if precomp_T: leaves["transmat_precomp"] = tm.to(d).requires_grad_(True)
    else: leaves.update({k: g[k].to(d).requires_grad_(True) for k in ("scales", "rotations")})
    if sh: leaves["shs"] = g["shs"].to(d).requires_grad_(True)
    else: leaves["colors_precomp"] = g["colors_precomp"].to(d).requires_grad_(True)
    out_color, radii, allmap, weight = eager.rasterize(
        leaves["means3D"], leaves["opacities"], ca["viewmatrix"].to(d), ca["projmatrix"].to(d), ca["campos"].to(d), W, H,
        scales=leaves.get("scales"), rotations=leaves.get("rotations"), transmat_precomp=leaves.get("transmat_precomp"),
        shs=leaves.get("shs"), colors_precomp=leaves.get("colors_precomp"), sh_degree=3, bg=bg, scale_modifier=scale_modifier)
    loss = (out_color * dcol.to(d)).sum() + (allmap * dall.to(d)).sum()
    loss.backward()
    return g, fwd, bwd, (out_color, radii, allmap, weight), leaves, (frag, tainted)


def _compare(g, fwd, bwd, outs, leaves, sh, precomp_T, ok=None, clean=None):
    """The file's tolerances: radii equal, values 2e-4, gradients 2e-3 (of the tensor's scale).  Returns the measured (values, gradients) maxima."""
    out_color, radii, allmap, weight = outs
    if ok is None:
        ok = np.ones(fwd["allmap"][0].shape, bool)
    np.testing.assert_array_equal(fwd["radii"], radii.numpy())
    ev = [rel_err(fwd["out_color"][:, ok], out_color.detach().numpy()[:, ok])]
    assert ev[-1] < 2e-4
    for ch in (0, 1, 2, 3, 4):
        ev.append(rel_err(fwd["allmap"][ch][ok], allmap[ch].detach().numpy()[ok]))
        assert ev[-1] < 2e-4, ch
    # distortion = sum w (m^2 A + M2 - 2 m M1) cancels catastrophically in fp32 (the reference computes it in fp32 too)
    assert rel_err(fwd["allmap"][6][ok], allmap[6].detach().numpy()[ok]) < 5e-3
    # median depth is a selection: allow a handful of pixels to pick a neighbouring splat
    med_bad = np.abs(fwd["allmap"][5] - allmap[5].detach().numpy())[ok] > 1e-3
    assert med_bad.mean() < 2e-3
    # the per-surfel weight sums over every pixel, so it is compared on the surfels that touch no audited pixel (all of them when there is none)
    clean = np.ones(fwd["weight"].shape[0], bool) if clean is None else clean
    ev.append(rel_err(fwd["weight"][clean], weight.detach().numpy().reshape(-1)[clean]))
    assert ev[-1] < 2e-4

    tol = 2e-3
    eg = [rel_err(bwd["dopacities"], leaves["opacities"].grad.reshape(-1).numpy())]
    if sh:
        eg.append(rel_err(bwd["dshs"], leaves["shs"].grad.numpy()))
    else:
        eg.append(rel_err(bwd["dcolors"], leaves["colors_precomp"].grad.numpy()))
    if precomp_T:
        eg.append(rel_err(bwd["dtransmat_precomp"], leaves["transmat_precomp"].grad.numpy()))
        assert leaves["means3D"].grad is None or float(leaves["means3D"].grad.abs().max()) == 0.0
    else:
        eg.append(rel_err(bwd["dmeans3D"], leaves["means3D"].grad.numpy()))
        eg.append(rel_err(bwd["dscales"], leaves["scales"].grad.numpy()))
        # the kernel returns dL/d(q/|q|); torch's own normalize backward projects it -- compare projected
        q = g["rotations"].double()
        proj = lambda v: v - (v * q).sum(-1, keepdim=True) * q
        eg.append(rel_err(proj(torch.from_numpy(bwd["drots"]).double()).numpy(), proj(leaves["rotations"].grad).numpy()))
    assert max(eg) < tol, eg
    return max(ev), max(eg)


@pytest.mark.parametrize("sh,C,precomp_T", [(True, 3, False), (False, 5, False), (False, 7, True)])
def test_oracle_forward_and_backward_vs_autograd(sh, C, precomp_T):
    g, fwd, bwd, outs, leaves, _ = _run(sh, C, precomp_T, seed=3)
    assert (fwd["radii"] > 0).sum() > 100 and fwd["N"] > 500
    _compare(g, fwd, bwd, outs, leaves, sh, precomp_T)


# The axes the orbit camera at scale_modifier 1 never reaches (tests/util.py: CAMERAS, SMALL_IMAGES), on the CPU first: what the GPU parity tests
# compare the kernels with must itself be right there.  kw of _run; seeds chosen so that the float64 twin's radii equal the fp32 oracle's (a radius
# is a ceil(): one surfel of at_origin at P=1000, seed 3 sits on an fp32 / fp64 boundary) -- every camera here IS compared with float64.
NEW_AXES = [pytest.param(dict(sh=True, C=3, precomp_T=False, camera="in_cloud", P=600, seed=3), 100, id="in_cloud"),
            pytest.param(dict(sh=False, C=5, precomp_T=False, camera="at_origin", P=600, seed=3), 100, id="at_origin"),
            pytest.param(dict(sh=True, C=3, precomp_T=False, camera="aniso", P=300, seed=3), 100, id="aniso"),
            pytest.param(dict(sh=False, C=5, precomp_T=False, scale_modifier=0.5, seed=3), 100, id="mod0.5"),
            pytest.param(dict(sh=True, C=3, precomp_T=False, scale_modifier=1.7, seed=3), 100, id="mod1.7"),
            pytest.param(dict(sh=False, C=7, precomp_T=True, scale_modifier=1.7, seed=3), 100, id="mod1.7-precomp_T")] + \
           [pytest.param(dict(sh=True, C=3, precomp_T=False, HW=hw, fx=small_fx(hw[1]), seed=3), 1, id="%dx%d" % hw) for hw in SMALL_IMAGES]


@pytest.mark.parametrize("kw,min_visible", NEW_AXES)
def test_oracle_vs_autograd_on_other_cameras_modifiers_and_small_images(kw, min_visible, request):
    """Measured: values <= 3.8e-5 (at_origin; <= 1.5e-5 elsewhere), gradients <= 6.2e-5 (asserted at the file's 2e-4 / 2e-3).  The upstream gradient is zeroed at the audited pixels;
    the images smaller than 500 pixels must have none, so nothing at all is left out there."""
    g, fwd, bwd, outs, leaves, (frag, tainted) = _run(mask_fragile=True, **kw)
    H, W = frag.shape
    assert (fwd["radii"] > 0).sum() >= min_visible
    if kw.get("camera") in ("in_cloud", "at_origin"):
        assert (fwd["radii"] == 0).sum() > 50 and fwd["radii"].max() > 1000            # culled at the near plane; tile rectangles clamped on all sides
    assert frag.mean() <= FRAGILE_PX_MAX and (H * W >= 500 or not frag.any())
    ev, eg = _compare(g, fwd, bwd, outs, leaves, kw["sh"], kw["precomp_T"], ok=~frag, clean=~tainted)
    test = "oracle_cpu.raster." + request.node.callspec.id
    record_fragile(test, "fragile_px", frag, FRAGILE_PX_MAX)
    record(test, "values", ev, "(C oracle against float64 eager, max over the outputs)")
    record(test, "gradients", eg, "(C oracle against float64 autograd, max over the leaves)")


@pytest.mark.parametrize("kw", [pytest.param(dict(sh=True, C=3, precomp_T=False, P=300, seed=3), id="sphere300"),
                                pytest.param(dict(sh=False, C=5, precomp_T=False, P=600, seed=2), id="sphere600")])
def test_oracle_vs_autograd_on_a_saturated_surface(kw, request):
    """tests/saturated_scenes.py:surface_object (surfels on a sphere, 40 % at opacity 1.0f): blends that take the alpha cap, whose backward is the straight-through
    one, and pixels that end after two or three hits -- the random clouds above reach neither.  Measured: values <= 1.3e-5, gradients <= 8.4e-5 (asserted at the
    file's 2e-4 / 2e-3); no audited pixel at these seeds."""
    from tests.saturated_scenes import census_raster, raster_case
    g, fwd, bwd, outs, leaves, (frag, tainted) = _run(mask_fragile=True, saturated=True, **kw)
    c = census_raster(*raster_case(kw["P"], 48, 64, kw["seed"], C=kw["C"]), sh=kw["sh"], exclude=frag)
    assert c["capped"] >= 20 and c["stopped_px"] >= 20, c
    assert frag.mean() <= FRAGILE_PX_MAX
    ev, eg = _compare(g, fwd, bwd, outs, leaves, kw["sh"], kw["precomp_T"], ok=~frag, clean=~tainted)
    test = "oracle_cpu.raster.saturated_" + request.node.callspec.id
    record_fragile(test, "fragile_px", frag, FRAGILE_PX_MAX)
    record(test, "capped_blends", c["capped"], "(float64 twin; %d of %d pixels end early)" % (c["stopped_px"], c["pixels"]))
    record(test, "values", ev, "(C oracle against float64 eager, max over the outputs)")
    record(test, "gradients", eg, "(C oracle against float64 autograd, max over the leaves)")


def test_means2d_grad_is_the_densification_proxy():
    g, fwd, bwd, _, _, _ = _run(True, 3, False, seed=5)
    W, H = fwd["W"], fwd["H"]
    vis = fwd["radii"] > 0
    exp_x = (bwd["rec_dT"][:, 2] * fwd["transmat"][:, 8] * 0.5 * W)[vis]
    exp_y = (bwd["rec_dT"][:, 5] * fwd["transmat"][:, 8] * 0.5 * H)[vis]
    np.testing.assert_allclose(bwd["dmeans2D"][vis, 0], exp_x, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(bwd["dmeans2D"][vis, 1], exp_y, rtol=1e-5, atol=1e-12)
    assert np.all(bwd["dmeans2D"][:, 2] == 0) and np.all(bwd["dmeans2D"][~vis] == 0)
    assert np.abs(bwd["dmeans2D"][vis]).max() > 0
