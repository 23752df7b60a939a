"""CPU: the brute-force C tracer oracle (forward + analytic backward) against float64 autograd of the dense
torch-eager restatement (oracle/eager_trace.py)."""
import numpy as np
import pytest
import torch

from envgs_amd import synth
from oracle import eager_trace, trace as otr
from tests.util import rel_err, record


def trace_scene(P=150, R=400, seed=0, camera=True):
    """Surfels scattered in a shell around the origin, rays from inside (reflection-like) or from a camera."""
    g = torch.Generator().manual_seed(seed)
    dirs = torch.randn(P, 3, generator=g); dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    means = dirs * (3.0 + 4.0 * torch.rand(P, 1, generator=g))
    scales = 0.5 + 1.2 * torch.rand(P, 2, generator=g)
    q = torch.randn(P, 4, generator=g); rots = q / q.norm(dim=-1, keepdim=True)
    opac = torch.sigmoid(torch.randn(P, 1, generator=g))
    shs = torch.cat([torch.rand(P, 1, 3, generator=g) * 3 - 1.5, torch.randn(P, 15, 3, generator=g) * 0.2], dim=1)
    others = torch.rand(P, 2, generator=g)
    if camera:
        cam = synth.orbit_camera(2, H=20, W=20, fx=25.0, radius=1.0)
        ro, rd = synth.get_rays(cam)
        ro, rd = ro.reshape(-1, 3)[:R], rd.reshape(-1, 3)[:R]
    else:
        ro = torch.randn(R, 3, generator=g) * 0.3
        rd = torch.randn(R, 3, generator=g); rd = rd / rd.norm(dim=-1, keepdim=True) * (0.5 + torch.rand(R, 1, generator=g))
    return dict(means3D=means, scales=scales, rotations=rots, opacities=opac, shs=shs, others=others,
                colors_precomp=torch.rand(P, 3, generator=g)), ro.contiguous(), rd.contiguous()


_ORACLE_CASES = [(True, True, 3), (False, False, 0), (True, False, 2)]


@pytest.mark.parametrize("use_sh,camera,deg,scale_modifier",
                         [pytest.param(*c, 1.0, id="-".join(str(x) for x in c)) for c in _ORACLE_CASES] +          # (the ids from before the modifier)
                         [pytest.param(*c, m, id="-".join(str(x) for x in c) + "-mod%g" % m) for m in (0.5, 1.7) for c in _ORACLE_CASES])
def test_trace_oracle_vs_autograd(use_sh, camera, deg, scale_modifier, request):
    """scale_modifier != 1 (the reference's viewer and test loops pass it through, optix_utils.py:110): measured at 0.5 / 1.7: values <= 2.8e-6, gradients <= 1.0e-5."""
    _oracle_vs_autograd(*trace_scene(seed=3, camera=camera), use_sh, camera, deg, scale_modifier, "oracle_cpu.trace." + request.node.callspec.id)


def test_trace_oracle_vs_autograd_on_a_saturated_room():
    """tests/saturated_scenes.py:room (surfels on a wall, 40 % at opacity 1.0f, a third of the rays aimed into a cap zone): the alpha cap's straight-through
    gradient and rays that end after a few hits, which trace_scene never reaches.  At the committed seed the audit marks no ray, so nothing is left out.
    Measured: values 6.0e-7, gradients 3.5e-6 (asserted at the file's 2e-4 / 2e-3)."""
    from tests.saturated_scenes import trace_scene_of, census_trace
    g, ro, rd, c = trace_scene_of("room200")
    assert census_trace(g, ro, rd, c["camera"])["capped_rays"] >= 50
    _oracle_vs_autograd(g, ro, rd, True, c["camera"], 3, 1.0, "oracle_cpu.trace.saturated_room200")


def _oracle_vs_autograd(g, ro, rd, use_sh, camera, deg, scale_modifier, test):
    R = ro.shape[0]
    bg = torch.tensor([0.3, 0.1, 0.7])
    gen = torch.Generator().manual_seed(9)
    gr = [torch.randn(R, 3, generator=gen), torch.randn(R, generator=gen), torch.randn(R, generator=gen),
          torch.randn(R, 3, generator=gen), torch.randn(R, 2, generator=gen)]
    ckw = dict(shs=g["shs"].numpy(), sh_degree=deg) if use_sh else dict(colors_precomp=g["colors_precomp"].numpy())
    fwd = otr.trace_forward(ro.numpy(), rd.numpy(), g["means3D"].numpy(), g["scales"].numpy(), g["rotations"].numpy(),
                            g["opacities"].numpy(), others=g["others"].numpy(), bg=bg.numpy(), start_from_first=camera, scale_modifier=scale_modifier, **ckw)
    bwd = otr.trace_backward(fwd, *[x.numpy() for x in gr])
    assert fwd["nhits"].mean() > (2 if scale_modifier >= 1 else 1)

    d = torch.float64
    L = {k: g[k].to(d).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "others")}
    if use_sh: L["shs"] = g["shs"].to(d).requires_grad_(True)
    else: L["colors_precomp"] = g["colors_precomp"].to(d).requires_grad_(True)
    o64 = ro.to(d).requires_grad_(True); d64 = rd.to(d).requires_grad_(True)
    rgb, dpt, acc, norm, aux, wet = eager_trace.trace(o64, d64, L["means3D"], L["scales"], L["rotations"], L["opacities"],
                                                      shs=L.get("shs"), colors_precomp=L.get("colors_precomp"), others=L["others"],
                                                      sh_degree=deg, bg=bg, start_from_first=camera, scale_modifier=scale_modifier)
    ev = [rel_err(a, b.detach().numpy()) for a, b in ((fwd["rgb"], rgb), (fwd["dpt"], dpt), (fwd["acc"], acc), (fwd["norm"], norm), (fwd["aux"], aux), (fwd["wet"], wet))]
    record(test, "values", max(ev), "(C oracle against float64 eager, max over the outputs; %.2f hits per ray)" % fwd["nhits"].mean())
    assert max(ev) < 2e-4, ev
    loss = sum((x * y.to(d)).sum() for x, y in zip((rgb, dpt, acc, norm, aux), gr))
    loss.backward()
    tol = 2e-3
    q = g["rotations"].double()
    proj = lambda v: v - (v * q).sum(-1, keepdim=True) * q
    eg = dict(dmeans3D=rel_err(bwd["dmeans3D"], L["means3D"].grad.numpy()), dscales=rel_err(bwd["dscales"], L["scales"].grad.numpy()),
              dopacities=rel_err(bwd["dopacities"], L["opacities"].grad.reshape(-1).numpy()), dothers=rel_err(bwd["dothers"], L["others"].grad.numpy()),
              drots=rel_err(proj(torch.from_numpy(bwd["drots"])).numpy(), proj(L["rotations"].grad).numpy()),
              dcolor=(rel_err(bwd["dshs"], L["shs"].grad.numpy()) if use_sh else rel_err(bwd["dcolors"], L["colors_precomp"].grad.numpy())),
              dray_o=rel_err(bwd["dray_o"], o64.grad.numpy()), dray_d=rel_err(bwd["dray_d"], d64.grad.numpy()))
    record(test, "gradients", max(eg.values()), "(C oracle against float64 autograd, max over the leaves and the rays)")
    for k, e in eg.items():
        assert e < tol, (k, e)


def test_trace_oracle_bounces_fill_mid():
    g, ro, rd = trace_scene(seed=4, camera=True)
    fwd = otr.trace_forward(ro.numpy(), rd.numpy(), g["means3D"].numpy(), g["scales"].numpy(), g["rotations"].numpy(),
                            g["opacities"].numpy(), shs=g["shs"].numpy(), sh_degree=1, others=g["others"].numpy(),
                            max_trace_depth=2, specular_threshold=0.1, start_from_first=True)
    mid = fwd["mid"].reshape(-1, 3, 16)
    np.testing.assert_allclose(mid[:, 0, 0:3], ro.numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(mid[:, 0, 6], fwd["dpt"], rtol=1e-6)
    np.testing.assert_allclose(mid[:, 0, 11:13], fwd["aux"], rtol=1e-6)
    bounced = np.abs(mid[:, 1, 3:6]).sum(-1) > 0
    assert bounced.any() and (~bounced).any()
    # a bounced ray starts on the stage-0 surface point
    o1 = ro.numpy() + rd.numpy() * (fwd["dpt"] / np.maximum(fwd["acc"], 1e-9))[:, None]
    np.testing.assert_allclose(mid[bounced, 1, 0:3], o1[bounced], rtol=1e-4, atol=1e-5)


# fp32 round trip frame -> transMat -> frame: a 4x4 product, a 3x3 inverse, two norms and a quaternion extraction, about 16 roundings of 6e-8
# (measured over three seeds, two cameras and the modifiers 0.5 / 1 / 1.7: scales <= 4.4e-7 relative, quaternion <= 1.8e-7)
FRAME_ROUND_TRIP = 1e-6


@pytest.mark.parametrize("scale_modifier", [1.0, 1.7])
def test_frame_from_transmat_round_trip(scale_modifier, request):
    """cov3D_precomp in the tracer: frame_from_transmat divides the modifier out of the scales it recovers, because the kernel multiplies it in again.
    With the caller's pair (transmat_python(..., scale_modifier=m), settings.scale_modifier = m) it must return the given scales and rotation -- no
    threshold is involved, so this is where a modifier applied twice, or not at all, shows as a factor m."""
    from envgs_amd import tracing
    from tests.util import CAMERAS
    m = scale_modifier
    g, _, _ = trace_scene(P=200, R=8, seed=5, camera=False)
    rn = g["rotations"] / g["rotations"].norm(dim=-1, keepdim=True)
    for name, cam in (("orbit", synth.orbit_camera(1, H=64, W=80, fx=100.0)), ("aniso", CAMERAS["aniso"](64, 80))):
        st = tracing.SurfelTracingSettings(image_height=64, image_width=80, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3), scale_modifier=m,
                                           viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=torch.tensor([2]),
                                           campos=cam.camera_center, prefiltered=False, debug=False, max_trace_depth=0, specular_threshold=0.0)
        s_rec, q_rec = tracing.frame_from_transmat(synth.transmat_python(cam, g["means3D"], g["scales"], rn, scale_modifier=m), st)
        e_s = float(((s_rec - g["scales"]).abs() / g["scales"]).max())
        e_q = float((q_rec * torch.sign((q_rec * rn).sum(-1, keepdim=True)) - rn).abs().max())
        record("frame_round_trip_cpu.%s.mod%g" % (name, m), "scales", e_s, "(relative; bound %.0e)" % FRAME_ROUND_TRIP)
        record("frame_round_trip_cpu.%s.mod%g" % (name, m), "quaternion", e_q, "(absolute, up to sign; bound %.0e)" % FRAME_ROUND_TRIP)
        assert e_s <= FRAME_ROUND_TRIP and e_q <= FRAME_ROUND_TRIP, (name, e_s, e_q)
