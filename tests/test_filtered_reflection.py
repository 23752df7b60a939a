"""Filtered reflection rays (easyvolcap/models/samplers/envgs_sampler.py:433-455, :461-476): late in training the reference traces only the
pixels of a mask -- (1,S,3) rays -- and scatters the traced colour back.  envgs_step.FILTER switches the step caller to that form; its torch
twins (reflection_mask / filtered_rays / filtered_blend) restate the reference's expressions, the fused form runs them as HIP kernels
(fused.select_pixels / reflect_filtered / blend_filtered).

CPU: the twins against the reference's own recorded filtered step (tests/golden/sampler_golden.pt, tag specular_filtered_rays), bit for bit.
GPU: the selection against cumsum, the two kernels against the torch expressions of tests/test_fused_glue.py followed by [mask], the step link
     by link (tests/stagewise.py) in both caller forms, and the deferred / colour-only tracer options with the filter on."""
import os

import numpy as np
import pytest
import torch

from envgs_amd import envgs_step, synth
from tests import stagewise
from tests.util import record, record_fragile, FRAGILE_RAYS_MAX

HERE = os.path.dirname(os.path.abspath(__file__))
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    """The reference's recorded filtered step: raster output img (5,24,32), traced colour (1,192,3), and what its sampler made of them."""
    fx = torch.load(os.path.join(HERE, "golden", "sampler_golden.pt"), weights_only=False)
    step = {s["tag"]: s for s in fx["steps"]}["specular_filtered_rays"]
    a, b = step["call_range"]
    calls = [(fx["contract"][i], fx["call_tensors"][i]) for i in range(a, b)]
    (img,) = [t["outputs"][0] for c, t in calls if c["what"] == "call" and c["package"].startswith("diff_surfel_rasterization")]
    (allmap,) = [t["outputs"][2] for c, t in calls if c["what"] == "call" and c["package"].startswith("diff_surfel_rasterization")]
    (env,) = [t["outputs"][0] for c, t in calls if c["what"] == "call" and c["package"] == "diff_surfel_tracing"]
    return dict(H=fx["H"], W=fx["W"], img=img, allmap=allmap, rgb_env=env, out=step["outputs"])


# ---------------------------------------------------------------------------------------------------------------- 1. CPU: the twins
def test_twins_reproduce_the_recorded_filtered_step(recorded):
    r, out = recorded, recorded["out"]
    H, W = r["H"], r["W"]
    assert r["rgb_env"].shape == (1, 192, 3) and H * W == 768
    spec = r["img"][3:4].permute(1, 2, 0).reshape(1, H * W, 1)
    assert torch.equal(spec, out["spec_map"]) and torch.equal(r["allmap"][1].reshape(1, H * W, 1), out["acc_map"])
    mask = envgs_step.reflection_mask("specular", spec=out["spec_map"], specular_percent=envgs_step.FILTER["specular_percent"])
    assert mask.dtype == torch.bool and torch.equal(mask, out["ref_msk"]) and int(mask.sum()) == 192
    rgb, ref_rgb = envgs_step.filtered_blend(r["img"][:3].permute(1, 2, 0).reshape(1, H * W, 3), spec, r["rgb_env"], mask)
    assert torch.equal(rgb, out["rgb_map"]) and torch.equal(ref_rgb, out["ref_rgb_map"])
    # the acc filter on the recorded accumulation map: the strict comparison of :443
    acc = envgs_step.reflection_mask("acc", alpha=out["acc_map"], acc_threshold=0.75)
    assert torch.equal(acc, out["acc_map"][..., 0] > 0.75) and int(acc.sum()) == 268
    ro, rd = envgs_step.filtered_rays(torch.arange(768 * 3.0).reshape(1, 768, 3), -torch.arange(768 * 3.0).reshape(1, 768, 3), mask)
    assert ro.shape == rd.shape == (1, 192, 3) and torch.equal(ro[0, :, 0], torch.nonzero(mask[0])[:, 0] * 3.0) and torch.equal(rd, -ro)


# ---------------------------------------------------------------------------------------------------------------- 2. GPU: the selection
def _masks(H, W):
    P = H * W
    gen = torch.Generator().manual_seed(H)
    z = lambda: torch.zeros(P, dtype=torch.bool)
    m = {"random": torch.rand(P, generator=gen) < 0.5, "none": z(), "all": ~z(), "last": z(), "first_1024": z(), "first_1023": z(),
         "from_1024": z(), "blocks_of_64": (torch.arange(P) // 64) % 2 == 0}
    m["last"][-1] = True
    m["first_1024"][:1024] = True; m["first_1023"][:1023] = True; m["from_1024"][1024:] = True
    return {k: v.reshape(H, W) for k, v in m.items()}


@gpu
@pytest.mark.parametrize("H,W", [(37, 53), (40, 56)])
def test_select_pixels_positions_and_count(H, W):
    """37x53 = 1961 pixels crosses the scan's 1024-counter workgroup boundary; runs that switch at pixel 1023 / 1024 and 64-aligned blocks."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    for name, mask in _masks(H, W).items():
        sel = fused.select_pixels(mask=mask.to(dev))
        flat = mask.reshape(-1)
        assert sel.count == int(flat.sum()), name
        assert sel.mask.shape == (H, W) and sel.mask.dtype == torch.bool and torch.equal(sel.mask.cpu(), mask), name
        want = torch.cumsum(flat.long(), 0) - 1
        assert torch.equal(sel.positions.cpu().long()[:H * W][flat], want[flat]), name
        assert torch.equal(sel.keep.cpu().bool(), flat), name
    # the acc filter: the same selection as mask = allmap[1] > 0.75; pixels at exactly 0.75 are not kept
    gen = torch.Generator().manual_seed(W)
    allmap = torch.randn(7, H, W, generator=gen)
    allmap[1] = torch.rand(H, W, generator=gen)
    allmap[1, 3, :9] = 0.75; allmap[1, -1, -1] = 0.75; allmap[1, 0, 0] = float(np.nextafter(np.float32(0.75), np.float32(1.0)))
    want = allmap[1] > 0.75
    assert not want[3, :9].any() and not want[-1, -1] and want[0, 0]
    a = fused.select_pixels(allmap=allmap.to(dev), acc_threshold=0.75)
    b = fused.select_pixels(mask=want.to(dev))
    assert a.count == b.count == int(want.sum()) and torch.equal(a.mask.cpu(), want)
    assert torch.equal(a.keep, b.keep) and torch.equal(a.positions[:H * W][a.mask.reshape(-1)], b.positions[:H * W][b.mask.reshape(-1)])
    with pytest.raises(ValueError):
        fused.select_pixels()
    with pytest.raises(ValueError):
        fused.select_pixels(mask=want.to(dev), allmap=allmap.to(dev))


# ---------------------------------------------------------------------------------------------------------------- 3. GPU: reflect_filtered
def _reflect_inputs(dev):
    """The inputs of tests/test_fused_glue.py::test_reflect_matches_torch."""
    H, W = 40, 56
    cam = synth.orbit_camera(2, H=H, W=W, fx=1111.1 * W / 800.0, device=dev)
    ro, rd = synth.get_rays(cam)
    gen = torch.Generator().manual_seed(3)
    allmap = torch.randn(7, H, W, generator=gen).to(dev)
    allmap[1] = torch.rand(H, W, generator=gen).to(dev) * 0.9 + 0.05
    allmap[0] = allmap[1] * (3 + torch.rand(H, W, generator=gen).to(dev))
    allmap[1, :2] = 0; allmap[0, :2] = 0                  # empty pixels: 0/0 -> nan_to_num -> 0, zero gradient
    allmap[2:5, 5, :4] = 0                                # zero normal: x/(|x|+eps) stays finite
    return H, W, cam, ro, rd, allmap


@gpu
@pytest.mark.parametrize("kind", ["random", "none", "all"])
@pytest.mark.parametrize("ratio", [0.0, 0.3])
def test_reflect_filtered_matches_torch(ratio, kind):
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    H, W, cam, ro, rd, allmap = _reflect_inputs(dev)
    mask = _masks(H, W)[kind].to(dev)                     # (random: empty pixels and zero normals on both sides of it)
    sel = fused.select_pixels(mask=mask)
    S = int(mask.sum())
    assert sel.count == S
    a1 = allmap.clone().requires_grad_(True); o1 = ro.clone().requires_grad_(True); d1 = rd.clone().requires_grad_(True)
    nw, dep, ref_o, ref_d = fused.reflect_filtered(a1, o1, d1, cam.world_view_transform, sel, ratio)
    assert nw.shape == (3, H, W) and dep.shape == (1, H, W) and ref_o.shape == ref_d.shape == (1, S, 3)

    a2 = allmap.clone().requires_grad_(True); o2 = ro.clone().requires_grad_(True); d2 = rd.clone().requires_grad_(True)
    alpha = a2[1:2]
    nw2 = (a2[2:5].permute(1, 2, 0) @ cam.world_view_transform[:3, :3].T).permute(2, 0, 1)          # gaussian2d_utils.py:1123
    de = torch.nan_to_num(a2[0:1] / alpha, 0, 0); dm = torch.nan_to_num(a2[5:6], 0, 0)               # :1126-1131
    dep2 = de * (1 - ratio) + dm * ratio                                                               # :1136
    nn_ = nw2.permute(1, 2, 0); nn_ = nn_ / (nn_.norm(dim=-1, keepdim=True) + 1e-8)                    # math_utils.normalize
    ref_d2 = (d2 - 2 * (d2 * nn_).sum(-1, keepdim=True) * nn_)[mask][None]                             # envgs_sampler.py:424, :445
    ref_o2 = (o2 + d2 * dep2.permute(1, 2, 0))[mask][None]                                             # :427, :444
    for x, y in ((nw, nw2), (dep, dep2), (ref_o, ref_o2), (ref_d, ref_d2)):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-5)
    # the dense maps are those of the dense kernel
    with torch.no_grad():
        nw0, dep0, _, _ = fused.reflect(allmap, ro, rd, cam.world_view_transform, ratio)
    torch.testing.assert_close(nw.detach(), nw0, rtol=0, atol=1e-6)
    torch.testing.assert_close(dep.detach(), dep0, rtol=0, atol=1e-6)
    ws = [torch.randn_like(t) for t in (nw2, dep2, ref_o2, ref_d2)]
    sum((x * w).sum() for x, w in zip((nw, dep, ref_o, ref_d), ws)).backward()
    sum((x * w).sum() for x, w in zip((nw2, dep2, ref_o2, ref_d2), ws)).backward()
    # (torch's backward of nan_to_num(0/0) is NaN at empty pixels, the kernel's 0: compare where alpha > 0, require finiteness everywhere)
    live = allmap[1] > 0
    torch.testing.assert_close(a1.grad[2:], a2.grad[2:], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(a1.grad[:2][:, live], a2.grad[:2][:, live], rtol=1e-4, atol=1e-4)
    assert float(a1.grad[:2][:, ~live].abs().max()) == 0.0
    torch.testing.assert_close(o1.grad, o2.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(d1.grad, d2.grad, rtol=1e-4, atol=1e-4)
    assert torch.isfinite(a1.grad).all()
    if S < H * W:
        assert float(o1.grad[~mask].abs().max()) == 0.0 and float(d1.grad[~mask].abs().max()) == 0.0
    # upstream gradient on the compact rays only: a pixel that is not kept receives exactly nothing
    a3 = allmap.clone().requires_grad_(True)
    _, _, ro3, rd3 = fused.reflect_filtered(a3, ro, rd, cam.world_view_transform, sel, ratio)
    ((ro3 * ws[2]).sum() + (rd3 * ws[3]).sum()).backward()
    assert torch.isfinite(a3.grad).all()
    if S < H * W:
        assert float(a3.grad[:, ~mask].abs().max()) == 0.0
    if S > 0:
        assert float(a3.grad[:, mask].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- 4. GPU: blend_filtered
@gpu
@pytest.mark.parametrize("C", [5, 7])
def test_blend_filtered_matches_the_twin(C):
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    H, W, S = 37, 53, C - 4
    gen = torch.Generator().manual_seed(4)
    mask = _masks(H, W)["random"].to(dev)
    n = int(mask.sum())
    img = torch.rand(C, H, W, generator=gen).to(dev).requires_grad_(True)
    env = torch.rand(1, n, 3, generator=gen).to(dev).requires_grad_(True)
    up = torch.randn(H, W, 3, generator=gen).to(dev)
    sel = fused.select_pixels(mask=mask)
    out, ref_rgb = fused.blend_filtered(img, env, sel)
    assert out.shape == ref_rgb.shape == (H, W, 3) and not ref_rgb.requires_grad
    (out * up).sum().backward()
    gi, ge = img.grad.clone(), env.grad.clone()
    img.grad = None; env.grad = None
    want, want_ref = envgs_step.filtered_blend(img[:3].permute(1, 2, 0), img[3:3 + S].permute(1, 2, 0), env, mask)
    (want * up).sum().backward()
    assert float((out - want).abs().max()) <= 1e-6 and float((ref_rgb - want_ref).abs().max()) <= 1e-6
    assert ge.shape == env.shape
    assert float((gi - img.grad).abs().max()) <= 1e-5 * float(img.grad.abs().max()) and float((ge - env.grad).abs().max()) <= 1e-6
    # exactly: the base colour and its gradient pass through a pixel that is not kept; nothing reaches the roughness channel
    d = img.detach()
    assert torch.equal(out.detach()[~mask], d[:3].permute(1, 2, 0)[~mask]) and float(ref_rgb[~mask].abs().max()) == 0.0
    assert torch.equal(gi[:3].permute(1, 2, 0)[~mask], up[~mask]) and float(gi[3:][:, ~mask].abs().max()) == 0.0
    assert float(gi[C - 1].abs().max()) == 0.0
    # the (S,3) form of rgb_env; every pixel kept: the dense blend; none kept: the base colour
    out2, _ = fused.blend_filtered(d, env.detach()[0], sel)
    assert torch.equal(out2, out.detach())
    full = torch.rand(H, W, 3, generator=gen).to(dev)
    every = fused.select_pixels(mask=torch.ones(H, W, dtype=torch.bool, device=dev))
    assert every.count == H * W
    out3, ref3 = fused.blend_filtered(d, full.reshape(1, H * W, 3), every)
    assert torch.equal(out3, fused.blend(d, full))
    nothing = fused.select_pixels(mask=torch.zeros(H, W, dtype=torch.bool, device=dev))
    assert nothing.count == 0
    out4, ref4 = fused.blend_filtered(d, torch.empty(1, 0, 3, device=dev), nothing)
    assert torch.equal(out4, d[:3].permute(1, 2, 0)) and float(ref4.abs().max()) == 0.0


@gpu
def test_blend_filtered_reproduces_the_recorded_filtered_step(recorded):
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    r, out = recorded, recorded["out"]
    H, W = r["H"], r["W"]
    sel = fused.select_pixels(mask=out["ref_msk"].reshape(H, W).to(dev))
    assert sel.count == 192
    rgb, ref_rgb = fused.blend_filtered(r["img"].to(dev), r["rgb_env"].to(dev), sel)
    torch.testing.assert_close(rgb.cpu().reshape(1, H * W, 3), out["rgb_map"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(ref_rgb.cpu().reshape(1, H * W, 3), out["ref_rgb_map"], rtol=1e-6, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- 5. GPU: the step
def _scene(dev, H=48, W=64):
    """The scene of tests/test_envgs_step_parity.py with the base scales x 2.5 instead of x 5: about half of the pixels have alpha > 0.75
    (at x 5, 93 % do)."""
    base = synth.base_gaussians(1500, seed=3)
    base["scales"] = base["scales"] * 2.5
    base["opacities"] = torch.sigmoid(torch.randn(1500, 1, generator=torch.Generator().manual_seed(1)) + 1.5)
    env = synth.env_gaussians(800, seed=4, bound=12.0)
    mv = lambda d: {k: v.to(dev).clone().requires_grad_(True) for k, v in d.items()}
    camd = synth.orbit_camera(1, H=H, W=W, fx=1111.1 * W / 800.0, device=dev)
    return mv(base), mv(env), camd


def _upstream(H, W, dev, keep=None, allmap=True):
    gen = torch.Generator().manual_seed(7)
    dcol = (torch.randn(H, W, 3, generator=gen) / (H * W)).to(dev)
    dall = (torch.randn(7, H, W, generator=gen) / (H * W)).to(dev); dall[5:] = 0
    if keep is not None:                                 # upstream gradient only where the oracle's audits call the pixel / its reflected ray determined
        k = keep.to(dev)
        dcol = dcol * k[..., None]; dall = dall * k[None]
    return dcol, (dall if allmap else None)


def _run(pkg, tpkg, tracer, dev, keep=None, backward=True, allmap_grad=True):
    base, env, cam = _scene(dev)
    rays = synth.get_rays(cam)
    bg = torch.zeros(3, device=dev); env_bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    out = envgs_step.envgs_forward(pkg, tpkg, tracer, cam, rays, base, env, bg, env_bg, torch.tensor([2], device=dev))
    g = {}
    if backward:
        dcol, dall = _upstream(cam.image_height, cam.image_width, dev, keep, allmap_grad)
        loss = (out["rgb"] * dcol).sum()
        if dall is not None:
            loss = loss + (out["base"]["allmap"] * dall).sum()
        loss.backward()
        g = {("base." + k): v.grad for k, v in base.items() if v.grad is not None}
        g.update({("env." + k): v.grad for k, v in env.items() if v.grad is not None})
    return out, g, (base, env, cam, rays)


n = lambda t: t.detach().cpu().numpy()


def _glue_f64(cam, rays, img, allmap, rgb_env, mask):
    """The filtered glue between the two extension calls in float64 on CPU tensors: the dense expressions of envgs_sampler.py:420-431 followed by
    the twins of :433-455 / :461-476."""
    V = cam.world_view_transform.detach().cpu().double()
    ray_o, ray_d = rays[0].detach().cpu().double(), rays[1].detach().cpu().double()
    alpha = allmap[1:2]
    normal = (allmap[2:5].permute(1, 2, 0) @ (V[:3, :3].T)).permute(2, 0, 1)
    depth = torch.nan_to_num(allmap[0:1] / alpha, 0, 0)
    nrm = normal.permute(1, 2, 0)
    nrm = nrm / (nrm.norm(dim=-1, keepdim=True) + 1e-8)
    ref_d = ray_d - 2 * (ray_d * nrm).sum(-1, keepdim=True) * nrm
    ref_o = ray_o + ray_d * depth.permute(1, 2, 0)
    ref_o, ref_d = envgs_step.filtered_rays(ref_o, ref_d, mask)
    rgb, _ = envgs_step.filtered_blend(img[:3].permute(1, 2, 0), img[3:4].permute(1, 2, 0), rgb_env, mask)
    return ref_o, ref_d, rgb


_REF_MSK = {}


@gpu
@pytest.mark.parametrize("fused_glue", [False, True])
def test_filtered_envgs_step_link_by_link(fused_glue):
    """FILTER = acc @ 0.75 in both caller forms: one raster call, one traced call of (1,S,3) rays; the traced call against the oracle on the rays
    the step built, the glue against the twins in float64 on the recorded tensors; the compact ray gradients reach the rasterizer at kept pixels
    and nothing reaches a pixel that is not kept.  (torch caller form: autograd's own backward of nan_to_num(0 / 0) is NaN at pixels with no
    coverage, in the dense step as well -- tests/test_fused_glue.py; the exact-zero claim is made there for the pixels that have coverage, and
    for every pixel in the fused form, whose kernel writes 0.)"""
    import diff_surfel_rasterization_wet_ch05 as pkg
    import diff_surfel_tracing as tpkg
    from oracle import raster as orc, trace as otr
    test = "filtered_step[%s]" % ("fused" if fused_glue else "torch")
    dev = torch.device("cuda:0")
    deg = 2
    was = (envgs_step.FUSED["on"], dict(envgs_step.FILTER))
    envgs_step.FUSED["on"] = fused_glue
    envgs_step.FILTER.update(mode="acc", acc_threshold=0.75)
    try:
        # 1. forward only: what the step hands to the two extensions; the oracle's audits of exactly that
        with torch.no_grad():
            out1, _, (base, env, cam, rays) = _run(pkg, tpkg, tpkg.SurfelTracer(), dev, backward=False)
        H, W = cam.image_height, cam.image_width
        msk = out1["ref_msk"].cpu()
        S = int(msk.sum())
        assert out1["ref_msk"].shape == (H, W) and out1["ref_msk"].dtype == torch.bool
        assert out1["ref_o"].shape == out1["ref_d"].shape == out1["rgb_env"].shape == (1, S, 3) and out1["ref_rgb"].shape == (H, W, 3)
        record(test, "kept_share", S / (H * W), "(S = %d of %d)" % (S, H * W))
        assert 0.3 <= S / (H * W) <= 0.7
        assert torch.equal(msk, out1["base"]["allmap"][1].cpu() > 0.75)
        ref = orc.raster_forward(n(base["means3D"]), n(base["opacities"]), n(cam.world_view_transform), n(cam.full_proj_transform), n(cam.camera_center), W, H,
                                 scales=n(base["scales"]), rotations=n(base["rotations"]), colors_precomp=n(out1["base"]["colors"]).astype(np.float32),
                                 bg=np.zeros(3, np.float32))
        frag_px = orc.raster_audit(ref)["fragile"]
        env_np = {k: v.detach().cpu() for k, v in env.items()}
        ra = otr.trace_audit(n(out1["ref_o"]).reshape(-1, 3), n(out1["ref_d"]).reshape(-1, 3), n(env["means3D"]), n(env["scales"]), n(env["rotations"]),
                             n(env["opacities"]), start_from_first=False, shs=n(env["shs"]), sh_degree=deg)
        frag_ray_px = np.zeros((H, W), bool)
        frag_ray_px[msk.numpy()] = ra["fragile"]
        keep_np = ~(frag_px | frag_ray_px)                  # (H,W): pixels that receive an upstream gradient
        keep_rays = keep_np[msk.numpy()]                    # (S,): their compact rays
        nex = int((~keep_rays).sum())
        record_fragile(test, "excluded_rays", ~keep_rays, FRAGILE_RAYS_MAX, "(%d fragile pixels, %d fragile reflected rays)" % (int(frag_px.sum()), int(ra["fragile"].sum())))
        keep = torch.from_numpy(keep_np)
        # 2. the step with gradients, every extension call tapped; upstream gradient only on the determined pixels
        with stagewise.RasterTap() as rtap, stagewise.TraceTap() as ttap:
            out, g_h, (base, env, cam, rays) = _run(pkg, tpkg, tpkg.SurfelTracer(), dev, keep)
        # 3. the same with the upstream gradient on rgb alone
        with stagewise.RasterTap() as rtap2:
            _run(pkg, tpkg, tpkg.SurfelTracer(), dev, keep, allmap_grad=False)
        torch.cuda.synchronize()
    finally:
        envgs_step.FUSED["on"] = was[0]
        envgs_step.FILTER.clear(); envgs_step.FILTER.update(was[1])
    assert len(rtap.calls) == 1 and len(ttap.calls) == 1 and len(rtap2.calls) == 1
    assert torch.equal(out["ref_o"], out1["ref_o"]) and torch.equal(out["base"]["img"], out1["base"]["img"]) and torch.equal(out["ref_msk"].cpu(), msk)
    # the two caller forms select the same pixels (the raster forward is deterministic)
    _REF_MSK[fused_glue] = msk
    if len(_REF_MSK) == 2:
        assert torch.equal(_REF_MSK[False], _REF_MSK[True])
    rc, tc = rtap.calls[0], ttap.calls[0]
    # ---- the traced call: (1,S,3) rays, S = ref_msk.sum() ------------------------------------------------------------------------------
    assert tc["sff"] is False
    assert tuple(tc["o_in"].shape) == tuple(tc["d_in"].shape) == (1, S, 3) and S == int(out["ref_msk"].sum())
    assert tuple(tc["outs"][0].shape) == (1, S, 3)
    # ---- link 2: the traced call against the oracle on the rays the step built ------------------------------------------------------------
    _, tb = stagewise.oracle_trace_call(test, "trace", tc, env_np, np.array([0.1, 0.2, 0.3], np.float32), deg, use_sh=True, others=False, nfr=nex, keep=keep_rays)
    stagewise.check_summed_param_grads(test, "trace", env, [tb], nfr=nex)
    assert float(out["rgb_env"].detach().abs().mean()) > 0.05 and float(out["base"]["spec"].detach().mean()) > 0.01
    assert float(np.abs(n(tc["o_in"].grad)).max()) > 0 and float(np.abs(tb["dray_d"]).max()) > 0
    # ---- link 3: the glue vs the twins in float64 on the recorded tensors -----------------------------------------------------------------
    dd = torch.float64
    img64 = out["base"]["img"].detach().cpu().to(dd).requires_grad_(True)
    all64 = out["base"]["allmap"].detach().cpu().to(dd).requires_grad_(True)
    env64 = out["rgb_env"].detach().cpu().to(dd).requires_grad_(True)
    ref_o, ref_d, rgb = _glue_f64(cam, rays, img64, all64, env64, msk)
    stagewise.glue_check(test, "glue.ref_o", out["ref_o"], ref_o, floor=1.0)
    stagewise.glue_check(test, "glue.ref_d", out["ref_d"], ref_d, floor=1.0)
    stagewise.glue_check(test, "glue.rgb", out["rgb"], rgb, floor=1.0)
    dcol, dall = _upstream(H, W, torch.device("cpu"), keep)
    loss = (rgb * dcol.to(dd)).sum() + (all64 * dall.to(dd)).sum() + (ref_o * tc["o_in"].grad.cpu().to(dd)).sum() + (ref_d * tc["d_in"].grad.cpu().to(dd)).sum()
    loss.backward()
    fl = lambda t: float(t[torch.isfinite(t)].abs().mean()) + 1e-12
    stagewise.glue_check(test, "glue.d_img", rc["dL_dcolor"], img64.grad, floor=fl(img64.grad))
    stagewise.glue_check(test, "glue.d_allmap", rc["dL_dallmap"], all64.grad, floor=fl(all64.grad))
    stagewise.glue_check(test, "glue.d_rgb_env", tc["up"][0], env64.grad, floor=fl(env64.grad))
    # ---- the compact ray gradients reach the rasterizer's depth / normal maps at kept pixels, and only there ----------------------------
    d2 = rtap2.calls[0]["dL_dallmap"].cpu()                  # upstream on rgb alone: everything in it came through the rays
    covered = out["base"]["allmap"][1].detach().cpu() > 0
    assert int((~covered).sum()) > 0 and not (msk & ~covered).any()
    assert float(d2[0:5][:, msk & keep].abs().max()) > 0 and float(rc["dL_dallmap"].cpu()[0:5][:, msk].abs().max()) > 0
    dropped = ~msk if fused_glue else (~msk & covered)
    assert float(d2[:, dropped].abs().max()) == 0.0
    if fused_glue:
        assert torch.isfinite(d2).all()
    assert {"base.means3D", "base.rotations", "base.specular", "env.shs", "env.means3D"} <= set(g_h)
    assert float(g_h["base.rotations"].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- 6. GPU: defer, colour-only
@gpu
def test_filtered_step_with_deferred_env_surfel_gradients():
    """FILTER with DEFER and COLOUR_ONLY: after join_deferred_gradients() the env leaves hold the gradients of the stream-ordered step (the tracer
    kernels are the same, only their ordering differs); S = 0 returns the base colour without an env pass."""
    import diff_surfel_rasterization_wet_ch05 as pkg
    import diff_surfel_tracing as tpkg
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    was = (envgs_step.FUSED["on"], envgs_step.DEFER["on"], envgs_step.COLOUR_ONLY["on"], dict(envgs_step.FILTER))
    res = {}
    try:
        envgs_step.FUSED["on"] = True; envgs_step.COLOUR_ONLY["on"] = True
        envgs_step.FILTER.update(mode="acc", acc_threshold=0.75)
        for defer in (False, True):
            envgs_step.DEFER["on"] = defer
            tracer = tpkg.SurfelTracer()
            out, g, (base, env, cam, rays) = _run(pkg, tpkg, tracer, dev)
            assert tracer.caps.colour_only and bool(tracer.caps.defer_reduce) == defer
            assert tracing._DEFERRED["pending"] == defer
            tracing.join_deferred_gradients()
            assert not tracing._DEFERRED["pending"]
            torch.cuda.synchronize()
            res[defer] = {k: v.clone() for k, v in g.items()}
            assert 0 < int(out["ref_msk"].sum()) < out["ref_msk"].numel()
        # nothing kept: no traced call, the base colour
        envgs_step.DEFER["on"] = False
        envgs_step.FILTER.update(acc_threshold=2.0)
        with stagewise.TraceTap() as ttap:
            out, g0, _ = _run(pkg, tpkg, tpkg.SurfelTracer(), dev, allmap_grad=False)
        assert len(ttap.calls) == 0 and int(out["ref_msk"].sum()) == 0 and out["rgb_env"].shape == (1, 0, 3) and out["ref_o"].shape == (1, 0, 3)
        assert torch.equal(out["rgb"].detach(), out["base"]["img"].detach()[:3].permute(1, 2, 0)) and float(out["ref_rgb"].abs().max()) == 0.0
        assert not any(k.startswith("env.") for k in g0) and float(g0["base.shs"].abs().max()) > 0
    finally:
        envgs_step.FUSED["on"], envgs_step.DEFER["on"], envgs_step.COLOUR_ONLY["on"] = was[:3]
        envgs_step.FILTER.clear(); envgs_step.FILTER.update(was[3])
    assert set(res[False]) == set(res[True]) and {"env.means3D", "env.shs", "env.opacities", "env.scales", "env.rotations"} <= set(res[True])
    for k in res[False]:
        a, b = res[False][k], res[True][k]
        assert float(a.abs().max()) > 0 or not k.startswith("env."), k
        if k.startswith("env."):
            assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max()), k
