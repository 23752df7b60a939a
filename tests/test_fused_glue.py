"""GPU: the fused caller-side glue (envgs_amd.fused) against the torch expressions it replaces (the reference's own lines,
re-derived in envgs_amd/envgs_step.py), forward and autograd backward.  Floating-point elementwise kernels: fp32 torch is the checker;
the surface normals are also compared with a float64 twin of the same expressions (below), whose CPU pin is the one test here that needs no GPU."""
import math

import numpy as np
import pytest
import torch

from envgs_amd import envgs_step, synth
from tests import reference_caller
from tests.util import look_at_camera



def _sh_colors_cases():
    """Every degree x M in {16, (D+1)^2} (plus M = 9 at degree 1) x P in {1, 3, 65, 5000}: partial quads, a partial wave and a partial workgroup of the
    four-lanes-per-surfel kernels.  The P = 5000 cases that predate the ladder keep their ids."""
    S_of = {(0, 16): 1, (2, 16): 1, (3, 16): 3, (2, 9): 1, (1, 4): 3, (0, 1): 3, (1, 16): 1, (1, 9): 1}
    out = []
    for (deg, M), S in S_of.items():
        for P in (5000, 1, 3, 65):
            out.append(pytest.param(deg, S, M, P, id="%d-%d-%d" % (deg, S, M) + ("" if P == 5000 else "-P%d" % P)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("deg,S,M,P", _sh_colors_cases())
def test_sh_colors_matches_torch(deg, S, M, P):
    """M = 16: the four-lanes-per-surfel kernels; other coefficient counts: the one-lane-per-surfel ones.  The stored coefficients beyond the active degree
    are large (tests/test_sh_degree_ladder.py:ladder_shs): they must reach no colour and receive exactly no gradient."""
    from envgs_amd import fused
    from tests.test_sh_degree_ladder import ladder_shs
    dev = torch.device("cuda:0")
    nb = (deg + 1) ** 2
    g = synth.base_gaussians(P, seed=deg)
    g["shs"] = ladder_shs(g["shs"], deg)[:, :M].contiguous()       # (a sixth of the surfels: strongly negative DC -- the clamp and its zero gradient)
    g = {k: v.to(dev) for k, v in g.items()}
    cam = synth.orbit_camera(1, device=dev)
    spec = torch.rand(P, S, device=dev)
    leaves = [g["means3D"].clone().requires_grad_(True), g["shs"].clone().requires_grad_(True), spec.clone().requires_grad_(True),
              g["roughness"].clone().requires_grad_(True)]
    out = fused.sh_colors(leaves[0], leaves[1], cam.camera_center, torch.tensor([deg], device=dev), leaves[2], leaves[3])
    ref_l = [t.detach().clone().requires_grad_(True) for t in leaves]
    d = ref_l[0] - cam.camera_center[None]; d = d / d.norm(dim=1, keepdim=True)
    ref = torch.cat([torch.clamp_min(envgs_step.eval_sh(deg, ref_l[1].transpose(1, 2), d) + 0.5, 0.0), ref_l[2], ref_l[3]], dim=-1)
    assert out.shape == ref.shape == (P, 3 + S + 1)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-6)
    w = torch.randn_like(ref)
    (out * w).sum().backward(); (ref * w).sum().backward()
    for a, b in zip(leaves, ref_l):
        bg = b.grad if b.grad is not None else torch.zeros_like(b)          # degree 0 does not depend on the view direction
        torch.testing.assert_close(a.grad, bg, rtol=1e-4, atol=1e-6)
    assert leaves[1].grad.shape == (P, M, 3)
    if M > nb:
        assert float(leaves[1].grad[:, nb:].abs().max()) == 0.0
    assert float(leaves[1].grad[:, :nb].abs().max()) > 0
    if P >= 6:
        assert (out[:P // 6, :3] == 0).any() and (out[P // 6:, :3] > 0).any()      # the clamp (and its zero gradient) is exercised


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [0.0, 0.3])
def test_reflect_matches_torch(ratio):
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    H, W = 40, 56
    cam = synth.orbit_camera(2, H=H, W=W, fx=1111.1 * W / 800.0, device=dev)
    ro, rd = synth.get_rays(cam)
    gen = torch.Generator().manual_seed(3)
    allmap = torch.randn(7, H, W, generator=gen).to(dev)
    allmap[1] = torch.rand(H, W, generator=gen).to(dev) * 0.9 + 0.05
    allmap[0] = allmap[1] * (3 + torch.rand(H, W, generator=gen).to(dev))
    allmap[1, :2] = 0; allmap[0, :2] = 0                  # empty pixels: 0/0 -> nan_to_num -> 0, zero gradient
    allmap[2:5, 5, :4] = 0                                # zero normal: x/(|x|+eps) stays finite
    a1 = allmap.clone().requires_grad_(True); o1 = ro.clone().requires_grad_(True); d1 = rd.clone().requires_grad_(True)
    nw, dep, ref_o, ref_d = fused.reflect(a1, o1, d1, cam.world_view_transform, ratio)

    a2 = allmap.clone().requires_grad_(True); o2 = ro.clone().requires_grad_(True); d2 = rd.clone().requires_grad_(True)
    alpha = a2[1:2]
    nw2 = (a2[2:5].permute(1, 2, 0) @ cam.world_view_transform[:3, :3].T).permute(2, 0, 1)          # gaussian2d_utils.py:1123
    de = torch.nan_to_num(a2[0:1] / alpha, 0, 0); dm = torch.nan_to_num(a2[5:6], 0, 0)               # :1126-1131
    dep2 = de * (1 - ratio) + dm * ratio                                                               # :1136
    n = nw2.permute(1, 2, 0); n = n / (n.norm(dim=-1, keepdim=True) + 1e-8)                           # math_utils.normalize
    ref_d2 = d2 - 2 * (d2 * n).sum(-1, keepdim=True) * n                                               # envgs_sampler.py:424
    ref_o2 = o2 + d2 * dep2.permute(1, 2, 0)                                                           # :427
    for x, y in ((nw, nw2), (dep, dep2), (ref_o, ref_o2), (ref_d, ref_d2)):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-5)
    ws = [torch.randn_like(t) for t in (nw2, dep2, ref_o2, ref_d2)]
    sum((x * w).sum() for x, w in zip((nw, dep, ref_o, ref_d), ws)).backward()
    sum((x * w).sum() for x, w in zip((nw2, dep2, ref_o2, ref_d2), ws)).backward()
    # torch's own backward of nan_to_num(0/0) is 0 * inf = NaN at empty pixels (harmless upstream: such pixels have no contributors);
    # the fused kernel returns 0 there, so compare where alpha > 0 and require finiteness everywhere
    live = allmap[1] > 0
    torch.testing.assert_close(a1.grad[2:], a2.grad[2:], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(a1.grad[:2][:, live], a2.grad[:2][:, live], rtol=1e-4, atol=1e-4)
    assert float(a1.grad[:2][:, ~live].abs().max()) == 0.0
    torch.testing.assert_close(o1.grad, o2.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(d1.grad, d2.grad, rtol=1e-4, atol=1e-4)
    assert torch.isfinite(a1.grad).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [0.0, 0.4])
def test_surface_normal_matches_torch(ratio):
    """fused.surface_normal (depth select + dpt2norm + alpha scaling, one kernel each way) vs the torch expressions of render()'s tail
    (tests/reference_caller.py: surface_maps; its dpt2norm is pinned against the reference's by tests/test_golden.py)."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    H, W = 44, 60
    cam = synth.orbit_camera(3, H=H, W=W, fx=1111.1 * W / 800.0, device=dev)
    gen = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    allmap = torch.randn(7, H, W, generator=gen)
    allmap[1] = torch.rand(H, W, generator=gen) * 0.9 + 0.05
    allmap[0] = allmap[1] * (3.0 + 0.01 * xx + 0.3 * torch.sin(yy / 5.0) + 0.05 * torch.rand(H, W, generator=gen))
    allmap[5] = 3.2 + 0.02 * yy + 0.05 * torch.rand(H, W, generator=gen)
    allmap[1, :3, :7] = 0; allmap[0, :3, :7] = 0          # empty pixels: depth 0/0 -> 0
    allmap = allmap.to(dev)
    a1 = allmap.clone().requires_grad_(True)
    sd, sn = fused.surface_normal(a1, cam, ratio)
    a2 = allmap.clone().requires_grad_(True)
    sd2, sn2 = reference_caller.surface_maps(cam, a2, ratio)
    assert sd.shape == (1, H, W) and sn.shape == (3, H, W)
    torch.testing.assert_close(sd, sd2, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(sn, sn2, rtol=2e-4, atol=2e-5)
    snd = sn.detach()
    assert float(snd[:, 0].abs().max()) == 0 and float(snd[:, :, -1].abs().max()) == 0 and float(snd[:, 5:-5, 10:-5].abs().min(dim=0).values.max()) > 0
    wd, wn = torch.randn_like(sd2), torch.randn_like(sn2)
    ((sd * wd).sum() + (sn * wn).sum()).backward()
    ((sd2 * wd).sum() + (sn2 * wn).sum()).backward()
    live = allmap[1] > 0
    g1, g2 = a1.grad, a2.grad
    assert torch.isfinite(g1).all()
    scale = float(g2[:, live].abs().max())
    for ch in (0, 1, 5):
        err = (g1[ch][live] - g2[ch][live]).abs().max()
        assert float(err) <= 2e-4 * scale + 1e-6, (ch, float(err), scale)
    assert float(g1[[2, 3, 4, 6]].abs().max()) == 0 and float(g1[:2][:, ~live].abs().max()) == 0


@pytest.mark.gpu
def test_surfel_quads_match_get_disks():
    """fused.surfel_quads == the python get_disks twin (itself pinned against the reference's own output by tests/test_golden.py)."""
    from envgs_amd import fused, synth
    dev = torch.device("cuda:0")
    e = synth.env_gaussians(5000, seed=3, device=dev)
    q = e["rotations"] * (0.5 + torch.rand(5000, 1, device=dev))           # un-normalised quaternions, as the optimizer leaves them
    v, f = fused.surfel_quads(e["means3D"], e["scales"], q)
    v2, f2 = synth.get_disks(e["means3D"], e["scales"], q)
    assert v.shape == v2.shape and f.shape == f2.shape and f.dtype == f2.dtype
    assert torch.equal(f, f2)
    assert float((v - v2).abs().max()) <= 2e-6 * float(v2.abs().max())
    v3, f3 = fused.surfel_quads(e["means3D"], e["scales"], q)               # the cached face table
    assert f3 is f and torch.equal(v3, v)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [5, 7])
def test_blend_matches_torch(C):
    """fused.blend == (1 - spec) * rgb_base + spec * rgb_env on slices of the rasterizer's output, values and both gradients."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    H, W, S = 37, 53, C - 4
    gen = torch.Generator().manual_seed(4)
    img = torch.rand(C, H, W, generator=gen).to(dev).requires_grad_(True)
    env = torch.rand(H, W, 3, generator=gen).to(dev).requires_grad_(True)
    up = torch.randn(H, W, 3, generator=gen).to(dev)
    out = fused.blend(img, env)
    (out * up).sum().backward()
    gi, ge = img.grad.clone(), env.grad.clone()
    img.grad = None; env.grad = None
    spec = img[3:3 + S].permute(1, 2, 0)
    ref = (1 - spec) * img[:3].permute(1, 2, 0) + spec * env
    (ref * up).sum().backward()
    assert float((out - ref).abs().max()) <= 1e-6
    assert float((gi - img.grad).abs().max()) <= 1e-5 * float(img.grad.abs().max()) and float((ge - env.grad).abs().max()) <= 1e-6
    assert float(gi[C - 1].abs().max()) == 0.0



@pytest.mark.gpu
def test_bounce_stage_glue_matches_torch_f64():
    """fused.bounce_rays / bounce_blend / bounce_pack_mid == the torch expressions of a bounce stage (gaussian2d_sampler.py:413-426 as restated in
    tracing.py:_forward_bounces), values and every gradient against float64 autograd; rows that do not bounce receive exactly zero (rays) or pass
    their gradient through (colour)."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    R = 5000
    gen = torch.Generator().manual_seed(11)
    mk = lambda *s: torch.randn(*s, generator=gen)
    o, d = mk(R, 3), mk(R, 3)
    d = d / d.norm(dim=-1, keepdim=True)
    dpt = torch.rand(R, 1, generator=gen) * 3 + 0.5; acc = torch.rand(R, 1, generator=gen) * 0.5 + 0.5
    norm = mk(R, 3) * 0.3; aux = torch.rand(R, 2, generator=gen); rgb = torch.rand(R, 3, generator=gen)
    sel = torch.nonzero(torch.rand(R, generator=gen) < 0.6)[:, 0]
    n = sel.numel()
    col_next = torch.rand(n, 3, generator=gen)
    up_o, up_d, up_c = mk(n, 3), mk(n, 3), mk(R, 3)

    def run(dtype, device, fusedp):
        L = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in (o, d, dpt, acc, norm, aux, rgb, col_next)]
        o_, d_, dpt_, acc_, norm_, aux_, rgb_, cn_ = L
        s_ = sel.to(device)
        if fusedp:
            o2, d2 = fused.bounce_rays(o_, d_, dpt_, acc_, norm_, s_)
            col = fused.bounce_blend(rgb_, aux_, cn_, s_)
        else:
            nh = norm_[s_] / norm_[s_].norm(dim=-1, keepdim=True)
            o2 = o_[s_] + d_[s_] * (dpt_[s_] / acc_[s_])
            d2 = d_[s_] - 2.0 * (d_[s_] * nh).sum(-1, keepdim=True) * nh
            sp = aux_[s_, 0:1]
            col = rgb_.index_put((s_,), (1.0 - sp) * rgb_[s_] + sp * cn_)
        loss = (o2 * up_o.to(device=device, dtype=dtype)).sum() + (d2 * up_d.to(device=device, dtype=dtype)).sum() + (col * up_c.to(device=device, dtype=dtype)).sum()
        loss.backward()
        return [x.detach().double().cpu() for x in (o2, d2, col)], [t.grad.detach().double().cpu() for t in L]

    (ro2, rd2, rcol), rg = run(torch.float64, "cpu", False)
    (go2, gd2, gcol), gg = run(torch.float32, dev, True)
    for a, b in ((ro2, go2), (rd2, gd2), (rcol, gcol)):
        assert float((a - b).abs().max()) <= 2e-6 * (1.0 + float(a.abs().max()))
    names = ("ray_o", "ray_d", "dpt", "acc", "norm", "aux", "rgb", "col_next")
    for nm, a, b in zip(names, rg, gg):
        assert float((a - b).abs().max()) <= 2e-5 * (float(a.abs().max()) + 1e-12), nm
    keep = torch.ones(R, dtype=torch.bool); keep[sel] = False
    for i in (0, 1, 2, 3, 4):                                                # ray-side inputs: rows that do not bounce get exactly nothing
        assert float(gg[i][keep].abs().max()) == 0.0
    assert torch.equal(gg[6][keep].float(), up_c[keep])                      # colour: passed through
    # mid: 16 channels of stage 1 at the rows `sel`, stage 0 at every row
    mid = torch.zeros(R, 32, device=dev)
    st0 = [t.to(dev) for t in (o, d, dpt, acc, norm, aux, rgb)]
    fused.bounce_pack_mid(mid, 0, 2, None, *st0)
    st1 = [t.to(dev) for t in (go2.float(), gd2.float(), dpt[sel], acc[sel], norm[sel], aux[sel], col_next)]
    fused.bounce_pack_mid(mid, 1, 2, sel.to(dev), *st1)
    want = torch.zeros(R, 32)
    want[:, :16] = torch.cat([o, d, dpt, acc, norm, aux, rgb], 1)
    want[sel, 16:] = torch.cat([t.cpu() for t in st1], 1)
    assert torch.equal(mid.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# Surface normals against float64.  reference_caller.surface_maps is float32 only (its K and pixel grid are float32 tensors) and bench.py runs
# through it, so the float64 ground truth is a dtype-generic twin of the same expressions, kept here and pinned bit for bit, in float32, to
# reference_caller's.  The bound is  max(1e-4, K * e_twin32):  e_twin32 = the float32 twin (CPU) against the float64 twin, the realised error
# of one float32 evaluation of these expressions (at the training focal length P[y+1] - P[y-1] loses about three digits in ANY float32
# implementation); K as for the image loss (tests/test_loss.py: 4, or 2 when every measured ratio is below 1).
K_F32 = 4.0


def _twin_dpt2norm(cam, dpt):
    """reference_caller.dpt2norm with every tensor in dpt's dtype."""
    import math
    dt, dev = dpt.dtype, dpt.device
    c2w = torch.linalg.inv(cam.world_view_transform.to(device=dev, dtype=dt).T)
    W, H = cam.image_width, cam.image_height
    fx = W / (2 * math.tan(cam.FoVx / 2.)); fy = H / (2 * math.tan(cam.FoVy / 2.))
    K = torch.tensor([[fx, 0., W / 2.], [0., fy, H / 2.], [0., 0., 1.0]], dtype=dt, device=dev)
    u, v = torch.meshgrid(torch.arange(W, dtype=dt, device=dev), torch.arange(H, dtype=dt, device=dev), indexing='xy')
    pix = torch.stack([u, v, torch.ones_like(u)], dim=-1).reshape(-1, 3)
    ray_d = pix @ torch.linalg.inv(K).mT @ c2w[:3, :3].mT
    xyz = (dpt.reshape(-1, 1) * ray_d + c2w[:3, 3]).reshape(H, W, 3)
    out = torch.zeros_like(xyz)
    dx = xyz[2:, 1:-1] - xyz[:-2, 1:-1]
    dy = xyz[1:-1, 2:] - xyz[1:-1, :-2]
    out[1:-1, 1:-1, :] = torch.nn.functional.normalize(torch.cross(dx, dy, dim=-1), dim=-1)
    return out


def _twin_surface_maps(cam, allmap, depth_ratio=0.0):
    """reference_caller.surface_maps in allmap's dtype."""
    alpha = allmap[1:2]
    median = torch.nan_to_num(allmap[5:6], 0, 0)
    expect = torch.nan_to_num(allmap[0:1] / alpha, 0, 0)
    depth = expect * (1 - depth_ratio) + median * depth_ratio
    normal = _twin_dpt2norm(cam, depth).permute(2, 0, 1) * alpha.detach()
    return depth, normal


# (H, W, fx): today's input; the training focal length on a crop, and twice it; then fx scaled with W as tests/util.py:small_scene does --
# one interior pixel, one interior row / column, a row longer than a workgroup, a width that is the tile of other kernels
# Then fx != fy (with fx == fy everywhere, exchanging the two in the kernels' pixel direction would pass), one of them rolled about the viewing axis
# as well: there the third entry is (fx, fy, roll), fx = None scaling with W as above.
SURF_ANISO = (44, 60, (83.3, 50.0, 0.0))
SURF_SHAPES = [(44, 60, 83.3), (44, 60, 1111.1), (20, 33, 2222.2), (3, 3, None), (3, 70, None), (70, 3, None), (4, 257, None), (17, 16, None),
               pytest.param(*SURF_ANISO, id="44-60-fx83.3-fy50"), pytest.param(20, 33, (1111.1, 700.0, 0.5), id="20-33-fx1111.1-fy700-roll0.5"),
               pytest.param(17, 16, (None, 0.6 * 1111.1 * 16 / 800.0, 0.0), id="17-16-scaled-fy0.6fx")]
ORBIT_EYE_3 = (4.0 * math.cos(math.radians(20.0)) * math.cos(0.75 * math.pi), 4.0 * math.cos(math.radians(20.0)) * math.sin(0.75 * math.pi),
               4.0 * math.sin(math.radians(20.0)))             # where synth.orbit_camera(3) stands


def _surf_cam(H, W, focal, device="cpu"):
    """View 3 of synth.orbit_camera through tests/util.py:look_at_camera (the same matrices when fy == fx and roll == 0)."""
    fx, fy, roll = focal if isinstance(focal, tuple) else (focal, None, 0.0)
    fx = fx if fx is not None else 1111.1 * W / 800.0
    return look_at_camera(ORBIT_EYE_3, (0.0, 0.0, 0.0), H, W, fx, fy, roll=roll, device=device)


def _focal_id(focal):
    fx, fy, roll = focal if isinstance(focal, tuple) else (focal, None, 0.0)
    return ("scaled" if fx is None else "%g" % fx) + ("" if fy is None else "-fy%g-roll%g" % (fy, roll))


def _surf_input(H, W, fx, seed=5):
    """allmap (7,H,W) with a smooth depth under 1e-3 noise and, away from the border and on at most a tenth of the pixels: a block (8 x 8 where it fits)
    of empty pixels (allmap[0] = allmap[1] = 0: 0/0), pixels with allmap[0] > 0, allmap[1] = 0 (+inf) and pixels with a NaN median."""
    cam = _surf_cam(H, W, fx)
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    allmap = torch.randn(7, H, W, generator=gen)
    allmap[1] = torch.rand(H, W, generator=gen) * 0.9 + 0.05
    allmap[0] = allmap[1] * (3.0 + 0.6 * xx / W + 0.3 * torch.sin(8.0 * yy / H) + 1e-3 * torch.randn(H, W, generator=gen))
    allmap[5] = 3.2 + 0.9 * yy / H + 0.2 * torch.cos(5.0 * xx / W) + 1e-3 * torch.randn(H, W, generator=gen)
    budget = (H * W) // 10
    n_few = 3 if budget >= 70 else (1 if budget >= 2 else 0)
    bh, bw = max(0, min(8, H - 4)), max(0, min(8, W - 4))
    while bh * bw + 2 * n_few > budget and bw > 0:
        bw -= 1
    empty = torch.zeros(H, W, dtype=torch.bool)
    if bh * bw:
        y0, x0 = (H - bh) // 2, (W - bw) // 2
        empty[y0:y0 + bh, x0:x0 + bw] = True
    inner = torch.zeros(H, W, dtype=torch.bool); inner[1:-1, 1:-1] = True
    free = torch.nonzero((inner & ~empty).reshape(-1))[:, 0]
    pick = free[torch.randperm(free.numel(), generator=gen)[:2 * n_few]]
    inf_px, nan_px = torch.zeros(H * W, dtype=torch.bool), torch.zeros(H * W, dtype=torch.bool)
    inf_px[pick[:n_few]] = True; nan_px[pick[n_few:]] = True
    inf_px, nan_px = inf_px.reshape(H, W), nan_px.reshape(H, W)
    allmap[0][empty] = 0; allmap[1][empty] = 0
    allmap[1][inf_px] = 0
    allmap[5][nan_px] = float("nan")
    assert int(empty.sum() + inf_px.sum() + nan_px.sum()) <= budget
    wd, wn = torch.randn(1, H, W, generator=gen), torch.randn(3, H, W, generator=gen)
    return cam, allmap, dict(empty=empty, inf=inf_px, nan=nan_px), wd, wn


def _twin_run(cam, allmap, ratio, wd, wn, dtype):
    a = allmap.detach().to(dtype).clone().requires_grad_(True)
    sd, sn = _twin_surface_maps(cam, a, ratio)
    loss = 0
    if wd is not None: loss = loss + (sd * wd.to(dtype)).sum()
    if wn is not None: loss = loss + (sn * wn.to(dtype)).sum()
    loss.backward()
    return sd.detach(), sn.detach(), a.grad


def test_surface_twin_is_reference_caller_in_float32():
    """The twin, in float32 on the CPU, is reference_caller.surface_maps bit for bit: values and gradients (NaN where torch's own backward of
    nan_to_num(0/0) gives NaN)."""
    for H, W, fx in ((44, 60, 1111.1), (17, 16, None), (3, 3, None), SURF_ANISO):
        cam, allmap, _, wd, wn = _surf_input(H, W, fx)
        assert isinstance(fx, tuple) == (abs(float(cam.K[0, 0] - cam.K[1, 1])) > 1)
        for ratio in (0.0, 0.4, 1.0):
            a = allmap.clone().requires_grad_(True)
            sd, sn = reference_caller.surface_maps(cam, a, ratio)
            ((sd * wd).sum() + (sn * wn).sum()).backward()
            sd2, sn2, g2 = _twin_run(cam, allmap, ratio, wd, wn, torch.float32)
            assert sd2.dtype == torch.float32 and torch.equal(sd2, sd.detach()) and torch.equal(sn2, sn.detach())
            assert torch.allclose(g2, a.grad, rtol=0, atol=0, equal_nan=True)
            assert float(sn2.abs().max()) > 0
        assert _twin_run(cam, allmap, 0.4, wd, wn, torch.float64)[1].dtype == torch.float64


def _surf_compare(name, H, W, fx, ratio, use_d=True, use_n=True):
    """fused.surface_normal against the float64 twin, bounded by the float32 twin's own error."""
    from envgs_amd import fused
    from tests.util import check_close, floor_rel_err, record
    dev = torch.device("cuda:0")
    cam, allmap, px, wd, wn = _surf_input(H, W, fx)
    wd, wn = (wd if use_d else None), (wn if use_n else None)
    sd64, sn64, g64 = _twin_run(cam, allmap, ratio, wd, wn, torch.float64)
    sd32, sn32, g32 = _twin_run(cam, allmap, ratio, wd, wn, torch.float32)
    a1 = allmap.to(dev).detach().clone().requires_grad_(True)
    camd = _surf_cam(H, W, fx, device=dev)
    sd, sn = fused.surface_normal(a1, camd, ratio)
    loss = 0
    if use_d: loss = loss + (sd * wd.to(dev)).sum()
    if use_n: loss = loss + (sn * wn.to(dev)).sum()
    loss.backward()
    g = a1.grad.cpu()
    sd, sn = sd.detach().cpu(), sn.detach().cpu()
    assert sd.shape == (1, H, W) and sn.shape == (3, H, W) and g.shape == (7, H, W)
    assert torch.isfinite(sd).all() and torch.isfinite(sn).all() and torch.isfinite(g).all()
    dead = px["empty"] | px["inf"]                       # alpha == 0: depth 0, no gradient (torch: NaN)
    assert float(g[[2, 3, 4, 6]].abs().max()) == 0.0
    assert float(g[:2][:, dead].abs().max() if dead.any() else 0.0) == 0.0 and float(g[5][px["nan"]].abs().max() if px["nan"].any() else 0.0) == 0.0
    assert float(sn[:, dead].abs().max() if dead.any() else 0.0) == 0.0
    # the surface depth: one division and one mix, a few float32 roundings
    assert float((sd.double() - sd64).abs().max()) <= 1e-6 * float(sd64.abs().max())
    live = ~dead
    pairs = [("normal", sn, sn32, sn64, live[None].expand(3, H, W)), ("dallmap[0]", g[0], g32[0], g64[0], live), ("dallmap[1]", g[1], g32[1], g64[1], live),
             ("dallmap[5]", g[5], g32[5], g64[5], ~px["nan"])]
    for what, hip, t32, t64, keep in pairs:
        keep = keep.numpy()
        b = t64.numpy()[keep]
        assert np.isfinite(b).all()
        if not np.any(b):                                # ratio 0 / 1, or no upstream reaches it: exactly nothing
            assert float(hip.abs().max()) == 0.0, what
            continue
        e_twin = float(floor_rel_err(t32.numpy()[keep], b)[0].max())
        bound = max(1e-4, K_F32 * e_twin)
        e_hip = float(floor_rel_err(hip.numpy()[keep], b)[0].max())
        print("%s %s: e_hip %.3e  e_twin32 %.3e  ratio %.3f" % (name, what, e_hip, e_twin, e_hip / max(e_twin, 1e-30)))
        record(name, what + " e_twin32", e_twin, note="float32 twin (CPU) vs float64 twin")
        record(name, what + " ratio", e_hip / max(e_twin, 1e-30), note="e_hip / e_twin32")
        check_close(name, what, hip.numpy(), t64.numpy(), tol=bound, keep=keep)



@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [0.0, 0.4, 1.0])
@pytest.mark.parametrize("H,W,fx", SURF_SHAPES)
def test_surface_normal_matches_float64_twin(H, W, fx, ratio):
    """Forward and dallmap[0, 1, 5] at every pixel that has a gradient, the neighbours of the holes (whose normals see a jump to depth 0) included."""
    name = "test_surface_normal_matches_float64_twin[%d-%d-%s-%g]" % (H, W, _focal_id(fx), ratio)
    _surf_compare(name, H, W, fx, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["normal_only", "depth_only"])
def test_surface_normal_single_upstream(which):
    """Only one of the two outputs reaches the loss: the other upstream pointer is NULL."""
    _surf_compare("test_surface_normal_single_upstream[%s]" % which, 20, 33, 2222.2, 0.4, use_d=which == "depth_only", use_n=which == "normal_only")


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(1, 5), (2, 2), (5, 1)])
def test_surface_normal_without_interior(H, W):
    """No pixel has four neighbours: every normal is zero, the depth is still the depth, and the backward is the direct dsurf_depth term alone
    (bit for bit what a call without dsurf_normal gives)."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    cam = synth.orbit_camera(3, H=H, W=W, fx=50.0, device=dev)
    gen = torch.Generator().manual_seed(8)
    allmap = torch.randn(7, H, W, generator=gen)
    allmap[1] = torch.rand(H, W, generator=gen) * 0.9 + 0.05
    allmap[0] = allmap[1] * (3.0 + torch.rand(H, W, generator=gen))
    allmap[5] = 3.0 + torch.rand(H, W, generator=gen)
    wd, wn = torch.randn(1, H, W, generator=gen), torch.randn(3, H, W, generator=gen)
    ratio = 0.4
    grads = []
    for with_n in (True, False):
        a = allmap.to(dev).detach().clone().requires_grad_(True)
        sd, sn = fused.surface_normal(a, cam, ratio)
        ((sd * wd.to(dev)).sum() + ((sn * wn.to(dev)).sum() if with_n else 0)).backward()
        grads.append(a.grad.cpu())
    assert float(sn.detach().abs().max()) == 0.0
    A = allmap.double()
    want = A[0] / A[1] * (1 - ratio) + A[5] * ratio
    assert float((sd.detach().cpu().double()[0] - want).abs().max()) <= 1e-6 * float(want.abs().max())
    g = grads[0]
    assert torch.isfinite(g).all() and torch.equal(g, grads[1])
    w = wd.double()[0]
    direct = torch.zeros(7, H, W, dtype=torch.float64)
    direct[0] = w * (1 - ratio) / A[1]; direct[1] = -w * (1 - ratio) * A[0] / (A[1] * A[1]); direct[5] = w * ratio
    assert float((g.double() - direct).abs().max()) <= 1e-6 * float(direct.abs().max())
    assert float(g[[2, 3, 4, 6]].abs().max()) == 0.0


@pytest.mark.gpu
def test_surface_normal_sends_minus_infinity_to_zero():
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    H, W = 5, 6
    cam = synth.orbit_camera(3, H=H, W=W, fx=50.0, device=dev)
    allmap = torch.rand(7, H, W, generator=torch.Generator().manual_seed(2)) + 0.5
    allmap[5, 2, 3] = float("-inf")                       # a -inf median
    allmap[0, 3, 2] = -1.0; allmap[1, 3, 2] = 0.0         # -1 / 0: a -inf expected depth
    a = allmap.to(dev).detach().clone().requires_grad_(True)
    sd, sn = fused.surface_normal(a, cam, 1.0)
    sd0, _ = fused.surface_normal(allmap.to(dev), cam, 0.0)
    (sd.sum() + sn.sum()).backward()
    # The kernels send -inf to 0, like NaN and +inf.  The reference's nan_to_num(x, 0, 0) leaves neginf at its default and sends -inf to the lowest
    # finite float (-3.4e38); the rasterizer cannot produce it (depths are >= 0.2), so the difference is pinned here and not reproduced.
    assert float(sd[0, 2, 3]) == 0.0 and float(sd0[0, 3, 2]) == 0.0 and float(torch.nan_to_num(allmap[5:6], 0, 0)[0, 2, 3]) < -3e38
    assert torch.isfinite(sd).all() and torch.isfinite(sn).all() and torch.isfinite(a.grad).all() and float(a.grad[5, 2, 3]) == 0.0
