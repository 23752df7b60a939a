"""Filtered reflection rays (envgs_step.FILTER, mode "acc" at 0.75) at 800 x 800 on the bench scene (300 000 base / 163 840 environment
surfels, -ch05, fused caller with bench.py's defaults):

  glue   the launches between the two extension calls -- pixel selection, reflected rays, blend, and their backward -- on the tensors of one
         recorded step:  torch = the twins of envgs_step.py (reflection_mask / filtered_rays / filtered_blend after the dense torch expressions,
         autograd replaying them),  fused = fused.select_pixels / reflect_filtered / blend_filtered;
  step   forward + backward + optimizer step of the fused caller with the filter on against the same step unfiltered (every pixel traced).

Both pairs in one process, alternating, warmed up; device events around ITERS iterations each; median of REPEATS repeats, with the spread.
    python profiles/filtered_reflection_timing.py [--iters 50] [--repeats 5] [--out FILE]
Needs a GPU; there is no CPU path.  Recorded numbers, nothing is asserted."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]          # profiles/numbers.py must not stand in for the standard library's
sys.path.insert(0, os.path.dirname(HERE))

import argparse  # noqa: E402
import statistics  # noqa: E402

import torch  # noqa: E402

H = W = 800
P_BASE, P_ENV = 300000, 163840
THR = 0.75


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filtered_reflection_timing.py needs a GPU")
    import diff_surfel_rasterization_wet_ch05 as pkg
    import diff_surfel_tracing as tpkg
    from envgs_amd import envgs_step, fused, synth, tracing
    from envgs_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    names = ["means3D", "shs", "opacities", "scales", "rotations", "specular", "roughness"]
    g = synth.base_gaussians(P_BASE, seed=0, device=dev)
    base = {k: g[k].clone().requires_grad_(True) for k in names}
    ge = synth.env_gaussians(P_ENV, seed=1, device=dev)
    env = {k: ge[k].clone().requires_grad_(True) for k in names[:5]}
    cams = [synth.orbit_camera(v, n_views=8, H=H, W=W, fx=1111.1 * W / 800.0, device=dev) for v in range(8)]
    rays = [synth.get_rays(c) for c in cams]
    gen = torch.Generator().manual_seed(1)
    dcol = (torch.randn(H, W, 3, generator=gen) / (H * W)).to(dev)
    dall = (torch.randn(7, H, W, generator=gen) / (H * W)).to(dev); dall[6] = 0
    bg, env_bg, deg = torch.zeros(3, device=dev), torch.zeros(3, device=dev), torch.tensor([3], device=dev)
    opt = FusedAdam([{"params": [v], "lr": 0.0} for v in list(base.values()) + list(env.values())], lr=0.0, eps=1e-15)      # (lr 0: the scene, and S, stay put)
    tracer = tpkg.SurfelTracer()
    envgs_step.FUSED["on"] = True
    envgs_step.DEFER["on"] = True
    envgs_step.FILTER.update(acc_threshold=THR)

    def step(it, filtered):
        envgs_step.FILTER["mode"] = "acc" if filtered else None
        vi = it % 8
        out = envgs_step.envgs_forward(pkg, tpkg, tracer, cams[vi], rays[vi], base, env, bg, env_bg, deg)
        ((out["rgb"] * dcol).sum() + (out["base"]["allmap"] * dall).sum()).backward()
        opt.step()                                                         # (joins the deferred env-surfel gradients)
        for p_ in opt.param_groups:
            p_["params"][0].grad = None
        return out

    shares = [int(step(v, True)["ref_msk"].sum()) / (H * W) for v in range(8)]
    lines = ["filtered reflection rays, acc > %.2f, %d x %d pixels, %d base / %d environment surfels, -ch05, fused caller" % (THR, H, W, P_BASE, P_ENV),
             "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "S / (H*W) over the 8 views: mean %.4f  min %.4f  max %.4f" % (sum(shares) / 8, min(shares), max(shares))]

    # ---- the glue launches on the tensors of one recorded step (view 0) ---------------------------------------------------------------------
    out = step(0, True)
    torch.cuda.synchronize()
    cam, (ray_o, ray_d) = cams[0], rays[0]
    allmap = out["base"]["allmap"].detach().clone().requires_grad_(True)
    img = out["base"]["img"].detach().clone().requires_grad_(True)
    rgb_env = out["rgb_env"].detach().clone().requires_grad_(True)
    S = rgb_env.shape[1]
    g_o, g_d = torch.randn(1, S, 3, device=dev) / (H * W), torch.randn(1, S, 3, device=dev) / (H * W)
    del out

    def glue(form):
        if form == "fused":
            sel = fused.select_pixels(allmap=allmap, acc_threshold=THR)
            _, _, ro, rd = fused.reflect_filtered(allmap, ray_o, ray_d, cam.world_view_transform, sel, 0.0)
            rgb, _ = fused.blend_filtered(img, rgb_env, sel)
        else:
            alpha = allmap[1:2]                                               # envgs_step.base_pass / envgs_forward, torch caller form
            normal = (allmap[2:5].permute(1, 2, 0) @ (cam.world_view_transform[:3, :3].T)).permute(2, 0, 1)
            depth = torch.nan_to_num(allmap[0:1] / alpha, 0, 0)
            nrm = normal.permute(1, 2, 0)
            nrm = nrm / (nrm.norm(dim=-1, keepdim=True) + 1e-8)
            ref_d = ray_d - 2 * (ray_d * nrm).sum(-1, keepdim=True) * nrm
            ref_o = ray_o + ray_d * depth.permute(1, 2, 0)
            mask = envgs_step.reflection_mask("acc", alpha=alpha.detach().permute(1, 2, 0), acc_threshold=THR)
            ro, rd = envgs_step.filtered_rays(ref_o, ref_d, mask)
            rgb, _ = envgs_step.filtered_blend(img[:3].permute(1, 2, 0), img[3:4].permute(1, 2, 0), rgb_env, mask)
        return torch.autograd.grad([rgb, ro, rd], [allmap, img, rgb_env], [dcol, g_o, g_d])

    ga, gb = glue("fused"), glue("torch")
    for nm, a, b in zip(("d allmap", "d img", "d rgb_env"), ga, gb):
        ok = torch.isfinite(b)
        lines.append("glue %-10s max|fused - torch| / max|torch| %.2e" % (nm, float((a[ok] - b[ok]).abs().max() / b[ok].abs().max())))

    def timed(pairs, iters):
        for fn in pairs.values():
            for i in range(8):
                fn(i)
        torch.cuda.synchronize()
        times = {k: [] for k in pairs}
        for r in range(args.repeats):
            for k, fn in pairs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(iters):
                    fn(i)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / iters)
        return times

    def report(title, times, a, b):
        for k, t in times.items():
            lines.append("%s %-10s median %.4f ms  min %.4f  max %.4f  (%d repeats x %d iterations; per repeat: %s)" % (
                title, k, statistics.median(t), min(t), max(t), args.repeats, args.iters, " ".join("%.4f" % v for v in t)))
        lines.append("%s ratio %s / %s (medians): %.2f" % (title, a, b, statistics.median(times[a]) / statistics.median(times[b])))

    report("glue", timed({"torch": lambda i: glue("torch"), "fused": lambda i: glue("fused")}, args.iters), "torch", "fused")
    report("step", timed({"unfiltered": lambda i: step(i, False), "filtered": lambda i: step(i, True)}, args.iters), "unfiltered", "filtered")
    tracing.join_deferred_gradients()
    torch.cuda.synchronize()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
