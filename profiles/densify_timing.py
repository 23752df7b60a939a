"""What the densification bookkeeping costs a trainer, staged (`SurfelSet`'s default: the reference's boolean-mask expressions over the HIP compaction
kernels) against the device-resident mode (`SurfelSet(device_schedule=True)`, include/envgs_densify.h), at the bench scene: 800 x 800 pixels,
300 000 base + 163 840 environment surfels.

  step   HOST WALL time per step of a loop that runs the fused EnvGS step (bench.py's: envgs_step.envgs_forward, backward, the deferred join) +
         FusedAdam + `add_densification_stats` for both sets -- with the statistics left out, staged, and as the one launch.  The base set's
         statistics take what the step produced (the gradient of means2D, radii > 0, the rasterizer's weights and radii); the environment set's
         take a fixed (P,3) gradient and the surfels the trace touched (a fixed mask if the tracer's weights are not per surfel).  Wall time, not
         device time: the staged form's cost is the host waiting for the queue to drain a dozen times per set.
  pass   clone + split + prune by opacity / gradient at P = 300 000 with Adam moments: the staged three stages against `grow_and_prune`,
         milliseconds (synchronised on both sides) and peak allocated bytes above the set's own.

    python profiles/densify_timing.py [--steps 40] [--repeats 5] [--out FILE]
Needs a GPU; there is no CPU path."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]          # profiles/numbers.py must not stand in for the standard library's
sys.path.insert(0, os.path.dirname(HERE))

import argparse  # noqa: E402
import statistics  # noqa: E402
import time  # noqa: E402

import torch  # noqa: E402

P_BASE, P_ENV, RES = 300000, 163840, 800
NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_specular", "_roughness")
PASS_ARGS = dict(min_opacity=0.05, min_gradient=0.02, grad_threshold=0.25, size_threshold=0.01, split_screen_threshold=40.0)


def step_loop(dev, steps, repeats, lines):
    import diff_surfel_rasterization_wet_ch05 as pkg
    import diff_surfel_tracing as tpkg
    from envgs_amd import densify, envgs_step, synth, tracing
    from envgs_amd.optim import FusedAdam
    H = W = RES
    HW = H * W
    names = ["means3D", "shs", "opacities", "scales", "rotations"]
    g = synth.base_gaussians(P_BASE, seed=0, device=dev)
    ge = synth.env_gaussians(P_ENV, seed=1, device=dev)
    params = {k: g[k].clone().requires_grad_(True) for k in names}
    params["specular"] = g["specular"].contiguous().clone().requires_grad_(True)
    params["roughness"] = g["roughness"].clone().requires_grad_(True)
    env_params = {k: ge[k].clone().requires_grad_(True) for k in names}
    cams = [synth.orbit_camera(v, n_views=8, H=H, W=W, fx=1111.1 * W / 800.0, device=dev) for v in range(8)]
    rays = [synth.get_rays(c) for c in cams]
    bg, env_bg, sh_degree = torch.zeros(3, device=dev), torch.zeros(3, device=dev), torch.tensor([3], device=dev)
    gen = torch.Generator().manual_seed(1)
    dcol = (torch.randn(5, H, W, generator=gen) / HW).to(dev)
    dall = (torch.randn(7, H, W, generator=gen) / HW).to(dev)
    dall[6] = 0
    dcol_hw3 = dcol[:3].permute(1, 2, 0).contiguous()
    envgs_step.FUSED["on"] = True
    envgs_step.DEFER["on"] = True
    tracer = tpkg.SurfelTracer()
    all_params = list(params.values()) + list(env_params.values())
    opt = FusedAdam([{"params": [v], "lr": 0.0, "name": k} for k, v in params.items()]
                    + [{"params": [v], "lr": 0.0, "name": "env_" + k} for k, v in env_params.items()], lr=0.0, eps=1e-15)
    env_grad = torch.randn(P_ENV, 3, generator=gen).to(dev)
    env_mask = (torch.rand(P_ENV, generator=gen) > 0.3).to(dev)
    sets = {form: (densify.SurfelSet({"_xyz": params["means3D"].detach()}, None, device_schedule=form == "device"),
                   densify.SurfelSet({"_xyz": env_params["means3D"].detach()}, None, device_schedule=form == "device")) for form in ("staged", "device")}

    def step(it, form):
        vi = it % 8
        out = envgs_step.envgs_forward(pkg, tpkg, tracer, cams[vi], rays[vi], params, dict(env_params), bg, env_bg, sh_degree)
        b = out["base"]
        loss = (out["rgb"] * dcol_hw3).sum() + (b["allmap"] * dall).sum()
        loss.backward()
        tracing.join_deferred_gradients()
        opt.step()
        if form != "none":
            base_set, env_set = sets[form]
            base_set.add_densification_stats(b["means2D"].grad, b["radii"] > 0, b["weight"].reshape(-1, 1), b["radii"])
            wet = out["env_wet"]
            env_set.add_densification_stats(env_grad, (wet.reshape(-1) > 0) if wet is not None and wet.numel() == P_ENV else env_mask)
        for p_ in all_params:
            p_.grad = None

    for it in range(6):
        for form in ("none", "staged", "device"):
            step(it, form)
    torch.cuda.synchronize()
    times = {"none": [], "staged": [], "device": []}
    for r in range(repeats):
        for form in ("none", "staged", "device"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in range(steps):
                step(it, form)
            torch.cuda.synchronize()
            times[form].append((time.perf_counter() - t0) * 1e3 / steps)
    for form in ("none", "staged", "device"):
        t = times[form]
        lines.append("step  statistics %-6s  median %.3f ms  min %.3f  max %.3f  (host wall per step; %d repeats x %d steps; per repeat: %s)" % (
            form, statistics.median(t), min(t), max(t), repeats, steps, " ".join("%.3f" % v for v in t)))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append("step  statistics cost per step (medians): staged %+.3f ms, device %+.3f ms" % (med["staged"] - med["none"], med["device"] - med["none"]))
    a, b = sets["staged"][0].stats, sets["device"][0].stats
    lines.append("step  base set after the run: denom equal %s, max_radii2D equal %s, max |gradient accum difference| / max %.2e" % (
        bool(torch.equal(a["denom"], b["denom"])), bool(torch.equal(a["max_radii2D"], b["max_radii2D"])),
        float((a["xyz_gradient_accum"] - b["xyz_gradient_accum"]).abs().max() / a["xyz_gradient_accum"].abs().max().clamp_min(1e-30))))


def pass_timing(dev, repeats, lines):
    from envgs_amd import densify, synth
    g = synth.base_gaussians(P_BASE, seed=0)
    raw = {"_xyz": g["means3D"], "_features_dc": g["shs"][:, :1], "_features_rest": g["shs"][:, 1:], "_scaling": torch.log(g["scales"]), "_rotation": g["rotations"] * 1.3,
           "_opacity": torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4)), "_specular": torch.logit(g["specular"]), "_roughness": torch.logit(g["roughness"])}
    raw = {k: v.to(dev).contiguous() for k, v in raw.items()}
    gen = torch.Generator().manual_seed(5)
    denom = torch.randint(0, 6, (P_BASE, 1), generator=gen).float()
    stats = {"xyz_gradient_accum": torch.rand(P_BASE, 1, generator=gen) * denom, "denom": denom, "max_radii2D": torch.rand(P_BASE, generator=gen) * 50,
             "xyz_weight_accum": torch.rand(P_BASE, 1, generator=gen) * 3 * denom}
    scale_med = float(torch.exp(raw["_scaling"]).max(dim=1).values.median())
    args = dict(PASS_ARGS, size_threshold=scale_med)                      # half of the surfels on each side of the clone / split divide

    def build(device_schedule):
        prm = {k: torch.nn.Parameter(raw[k].clone()) for k in NAMES}
        opt = torch.optim.Adam([{"params": [prm[k]], "lr": 1e-3, "name": k} for k in NAMES], lr=0.0, eps=1e-15)
        for k in NAMES:
            opt.state[prm[k]] = {"step": torch.tensor(2.0), "exp_avg": torch.randn_like(prm[k]) * 0.1, "exp_avg_sq": torch.rand_like(prm[k]) * 0.01}
        s = densify.SurfelSet(prm, opt, "", generator=torch.Generator(device=dev).manual_seed(9), device_schedule=device_schedule)
        for k in s.STATS:
            s.stats[k] = stats[k].to(dev).clone()
        return s

    def run(s, form):
        if form == "one-pass":
            s.grow_and_prune(**args)
        else:
            s.densify_and_clone(args["grad_threshold"], args["size_threshold"])
            s.densify_and_split(args["grad_threshold"], args["size_threshold"], args["split_screen_threshold"])
            s.prune_min_opacity_and_gradients(args["min_opacity"], args["min_gradient"])

    res = {"staged": [], "one-pass": []}
    logs = {}
    for r in range(repeats + 1):                                          # (the first round warms both forms up and is dropped)
        for form in ("staged", "one-pass"):
            s = build(form == "one-pass")
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            t0 = time.perf_counter()
            run(s, form)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            peak = torch.cuda.max_memory_allocated(dev) - base
            if r:
                res[form].append((ms, peak))
            logs[form] = (list(s.log), s.number)
            del s
    lines.append("pass  P = %d, 8 parameters with both Adam moments, thresholds %s" % (P_BASE, args))
    lines.append("pass  events %s -> %d surfels; the two forms agree: %s" % (logs["staged"][0], logs["staged"][1], logs["staged"] == logs["one-pass"]))
    for form in ("staged", "one-pass"):
        ms = [v[0] for v in res[form]]
        lines.append("pass  %-8s  median %.3f ms  min %.3f  max %.3f  peak allocated above the set %.1f MB  (%d repeats: %s)" % (
            form, statistics.median(ms), min(ms), max(ms), max(v[1] for v in res[form]) / 1e6, repeats, " ".join("%.3f" % v for v in ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densify_timing.py needs a GPU")
    dev = torch.device("cuda", 0)
    lines = ["densification bookkeeping, staged against device-resident: %d x %d pixels, %d base + %d environment surfels" % (RES, RES, P_BASE, P_ENV),
             "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]
    pass_timing(dev, args.repeats, lines)
    step_loop(dev, args.steps, args.repeats, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
