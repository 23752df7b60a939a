"""Forward + backward time of the front end from RAW surfel parameters to the extensions' inputs, at the sizes of the EnvGS step:

  base  300 000 surfels, S = 1, M = 16, degree 3: colours (P,5) + opacities + scales + rotations       (what the rasterizer takes)
  env   163 840 surfels, no reflection parameters, M = 16: shs + opacities + scales + rotations + the 3-sigma quads   (what the tracer takes)

  torch  the path before envgs_amd.model existed: ckpt.activate (exp, F.normalize, sigmoids, cat(dc, rest)) + fused.sh_colors / fused.surfel_quads,
         autograd replaying the activations and splitting the cat's gradient;
  fused  model.raster_inputs / model.tracer_inputs (include/envgs_model.h): one launch each way.

The upstream gradients are fixed tensors handed to torch.autograd.grad, so neither form pays for a loss expression.  Both in one process,
alternating, warmed up; device events around ITERS iterations each; median of REPEATS repeats, with the spread.  Bytes: the algorithmic minimum of
the fused form (every raw byte read once, every output byte written once per direction), from the shapes.
    python profiles/model_inputs_timing.py [--iters 200] [--repeats 5] [--out FILE]
    python profiles/model_inputs_timing.py --trace fused|torch     # a few iterations only: the program to put behind `rocprofv3 --kernel-trace --stats --`
Needs a GPU; there is no CPU path."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]          # profiles/numbers.py must not stand in for the standard library's
sys.path.insert(0, os.path.dirname(HERE))

import argparse  # noqa: E402
import statistics  # noqa: E402

import torch  # noqa: E402

P_BASE, P_ENV, DEG = 300000, 163840, 3


def raw_of(g, dev, reflect):
    raw = {"_xyz": g["means3D"], "_features_dc": g["shs"][:, :1], "_features_rest": g["shs"][:, 1:], "_scaling": torch.log(g["scales"]),
           "_rotation": g["rotations"] * 1.3, "_opacity": torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4))}
    if reflect:
        raw["_specular"], raw["_roughness"] = torch.logit(g["specular"]), torch.logit(g["roughness"])
    return {k: v.to(dev).contiguous().requires_grad_(True) for k, v in raw.items()}


def byte_model(P, M, S, colours, shs, quads):
    """(forward, backward) bytes of the fused form: raw reads + output writes; upstream + raw re-reads + raw-gradient writes."""
    f4 = 4
    raw_small = (2 + 4 + 1 + (S + 1 if S else 0)) * f4                       # scaling, rotation, opacity, specular, roughness
    act_small = raw_small
    feats = 3 * M * f4
    C = (3 + S + 1 if S else 3) * f4
    fwd = raw_small + (2 + 4 + 1) * f4                                       # scales, rotations, opacities out
    bwd = (2 + 4 + 1) * f4 + raw_small + act_small + feats                   # upstreams, raw re-read, raw gradients (the feature gradients are fully written)
    if colours:
        fwd += 3 * f4 + feats + C + 3                                        # xyz, dc / rest in place, colours, clamped
        bwd += C + 3 + 3 * f4 + feats + 3 * f4                               # d colours, clamped, xyz, coefficients re-read, d xyz
    if shs:
        fwd += 2 * feats; bwd += feats                                       # copy; upstream read
    if quads:
        fwd += 3 * f4 + 12 * f4
    return P * fwd, P * bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", choices=("fused", "torch"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("model_inputs_timing.py needs a GPU")
    from envgs_amd import ckpt, fused, model, synth
    dev = torch.device("cuda", 0)
    base = raw_of(synth.base_gaussians(P_BASE, seed=0), dev, True)
    env = raw_of(synth.env_gaussians(P_ENV, seed=1), dev, False)
    campos = synth.orbit_camera(1, device=dev).camera_center
    deg = torch.tensor([DEG], device=dev)
    gen = torch.Generator().manual_seed(3)
    up = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    g_base = [up(P_BASE, 5), up(P_BASE, 1), up(P_BASE, 2), up(P_BASE, 4)]
    g_env = [up(P_ENV, 16, 3), up(P_ENV, 1), up(P_ENV, 2), up(P_ENV, 4)]
    base_leaves, env_leaves = list(base.values()), list(env.values())[1:]     # (no gradient reaches the env positions from here: the quads carry none)

    def step_base(form):
        if form == "fused":
            o = model.raster_inputs(base, campos, deg)
            outs = [o["colors_precomp"], o["opacities"], o["scales"], o["rotations"]]
        else:
            a = ckpt.activate(base)
            outs = [fused.sh_colors(a["means3D"], a["shs"], campos, deg, a["specular"], a["roughness"]), a["opacities"], a["scales"], a["rotations"]]
        return outs, torch.autograd.grad(outs, base_leaves, g_base)

    def step_env(form):
        if form == "fused":
            o = model.tracer_inputs(env)
            v = o["v"]
        else:
            o = ckpt.activate(env)
            v, _ = fused.surfel_quads(o["means3D"], o["scales"], o["rotations"])
        outs = [o["shs"], o["opacities"], o["scales"], o["rotations"]]
        return outs + [v], torch.autograd.grad(outs, env_leaves, g_env)

    sets = (("base", step_base, byte_model(P_BASE, 16, 1, True, False, False)), ("env", step_env, byte_model(P_ENV, 16, 0, False, True, True)))
    lines = ["front end from raw surfel parameters, forward + backward: base %d surfels (S = 1, M = 16, degree %d, colours), env %d surfels (shs + quads)"
             % (P_BASE, DEG, P_ENV), "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]
    for name, step, _ in sets:                                                # the two forms compute the same thing at the sizes that are timed
        (of, gf), (ot, gt) = step("fused"), step("torch")
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        lines.append("%-4s max|fused - torch| / max|torch|: outputs %.2e, raw gradients %.2e" % (
            name, max(rel(a, b) for a, b in zip(of, ot)), max(rel(a, b) for a, b in zip(gf, gt))))
    if args.trace:
        for _ in range(10):
            for _, step, _ in sets:
                step(args.trace)
        torch.cuda.synchronize()
        print("\n".join(lines))
        print("traced 1 + 10 iterations of the %s form (plus one of the other, for the comparison above)" % args.trace)
        return
    for name, step, (bf, bb) in sets:
        for _ in range(20):
            step("fused"); step("torch")
        torch.cuda.synchronize()
        times = {"fused": [], "torch": []}
        for r in range(args.repeats):
            for form in ("torch", "fused"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    step(form)
                e1.record()
                torch.cuda.synchronize()
                times[form].append(e0.elapsed_time(e1) / args.iters)
        for form in ("torch", "fused"):
            t = times[form]
            lines.append("%-4s %-5s  median %.4f ms  min %.4f  max %.4f  (%d repeats x %d iterations; per repeat: %s)" % (
                name, form, statistics.median(t), min(t), max(t), args.repeats, args.iters, " ".join("%.4f" % v for v in t)))
        mf = statistics.median(times["fused"])
        lines.append("%-4s ratio torch / fused (medians): %.2f;  fused byte model %.1f MB forward + %.1f MB backward -> %.2f TB/s over the whole call "
                     "(launch gaps and allocations included: an end-to-end rate, not a kernel's)" % (
                         name, statistics.median(times["torch"]) / mf, bf / 1e6, bb / 1e6, (bf + bb) / (mf * 1e-3) / 1e12))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
