"""Forward + backward time of the geometry regularisers at 800 x 800 pixels / 163 840 environment surfels with the options of
configs/models/envgs.yaml (norm_loss 0.01 + gs_norm_loss 0.04, both scaled by the normalised depth):

  torch  the expression form a user had to run before envgs_amd.loss.EnvGSGeometryLoss existed: the formulas of tests/reference_supervisor.py
         as torch ops on the GPU, autograd replaying them -- the depth scale evaluated once per term, i.e. four topk(k = 1 % of the pixels);
  fused  EnvGSGeometryLoss (include/envgs_supervisor.h).

Both in one process, alternating, warmed up; device events around ITERS iterations each; median of REPEATS repeats, with the spread.
    python profiles/supervisor_timing.py [--iters 200] [--repeats 5] [--out FILE]
    python profiles/supervisor_timing.py --trace fused|torch     # a few iterations only: the program to put behind `rocprofv3 --kernel-trace --stats --`
Needs a GPU; there is no CPU path."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]          # profiles/numbers.py must not stand in for the standard library's
sys.path.insert(0, os.path.dirname(HERE))

import argparse  # noqa: E402
import statistics  # noqa: E402

import torch  # noqa: E402

H, W, P = 800, 800, 163840
OPTS = dict(gs_norm_loss_weight=0.04, gs_norm_loss_start_iter=0, use_dpt_scale_gs_norm_loss=True, norm_loss_weight=0.01, norm_loss_start_iter=0,
            use_dpt_scale_norm_loss=True)


def make_inputs(dev):
    g = torch.Generator().manual_seed(7)
    N = H * W
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)
    nm = unit(torch.randn(N, 3, generator=g)) * (0.3 + 0.7 * torch.rand(N, 1, generator=g))
    nm[torch.rand(N, generator=g) < 0.1] = 0.0
    sn = unit(torch.randn(N, 3, generator=g)) * (0.3 + 0.7 * torch.rand(N, 1, generator=g))
    prior = unit(torch.randn(N, 3, generator=g)) * 0.5 + 0.5
    out = dict(norm_map=nm[None], surf_norm_map=sn[None], acc_map=torch.rand(1, N, 1, generator=g), dpt_map=1.0 + 5.0 * torch.rand(1, N, 1, generator=g),
               dist_map=0.1 * torch.rand(1, N, 1, generator=g), env_opacity=torch.rand(P, 1, generator=g))
    batch = dict(norm=prior[None], msk=(torch.rand(1, N, 1, generator=g) > 0.3).float(), R=torch.linalg.qr(torch.randn(3, 3, generator=g))[0][None])
    out = {k: v.to(dev).requires_grad_(k != "dpt_map") for k, v in out.items()}
    return out, {k: v.to(dev) for k, v in batch.items()}


def _unit(x):
    return x / (x.norm(dim=-1, keepdim=True) + 1e-8)


def _depth_scale(d):
    d = d.detach().clone()
    n = int(d.numel() * 0.01)
    near = d.ravel().topk(n, largest=False)[0].max()
    far = d.ravel().topk(n, largest=True)[0].min()
    return (1 - (d - near) / (far - near)).clip(0, 1)


def torch_form(out, batch):
    a = _unit(_unit(out["norm_map"]) @ batch["R"].mT)
    g = _unit(batch["norm"] * 2.0 - 1.0)
    norm_loss = (a - g).abs().sum(dim=-1) + 1 - torch.nn.functional.cosine_similarity(a, g, dim=-1)
    norm_loss = (norm_loss * _depth_scale(out["dpt_map"][..., 0])).mean()
    gs_norm_loss = 1 - (out["norm_map"] * out["surf_norm_map"]).sum(dim=-1)
    gs_norm_loss = (gs_norm_loss * _depth_scale(out["dpt_map"][..., 0])).mean()
    return OPTS["norm_loss_weight"] * norm_loss + OPTS["gs_norm_loss_weight"] * gs_norm_loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", choices=("fused", "torch"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("supervisor_timing.py needs a GPU")
    from envgs_amd.loss import EnvGSGeometryLoss
    dev = torch.device("cuda", 0)
    out, batch = make_inputs(dev)
    reg = EnvGSGeometryLoss(**OPTS)
    leaves = [out["norm_map"], out["surf_norm_map"]]

    def step(form):
        loss = reg(out, batch, 100)[0] if form == "fused" else torch_form(out, batch)
        return loss, torch.autograd.grad(loss, leaves)

    lf, gf = step("fused")
    lt, gt = step("torch")
    lines = ["geometry regularisers, %d x %d pixels, P = %d, envgs.yaml options, forward + backward" % (H, W, P),
             "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "loss fused %.9g  torch %.9g  (rel diff %.2e)" % (float(lf), float(lt), abs(float(lf) - float(lt)) / abs(float(lt)))]
    zero = (out["norm_map"].detach()[0] == 0).all(-1)
    for name, a, b in (("d norm_map", gf[0][0], gt[0][0]), ("d surf_norm_map", gf[1][0], gt[1][0])):
        for part, sel in (("norm_map != 0", ~zero), ("norm_map == 0", zero)):
            lines.append("%-16s %-14s max|fused - torch| / max|torch| %.2e" % (name, part, float((a[sel] - b[sel]).abs().max() / b[sel].abs().max())))
    if args.trace:
        for _ in range(10):
            step(args.trace)
        torch.cuda.synchronize()
        print("traced 1 + 10 iterations of the %s form (plus one of the other, for the comparison above)" % args.trace)
        return
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
        lines.append("%-5s  median %.4f ms  min %.4f  max %.4f  (%d repeats x %d iterations; per repeat: %s)" % (
            form, statistics.median(t), min(t), max(t), args.repeats, args.iters, " ".join("%.4f" % v for v in t)))
    lines.append("ratio torch / fused (medians): %.2f" % (statistics.median(times["torch"]) / statistics.median(times["fused"])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
