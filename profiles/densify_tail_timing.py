"""What the pruning tail of a densification costs, staged (`torch.quantile` / `torch.topk` + boolean masks over the HIP compaction kernels: the default
and `device_schedule=True`) against the device tail (`SurfelSet(device_schedule="all")`: radix select + mask + one compaction, include/envgs_densify.h),
at the bench scene's two set sizes, P = 300 000 and 163 840, 8 parameters with both Adam moments.

  visibility   `prune_visibility` with n_prune = 5 % of P
  oversize     `prune_max_scene_and_screen` with the scene, screen and weight thresholds given (quantile 0.3)

Every call runs on a freshly built set (the call consumes it); the set is built outside the timed window.  Per call: DEVICE time between two
events on the stream (for the staged form this includes the gaps in which the queue is empty while the host reads a count back) and HOST WALL
time from before the call to a synchronise after it.  The forms alternate inside every round and the first round is dropped.

    python profiles/densify_tail_timing.py [--repeats 20] [--out FILE]
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

SIZES = (300000, 163840)
NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_specular", "_roughness")
OVERSIZE = dict(max_screen_threshold=45.0, min_weight_threshold=0.3)      # (the scene threshold is set from the scene's scales)


def scene(P, dev):
    from envgs_amd import synth
    g = synth.base_gaussians(P, seed=0)
    raw = {"_xyz": g["means3D"], "_features_dc": g["shs"][:, :1], "_features_rest": g["shs"][:, 1:], "_scaling": torch.log(g["scales"]), "_rotation": g["rotations"] * 1.3,
           "_opacity": torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4)), "_specular": torch.logit(g["specular"]), "_roughness": torch.logit(g["roughness"])}
    raw = {k: v.to(dev).contiguous() for k, v in raw.items()}
    gen = torch.Generator().manual_seed(5)
    denom = torch.randint(0, 6, (P, 1), generator=gen).float()
    stats = {"xyz_gradient_accum": torch.rand(P, 1, generator=gen) * denom, "denom": denom, "max_radii2D": torch.rand(P, generator=gen) * 50,
             "xyz_weight_accum": torch.rand(P, 1, generator=gen) * 3 * denom}
    return raw, {k: v.to(dev) for k, v in stats.items()}


def build(raw, stats, mode, max_gs, dev):
    from envgs_amd import densify
    prm = {k: torch.nn.Parameter(raw[k].clone()) for k in NAMES}
    opt = torch.optim.Adam([{"params": [prm[k]], "lr": 1e-3, "name": k} for k in NAMES], lr=0.0, eps=1e-15)
    for k in NAMES:
        opt.state[prm[k]] = {"step": torch.tensor(2.0), "exp_avg": torch.randn_like(prm[k]) * 0.1, "exp_avg_sq": torch.rand_like(prm[k]) * 0.01}
    s = densify.SurfelSet(prm, opt, "", max_gs=max_gs, generator=torch.Generator(device=dev).manual_seed(9), device_schedule=mode)
    for k in s.STATS:
        s.stats[k] = stats[k].clone()
    return s


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def measure(P, dev, repeats, lines):
    raw, stats = scene(P, dev)
    n_prune = P // 20
    scene_thr = float(torch.exp(raw["_scaling"]).max(dim=1).values.quantile(0.9))       # a tenth of the surfels are oversized in the scene
    stages = {"visibility": lambda s: s.prune_visibility(),
              "oversize": lambda s: s.prune_max_scene_and_screen(scene_thr, OVERSIZE["max_screen_threshold"], OVERSIZE["min_weight_threshold"])}
    for stage, call in stages.items():
        res = {"staged": [], "device": []}
        logs = {}
        for r in range(repeats + 1):                                      # (the first round warms both forms up and is dropped)
            for form in ("staged", "device"):
                s = build(raw, stats, "all" if form == "device" else False, P - n_prune, dev)
                t = timed(lambda: call(s))
                if r:
                    res[form].append(t)
                logs[form] = (list(s.log), s.number)
                del s
        lines.append("%-10s P = %d: events %s -> %d surfels; the two forms agree on them: %s" % (stage, P, logs["staged"][0], logs["staged"][1], logs["staged"] == logs["device"]))
        for form in ("staged", "device"):
            d, w = [v[0] for v in res[form]], [v[1] for v in res[form]]
            lines.append("%-10s P = %d  %-6s  device median %.3f ms (min %.3f max %.3f)  host wall median %.3f ms (min %.3f max %.3f)  %d calls" % (
                stage, P, form, statistics.median(d), min(d), max(d), statistics.median(w), min(w), max(w), repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densify_tail_timing.py needs a GPU")
    dev = torch.device("cuda", 0)
    lines = ["pruning tail of a densification, staged against the device tail; n_prune = 5 %% of P, thresholds %s" % (OVERSIZE,),
             "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]
    for P in SIZES:
        measure(P, dev, args.repeats, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
