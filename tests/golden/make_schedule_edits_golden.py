"""Generate tests/golden/schedule_edits_golden.pt by RUNNING the reference's GaussianModel schedule edits on CPU (authoring container only;
/root/reference does not exist on the GPU box): `enlarge_opacity`, `enlarge_scaling` (normal propagation) and `distort_color` (colour
sabotage).  One scenario per edit, each on the `model()` recipe of make_densify_golden.py at P = 60: the inputs (raw parameters, Adam moments
after two optimizer steps, the arguments, the RNG seed set right before `distort_color`) and what the reference left behind (parameters,
moments, whether the replaced parameter carries a `.grad`).  Data only.  Re-run:  python tests/golden/make_schedule_edits_golden.py"""
import json
import os
import sys
from unittest.mock import MagicMock

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_specular", "_roughness")
PREFIX = "sampler.pcd."


def snapshot(m, opt):
    out = {"params": {k: getattr(m, k).detach().clone() for k in NAMES}, "m": {}, "v": {}}
    for g in opt.param_groups:
        st = opt.state[g["params"][0]]
        out["m"][g["name"][len(PREFIX):]] = st["exp_avg"].clone()
        out["v"][g["name"][len(PREFIX):]] = st["exp_avg_sq"].clone()
    return out


def main():
    for mod in ("pdbr", "pdbr.utils", "ruamel", "ruamel.yaml", "plyfile", "diff_surfel_tracing"):
        sys.modules[mod] = MagicMock()
    sys.modules["ujson"] = json
    sys.path.insert(0, "/root/reference")
    from easyvolcap.utils import gaussian2d_utils as g2d

    def model(P, seed):
        torch.manual_seed(seed)
        m = g2d.GaussianModel(xyz=torch.rand(P, 3) * 2 - 1, colors=torch.rand(P, 3), init_occ=0.1, init_scale=torch.log(torch.rand(P, 2) * 0.095 + 0.005), sh_degree=1,
                              init_sh_degree=1, render_reflection=True, xyz_lr_scheduler=None, max_gs=10 ** 6, max_gs_threshold=1.0, spatial_scale=1.0)
        with torch.no_grad():
            for k in NAMES:
                if k not in ("_xyz", "_scaling"):
                    getattr(m, k).add_(torch.randn_like(getattr(m, k)))
        opt = torch.optim.Adam([{"params": [getattr(m, k)], "lr": 1e-3, "name": PREFIX + k} for k in NAMES], lr=0.0, eps=1e-15)
        for _ in range(2):
            for k in NAMES:
                getattr(m, k).grad = torch.randn_like(getattr(m, k))
            opt.step()
        return m, opt

    # thresholds inside the spread of sigmoid(_specular) of the recipe, so that either branch of every mask holds rows
    scenarios = {
        "enlarge_opacity": dict(seed=11, target="_opacity", call=lambda m, o: m.enlarge_opacity(0.1, o, PREFIX), args=dict(value=0.1)),
        "enlarge_scaling": dict(seed=12, target="_scaling", call=lambda m, o: m.enlarge_scaling(1.5, 0.001, o, PREFIX), args=dict(ratio=1.5, threshold=0.001)),
        "distort_color": dict(seed=13, target="_features_dc", rng=321, call=lambda m, o: m.distort_color(0.4, 0.001, o, PREFIX), args=dict(range=0.4, threshold=0.001)),
    }
    out = {}
    for name, sc in scenarios.items():
        m, opt = model(60, sc["seed"])
        before = snapshot(m, opt)
        if "rng" in sc:
            torch.manual_seed(sc["rng"])
        sc["call"](m, opt)
        after = snapshot(m, opt)
        changed = int((after["params"][sc["target"]] != before["params"][sc["target"]]).flatten(1).any(-1).sum())
        out[name] = {"args": sc["args"], "target": sc["target"], "rng": sc.get("rng"), "before": before, "after": after,
                     "grad_is_none": getattr(m, sc["target"]).grad is None, "rows_changed": changed}
        print(name, "rows changed:", changed, "of 60; .grad is None:", out[name]["grad_is_none"])
    torch.save(out, os.path.join(HERE, "schedule_edits_golden.pt"))


if __name__ == "__main__":
    main()
