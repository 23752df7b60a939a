"""Generate tests/golden/supervisor_golden.npz by RUNNING the reference's own supervisor code -- EnvGSSupervisor.compute_loss
(easyvolcap/models/supervisors/envgs_supervisor.py:139-235, with math_utils.normalize, depth_utils.normalize_depth, loss_utils.mse / l1_reg) --
on the CPU in the authoring container, in float64, over float32-representable seeded inputs.

compute_loss is called UNBOUND on a types.SimpleNamespace that carries the option fields (the constructor wants a network and the global
config; compute_loss reads nothing but those fields).  The imports need the stand-ins tests/golden/make_sampler_golden.py installs, plus
torchvision.models / torchvision.models.vgg (the perceptual loss of loss_utils, never called here).

One set of inputs (by default H x W = 48 x 64 pixels, n = int(0.01 N) = 30, P = 1000 environment opacities), four option sets:
  a  configs/models/envgs.yaml       : norm_loss 0.01 + gs_norm_loss 0.04, both scaled by the normalised depth, windows open from iteration 0
  b  configs/models/envgs_synth.yaml : the same two terms scaled by acc_map, windows open from iteration 4000
  c  all five terms, both scales on both normal terms, 'l1' environment opacity
  d  the options of c at an iteration outside every window: loss 0, no gradient
(the 'sparse' opacity form is part of a and b, with a small weight, so that every branch compute_loss has is pinned).
Inputs contain a block of pixels with norm_map == 0, a block with batch.norm == 0.5 (a zero prior), a block with dpt_map == 0 and ties at both
depth percentiles.  Per case the file holds the five scalar_stats, the loss, the float64 autograd gradients, and -- for the pixels with
norm_map == 0, where two `x / (|x| + 1e-8)` and one cosine clamp amplify the gradient by 1e8 each -- the elementwise relative error of the
reference's own FLOAT32 run against its float64 run (the noise floor the GPU test scales its bound from).
Adaptation: loss_utils.mse casts its operands with .float(); during the float64 run Tensor.float casts to float64 instead, so that msk_loss is float64 too.
The fixture is DATA.  Re-run: python tests/golden/make_supervisor_golden.py
A second fixture at a size that is no multiple of the kernel's workgroup (11 x 29 = 319 pixels, n = 3, P = 257, cases a and c; the planted blocks
keep their share of the pixels):  python tests/golden/make_supervisor_golden.py 11 29 257 supervisor_golden_ragged.npz a,c"""
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

H, W, P = 48, 64, 1000

# every option field compute_loss reads, at the constructor's defaults
DEFAULTS = dict(
    norm_loss_weight=0.0, norm_loss_start_iter=7000, norm_loss_until_iter=None, use_acc_scale_norm_loss=False, use_dpt_scale_norm_loss=False,
    max_dpt_scale_percet=False,
    gs_norm_loss_weight=0.0, gs_norm_loss_start_iter=7000, gs_norm_loss_until_iter=None, use_acc_scale_gs_norm_loss=False,
    use_dpt_scale_gs_norm_loss=False, gs_dist_loss_weight=0.0, gs_dist_loss_start_iter=3000, gs_dist_loss_until_iter=None,
    env_opacity_loss_weight=0.0, env_opacity_loss_type="sparse", env_opacity_loss_start_iter=0,
    msk_loss_weight=0.0, msk_loss_start_iter=7000, msk_loss_until_iter=None)

CASES = {
    "a": (dict(gs_norm_loss_weight=0.04, gs_norm_loss_start_iter=0, use_dpt_scale_gs_norm_loss=True, norm_loss_weight=0.01, norm_loss_start_iter=0,
               use_dpt_scale_norm_loss=True, env_opacity_loss_weight=0.001), 10),
    "b": (dict(gs_norm_loss_weight=0.04, gs_norm_loss_start_iter=4000, use_acc_scale_gs_norm_loss=True, norm_loss_weight=0.01,
               norm_loss_start_iter=4000, use_acc_scale_norm_loss=True, env_opacity_loss_weight=0.001), 4000),
    "c": (dict(gs_norm_loss_weight=0.04, gs_norm_loss_start_iter=100, gs_norm_loss_until_iter=9000, use_acc_scale_gs_norm_loss=True,
               use_dpt_scale_gs_norm_loss=True, norm_loss_weight=0.01, norm_loss_start_iter=100, norm_loss_until_iter=9000,
               use_acc_scale_norm_loss=True, use_dpt_scale_norm_loss=True, gs_dist_loss_weight=100.0, gs_dist_loss_start_iter=100,
               gs_dist_loss_until_iter=9000, env_opacity_loss_weight=0.01, env_opacity_loss_type="l1", env_opacity_loss_start_iter=100,
               msk_loss_weight=0.1, msk_loss_start_iter=100, msk_loss_until_iter=9000), 5000),
}
CASES["d"] = (dict(CASES["c"][0], env_opacity_loss_start_iter=9500), 9000)          # until_iter is exclusive; the opacity term has a start only

GRAD_KEYS = ("norm_map", "surf_norm_map", "acc_map", "dist_map", "env_opacity")
STAT_KEYS = ("env_opacity_loss", "norm_loss", "gs_norm_loss", "msk_loss", "gs_dist_loss")


def make_inputs(H=H, W=W, P=P):
    """The planted blocks are stated for the default N = 3072 and keep their share of the pixels at any other N (at = the identity at 3072)."""
    N = H * W
    at = lambda i: i * N // 3072
    g = torch.Generator().manual_seed(20240607)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)
    norm_map = unit(rn(N, 3)) * (0.3 + 0.7 * r(N, 1))                    # rendered normals: alpha-weighted, so shorter than 1
    norm_map[at(0):at(200)] = 0.0                                       # background: no contributing surfel
    surf_norm_map = unit(rn(N, 3)) * (0.3 + 0.7 * r(N, 1))
    surf_norm_map[at(100):at(260)] = 0.0
    prior = unit(rn(N, 3)) * 0.5 + 0.5                                   # how normals are stored on disk
    prior[at(150):at(350)] = 0.5                                        # a zero prior
    prior[at(350):at(380)] = 0.5 + 0.1 * rn(at(380) - at(350), 3)       # short priors
    prior[at(380):at(420)] = 0.1 * r(at(420) - at(380), 3)              # |batch.norm| below the mask's 0.25
    acc = r(N, 1)
    acc[at(0):at(100)] = 0.0                                            # half of the background block; the other half keeps the acc-scaled terms alive there
    msk = (r(N, 1) > 0.3).float()
    msk[at(500):at(520)] = 0.5                                          # not > 0.5
    dpt = 1.0 + 5.0 * r(N, 1)
    dpt[at(300):at(320)] = 0.0                                          # 20 zeros: fewer than n, so the low percentile is a positive depth
    n = int(N * 0.01)
    order = torch.argsort(dpt[:, 0])
    dpt[order[n - 3:n + 3], 0] = dpt[order[n - 1], 0].clone()            # ties straddling the n-th smallest ...
    dpt[order[N - n - 3:N - n + 3], 0] = dpt[order[N - n], 0].clone()    # ... and the n-th largest
    dist = 0.1 * r(N, 1) ** 2
    env = r(P, 1)
    env[0:20] = 0.0005 * r(20, 1)                                        # below / above the clamp of the 'sparse' form
    env[20:40] = 1.0 - 0.0005 * r(20, 1)
    env[40:44] = torch.tensor([[0.0], [1.0], [0.001], [0.999]])
    q = unit(rn(4))
    w_, x_, y_, z_ = q.tolist()
    R = torch.tensor([[1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - w_ * z_), 2 * (x_ * z_ + w_ * y_)],
                      [2 * (x_ * y_ + w_ * z_), 1 - 2 * (x_ * x_ + z_ * z_), 2 * (y_ * z_ - w_ * x_)],
                      [2 * (x_ * z_ - w_ * y_), 2 * (y_ * z_ + w_ * x_), 1 - 2 * (x_ * x_ + y_ * y_)]], dtype=torch.float32)
    return dict(norm_map=norm_map[None], surf_norm_map=surf_norm_map[None], acc_map=acc[None], dpt_map=dpt[None], dist_map=dist[None],
                env_opacity=env, norm=prior[None], msk=msk[None], R=R[None])


def _install_mocks():
    import make_sampler_golden as msg
    stub = types.SimpleNamespace(_recording_raster_pkg=lambda name, C: MagicMock(), _recording_trace_pkg=lambda: MagicMock())
    msg._install_mocks(stub)
    for m in ("torchvision.models", "torchvision.models.vgg"):
        sys.modules[m] = MagicMock()


def run_reference(compute_loss, dotdict, inputs, opts, it, dtype):
    ns = types.SimpleNamespace(**dict(DEFAULTS, **opts))
    leaves = {k: inputs[k].to(dtype).clone().requires_grad_(True) for k in GRAD_KEYS}
    output = dotdict(leaves)
    output.dpt_map = inputs["dpt_map"].to(dtype).clone().requires_grad_(True)       # the reference detaches it: its gradient must stay None
    output.iter = it
    batch = dotdict(norm=inputs["norm"].to(dtype), msk=inputs["msk"].to(dtype), R=inputs["R"].to(dtype))
    stats = dotdict()
    keep = torch.Tensor.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self: self.to(torch.float64)       # loss_utils.mse casts to float32; the float64 run is the exact statement
    try:
        loss = compute_loss(ns, output, batch, torch.zeros((), dtype=dtype), stats, dotdict())
    finally:
        torch.Tensor.float = keep
    grads = {k: None for k in GRAD_KEYS}
    if loss.requires_grad:
        loss.backward()
        grads = {k: leaves[k].grad for k in GRAD_KEYS}
        assert output.dpt_map.grad is None
    return loss.detach(), {k: v.detach() for k, v in stats.items()}, grads


def main(H=H, W=W, P=P, name="supervisor_golden.npz", tags=tuple(CASES)):
    _install_mocks()
    sys.path.insert(0, "/root/reference")
    sys.argv = ["evc"]
    from easyvolcap.engine import cfg  # noqa: F401
    from easyvolcap.utils.base_utils import dotdict
    from easyvolcap.models.supervisors.envgs_supervisor import EnvGSSupervisor
    compute_loss = EnvGSSupervisor.compute_loss

    inputs = make_inputs(H, W, P)
    out = {"in_" + k: v.numpy() for k, v in inputs.items()}
    out["H"], out["W"], out["P"] = np.int64(H), np.int64(W), np.int64(P)
    zero = (inputs["norm_map"][0] == 0).all(dim=-1).numpy()
    for tag in tags:
        opts, it = CASES[tag]
        loss, stats, grads = run_reference(compute_loss, dotdict, inputs, opts, it, torch.float64)
        loss32, _, grads32 = run_reference(compute_loss, dotdict, inputs, opts, it, torch.float32)
        out["iter_" + tag] = np.int64(it)
        out["opts_" + tag] = np.array(repr(sorted(opts.items())))
        out["loss_" + tag] = loss.numpy()
        out["stats_" + tag] = np.array(sorted(stats))
        for k in STAT_KEYS:
            if k in stats:
                out["%s_%s" % (k, tag)] = stats[k].numpy()
        noise = 0.0
        for k in GRAD_KEYS:
            if grads[k] is None:
                continue
            g64 = grads[k].numpy()
            out["grad_%s_%s" % (k, tag)] = g64
            if k == "norm_map":
                g32 = grads32[k].double().numpy()
                a, b = g32[0][zero], g64[0][zero]
                nz = b != 0
                assert np.isfinite(a).all() and (a[~nz] == 0).all()
                noise = float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0
                rest = np.abs(g32[0][~zero] - g64[0][~zero]).max() / np.abs(g64[0][~zero]).max()
                print("case %s: d norm_map, float32 run vs float64 run: zero-normal pixels max elementwise rel %.3e (max |g| %.3e), rest max-norm rel %.3e (max |g| %.3e)"
                      % (tag, noise, np.abs(b).max() if b.size else 0.0, rest, np.abs(g64[0][~zero]).max()))
        out["f32_noise_zero_normal_" + tag] = np.float64(noise)
        print("case %s iter %d: loss %.12g (float32 run: %.9g)  stats %s  gradients %s" % (
            tag, it, float(loss), float(loss32), {k: float(v) for k, v in stats.items()}, [k for k in GRAD_KEYS if grads[k] is not None]))
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print("fixture bytes:", os.path.getsize(path))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], tuple(sys.argv[5].split(",")) if len(sys.argv) > 5 else tuple(CASES))
    else:
        main()
