"""The device-resident mode of envgs_amd.densify.SurfelSet (`device_schedule=True`; include/envgs_densify.h, second half).

  * `add_densification_stats` as one launch of envgs_densify_stats: bit-equal to the staged torch form where the arithmetic is a copy / add / max,
    the gradient norm within its rounding bound of a float64 norm, no host synchronisation;
  * `grow_and_prune` (clone + split + prune by opacity / gradient as one plan, one read-back, one rewrite) against the staged three stages run on
    the same GPU with an identically seeded generator: the same `log`, shapes, copied rows, Adam moments and statistics to the bit; the split
    children's `_xyz` / `_scaling` against a float64 evaluation of the same fp32 inputs and samples.
"""
import ctypes
import os
import warnings

import pytest
import torch

from envgs_amd import densify

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify_golden.pt")
PREFIX = "sampler.pcd."
NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_specular", "_roughness")
U = 2.0 ** -24                                     # unit roundoff of fp32
SYNTH_ARGS = dict(min_opacity=0.05, min_gradient=0.15, grad_threshold=0.1, size_threshold=0.03, split_screen_threshold=20.0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _synthetic(P, seed=11):
    """A `before` state in the golden file's layout: scales on both sides of the size threshold, denom 0..4 (0 / 0 and x / 0 averages included),
    weights >= 0, radii on both sides of the split-screen threshold, opacities on both sides of min_opacity."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    params = {"_xyz": ru(P, 3) * 2 - 1, "_features_dc": rn(P, 1, 3), "_features_rest": rn(P, 3, 3), "_scaling": torch.log(ru(P, 2) * 0.095 + 0.005),
              "_rotation": rn(P, 4), "_opacity": rn(P, 1) * 2, "_specular": rn(P, 1), "_roughness": rn(P, 1)}
    denom = torch.randint(0, 5, (P, 1), generator=g).float()
    ga = ru(P, 1) * 0.5 * denom
    ga[::97] = ru(P, 1)[::97] * (denom[::97] == 0)                    # a few x / 0 = inf averages
    stats = {"xyz_gradient_accum": ga, "denom": denom, "max_radii2D": ru(P) * 50, "xyz_weight_accum": ru(P, 1) * 3 * denom}
    return {"params": params, "stats": stats, "m": {k: rn(*v.shape) * 0.1 for k, v in params.items()}, "v": {k: ru(*v.shape) * 0.01 for k, v in params.items()}}


def _golden(name):
    sc = torch.load(GOLD, weights_only=True)[name]
    a = sc["args"]
    args = dict(min_opacity=a["min_opacity"], min_gradient=a["min_gradient"], grad_threshold=a["densify_grad_threshold"],
                size_threshold=a["densify_size_threshold"], split_screen_threshold=a.get("split_screen_threshold"))
    return sc, args


def _build(before, cfg, device_schedule, seed=1234, dev="cuda:0", names=NAMES, optimizer="state", row_ops=None):
    """optimizer: "state" (Adam with both moments on every parameter), "empty" (Adam that has not stepped yet: no state) or None (no optimizer)."""
    params = {k: torch.nn.Parameter(before["params"][k].to(dev).clone()) for k in names}
    opt = None
    if optimizer is not None:
        opt = torch.optim.Adam([{"params": [params[k]], "lr": 1e-3, "name": PREFIX + k} for k in names], lr=0.0, eps=1e-15)
    if optimizer == "state":
        for k in names:
            opt.state[params[k]] = {"step": torch.tensor(2.0), "exp_avg": before["m"][k].to(dev).clone(), "exp_avg_sq": before["v"][k].to(dev).clone()}
    gen = torch.Generator(device=dev).manual_seed(seed)
    s = densify.SurfelSet(params, opt, PREFIX, spatial_scale=cfg.get("spatial_scale", 1.0), max_gs=cfg.get("max_gs"), max_gs_threshold=cfg.get("max_gs_threshold", 1.0),
                          row_ops=row_ops, generator=gen, device_schedule=device_schedule)
    for k in s.STATS:
        s.stats[k] = before["stats"][k].to(dev).clone()
    return s, opt


def _state(s, opt, names=NAMES, optimizer="state"):
    out = {"params": {k: s.p[k].detach().clone() for k in names}, "m": {}, "v": {}, "stats": {k: v.clone() for k, v in s.stats.items()}}
    assert tuple(s.p) == tuple(names)
    if optimizer is None:
        assert opt is None and s.optimizer is None
        return out
    for g in opt.param_groups:
        k = g["name"][len(PREFIX):]
        assert g["params"][0] is s.p[k]                                    # the optimizer trains the surfel set's current parameters
        if optimizer == "state":
            st = opt.state[g["params"][0]]
            out["m"][k], out["v"][k] = st["exp_avg"], st["exp_avg_sq"]
    assert len(opt.state) == (len(names) if optimizer == "state" else 0)   # no stale entries of replaced parameters; an empty state stays empty
    return out


def _staged_three(s, a, N=2):
    s.densify_and_clone(a["grad_threshold"], a["size_threshold"])
    s.densify_and_split(a["grad_threshold"], a["size_threshold"], a["split_screen_threshold"], N)
    s.prune_min_opacity_and_gradients(a["min_opacity"], a["min_gradient"])


def _classes(before, cfg, a, dev="cuda:0", N=2, ratio=0.8):
    """The rule of the issue, written with torch on the state before the pass."""
    st = {k: v.to(dev) for k, v in before["stats"].items()}
    ga, dn, mr = st["xyz_gradient_accum"][:, 0], st["denom"][:, 0], st["max_radii2D"]
    scal = torch.exp(before["params"]["_scaling"].to(dev))
    opac = torch.sigmoid(before["params"]["_opacity"].to(dev))[:, 0]

    def avg(x):
        q = x / dn
        q[q.isnan()] = 0.0
        return q
    high = avg(ga) >= a["grad_threshold"]
    small = scal.max(dim=1).values <= a["size_threshold"] * cfg.get("spatial_scale", 1.0)
    clone = small & high
    big = ~small
    if a["split_screen_threshold"] is not None:
        big = big | (mr > a["split_screen_threshold"])
    split = high & big
    none = torch.zeros_like(high)
    occ = opac < a["min_opacity"] if a["min_opacity"] is not None else none
    r = 1.0 / (ratio * N)
    pr_1 = occ | ((avg(ga) <= a["min_gradient"]) & (dn != 0) if a["min_gradient"] is not None else none)
    pr_s = occ | ((avg(ga * r) <= a["min_gradient"]) & (dn != 0) if a["min_gradient"] is not None else none)
    return dict(clone=clone, split=split, pr_1=pr_1, pr_s=pr_s, scal=scal)


# ---- statistics --------------------------------------------------------------------------------------------------------------------------
def _stat_set(P, device_schedule, dev="cuda:0"):
    raw = {"_xyz": torch.zeros(P, 3, device=dev)}
    return densify.SurfelSet(raw, None, row_ops=densify.torch_rows, device_schedule=device_schedule)


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [2, 3])
@pytest.mark.parametrize("P", [1, 255, 257, 70001])
def test_statistics_launch_equals_the_torch_form(P, cols):
    dev = "cuda:0"
    g = torch.Generator().manual_seed(P * 10 + cols)
    grad = (torch.randn(P, cols, generator=g) * torch.exp(torch.randn(P, 1, generator=g) * 3)).to(dev)
    grad2 = torch.randn(P, cols, generator=g).to(dev)
    weight = torch.rand(P, 1, generator=g).to(dev)
    radii = torch.randint(0, 60, (P,), generator=g, dtype=torch.int32).to(dev)
    filters = {"none": torch.zeros(P, dtype=torch.bool), "all": torch.ones(P, dtype=torch.bool), "random": torch.rand(P, generator=g) > 0.4}
    other = (torch.rand(P, generator=g) > 0.5).to(dev)
    n64 = grad.double().norm(dim=-1)
    n64b = grad2.double().norm(dim=-1)
    for fname, f in filters.items():
        f = f.to(dev)
        for w in (None, weight):
            for r in (None, radii):
                a, b = _stat_set(P, True), _stat_set(P, False)
                a.add_densification_stats(grad, f, w, r)
                b.add_densification_stats(grad, f, w, r)
                what = (fname, w is not None, r is not None)
                for k in ("denom", "xyz_weight_accum", "max_radii2D"):
                    assert torch.equal(a.stats[k], b.stats[k]), (k, what)
                ga = a.stats["xyz_gradient_accum"][:, 0].double()
                assert bool(((ga - n64 * f).abs() <= 3 * U * n64).all()), what              # gamma_3 on the sum of squares, halved by the root, + the root
                assert bool((ga[~f] == 0).all())
                # a second call accumulates, and leaves the rows outside ITS filter bit-untouched
                snap = {k: v.clone() for k, v in a.stats.items()}
                a.add_densification_stats(grad2, other, w, r // 2 if r is not None else None)
                b.add_densification_stats(grad2, other, w, r // 2 if r is not None else None)
                for k in a.stats:
                    assert torch.equal(a.stats[k][~other], snap[k][~other]), (k, what)
                for k in ("denom", "xyz_weight_accum", "max_radii2D"):
                    assert torch.equal(a.stats[k], b.stats[k]), (k, what)
                ga2 = a.stats["xyz_gradient_accum"][:, 0].double()
                exact = ga + n64b * other                                                    # fl(ga + n') with |n' - n| <= 3u n: one more rounding of the sum
                bound = (4 * U * n64b + U * ga) * (1 + 2.0 ** -10)
                assert bool(((ga2 - exact).abs() <= bound).all()), what
                assert bool((a.stats["denom"][:, 0] == f.float() + other.float()).all())


@pytest.mark.gpu
def test_statistics_launch_has_no_host_sync():
    dev, P = "cuda:0", 257
    g = torch.Generator().manual_seed(3)
    grad = torch.randn(P, 3, generator=g).to(dev); f = (torch.rand(P, generator=g) > 0.4).to(dev)
    w = torch.rand(P, 1, generator=g).to(dev); r = torch.randint(0, 60, (P,), generator=g, dtype=torch.int32).to(dev)
    a, b = _stat_set(P, True), _stat_set(P, False)
    a.add_densification_stats(grad, f, w, r)                              # (library loaded, kernels resident)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a.add_densification_stats(grad, f, w, r)
        with pytest.raises(RuntimeError):
            b.add_densification_stats(grad, f, w, r)                      # the staged form: boolean-mask indexing = nonzero + read-back
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool((a.stats["denom"][:, 0] == 2 * f.float()).all())


# ---- grow and prune ----------------------------------------------------------------------------------------------------------------------
def _check_grow(before, cfg, a, synthetic=False, N=2, ratio=0.8, seed=77, names=NAMES, optimizer="state", device_set=None, gen_state=None):
    """device_set: a (SurfelSet, optimizer) in device mode that holds `before` already, e.g. the result of an earlier pass; gen_state: the state
    of its generator, which the staged twin and the float64 children then start from instead of `seed`."""
    dev = "cuda:0"
    c = _classes(before, cfg, a, dev, N, ratio)
    clone, split, pr_1, pr_s = c["clone"], c["split"], c["pr_1"], c["pr_s"]
    if synthetic:                                                          # no branch is vacuous
        assert int((clone & split).sum()) > 0
        for seg in (~split & pr_1, clone & ~split & pr_1, split & pr_s, clone & split & pr_s):
            assert int(seg.sum()) > 0
    dv, do = device_set if device_set is not None else _build(before, cfg, True, seed, names=names, optimizer=optimizer)
    sg, so = _build(before, cfg, False, seed, names=names, optimizer=optimizer)
    if gen_state is not None:
        sg.generator.set_state(gen_state.clone())
    dv.grow_and_prune(a["min_opacity"], a["min_gradient"], a["grad_threshold"], a["size_threshold"], a["split_screen_threshold"], N, ratio)
    _staged_three(sg, a, N)
    assert dv.log == sg.log
    D, S = _state(dv, do, names, optimizer), _state(sg, so, names, optimizer)
    nA, nB = int((~split & ~pr_1).sum()), int((clone & ~split & ~pr_1).sum())
    keepD, keepE = split & ~pr_s, clone & split & ~pr_s
    nD, nE, nS = int(keepD.sum()), int(keepE.sum()), int(split.sum()) + int((clone & split).sum())
    total = nA + nB + N * (nD + nE)
    assert dict(dv.log) == {"clone": int(clone.sum()), "split": nS, "prune_occ_grad": clone.shape[0] + int(clone.sum()) + (N - 1) * nS - total}
    for k in names:
        assert D["params"][k].shape == S["params"][k].shape and D["params"][k].shape[0] == total, k
        if D["m"]:
            assert torch.equal(D["m"][k], S["m"][k]) and torch.equal(D["v"][k], S["v"][k]), k
        if k in ("_xyz", "_scaling"):
            assert torch.equal(D["params"][k][:nA + nB], S["params"][k][:nA + nB]), k
        else:
            assert torch.equal(D["params"][k], S["params"][k]), k
    for k in dv.STATS:
        assert D["stats"][k].shape == S["stats"][k].shape and torch.equal(D["stats"][k], S["stats"][k]), k
    if nS == 0 or nD + nE == 0:                                            # no split, or no child of one survives: no child to evaluate
        return dv, sg
    # the children, from the same fp32 inputs and the same samples in float64
    sel = torch.cat((torch.nonzero(split)[:, 0], torch.nonzero(clone & split)[:, 0]))            # S, in the staged order
    kept = torch.cat((keepD[split], keepE[clone & split]))
    stds = torch.cat((c["scal"][sel], torch.zeros(nS, 1, device=dev)), dim=-1).repeat(N, 1)
    gen = torch.Generator(device=dev).manual_seed(seed)
    if gen_state is not None:
        gen.set_state(gen_state.clone())
    samples = torch.normal(torch.zeros_like(stds), stds, generator=gen)
    par = sel.repeat(N)[kept.repeat(N)]
    smp = samples[kept.repeat(N)].double()
    q = before["params"]["_rotation"].to(dev)[par].double()
    q = q / q.norm(dim=-1, keepdim=True)
    rr, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - rr * z), 2 * (x * z + rr * y), 2 * (x * y + rr * z), 1 - 2 * (x * x + z * z), 2 * (y * z - rr * x),
                     2 * (x * z - rr * y), 2 * (y * z + rr * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    x0 = before["params"]["_xyz"].to(dev)[par].double()
    want = torch.bmm(R, smp.unsqueeze(-1)).squeeze(-1) + x0
    got = D["params"]["_xyz"][nA + nB:].double()
    bound = 16 * U * (x0.abs() + smp[:, 0:1].abs() + smp[:, 1:2].abs())
    err = (got - want).abs()
    print("children _xyz: max err / bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    want = torch.log(c["scal"][par].double() / (ratio * N))
    err = (D["params"]["_scaling"][nA + nB:].double() - want).abs()
    bound = 2.0 ** -23 * (1 + want.abs())
    print("children _scaling: max err / bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    return dv, sg


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["all_branches", "clone_split_prune"])
def test_grow_and_prune_equals_the_staged_stages_on_the_golden_scenes(name):
    sc, args = _golden(name)
    _check_grow(sc["before"], sc["config"], args)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [777, 70001])
def test_grow_and_prune_equals_the_staged_stages_on_a_synthetic_set(P):
    """Small surfels that are cloned and then split (split_screen_threshold), pruned rows in every segment; 70 001: the multi-block scan."""
    _check_grow(_synthetic(P), {}, SYNTH_ARGS, synthetic=True)


@pytest.mark.gpu
def test_grow_and_prune_with_three_children():
    _check_grow(_synthetic(777, seed=5), {"spatial_scale": 1.5}, dict(SYNTH_ARGS, size_threshold=0.02), N=3)


@pytest.mark.gpu
def test_nothing_selected_installs_and_draws_nothing():
    sc, args = _golden("nothing_selected")
    s, opt = _build(sc["before"], sc["config"], True)
    before = dict(s.p)
    stats = dict(s.stats)
    state = s.generator.get_state().clone()
    s.grow_and_prune(**args)
    assert s.log == [("clone", 0), ("split", 0), ("prune_occ_grad", 0)]
    assert all(s.p[k] is before[k] for k in NAMES) and all(s.stats[k] is stats[k] for k in s.STATS)
    assert torch.equal(s.generator.get_state(), state)


@pytest.mark.gpu
def test_densify_and_prune_end_to_end_clone_split_prune():
    sc, args = _golden("clone_split_prune")
    res = []
    for mode in (True, False):
        s, opt = _build(sc["before"], sc["config"], mode)
        s.densify_and_prune(**sc["args"])
        res.append((_state(s, opt), list(s.log)))
    (D, ld), (S, ls) = res
    assert ld == ls and D["params"]["_xyz"].shape[0] == sc["after"]["params"]["_xyz"].shape[0] != sc["before"]["params"]["_xyz"].shape[0]
    c = _classes(sc["before"], sc["config"], args)
    n_copied = int((~c["split"] & ~c["pr_1"]).sum()) + int((c["clone"] & ~c["split"] & ~c["pr_1"]).sum())
    for k in NAMES:
        assert D["params"][k].shape == S["params"][k].shape
        assert torch.equal(D["m"][k], S["m"][k]) and torch.equal(D["v"][k], S["v"][k]), k
        rows = n_copied if k in ("_xyz", "_scaling") else D["params"][k].shape[0]
        assert torch.equal(D["params"][k][:rows], S["params"][k][:rows]), k
    for k in D["stats"]:
        assert torch.equal(D["stats"][k], S["stats"][k])                  # reset, at the new size


@pytest.mark.gpu
def test_densify_and_prune_end_to_end_all_branches():
    sc, args = _golden("all_branches")
    # the later stages compare the children's scales with max_scene_threshold * spatial_scale: the two modes' children differ by rounding, so the
    # comparison is only required to agree when no child sits on the threshold
    s, opt = _build(sc["before"], sc["config"], False)
    _staged_three(s, args)
    c = _classes(sc["before"], sc["config"], args)
    n_copied = int((~c["split"] & ~c["pr_1"]).sum()) + int((c["clone"] & ~c["split"] & ~c["pr_1"]).sum())
    thr = sc["args"]["max_scene_threshold"] * sc["config"]["spatial_scale"]
    child = s.scaling()[n_copied:]
    assert child.shape[0] > 0 and bool(((child - thr).abs() > 1e-5 * thr).all())
    res = []
    for mode in (True, False):
        s, opt = _build(sc["before"], sc["config"], mode)
        s.densify_and_prune(**sc["args"])
        res.append((s.number, list(s.log), _state(s, opt)))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    ev = dict(res[0][1])
    assert ev["clone"] > 0 and ev["split"] > 0 and ev["prune_occ_grad"] > 0 and ev["prune_large"] > 0 and ev["split_large"] > 0 and ev["prune_visibility"] > 0


@pytest.mark.gpu
def test_split_draws_follow_the_generator_in_device_mode():
    sc, args = _golden("clone_split_prune")
    outs = []
    for junk in (0, 5):
        s, opt = _build(sc["before"], sc["config"], True, seed=4321)
        torch.manual_seed(junk); torch.cuda.manual_seed(junk); torch.rand(junk + 1, device="cuda:0")       # the global generators differ between the two "ranks"
        s.densify_and_prune(**sc["args"])
        outs.append(s.p["_xyz"].detach().clone())
    assert outs[0].shape == outs[1].shape and torch.equal(outs[0], outs[1])


@pytest.mark.gpu
def test_split_offsets_are_the_staged_torch_normal_draw():
    """`normal_offsets` leaves out torch.normal's host check of the standard deviations, nothing else: the same values, the same generator advance."""
    dev = "cuda:0"
    for n in (1, 37, 70001):
        stds = torch.cat((torch.rand(n, 2, generator=torch.Generator().manual_seed(n)) * 0.1, torch.zeros(n, 1)), dim=-1).to(dev)
        ga, gb = torch.Generator(device=dev).manual_seed(99), torch.Generator(device=dev).manual_seed(99)
        a = densify.normal_offsets(stds, ga)
        b = torch.normal(torch.zeros_like(stds), stds, generator=gb)
        assert torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(ga.get_state(), gb.get_state())
        assert torch.equal(densify.normal_offsets(stds, ga), torch.normal(torch.zeros_like(stds), stds, generator=gb))      # and the next draw


def _sync_warnings(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return [w for w in rec if "called a synchronizing" in str(w.message)]        # (not the notice set_sync_debug_mode itself prints)


@pytest.mark.gpu
def test_grow_and_prune_synchronises_once():
    before = _synthetic(777)
    warm, _ = _build(before, {}, True)
    warm.grow_and_prune(**SYNTH_ARGS)                                     # (library loaded, kernels resident)
    dv, _ = _build(before, {}, True)
    sg, _ = _build(before, {}, False)
    n_dev = len(_sync_warnings(lambda: dv.grow_and_prune(**SYNTH_ARGS)))
    n_staged = len(_sync_warnings(lambda: _staged_three(sg, SYNTH_ARGS)))
    print("sync warnings: one-pass %d, staged %d" % (n_dev, n_staged))
    assert n_dev == 1
    assert n_staged >= 8
    assert dv.log == sg.log


# ---- ABI, CPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from envgs_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_new_entries_reject_bad_arguments_before_any_gpu_work(lib):
    from envgs_amd import _lib
    buf = ctypes.create_string_buffer(256)
    x = ctypes.c_void_p(ctypes.addressof(buf))                             # never dereferenced: every call below returns before any GPU work
    ok = [x] * 8
    assert lib.envgs_densify_stats(-1, 3, *ok, None) == -1
    for cols in (0, 1, 4):
        assert lib.envgs_densify_stats(4, cols, *ok, None) == -1
    for missing in (0, 1, 4, 5):                                           # grad, filter, xyz_gradient_accum, denom
        args = list(ok); args[missing] = None
        assert lib.envgs_densify_stats(4, 3, *args, None) == -1
    args = list(ok); args[6] = None                                        # radii given, max_radii2D missing
    assert lib.envgs_densify_stats(4, 3, *args, None) == -1
    args = list(ok); args[7] = None                                        # weight given, xyz_weight_accum missing
    assert lib.envgs_densify_stats(4, 3, *args, None) == -1

    def plan(**kw):
        d = dict(P=4, N=2, flags=7, grad_threshold=0.1, size_limit=0.1, split_screen_threshold=1.0, min_opacity=0.1, min_gradient=0.1, r=0.625,
                 ga=x.value, dn=x.value, mr=x.value, wa=x.value, scal=x.value, opac=x.value, cls=x.value, scan=x.value, counters=x.value, temp=x.value,
                 temp_bytes=1 << 20)
        d.update(kw)
        return _lib.DensifyPlanArgs(*[d[n] for n, _ in _lib.DensifyPlanArgs._fields_])
    assert lib.envgs_densify_plan(None, None) == -1
    for bad in (dict(P=-1), dict(N=0), dict(N=17), dict(P=1 << 29), dict(counters=None), dict(ga=None), dict(dn=None), dict(mr=None), dict(wa=None), dict(scal=None),
                dict(opac=None), dict(cls=None), dict(scan=None), dict(temp=None)):
        assert lib.envgs_densify_plan(plan(**bad), None) == -1, bad
    assert lib.envgs_densify_plan(plan(temp_bytes=0), None) == -2
    assert lib.envgs_densify_split_stds(-1, 2, x, x, x, x, x, 4, None) == -1
    assert lib.envgs_densify_split_stds(4, 0, x, x, x, x, x, 4, None) == -1
    assert lib.envgs_densify_split_stds(4, 2, x, x, x, x, x, -1, None) == -1
    for missing in range(5):
        args = [x] * 5; args[missing] = None
        assert lib.envgs_densify_split_stds(4, 2, *args, 4, None) == -1

    one = (_lib.GrowTensor * 1)(_lib.GrowTensor(x.value, x.value, 12, 2, 0))

    def rewrite(tensors=one, **kw):
        d = dict(P=4, out_rows=8, n_samples=4, N=2, count=1, ratio_n=1.6, r=0.625, reserved0=0, cls=x.value, scan=x.value, counters=x.value, scal=x.value,
                 rotation=x.value, samples=x.value, tensors=tensors)
        d.update(kw)
        return _lib.DensifyRewriteArgs(*[d[n] for n, _ in _lib.DensifyRewriteArgs._fields_])
    assert lib.envgs_densify_rewrite(None, None) == -1
    for bad in (dict(P=-1), dict(N=0), dict(count=-1), dict(count=33), dict(tensors=None), dict(ratio_n=0.0), dict(out_rows=-1), dict(n_samples=-1), dict(cls=None),
                dict(scan=None), dict(counters=None), dict(rotation=None), dict(samples=None)):
        assert lib.envgs_densify_rewrite(rewrite(**bad), None) == -1, bad
    for t in (_lib.GrowTensor(None, x.value, 12, 0, 0), _lib.GrowTensor(x.value, None, 12, 0, 0), _lib.GrowTensor(x.value, x.value, 6, 0, 0),
              _lib.GrowTensor(x.value, x.value, 12, 8, 0), _lib.GrowTensor(x.value, x.value, 12, -1, 0), _lib.GrowTensor(x.value, x.value, 16, 2, 0),
              _lib.GrowTensor(x.value, x.value, 12, 3, 0), _lib.GrowTensor(x.value, x.value, 8, 4, 0)):
        assert lib.envgs_densify_rewrite(rewrite(tensors=(_lib.GrowTensor * 1)(t)), None) == -1


def test_device_schedule_refuses_cpu_tensors():
    raw = {k: v for k, v in torch.load(GOLD, weights_only=True)["resets"]["before"]["params"].items()}
    with pytest.raises(RuntimeError, match="no CPU path"):
        densify.SurfelSet(raw, None, device_schedule=True)
    s = densify.SurfelSet(raw, None, row_ops=densify.torch_rows)          # the default mode has no one-pass form
    with pytest.raises(RuntimeError, match="device_schedule"):
        s.grow_and_prune(0.05, None, 0.5, 0.03)
