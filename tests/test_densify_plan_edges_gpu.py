"""The one-pass densification plan (`SurfelSet.grow_and_prune`; csrc/densify_device.hip: grow_plan, grow_counters, grow_stds, grow_rewrite) where it
can be wrong without a parity test moving: rows exactly on its six thresholds, empty segments of its scan, tiny sets and workgroup borders, other
parameter layouts and optimizer forms, 1 and 16 children, flags off and thresholds of 0.0, weights of either sign, and a second pass.

Two checks per case (the inputs and their CPU proofs: tests/densify_plan_cases.py, tests/test_densify_plan_cases_cpu.py):
  * plan level: `envgs_densify_plan` through the C ABI against a NumPy float32 restatement of include/envgs_densify.h -- class bits, scan and
    counters equal, the weight maxima through their decoded values, canaries behind every output, scratch handed over full of junk;
  * end to end: `_check_grow` of tests/test_densify_device.py, i.e. the staged three stages on an identically built set and generator: rows,
    moments, statistics and `log` equal, the split children within that file's two derived bounds.  Nothing here has a tolerance of its own.
Last, `prune_max_scene_and_screen` (device_schedule="all") with rows on its two thresholds.
"""
import numpy as np
import pytest
import torch

from envgs_amd import _lib, densify
from tests import densify_plan_cases as pc
from tests.test_densify_device import _build, _check_grow, _state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CANARY = 64                                                            # bytes / words behind every output


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _assert_bit_equal(A, B, what=""):
    """Two `_state`s, every tensor through its int32 view: -0 is not +0, and a NaN equals itself."""
    for part in ("params", "m", "v", "stats"):
        assert A[part].keys() == B[part].keys(), (what, part)
        for k in A[part]:
            assert A[part][k].shape == B[part][k].shape and torch.equal(_bits(A[part][k]), _bits(B[part][k])), (what, part, k)


# ---- plan level --------------------------------------------------------------------------------------------------------------------------------
def _check_plan(lib, ga, dn, mr, wa, scal, opac, thr, N, ratio=0.8):
    """envgs_densify_plan on these arrays (NumPy float32; scal / opac activated) against pc.plan_reference."""
    ref = pc.plan_reference(ga, dn, mr, wa, scal, opac, thr, N, ratio)
    P = int(np.asarray(ga).size)
    up = lambda x, shape: torch.from_numpy(np.ascontiguousarray(np.asarray(x, F).reshape(shape))).to(DEV)
    d_ga, d_dn, d_mr, d_wa, d_opac = (up(x, (P,)) for x in (ga, dn, mr, wa, opac))
    d_scal = up(scal, (P, 2))
    tb = lib.envgs_densify_plan_temp_bytes(P)
    assert tb > 0
    cls = torch.full((P + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    scan = torch.full((6 * P + CANARY,), 0x5EADBEEF, dtype=torch.int32, device=DEV)
    counters = torch.full((16 + CANARY,), 0x5EADBEEF, dtype=torch.int32, device=DEV)
    temp = torch.full((tb + CANARY,), 0xC3, dtype=torch.uint8, device=DEV)                # junk: the call clears what it uses
    opt = lambda k: float(thr[k]) if thr.get(k) is not None else 0.0
    args = _lib.DensifyPlanArgs(P, N, pc.plan_flags(thr), float(thr["grad_threshold"]), float(thr["size_limit"]), opt("split_screen_threshold"), opt("min_opacity"),
                                opt("min_gradient"), pc.split_r(N, ratio), d_ga.data_ptr(), d_dn.data_ptr(), d_mr.data_ptr(), d_wa.data_ptr(), d_scal.data_ptr(),
                                d_opac.data_ptr(), cls.data_ptr(), scan.data_ptr(), counters.data_ptr(), temp.data_ptr(), tb)
    _lib.check(lib.envgs_densify_plan(args, densify._stream(torch.device(DEV))), "envgs_densify_plan")
    torch.cuda.synchronize()
    got_cls, got_scan = cls.cpu().numpy(), scan.cpu().numpy().view(np.uint32)
    got_counters, got_temp = counters.cpu().numpy().view(np.uint32), temp.cpu().numpy()
    assert np.array_equal(got_cls[:P], ref["cls"]), np.flatnonzero(got_cls[:P] != ref["cls"])[:8]
    assert np.array_equal(got_scan[:6 * P], ref["scan"]), np.flatnonzero(got_scan[:6 * P] != ref["scan"])[:8]
    assert got_counters[:7].tolist() == ref["counters"]
    assert bool((got_cls[P:] == 0xA5).all()) and bool((got_scan[6 * P:] == 0x5EADBEEF).all()) and bool((got_counters[16:] == 0x5EADBEEF).all())
    assert bool((got_temp[tb:] == 0xC3).all())
    # the weight maxima, through what the rewrite makes of them
    assert pc.float_of_key(got_counters[7]) == ref["w_all"]
    if ref["counters"][6]:
        assert pc.float_of_key(got_counters[8]) == ref["w_clone_max"]
        assert pc.float_of_key(~int(got_counters[9])) == ref["w_clone_min"]
    return ref


def _check_plan_of_state(lib, before, cfg, args, N):
    scal, opac = pc.activated(before, DEV)
    st = {k: v.numpy() for k, v in before["stats"].items()}
    thr = dict(args, size_limit=float(F(args["size_threshold"] * cfg.get("spatial_scale", 1.0))))
    return _check_plan(lib, st["xyz_gradient_accum"], st["denom"], st["max_radii2D"], st["xyz_weight_accum"], scal, opac, thr, N)


@pytest.mark.parametrize("off", [(), ("min_opacity",), ("min_gradient",), ("split_screen_threshold",), ("min_opacity", "min_gradient", "split_screen_threshold")])
@pytest.mark.parametrize("N", [1, 2, 3, 16])
def test_plan_on_non_finite_statistics(lib, N, off):
    """NaN / d -> 0, +inf, x / 0 = +inf ("high"), 0 / 0 -> 0, -inf: rows the end-to-end comparison cannot carry conveniently."""
    ga, dn, mr, wa, scal, opac = pc.special_rows()
    thr = dict(grad_threshold=0.1, size_limit=0.03, split_screen_threshold=20.0, min_opacity=0.05, min_gradient=0.15)
    thr.update({k: None for k in off})
    ref = _check_plan(lib, ga, dn, mr, wa, scal, opac, thr, N)
    if not off:
        nan_row = np.isnan(ga) & (dn != 0)
        assert bool((ref["pr_1"][nan_row]).all()) and not ref["high"][nan_row].any()                 # avg 0: low and counted
        assert bool(ref["high"][(ga > 0) & (dn == 0) & ~np.signbit(dn)].all()) and not ref["pr_1"][dn == 0].any()       # +inf: high; never counted: never pruned by gradient


# ---- every case, both checks ---------------------------------------------------------------------------------------------------------------------
def _case_on_device(case_id):
    c = pc.GROW_CASES[case_id]()
    before, cfg, N = c["before"], c["cfg"], c["N"]
    args = c["args"](DEV)
    if "tags" in c:                                                    # non-vacuity on the DEVICE's activated values
        scal, opac = pc.activated(before, DEV)
        wit = pc.threshold_witness(before, c["tags"], args, cfg, N, scal, opac)
        print(wit)
        for name, (below, equal, above) in wit.items():
            assert below > 0 and equal > 0 and above > 0, (name, below, equal, above)
    return c, before, cfg, N, args


@pytest.mark.parametrize("case_id", list(pc.GROW_CASES))
def test_plan_case(lib, case_id):
    c, before, cfg, N, args = _case_on_device(case_id)
    _check_plan_of_state(lib, before, cfg, args, N)


@pytest.mark.parametrize("case_id", list(pc.GROW_CASES))
def test_grow_and_prune_case(case_id):
    c, before, cfg, N, args = _case_on_device(case_id)
    ref = pc.plan_of(before, cfg, args, N, dev=DEV)
    dv, sg = _check_grow(before, cfg, args, N=N, names=c["names"], optimizer=c["optimizer"])
    assert dv.log == ref["log"] and dv.number == ref["total"]
    _assert_bit_equal({"params": {}, "m": {}, "v": {}, "stats": dv.stats}, {"params": {}, "m": {}, "v": {}, "stats": sg.stats}, case_id)
    assert torch.equal(dv.generator.get_state(), sg.generator.get_state())
    if c["optimizer"] == "empty":
        assert len(dv.optimizer.state) == 0


@pytest.mark.parametrize("P", pc.EDGE_SIZES)
def test_nothing_selected_returns_early(P):
    c = pc.GROW_CASES["nothing-P%d" % P]()
    args = c["args"](DEV)
    s, opt = _build(c["before"], c["cfg"], True)
    params, stats, state = dict(s.p), dict(s.stats), s.generator.get_state().clone()
    s.grow_and_prune(**args)
    assert s.log == [("clone", 0), ("split", 0), ("prune_occ_grad", 0)]
    assert all(s.p[k] is params[k] for k in params) and all(s.stats[k] is stats[k] for k in s.STATS)     # nothing installed
    assert torch.equal(s.generator.get_state(), state)                                                    # nothing drawn
    assert len(opt.state) == len(params) and all(p in opt.state for p in params.values())


def test_a_second_pass_continues_from_the_first():
    """Pass 1 as in every other case; then one `add_densification_stats` at the new size on the device set, and pass 2 on that very object
    against a staged twin built from its state (and its generator's state) at that moment."""
    P = 257
    before = pc.mixed_state(P, seed=23)
    dv, sg = _check_grow(before, {}, pc.MIXED_ARGS, seed=5)
    P1 = dv.number
    assert P1 == sg.number and P1 != P
    g = torch.Generator().manual_seed(1)
    grad = (torch.randn(P1, 3, generator=g) * 0.2).to(DEV)
    flt = (torch.rand(P1, generator=g) > 0.3).to(DEV)
    weight = torch.rand(P1, 1, generator=g).to(DEV)
    radii = torch.randint(0, 60, (P1,), generator=g, dtype=torch.int32).to(DEV)
    dv.add_densification_stats(grad, flt, weight, radii)
    do = dv.optimizer
    st = _state(dv, do)
    before2 = {part: {k: v.cpu() for k, v in st[part].items()} for part in ("params", "stats", "m", "v")}
    assert before2["stats"]["denom"].shape[0] == P1 and float(before2["stats"]["denom"].max()) >= 2
    gen_state = dv.generator.get_state().clone()
    dv.log.clear()
    dv2, sg2 = _check_grow(before2, {}, pc.MIXED_ARGS, device_set=(dv, do), gen_state=gen_state)
    assert dv2 is dv
    ev = dict(dv.log)
    assert ev["clone"] > 0 and ev["split"] > 0 and ev["prune_occ_grad"] > 0, ev
    _assert_bit_equal({"params": {}, "m": {}, "v": {}, "stats": dv.stats}, {"params": {}, "m": {}, "v": {}, "stats": sg2.stats})
    assert torch.equal(dv.generator.get_state(), sg2.generator.get_state())


# ---- the oversize masks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", [None, 0.3])
@pytest.mark.parametrize("spatial_scale", [1.0, 2.0, 0.5])
def test_oversize_masks_on_their_thresholds(spatial_scale, weight):
    before, tags, pick = pc.oversize_case()
    P = before["stats"]["denom"].shape[0]
    assert P == 65
    scal, _ = pc.activated(before, DEV)
    max_scene = float(scal[pick].max()) / spatial_scale                # the device's own value: spatial_scale * max_scene is it again, exactly
    limit = F(spatial_scale * max_scene)
    assert limit == scal[pick].max()
    for name, (below, equal, above) in pc.oversize_witness(before, tags, scal, limit).items():
        assert below > 0 and equal > 0 and above > 0, (name, below, equal, above)
    cfg = {"spatial_scale": spatial_scale}
    dv, do = _build(before, cfg, "all", seed=99)
    sg, so = _build(before, cfg, False, seed=99)
    dv.prune_max_scene_and_screen(max_scene, float(pc.T_MAX_SCREEN), weight)
    sg.prune_max_scene_and_screen(max_scene, float(pc.T_MAX_SCREEN), weight)
    big = (before["stats"]["max_radii2D"].numpy() > pc.T_MAX_SCREEN) | (scal.max(axis=1) > limit)
    n_big = int(big.sum())
    assert n_big == 2 + 3 + 3                                          # strictly above only: two radii, three scales per column
    ev = dict(dv.log)
    assert dv.log == sg.log and ev["prune_large"] + ev["split_large"] == n_big, (dv.log, sg.log)
    assert (ev["split_large"] == 0) if weight is None else (ev["prune_large"] > 0 and ev["split_large"] > 0), ev
    assert dv.number == P - ev["prune_large"] + 4 * ev["split_large"]
    _assert_bit_equal(_state(dv, do), _state(sg, so), (spatial_scale, weight))
    assert torch.equal(dv.generator.get_state(), sg.generator.get_state())
