"""CPU checks of tests/densify_plan_cases.py, the inputs of tests/test_densify_plan_edges_gpu.py:

  * the threshold rows are what they claim: every one of the plan's six comparisons has rows exactly on the threshold, strictly below and
    strictly above, in float32 arithmetic;
  * every end-to-end case goes through the staged three stages on the CPU (`row_ops=densify.torch_rows`) and leaves the `log` and the row count
    that the NumPy restatement of the plan predicts -- so a failure of the same case on the GPU cannot be blamed on an impossible input;
  * the uniform mixes, the one-of-each sets, the flag rows and the weight sets have the empty segments / decisive rows they were built for.
"""
import numpy as np
import pytest
import torch

from tests import densify_plan_cases as pc
from envgs_amd import densify
from tests.test_densify_device import _build, _staged_three

F = np.float32


def test_ulp_steps_and_key_decoding():
    assert pc.ulp_step(F(1.0), 1) == F(1.0) + F(2.0 ** -23) and pc.ulp_step(F(1.0), -1) == F(1.0) - F(2.0 ** -24)
    assert pc.ulp_step(F(-1.0), 1) == -(F(1.0) - F(2.0 ** -24)) and pc.ulp_step(F(-1.0), -1) == -(F(1.0) + F(2.0 ** -23))
    for f in (0.0, -0.0, 1.5, -1.5, 3e-39, float("inf"), -float("inf")):            # the encoder of csrc/float_key.h, then the decoder under test
        b = int(np.array(f, F).view(np.uint32))
        key = (~b & 0xFFFFFFFF) if b & 0x80000000 else b | 0x80000000
        assert int(np.array(pc.float_of_key(key), F).view(np.uint32)) == b
    assert np.isnan(pc.float_of_key(0)) and np.signbit(pc.float_of_key(0))          # key 0, "nothing yet": a negative NaN


def test_the_gradient_hits_exist_in_float32():
    r2 = F(pc.split_r(2))
    assert r2 == F(0.625) and float(r2) == pc.split_r(2)                             # N = 2, ratio 0.8: r is exact
    assert F(F(F(0.24000000953674316) * r2) / F(1.0)) == pc.T_MING
    for dn in (1, 2, 3, 4):
        lo, at, hi = pc.scaled_rows(pc.T_MING, dn, 2)
        assert pc.scaled_avg(lo, dn, r2)[0] < pc.T_MING == pc.scaled_avg(at, dn, r2)[0] < pc.scaled_avg(hi, dn, r2)[0]
    r3 = F(pc.split_r(3))
    assert float(r3) != pc.split_r(3)                                                # N = 3: r is rounded, the hit comes from the search
    lo, at, hi = pc.scaled_rows(pc.T_MING, 1, 3)
    assert pc.scaled_avg(lo, 1, r3)[0] < pc.T_MING == pc.scaled_avg(at, 1, r3)[0] < pc.scaled_avg(hi, 1, r3)[0]
    for T in (pc.T_GRAD, pc.T_MING):
        for dn in (1, 2, 3):
            lo, at, hi = pc.quotient_rows(T, dn)
            assert F(lo / F(dn)) < T == F(at / F(dn)) < F(hi / F(dn))
            assert pc.ulp_step(lo, 1) <= at <= pc.ulp_step(hi, -1)                   # one step of the free input beyond the rows that hit


@pytest.mark.parametrize("N,spatial_scale", [(2, 1.0), (2, 2.0), (2, 0.5), (3, 1.0)])
def test_threshold_rows_sit_below_on_and_above_every_comparison(N, spatial_scale):
    before, tags, picks = pc.threshold_case()
    assert before["stats"]["denom"].shape[0] == 320
    cfg = {"spatial_scale": spatial_scale}
    args = pc.data_thresholds(before, picks, spatial_scale, "cpu")
    assert F(args["size_threshold"] * spatial_scale) == F(args["size_threshold"]) * F(spatial_scale) == pc.activated(before)[0][picks["size"]].max()
    scal, opac = pc.activated(before, "cpu")
    wit = pc.threshold_witness(before, tags, args, cfg, N, scal, opac)
    print(wit)
    assert len(wit) == 9
    for name, (below, equal, above) in wit.items():
        assert below > 0 and equal > 0 and above > 0, (name, below, equal, above)
    # the rows decide something: flipping any one of the comparisons' strictness moves a class bit
    plan = pc.plan_of(before, cfg, args, N)
    t = {k: v for k, v in tags.items()}
    clone, split, pr_1, pr_s = plan["clone"], plan["split"], plan["pr_1"], plan["pr_s"]
    for tag in ("grad_small", "size_c0", "size_c1", "screen"):
        assert 0 < int(clone[t[tag]].sum()) and (tag == "screen" or int(clone[t[tag]].sum()) < len(t[tag])), tag
    for tag in ("grad_large", "size_c0", "size_c1", "screen", "opac_s", "mingrad_s%d" % N):
        assert 0 < int(split[t[tag]].sum()) and (tag in ("opac_s", "mingrad_s%d" % N) or int(split[t[tag]].sum()) < len(t[tag])), tag
    for tag in ("opac_1", "mingrad_1"):
        assert 0 < int(pr_1[t[tag]].sum()) < len(t[tag]) and not split[t[tag]].any(), tag
    for tag in ("opac_s", "mingrad_s%d" % N):
        assert 0 < int(pr_s[t[tag]].sum()) < len(t[tag]), tag
    assert not pr_1[t["dn0"]].any() and not pr_s[t["dn0"]].any() and int(split[t["dn0"]].sum()) == 1 and int(clone[t["dn0"]].sum()) == 1


@pytest.mark.parametrize("case_id", list(pc.GROW_CASES))
def test_the_staged_stages_complete_on_the_cpu_and_match_the_restated_plan(case_id):
    c = pc.GROW_CASES[case_id]()
    args = c["args"]("cpu")
    plan = pc.plan_of(c["before"], c["cfg"], args, c["N"])
    s, opt = _build(c["before"], c["cfg"], False, dev="cpu", names=c["names"], optimizer=c["optimizer"], row_ops=densify.torch_rows)
    _staged_three(s, args, c["N"])
    assert s.log == plan["log"], (s.log, plan["log"])
    assert s.number == plan["total"]
    for k in s.STATS:
        assert s.stats[k].shape[0] == plan["total"]
    for k in c["names"]:
        assert s.p[k].shape == (plan["total"],) + tuple(c["before"]["params"][k].shape[1:])


def _counters(case_id):
    c = pc.GROW_CASES[case_id]()
    plan = pc.plan_of(c["before"], c["cfg"], c["args"]("cpu"), c["N"])
    return plan, plan["counters"], c["before"]["stats"]["denom"].shape[0]


@pytest.mark.parametrize("P", pc.EDGE_SIZES)
def test_uniform_mixes_empty_the_segments_they_name(P):
    plan, (nA, nB, nD, nE, nS1, nS2, n_clone), _ = _counters("all_clone-P%d" % P)
    assert (nA, nB, nD, nE, nS1, nS2, n_clone) == (P, P, 0, 0, 0, 0, P)
    plan, (nA, nB, nD, nE, nS1, nS2, n_clone), _ = _counters("all_split-P%d" % P)
    assert (nA, nB, nD, nE, nS1, nS2, n_clone) == (0, 0, P, 0, P, 0, 0)
    plan, (nA, nB, nD, nE, nS1, nS2, n_clone), _ = _counters("all_clone_split-P%d" % P)
    assert (nA, nB, nD, nE, nS1, nS2, n_clone) == (0, 0, P, P, P, P, P)
    plan, (nA, nB, nD, nE, nS1, nS2, n_clone), _ = _counters("all_pruned-P%d" % P)
    assert plan["total"] == 0 and (nA, nB, nD, nE) == (0, 0, 0, 0) and (P < 4 or (n_clone > 0 and nS1 > 0 and nS2 > 0))
    plan, (nA, nB, nD, nE, nS1, nS2, n_clone), _ = _counters("prune_only-P%d" % P)
    assert (nB, nD, nE, nS1, nS2, n_clone) == (0,) * 6 and nA == P // 2 < P
    plan, (nA, nB, nD, nE, nS1, nS2, n_clone), _ = _counters("nothing-P%d" % P)
    assert (nA, nB, nD, nE, nS1, nS2, n_clone) == (P, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("kind", pc.ONE_OF_EACH)
def test_one_of_each_has_one_row_per_class_and_the_named_one_on_the_edge(kind):
    want = {"clone": (1, 0, 0), "split": (0, 1, 0), "clone_split": (1, 1, 0), "pruned": (0, 0, 1), "clone_pruned": (1, 0, 1), "split_pruned": (0, 1, 1),
            "clone_split_pruned": (1, 1, 1)}                                          # (cloned, split, pruned: by pr_s when split, by pr_1 otherwise)
    for at_end in (False, True):
        plan, _, P = _counters("one_%s_%s" % (kind, "last" if at_end else "first"))
        gone = np.where(plan["split"], plan["pr_s"], plan["pr_1"])
        fate = [(int(c), int(s), int(g)) for c, s, g in zip(plan["clone"], plan["split"], gone)]
        assert sorted(f for f in fate if f != (0, 0, 0)) == sorted(want.values())
        assert fate[P - 1 if at_end else 0] == want[kind]


def test_the_flag_rows_make_a_zero_threshold_decide():
    before = pc.flag_state()
    z = slice(0, pc.ZERO_ROWS)
    scal, opac = pc.activated(before)
    assert int((opac[z] == 0).sum()) >= 4 and bool((opac > 0).any())                 # saturated opacities: 0 < 0.0 is false
    base = pc.plan_of(before, {}, pc.MIXED_ARGS)
    for name, change in pc.FLAG_VARIANTS.items():
        plan = pc.plan_of(before, {}, dict(pc.MIXED_ARGS, **change))
        assert not np.array_equal(plan["cls"], base["cls"]), name                    # every variant changes the result
        assert not np.array_equal(plan["cls"][z], base["cls"][z]), name              # ... among the hand-made rows too
    st = before["stats"]
    mr, ga, dn = st["max_radii2D"].numpy()[z], st["xyz_gradient_accum"].numpy()[z, 0], st["denom"].numpy()[z, 0]
    p0 = pc.plan_of(before, {}, dict(pc.MIXED_ARGS, split_screen_threshold=0.0))
    small_high = p0["clone"][z]
    assert bool((small_high & (mr == 0) & ~p0["split"][z]).any()) and bool((small_high & (mr > 0) & p0["split"][z]).any())
    p0 = pc.plan_of(before, {}, dict(pc.MIXED_ARGS, min_gradient=0.0))
    zero_avg = (ga == 0) & (dn != 0)
    assert bool((zero_avg & p0["pr_1"][z] & (opac[z] > 0.05)).any()) and bool(((ga > 0) & (dn != 0) & ~p0["pr_1"][z]).any())
    assert bool(((ga == 0) & (dn == 0) & ~p0["pr_1"][z]).any())
    p0 = pc.plan_of(before, {}, dict(pc.MIXED_ARGS, min_opacity=0.0))
    assert not p0["pr_1"][z][(opac[z] == 0) & ~zero_avg & (pc.stat_avg(ga, dn) > 0.15)].any() and bool(((opac[z] == 0) & ~p0["pr_1"][z]).any())


def test_the_weight_sets_reach_both_branches_of_the_maximum():
    for kind in pc.WEIGHT_KINDS:
        before = pc.weight_state(kind)
        plan = pc.plan_of(before, {}, pc.MIXED_ARGS)
        wa = before["stats"]["xyz_weight_accum"].numpy()[:, 0]
        cl = plan["clone"]
        assert cl.any() and (cl & plan["split"]).any() and (plan["split"] & ~plan["pr_s"]).any()       # clone children and surviving split children exist
        w0 = wa.max()
        prod = wa[cl] * w0
        wmax1 = max(w0, prod.max())
        if kind == "zeros":
            assert w0 == 0 and wmax1 == 0 and not np.signbit(wa).any()
        elif kind == "negative":                                                     # the smallest cloned weight, not the largest, gives the largest product
            assert w0 < 0 and wa[cl].min() < wa[cl].max() and prod.max() == F(wa[cl].min() * w0) > F(wa[cl].max() * w0) and wmax1 == prod.max() > 0
        elif kind == "mixed_sign":
            assert w0 > 0 and wa[cl].min() < 0 < wa[cl].max() and wmax1 == F(wa[cl].max() * w0) > w0
        else:
            assert w0 > 0 and wa[cl].max() < 0 and wmax1 == w0
        # what the rewrite's rule (largest cloned weight when wmax0 >= 0, smallest otherwise) must reproduce
        sel = wa[cl].min() if w0 < 0 else wa[cl].max()
        assert wmax1 == max(w0, F(sel * w0))


def test_the_oversize_rows_sit_on_their_thresholds():
    before, tags, pick = pc.oversize_case()
    scal, _ = pc.activated(before)
    for spatial_scale in (1.0, 2.0, 0.5):
        max_scene = float(scal[pick].max()) / spatial_scale
        wit = pc.oversize_witness(before, tags, scal, F(spatial_scale * max_scene))
        for name, (below, equal, above) in wit.items():
            assert below > 0 and equal > 0 and above > 0, (name, below, equal, above)
    s, _ = _build(before, {}, False, dev="cpu", row_ops=densify.torch_rows)
    s.prune_max_scene_and_screen(float(scal[pick].max()), float(pc.T_MAX_SCREEN), 0.3)
    ev = dict(s.log)
    assert ev["prune_large"] > 0 and ev["split_large"] > 0


def test_special_rows_cover_the_non_finite_averages():
    ga, dn, mr, wa, scal, opac = pc.special_rows()
    avg = pc.stat_avg(ga, dn)
    assert bool((np.isnan(ga) & (dn != 0) & (avg == 0)).any())                       # NaN / d -> 0
    assert bool((np.isposinf(ga) & np.isposinf(avg)).any())
    assert bool(((ga > 0) & (dn == 0) & np.isposinf(avg)).any())                     # x / 0 = +inf: "high"
    assert bool(((ga == 0) & (dn == 0) & (avg == 0)).any())                          # 0 / 0 -> 0
    assert bool(np.isneginf(avg).any())
    thr = dict(grad_threshold=0.1, size_limit=0.03, split_screen_threshold=20.0, min_opacity=0.05, min_gradient=0.15)
    plan = pc.plan_reference(ga, dn, mr, wa, scal, opac, thr, 2)
    assert len(set(plan["cls"].tolist())) >= 5
