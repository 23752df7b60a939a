"""The schedule edits of envgs_amd.densify.SurfelSet between densifications -- `enlarge_opacity`, `enlarge_scaling` (normal propagation),
`distort_color` (colour sabotage), `set_learning_rate` -- against the reference's own GaussianModel methods, run on CPU by
tests/golden/make_schedule_edits_golden.py: same inputs, same RNG seed -> the same parameters and Adam moments, to the bit."""
import os
import warnings

import pytest
import torch

from envgs_amd import densify

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedule_edits_golden.pt")
PREFIX = "sampler.pcd."
NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_specular", "_roughness")
EDITS = ("enlarge_opacity", "enlarge_scaling", "distort_color")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=True)


def _build(before, device="cpu", generator=None):
    params = {k: torch.nn.Parameter(before["params"][k].to(device).clone()) for k in NAMES}
    opt = torch.optim.Adam([{"params": [params[k]], "lr": 1e-3, "name": PREFIX + k} for k in NAMES], lr=0.0, eps=1e-15)
    for k in NAMES:
        opt.state[params[k]] = {"step": torch.tensor(2.0), "exp_avg": before["m"][k].to(device).clone(), "exp_avg_sq": before["v"][k].to(device).clone()}
    return densify.SurfelSet(params, opt, PREFIX, row_ops=densify.torch_rows, generator=generator), opt


def _group(opt, k):
    return [g for g in opt.param_groups if g["name"] == PREFIX + k][0]


@pytest.mark.parametrize("name", EDITS)
def test_edit_matches_reference_run(gold, name):
    sc = gold[name]
    s, opt = _build(sc["before"])
    old = dict(s.p)
    for k in NAMES:
        s.p[k].grad = torch.ones_like(s.p[k])
    if sc["rng"] is not None:
        torch.manual_seed(sc["rng"])                                      # generator=None: the global generator, as the reference's rand_like
    getattr(s, name)(**sc["args"])
    assert 0 < sc["rows_changed"] < s.number                              # either side of the edit's mask holds rows
    for k in NAMES:
        prm = _group(opt, k)["params"][0]
        assert prm is s.p[k] and isinstance(prm, torch.nn.Parameter) and prm.requires_grad
        st = opt.state[prm]
        assert torch.equal(prm.detach(), sc["after"]["params"][k]), k
        assert torch.equal(st["exp_avg"], sc["after"]["m"][k]) and torch.equal(st["exp_avg_sq"], sc["after"]["v"][k]), k
        if k == sc["target"]:
            assert prm is not old[k] and prm.grad is None and sc["grad_is_none"]
            assert not torch.equal(prm.detach(), sc["before"]["params"][k])
            assert float(st["exp_avg"].abs().sum()) == 0 and float(st["exp_avg_sq"].abs().sum()) == 0
        else:                                                              # untouched groups keep their parameter, gradient and moments
            assert prm is old[k] and prm.grad is not None
            assert torch.equal(st["exp_avg"], sc["before"]["m"][k]) and float(st["exp_avg"].abs().sum()) > 0
    assert len(opt.state) == len(NAMES)                                    # no stale entries of replaced parameters


def test_distort_color_draws_from_the_sets_generator(gold):
    """With a generator the draw is that generator's and the global one is left alone; the values are the reference's for the same seed."""
    sc = gold["distort_color"]
    s, opt = _build(sc["before"], generator=torch.Generator().manual_seed(sc["rng"]))
    torch.manual_seed(5)
    state = torch.get_rng_state()
    s.distort_color(**sc["args"])
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(s.p["_features_dc"].detach(), sc["after"]["params"]["_features_dc"])


def test_edits_work_without_an_optimizer(gold):
    for name in EDITS:
        sc = gold[name]
        s = densify.SurfelSet(sc["before"]["params"], None, row_ops=densify.torch_rows)
        if sc["rng"] is not None:
            torch.manual_seed(sc["rng"])
        getattr(s, name)(**sc["args"])
        for k in NAMES:
            assert torch.equal(s.p[k].detach(), sc["after"]["params"][k]), (name, k)
        s.set_learning_rate("_opacity", 0.0)                               # nothing to set, nothing raised


def test_enlarging_edits_invalidate_the_tracers_structures(gold, monkeypatch):
    from envgs_amd import tracing
    calls = []
    monkeypatch.setattr(tracing, "invalidate_all_structures", lambda: calls.append(1))
    for name, n in (("enlarge_opacity", 1), ("enlarge_scaling", 1), ("distort_color", 0)):
        s, _ = _build(gold[name]["before"])
        del calls[:]
        getattr(s, name)(**gold[name]["args"])
        assert len(calls) == n, name


def test_set_learning_rate_changes_exactly_one_group(gold):
    s, opt = _build(gold["enlarge_opacity"]["before"])
    s.set_learning_rate("_opacity", 0.0)
    assert [g["lr"] for g in opt.param_groups] == [0.0 if g["name"] == PREFIX + "_opacity" else 1e-3 for g in opt.param_groups]
    s.set_learning_rate("_opacity", 0.05)
    s.set_learning_rate("_no_such_parameter", 7.0)                        # ignored, as in the reference
    s.set_learning_rate(PREFIX + "_xyz", 7.0)                             # the name is the bare one: prefix + prefix + name matches nothing
    assert [g["lr"] for g in opt.param_groups] == [0.05 if g["name"] == PREFIX + "_opacity" else 1e-3 for g in opt.param_groups]


@pytest.mark.gpu
def test_edits_on_device_tensors_do_not_synchronise(gold):
    dev = "cuda:0"
    sets = {}
    for name in EDITS:
        warm, _ = _build(gold[name]["before"], dev, torch.Generator(device=dev).manual_seed(1))
        getattr(warm, name)(**gold[name]["args"])                          # (kernels resident)
        sets[name] = _build(gold[name]["before"], dev, torch.Generator(device=dev).manual_seed(1))
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            for name in EDITS:
                getattr(sets[name][0], name)(**gold[name]["args"])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert [str(w.message) for w in rec if "called a synchronizing" in str(w.message)] == []
    for name in ("enlarge_opacity", "enlarge_scaling"):                    # deterministic edits: the CPU reference's values (exp / log to rounding)
        sc = gold[name]
        s, opt = sets[name]
        got, want, was = s.p[sc["target"]].detach().cpu(), sc["after"]["params"][sc["target"]], sc["before"]["params"][sc["target"]]
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-6)
        assert torch.equal((got != was).flatten(1).any(-1), (want != was).flatten(1).any(-1))
        st = opt.state[s.p[sc["target"]]]
        assert s.p[sc["target"]].grad is None and float(st["exp_avg"].abs().sum()) == 0 and float(st["exp_avg_sq"].abs().sum()) == 0
    sc = gold["distort_color"]
    got, was = sets["distort_color"][0].p["_features_dc"].detach().cpu(), sc["before"]["params"]["_features_dc"]
    kept = torch.sigmoid(sc["before"]["params"]["_specular"]).max(-1).values > sc["args"]["threshold"]
    assert torch.equal(got[kept], was[kept]) and bool(((got - was)[~kept].abs() <= sc["args"]["range"] * (1 + 1e-6)).all())
    assert bool(((got - was)[~kept].abs() > 0).any())
