"""GPU: the tracer's record backward hands its batches out longest first (include/envgs_trace.h: bwd_order), one workgroup per batch, instead of in
coherence order over a capped grid (ENVGS_DBG_BALANCE bit 1: the dispatch until round 7).  Which workgroup takes a batch changes no arithmetic: both
dispatches differentiate the SAME forward here (one graph, two backward passes -- two forwards would file a surfel's records in different slots, the
slots come from atomics) and must agree

  * bit for bit wherever the path has no float atomics: every gradient of a call without overflow rays and without sparse entries, except dL/d(others)
    (one two-lane atomic per (batch, surfel) entry, batch_surfel_bwd),
  * elsewhere at RUN_TO_RUN, the bound the suite already uses between two runs of such sums (tests/test_trace_parity.py: deferred surfel gradients;
    tests/test_raster_parity.py: LDS / L2 atomics in a different order): 2e-5 of the tensor's largest magnitude, far inside tests/util.py's TOL.

The order buffer itself is read back: a permutation of the batches, non-increasing in the class of the entry count, coherence order inside a class."""
import numpy as np
import pytest
import torch

from tests.test_oracle_trace import trace_scene
from tests.test_trace_parity import _Switch, _hip_forward
from tests.util import TOL

pytestmark = pytest.mark.gpu

RUN_TO_RUN = 2e-5
assert RUN_TO_RUN < TOL
BALANCE = 6                     # ENVGS_DBG_BALANCE
BG = torch.tensor([0.2, 0.3, 0.1])


def _scene(P, R, seed, shrink=0.3):
    g, ro, rd = trace_scene(P=P, R=R, seed=seed, camera=False)
    g["scales"] = g["scales"] * shrink
    return g, ro, rd


def _check_order(order, ne, classes):
    from envgs_amd import tracing
    cnt = ne.sum(1).cpu().numpy().astype(np.int64)
    order = order.cpu().numpy().astype(np.int64)
    assert order.shape == cnt.shape
    assert np.array_equal(np.sort(order), np.arange(cnt.size))                 # a permutation: every batch exactly once
    cls = tracing.bwd_order_class(cnt, classes)[order]
    step = np.diff(cls)
    assert (step <= 0).all()                                                   # longest class first
    assert (np.diff(order)[step == 0] > 0).all()                               # coherence order inside a class
    return cnt, order


def _both_dispatches(g, ro, rd, form, classes=0, **switches):
    """form: "colour" (only dL/drgb: the colour-only kernel), "generic", "others" (generic with others_precomp).  Returns the gradients under the default
    dispatch and under ENVGS_DBG_BALANCE = 1, the trace counts, and the checked (entry counts, order)."""
    from envgs_amd import tracing, _lib
    lib = _lib.load()
    old_keep = tracing.KEEP_LISTS["on"]
    tracing.KEEP_LISTS["on"] = True
    try:
        with _Switch(**switches):
            lib.envgs_debug_set(BALANCE, classes << 8)
            outs, L, o, d, g3 = _hip_forward(g, ro, rd, BG, 3, True, False, others=(form == "others"))
            rec = tracing.last_record_scratch()
            tc = tracing.last_trace_counts()
            cnt, order = _check_order(rec["bwd_order"][:(ro.shape[0] + 63) // 64], rec["n_entries"], classes or tracing.BWD_ORDER_CLASSES)
            R = o.shape[0]
            gen = torch.Generator().manual_seed(4)
            ups = [(torch.randn(R, c, generator=gen) / R).to(o.device) for c in (3, 1, 1, 3, 2)]
            rgb, dpt, acc, norm, dist, aux, mid, wet = outs
            used = [(rgb, ups[0])] if form == "colour" else list(zip((rgb, dpt, acc, norm, aux), ups))
            loss = sum((x.reshape(R, -1) * y).sum() for x, y in used)
            leaves = dict(L, ray_o=o, ray_d=d, grads3D=g3)
            res = []
            for bal in (0, 1):
                lib.envgs_debug_set(BALANCE, (classes << 8) | bal)
                for t in leaves.values():
                    t.grad = None
                loss.backward(retain_graph=True)
                torch.cuda.synchronize()
                res.append({k: t.grad.detach().clone() for k, t in leaves.items() if t.grad is not None})
    finally:
        lib.envgs_debug_set(BALANCE, 0)
        tracing.KEEP_LISTS["on"] = old_keep
    assert set(res[0]) == set(res[1]) and {"means3D", "shs", "ray_o", "ray_d"} <= set(res[0])
    return res[0], res[1], tc, cnt, order


def _compare(new, old, exact):
    for k in new:
        assert float(new[k].abs().max()) > 0 or float(old[k].abs().max()) == 0, k
        if exact and k != "others":
            assert torch.equal(new[k], old[k]), (k, float((new[k] - old[k]).abs().max()))
        else:
            err = float((new[k] - old[k]).abs().max())
            assert err <= RUN_TO_RUN * float(old[k].abs().max()) + 1e-12, (k, err)


def _no_atomics(tc):
    return tc["max_list"] <= tc["cap"] and tc["sparse_hits"] == 0 and tc["rays_without_rows"] == 0 and tc["stack_overflows"] == 0


@pytest.mark.parametrize("form", ["colour", "generic", "others"])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 64 * 9 + 1])
def test_longest_first_matches_coherence_order(R, form):
    g, ro, rd = _scene(1500, R, seed=31 + R)
    new, old, tc, cnt, order = _both_dispatches(g, ro, rd, form, force_cap=256, rows_per_ray=256.0, sparse="off")
    assert _no_atomics(tc) and cnt.sum() > 0
    _compare(new, old, exact=True)


@pytest.mark.parametrize("classes", [1, 8, 1024])
def test_order_at_other_class_counts(classes):
    """The K sweep's switch (ENVGS_DBG_BALANCE >> 8): 1 class = coherence order through the new dispatch, 1024 = a full sort of these counts."""
    g, ro, rd = _scene(1500, 64 * 40 + 7, seed=5)
    new, old, tc, cnt, order = _both_dispatches(g, ro, rd, "colour", classes=classes, force_cap=256, rows_per_ray=256.0, sparse="off")
    assert _no_atomics(tc)
    if classes == 1:
        assert np.array_equal(order, np.arange(order.size))
    if classes == 1024 and cnt.max() < 1024:
        assert (np.diff(cnt[order]) <= 0).all()
    _compare(new, old, exact=True)


def test_more_batches_than_the_old_grid():
    """8194 batches: more than the resident slots, and more than the 8192 workgroups the old dispatch was capped at (its first two ran two batches)."""
    R = 64 * 8193 + 5
    g, ro, rd = _scene(512, R, seed=2)
    new, old, tc, cnt, order = _both_dispatches(g, ro, rd, "colour", force_cap=128, rows_per_ray=64.0, sparse="off")
    assert cnt.size == 8194 and _no_atomics(tc)
    _compare(new, old, exact=True)


def test_skewed_batches():
    """Half of the rays miss everything (batches without an entry), and one batch of near-identical rays runs through a column of 150 faint surfels: the
    longest lists by far -- it must be the first batch handed out."""
    g, ro, rd = _scene(1500, 64 * 12, seed=8)
    gen = torch.Generator().manual_seed(3)
    n = 150
    col = dict(means3D=torch.stack([torch.zeros(n), torch.zeros(n), torch.linspace(1.0, 2.5, n)], 1),
               scales=torch.full((n, 2), 0.2), rotations=torch.tensor([[1.0, 0, 0, 0]]).repeat(n, 1), opacities=torch.full((n, 1), 0.05),
               shs=g["shs"][:n].clone(), others=g["others"][:n].clone(), colors_precomp=g["colors_precomp"][:n].clone())
    g = {k: torch.cat([g[k], col[k]]) for k in g}
    through = torch.cat([torch.randn(64, 2, generator=gen) * 0.01, torch.zeros(64, 1)], 1)
    miss_o = torch.tensor([100.0, 0, 0]) + torch.randn(64 * 13, 3, generator=gen)
    miss_d = torch.tensor([1.0, 0, 0]) + torch.randn(64 * 13, 3, generator=gen) * 0.05
    ro = torch.cat([ro, through, miss_o]).contiguous()
    rd = torch.cat([rd, torch.tensor([[0.0, 0, 1.0]]).repeat(64, 1), miss_d]).contiguous()
    new, old, tc, cnt, order = _both_dispatches(g, ro, rd, "generic", force_cap=512, rows_per_ray=512.0, sparse="off")
    assert _no_atomics(tc)
    assert (cnt == 0).sum() >= 8 and cnt.max() >= 150 and cnt.max() > 2 * np.median(cnt[cnt > 0])
    assert cnt[order[0]] == cnt.max() and cnt[order[-1]] == 0
    _compare(new, old, exact=True)


def test_with_overflow_rays():
    """Lists capped at 12 hits: the rays beyond take the K-buffer hand-off, whose atomics land in the same accumulators."""
    g, ro, rd = _scene(1500, 64 * 9 + 1, seed=11, shrink=0.6)
    new, old, tc, cnt, order = _both_dispatches(g, ro, rd, "others", force_cap=12, sparse="off")
    assert tc["max_list"] > 12
    _compare(new, old, exact=False)


def test_with_sparse_entries():
    """ENVGS_DBG_SPARSE: entries of at most four hits are filed per hit and differentiated by sparse_hits_bwd, which adds to the ray gradients."""
    g, ro, rd = _scene(1500, 64 * 9 + 1, seed=12)
    new, old, tc, cnt, order = _both_dispatches(g, ro, rd, "generic", force_cap=256, rows_per_ray=256.0, sparse="on", sparse_max=4)
    assert tc["sparse_hits"] > 0
    _compare(new, old, exact=False)
