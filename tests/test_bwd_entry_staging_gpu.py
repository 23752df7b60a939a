"""GPU: how batch_surfel_bwd stages a batch's entries (envgs_amd/csrc/trace_surfel_bwd.hip: stage()) -- descriptors loaded a group ahead, one pair load
per entry with scalar hit counts, record / slot words / SH block in one round trip, wavefront-scope syncs.  That can go wrong at the boundaries of a
group (15 entries) and of a run (5), on the single entries filed from the top of a batch's region, and on each storage form of the features -- not at
size.  So the scenes are tiny and a batch's entry count is KNOWN:

  * `P` faint surfels (opacity 0.05: after 46 hits the transmittance is still ~0.09, every hit is composited) stacked in front of every ray, so that each
    batch has exactly P entries, for P around every boundary, with 64 rays (one full batch), 130 (two full batches and one of two rays) and 1;
  * 64 rays that each run through their own cluster of 20 surfels: 1 280 distinct surfels in one batch, more than the 1 024 slots of its merge table,
    so part of them are single entries.

Every case asserts its entry counts first (a precondition: if it fails the scene is wrong, not the kernel) and that the oracle's audit finds no fragile
ray, then compares every gradient of all three instantiations of the kernel -- generic with `others`, generic without, colour-only -- with the CPU
oracle through tests/util.py:check_close at its K_UNC, the bound of tests/test_trace_parity.py.  Two backward passes over one forward must agree bit
for bit in the ray gradients and in the records themselves (the kernel has no atomics)."""
import math

import numpy as np
import pytest
import torch

from tests.test_trace_parity import _Switch, _hip_forward
from tests.util import check_close

pytestmark = pytest.mark.gpu

BG = torch.tensor([0.2, 0.3, 0.1])
ENTRY_COUNTS = [0, 1, 4, 5, 6, 14, 15, 16, 29, 30, 31, 46]
SWITCHES = dict(force_cap=64, rows_per_ray=64.0, sparse="off")      # every entry goes through the batch kernel; no ray leaves the list path


def _features(n, gen):
    """SH blocks whose colours stay clear of the clamp at zero (its decision is in no list and is not what these tests are about)."""
    shs = torch.cat([0.5 + 1.5 * torch.rand(n, 1, 3, generator=gen), torch.randn(n, 15, 3, generator=gen) * 0.1], 1)
    return dict(shs=shs, others=torch.rand(n, 2, generator=gen), colors_precomp=0.1 + 0.8 * torch.rand(n, 3, generator=gen))


def _stack_scene(P, R, seed):
    """P surfels stacked along +z in front of R near-parallel rays (P = 0: one surfel BEHIND the rays, so that the call still has its structures)."""
    gen = torch.Generator().manual_seed(seed)
    n = max(P, 1)
    z = 1.0 + 0.05 * torch.arange(n, dtype=torch.float32) + 0.01 * torch.rand(n, generator=gen)
    if P == 0:
        z = torch.tensor([-5.0])
    q = torch.cat([torch.ones(n, 1), 0.05 * torch.randn(n, 2, generator=gen), 0.3 * torch.randn(n, 1, generator=gen)], 1)
    g = dict(means3D=torch.cat([0.05 * torch.randn(n, 2, generator=gen), z[:, None]], 1), scales=0.6 + 0.2 * torch.rand(n, 2, generator=gen),
             rotations=q / q.norm(dim=-1, keepdim=True), opacities=torch.full((n, 1), 0.05), **_features(n, gen))
    ro = torch.cat([0.1 * (torch.rand(R, 2, generator=gen) * 2 - 1), torch.zeros(R, 1)], 1)
    rd = torch.cat([0.03 * torch.randn(R, 2, generator=gen), torch.ones(R, 1)], 1)
    return g, ro.contiguous(), (rd / rd.norm(dim=-1, keepdim=True)).contiguous()


def _cluster_scene(seed, rays=64, per_ray=20):
    """Each ray from the origin runs through its own stack of `per_ray` small surfels facing it (directions: a Fibonacci sphere, stacks 8 sigma apart)."""
    gen = torch.Generator().manual_seed(seed)
    i = torch.arange(rays, dtype=torch.float32)
    zc = 1 - 2 * (i + 0.5) / rays
    phi = i * math.pi * (3 - 5 ** 0.5)
    d = torch.stack([(1 - zc * zc).sqrt() * torch.cos(phi), (1 - zc * zc).sqrt() * torch.sin(phi), zc], 1)
    n = rays * per_ray
    dd = d.repeat_interleave(per_ray, 0)
    dist = 2.0 + 0.05 * torch.arange(per_ray, dtype=torch.float32).repeat(rays) + 0.01 * torch.rand(n, generator=gen)
    # the rotation that takes +z to the ray direction (w, x, y, z) = (1 + d.z, z x d), then a small tilt through the renormalisation of a perturbed quaternion
    q = torch.stack([1 + dd[:, 2], -dd[:, 1], dd[:, 0], torch.zeros(n)], 1) + 0.02 * torch.randn(n, 4, generator=gen)
    g = dict(means3D=dd * dist[:, None] + 0.005 * torch.randn(n, 3, generator=gen), scales=0.09 + 0.02 * torch.rand(n, 2, generator=gen),
             rotations=q / q.norm(dim=-1, keepdim=True), opacities=torch.full((n, 1), 0.05), **_features(n, gen))
    return g, torch.zeros(rays, 3), d.contiguous()


def _oracle(g, ro, rd, deg, use_sh, others, hits):
    """The oracle's forward, after its audit: no ray of these scenes is fragile and each composites exactly `hits` surfels."""
    from oracle import trace as otr
    shs = g["shs"].float().numpy()
    geo = [g[k].numpy() for k in ("means3D", "scales", "rotations", "opacities")]
    oth = g["others"].numpy() if others else None
    a = otr.trace_audit(ro.numpy(), rd.numpy(), *geo, others=oth, start_from_first=False, shs=(shs if use_sh else None), sh_degree=(deg if use_sh else 0))
    assert not a["fragile"].any(), "scene precondition: %d fragile rays" % int(a["fragile"].sum())
    assert (a["nhit"] == hits).all(), "scene precondition: hits per ray %s, wanted %d" % (np.unique(a["nhit"]), hits)
    ckw = dict(shs=shs, sh_degree=deg) if use_sh else dict(colors_precomp=g["colors_precomp"].float().numpy())
    return otr.trace_forward(ro.numpy(), rd.numpy(), *geo, others=oth, bg=BG.numpy(), start_from_first=False, **ckw)


def _upstream(R, seed=9):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(R, c, generator=gen) for c in (3, 1, 1, 3, 2)]


def _backward(ctx, ups, colour_only):
    """One backward pass over a kept graph: the five upstream gradients, or the colour's alone (the others arrive as None: the colour-only kernel)."""
    outs, L, o, d, g3 = ctx
    rgb, dpt, acc, norm, dist, aux, mid, wet = outs
    R = o.shape[0]
    used = [(rgb, ups[0])] if colour_only else list(zip((rgb, dpt, acc, norm, aux), ups))
    leaves = dict(L, ray_o=o, ray_d=d, grads3D=g3)
    for t in leaves.values():
        t.grad = None
    sum((x.reshape(R, -1) * y.to(o.device)).sum() for x, y in used).backward(retain_graph=True)
    torch.cuda.synchronize()
    return {k: (t.grad.detach().cpu().numpy() if t.grad is not None else None) for k, t in leaves.items()}


def _against_oracle(test, tag, got, ref, ups, colour_only, use_sh, others):
    from oracle import trace as otr
    gr = [u.numpy() if (i == 0 or not colour_only) else np.zeros_like(u.numpy()) for i, u in enumerate(ups)]
    rb = otr.trace_backward(ref, gr[0], gr[1][:, 0], gr[2][:, 0], gr[3], gr[4], want_cond=True)
    col = "shs" if use_sh else "colors_precomp"
    names = dict(means3D="dmeans3D", grads3D="dmeans3D", scales="dscales", rotations="drots", opacities="dopacities", ray_o="dray_o", ray_d="dray_d")
    names[col] = "dshs" if use_sh else "dcolors"
    if others and not colour_only:
        names["others"] = "dothers"
    for k, nm in names.items():
        assert got[k] is not None, (tag, k)
        want = rb[nm]
        check_close(test, "%s.%s" % (tag, k), got[k].reshape(want.shape), want, cond=rb["cond"][nm], unc=rb["unc"][nm])


def _entry_counts():
    from envgs_amd import tracing
    return tracing.last_record_scratch()["n_entries"].cpu().numpy().astype(np.int64)


def _run_forms(test, g, ro, rd, deg, use_sh, forms, hits, expect):
    """forms: subset of ("others", "generic", "colour").  expect(n_entries (batches, 2)) asserts the scene's entry counts."""
    from envgs_amd import tracing
    R = ro.shape[0]
    ups = _upstream(R)
    old_keep = tracing.KEEP_LISTS["on"]
    tracing.KEEP_LISTS["on"] = True
    try:
        with _Switch(**SWITCHES):
            for with_others in (True, False):
                mine = [f for f in forms if (f == "others") == with_others]
                if not mine:
                    continue
                ref = _oracle(g, ro, rd, deg, use_sh, with_others, hits)
                ctx = _hip_forward(g, ro, rd, BG, deg, use_sh, False, others=with_others)
                ne = _entry_counts()
                assert ne.shape == ((R + 63) // 64, 2)
                expect(ne)
                tc = tracing.last_trace_counts()
                assert tc["sparse_hits"] == 0 and tc["max_list"] <= tc["cap"] and tc["rays_without_rows"] == 0 and tc["stack_overflows"] == 0
                for f in mine:
                    got = _backward(ctx, ups, f == "colour")
                    _against_oracle(test, f, got, ref, ups, f == "colour", use_sh, with_others)
    finally:
        tracing.KEEP_LISTS["on"] = old_keep


@pytest.mark.parametrize("R", [64, 130, 1])
@pytest.mark.parametrize("P", ENTRY_COUNTS)
def test_entry_count_at_group_and_run_boundaries(P, R, request):
    g, ro, rd = _stack_scene(P, R, seed=100 + P)

    def expect(ne):
        assert (ne.sum(1) == P).all(), "scene precondition: entries per batch %s, wanted %d" % (ne.sum(1), P)
    _run_forms(request.node.name, g, ro, rd, 3, True, ("others", "generic", "colour"), P, expect)


def test_single_entries_filed_from_the_top(request):
    g, ro, rd = _cluster_scene(seed=5)

    def expect(ne):
        assert ne.shape[0] == 1 and ne[0, 1] > 0 and ne.sum() == 1280, "scene precondition: (table entries, singles) = %s" % (ne[0],)
    _run_forms(request.node.name, g, ro, rd, 3, True, ("others", "generic", "colour"), 20, expect)


@pytest.mark.parametrize("path", ["sh_deg0", "sh_deg1", "sh_deg2", "sh_deg3", "colors_precomp", "sh_fp16"])
def test_every_feature_storage_path(path, request):
    """16 entries per batch (one group and one entry of the next), 130 rays: SH degree 0 .. 3 of 16 stored coefficients (the words beyond the active
    degree are staged as zeros), precomputed colours, fp16 storage -- each with `others` and all five upstream gradients, without `others`, and
    with the colour's gradient alone."""
    P, R = 16, 130
    g, ro, rd = _stack_scene(P, R, seed=7)
    use_sh = path != "colors_precomp"
    deg = int(path[-1]) if path.startswith("sh_deg") else (3 if use_sh else 0)
    def expect(ne):
        assert (ne.sum(1) == P).all(), "scene precondition: entries per batch %s, wanted %d" % (ne.sum(1), P)
    if path == "sh_fp16":
        import envgs_amd
        g["shs"] = g["shs"].half().float()                      # what fp16 storage holds: the oracle evaluates these values
        envgs_amd.set_feature_storage("f16")                    # fp32 tensors in, half copies inside the node, fp32 gradients out
    try:
        _run_forms(request.node.name, g, ro, rd, deg, use_sh, ("others", "generic", "colour"), P, expect)
    finally:
        if path == "sh_fp16":
            envgs_amd.set_feature_storage("f32")


@pytest.mark.parametrize("scene", ["stack31", "clusters"])
def test_two_backward_passes_agree_bit_for_bit(scene, monkeypatch):
    """A fixed forward, two backward passes: bit-equal ray gradients and, for the same entries, bit-equal records (words 0 .. 62 of each; word 63 is padding
    nobody writes)."""
    from envgs_amd import tracing
    g, ro, rd = _stack_scene(31, 130, seed=3) if scene == "stack31" else _cluster_scene(seed=6)
    seen = []
    orig = tracing._scratch

    def spy(shape, dtype, dev):
        t = orig(shape, dtype, dev)
        if len(shape) == 2 and shape[1] == 64 and dtype == torch.float32:
            seen.append(t)
        return t
    monkeypatch.setattr(tracing, "_scratch", spy)
    ups = _upstream(ro.shape[0])
    with _Switch(**SWITCHES):
        for with_others, colour_only in ((True, False), (False, False), (False, True)):
            ctx = _hip_forward(g, ro, rd, BG, 3, True, False, others=with_others)
            assert tracing.last_trace_counts()["sparse_hits"] == 0
            runs = []
            for _ in range(2):
                del seen[:]
                got = _backward(ctx, ups, colour_only)
                tracing.join_deferred_gradients()
                torch.cuda.synchronize()
                assert len(seen) == 1, "the record buffer of the backward was not seen"
                runs.append((got, seen[0][:, :63].clone()))
            (a, ra), (b, rb) = runs
            assert ra.shape == rb.shape and ra.shape[0] > 0 and torch.equal(ra, rb), (with_others, colour_only)
            assert float(ra.abs().max()) > 0
            for k in ("ray_o", "ray_d"):
                assert np.abs(a[k]).max() > 0 and np.array_equal(a[k], b[k]), (k, with_others, colour_only)
