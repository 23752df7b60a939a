"""GPU: the acceleration structure as the tracer really builds it -- WITH the opacities (SurfelTracer hands them to build_bvh in every traced call, and
most training steps refit).  quad_box (csrc/trace_bvh.hip) then intersects every leaf box with the box of the disc where the surfel can still
contribute, or collapses it to the centre; tests/test_bvh_structure.py never passes opacities, and a box that is slightly too tight loses exactly the
hits at alpha ~ 1/255 that the trace parity tests leave to the audit.  Here: the structural invariants on tightened trees, every leaf box against
the float64 reference of tests/bvh_reference.py (conservative, never looser than the quad's box, tight, collapsed where nothing can contribute), a
refit against a fresh build bit for bit, envgs_bvh_quality against a host sum, and rays aimed at the contribution boundary end to end (and at the
centres of the surfels whose leaves are collapsed, which must stay unseen)."""
import numpy as np
import pytest
import torch

from envgs_amd import synth, tracing
from tests import bvh_reference as br
from tests.util import FRAGILE_RAYS_MAX, TOL, check_close, record, record_fragile

pytestmark = pytest.mark.gpu

SEED = 3                     # the seed tests/test_bvh_reference_cpu.py audits the boundary rays of


def _scene(P=256, seed=SEED, clustered=False):
    """(g, v): br.scene as numpy and its (4P,3) fp32 quad vertices."""
    g = br.scene(P, seed)
    if clustered:
        g["means3D"][: P // 2] = g["means3D"][0]                      # identical Morton codes: the id tie-break must still give a tree
    v, _ = synth.get_disks(*(torch.from_numpy(g[k]) for k in ("means3D", "scales", "rotations")))
    return g, v.numpy()


def _moved(g, seed):
    """The same surfels somewhere else: moved centres, rescaled, opacities shuffled (contributing surfels become collapsed and the reverse)."""
    rng = np.random.default_rng(seed)
    P = g["means3D"].shape[0]
    g2 = dict(g, means3D=(g["means3D"] + 0.3 * rng.standard_normal((P, 3))).astype(np.float32),
              scales=(g["scales"] * rng.uniform(0.5, 1.5, (P, 2))).astype(np.float32), opacities=g["opacities"][rng.permutation(P)])
    v2, _ = synth.get_disks(*(torch.from_numpy(g2[k]) for k in ("means3D", "scales", "rotations")))
    return g2, v2.numpy()


def _build(v, o, refit=None):
    nodes, n = tracing.build_bvh(torch.from_numpy(v).cuda(), torch.from_numpy(o).cuda(), refit=refit)
    torch.cuda.synchronize()
    assert n == v.shape[0] // 4 and tracing.LAST_STATS["bvh"] == ("build" if refit is None else "refit")
    return nodes


def _check_leaf_boxes(test, lo, hi, v, o, need_tightened=False):
    """(b): the stored leaf boxes (lo, hi) (P,3) fp32 of a tree over quads v and opacities o against the float64 reference."""
    lo = lo.astype(np.float64); hi = hi.astype(np.float64)
    P = lo.shape[0]
    mu, a, b = br.frame(v)
    qlo, qhi = br.quad_box(v)
    # conservative: everything that contributes with a margin of 1e-5 in alpha (2.5 x the margin below which the oracle's audit calls the alpha test
    # undecidable) is inside the stored box -- no tolerance.  (At delta = 0 this cannot be demanded: for o within ~1e-4 relative of 1/255 the fp32
    # rounding of 255 o inside the logarithm moves the radius by more than the pad.)
    clo, chi, cm = br.contributing_box(v, o, 1e-5)
    assert (lo[cm] <= clo[cm]).all() and (hi[cm] >= chi[cm]).all(), "a leaf box cuts into its surfel's contributing region"
    # never looser than the untightened box
    qp = br.pad(qlo, qhi)
    assert (lo >= qlo - 2 * qp).all() and (hi <= qhi + 2 * qp).all()
    # tight: kernel radius = sqrt(tau) (1 + 1e-4), plus the rounding of the logarithm and two square roots (3e-4 he in all), plus the pad and its rounding
    r2, _ = br.radius2(o)
    tm = r2 >= 1e-2
    if tm.any():
        rlo, rhi, _ = br.contributing_box(v, o, 0.0)
        he = np.minimum(br.disc_half_extent(v, o, 0.0)[0], 3.0 * (np.abs(a) + np.abs(b)))      # (a disc beyond the quad's corner: the face is the quad's)
        bound = 3e-4 * he + 2 * br.pad(rlo, rhi)
        slack = np.maximum(rlo - lo, hi - rhi)
        ratio = float((slack[tm] / bound[tm]).max())
        record(test, "leaf_box_slack/bound", ratio, "(%d surfels; asserted <= 1)" % int(tm.sum()))
        assert ratio <= 1.0, "a tightened leaf box is looser than the kernel's documented margins allow (%.3g x)" % ratio
    # collapsed: nothing of the surfel can contribute -> the centre +- pad
    with np.errstate(invalid="ignore"):
        o32 = np.asarray(o, np.float32).reshape(-1)
        col = (np.float32(255.0) * o32 <= np.float32(1.0)) | np.isnan(o32) | (o32 <= 0)
    assert not (col & cm).any()
    mp = br.pad(mu, mu)
    assert (lo[col] >= mu[col] - 2 * mp[col]).all() and (lo[col] <= mu[col]).all() and (hi[col] <= mu[col] + 2 * mp[col]).all() and (hi[col] >= mu[col]).all()
    # tightening is on: a surfel of opacity <= 0.5 (disc radius <= 3.12) in general position (no a_c, b_c zero) is smaller than its quad's box along some
    # axis, padded against unpadded.  The disc's box r sqrt(a_c^2 + b_c^2) is narrower than the quad's 3 (|a_c| + |b_c|) only where a_c and b_c are
    # comparable: a needle (|b| = 0.02 |a|) of opacity 0.36 .. 0.5 has 3 < r <= 3.12 and a disc box WIDER than its quad on every axis, so the
    # reference itself says there is nothing to tighten.  Left out are exactly those: surfels whose reference box is not smaller than the quad's box by
    # more than the margins of the tightness bound above on any axis (a handful of needles per 256).
    he0 = br.disc_half_extent(v, o, 0.0)[0]
    tlo, thi, _ = br.contributing_box(v, o, 0.0)
    can = ((qhi - qlo) - (thi - tlo) > 2 * (3e-4 * he0 + 2 * br.pad(tlo, thi))).any(axis=1)
    low = (np.asarray(o, np.float64).reshape(-1) <= 0.5) & ((a != 0) & (b != 0)).all(axis=1)
    smaller = ((hi - lo) < (qhi - qlo)).any(axis=1)
    if need_tightened:
        assert (low & can).sum() >= 0.4 * P and (low & ~can).sum() <= 0.02 * P
    assert smaller[low & can].all()
    return int(cm.sum()), int(col.sum())


def _check_all(test, flat, v, o, need_tightened=False):
    P = v.shape[0] // 4
    br.check_tree(flat, P)
    lo, hi = br.leaf_boxes(flat, P)
    return _check_leaf_boxes(test, lo, hi, v, o, need_tightened)


@pytest.mark.parametrize("P,clustered", [(1, False), (2, False), (3, False), (63, False), (64, False), (65, False), (4095, False), (4096, False), (4097, False),
                                         (8193, False), (20000, False), (20000, True), (777, True)])
def test_tightened_tree_structure_and_leaf_boxes(P, clustered):
    """(a) + (b) at the sizes of the three-tier table: the 64-leaf window, the 64-block level, the 4096-leaf super-block."""
    g, v = _scene(P, SEED + P, clustered)
    flat = _build(v, g["opacities"]).cpu().numpy()
    _check_all("bvh_tightened", flat, v, g["opacities"], need_tightened=P >= 256)


@pytest.mark.parametrize("P", [2, 300, 4097])
def test_every_leaf_collapsed(P):
    """No surfel can contribute (the mix of values at and below 1/255, zero, negative, NaN): every leaf is a padded point and the tree is still a tree."""
    g, v = _scene(P, SEED)
    o = np.resize(np.array(br.EDGE_OPACITIES, np.float32), P)
    flat = _build(v, o).cpu().numpy()
    n_contrib, n_col = _check_all("bvh_tightened.all_collapsed", flat, v, o)
    assert n_contrib == 0 and n_col == P


@pytest.mark.parametrize("P", [2, 65, 4097, 9000])
def test_refit_equals_build(P):
    """(c) envgs_bvh_refit runs quad_box from st_table<1>, a build from quad_boxes: the same function, so the same boxes bit for bit -- over moved
    vertices and shuffled opacities, and after the 0.01 opacity reset."""
    g, v = _scene(P, SEED + P, clustered=P == 9000)
    first = _build(v, g["opacities"])
    topo0, order0 = br.topology_words(first.cpu().numpy(), P)
    g2, v2 = _moved(g, SEED + 1)
    for name, vv, oo in (("moved", v2, g2["opacities"]), ("reset", v2, np.full(P, 0.01, np.float32)), ("reset_in_place", v, np.full(P, 0.01, np.float32))):
        refit = _build(vv, oo, refit=first)
        assert refit.data_ptr() != first.data_ptr()
        flat = refit.cpu().numpy()
        topo, order = br.topology_words(flat, P)
        assert np.array_equal(topo, topo0) and np.array_equal(order, order0), name
        _check_all("bvh_tightened.refit." + name, flat, vv, oo)
        fresh = _build(vv, oo).cpu().numpy()
        lo_r, hi_r = br.leaf_boxes(flat, P)
        lo_b, hi_b = br.leaf_boxes(fresh, P)
        assert np.array_equal(lo_r.view(np.int32), lo_b.view(np.int32)) and np.array_equal(hi_r.view(np.int32), hi_b.view(np.int32)), \
            "%s: refit and build disagree on a leaf box" % name


def _quality(nodes, P):
    from envgs_amd import _lib
    lib = _lib.load()
    out = torch.full((2,), -1.0, dtype=torch.float32, device=nodes.device)
    _lib.check(lib.envgs_bvh_quality(P, _lib.ptr(nodes), _lib.ptr(out), tracing._stream(nodes.device)), "envgs_bvh_quality")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


def _host_quality(flat, P):
    """The kernel's rules in float64: per binary node the half-areas of both child boxes (extents clamped at 0, a node's term dropped when it is
    >= 1e30 or NaN); the root's half-area from the union of its two child boxes."""
    _, boxes, _, _ = br.split_tree(flat, P)
    bx = boxes.astype(np.float64)
    e = np.maximum(bx[:, :, 1] - bx[:, :, 0], 0.0)                    # (node, side, xyz)
    term = (e[:, :, 0] * e[:, :, 1] + e[:, :, 1] * e[:, :, 2] + e[:, :, 2] * e[:, :, 0]).sum(axis=1)
    term = np.where(term < 1e30, term, 0.0)
    r = np.maximum(bx[0, 0, 1], bx[0, 1, 1]) - np.minimum(bx[0, 0, 0], bx[0, 1, 0])
    return float(term.sum()), float(r[0] * r[1] + r[1] * r[2] + r[2] * r[0])


@pytest.mark.parametrize("P", [2, 1000, 20000])
def test_bvh_quality_against_the_host(P):
    """(d) the measure that steers SurfelTracer's build-or-refit policy.  out[0]: an fp32 sum of n non-negative terms errs by at most (n - 1) 2^-24
    relative in any order; the chain of one atomic per 256-node workgroup is the longest one: (P / 256 + 16) 2^-23 with the terms' own rounding."""
    g, v = _scene(P, SEED + P)
    built = _build(v, g["opacities"])
    g2, v2 = _moved(g, SEED + 2)
    refit = _build(v2, g2["opacities"], refit=built)
    for name, nodes in (("build", built), ("refit", refit)):
        got = _quality(nodes, P)
        want = _host_quality(nodes.cpu().numpy(), P)
        assert want[0] > 0 and want[1] > 0
        e0, e1 = abs(got[0] - want[0]) / want[0], abs(got[1] - want[1]) / want[1]
        record("bvh_quality." + name, "area_sum_rel_err/bound", e0 / ((P / 256 + 16) * 2.0 ** -23), "(P = %d)" % P)
        record("bvh_quality." + name, "root_area_rel_err/bound", e1 / (4 * 2.0 ** -23), "(P = %d)" % P)
        assert e0 <= (P / 256 + 16) * 2.0 ** -23, (name, got, want)
        assert e1 <= 4 * 2.0 ** -23, (name, got, want)


# ---- (e) no hit lost at the contribution boundary, end to end -----------------------------------------------------------------------------------
_AUDITS = {}


def _ray_case(kind, delta):
    """The P = 256 scene, its boundary (or axis-parallel) rays and the oracle's audit of them: computed once, shared, never modified."""
    key = (kind, delta)
    if key not in _AUDITS:
        from oracle import trace as otr
        g, v = _scene()
        g["colors_precomp"] = np.random.default_rng(SEED + 5).uniform(0.0, 1.0, (256, 3)).astype(np.float32)
        rng = np.random.default_rng(SEED + 1)
        if kind == "boundary":
            ro, rd, tid = br.boundary_rays(v, g["opacities"], delta, rng)
            along = np.ones(len(tid), bool)
        elif kind == "centre":
            _, contributes = br.radius2(g["opacities"])
            ro, rd, tid = br.centre_rays(v, np.nonzero(~contributes)[0], rng)
            along = np.ones(len(tid), bool)
        else:
            ro, rd, tid, along = br.axis_rays(v, g["opacities"], delta, rng)
        a = otr.trace_audit(ro, rd, g["means3D"], g["scales"], g["rotations"], g["opacities"], start_from_first=False)
        _AUDITS[key] = (g, v, ro, rd, tid, along, a)
    return _AUDITS[key]


def _settings(dev):
    import diff_surfel_tracing as mod
    I = torch.eye(4, device=dev)
    return mod.SurfelTracingSettings(image_height=1, image_width=1, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=I,
                                     projmatrix=I, sh_degree=torch.tensor([0], device=dev), campos=torch.zeros(3, device=dev), prefiltered=False,
                                     debug=False, max_trace_depth=0, specular_threshold=0.0)


def _trace(nodes, g, ro, rd, use_lists):
    dev = nodes.device
    t = lambda x: torch.from_numpy(x).to(dev)
    outs, _ = tracing.trace_forward(nodes, t(ro), t(rd), t(g["means3D"]), None, t(g["colors_precomp"]), None, t(g["opacities"]).reshape(-1, 1), t(g["scales"]),
                                    t(g["rotations"]), _settings(dev), False, use_lists=use_lists, need_grad=False)
    torch.cuda.synchronize()
    return outs


def _check_lists(test, nodes, case, hit=True):
    """List path: every non-fragile ray's composited (front-to-back) id list == the oracle's, exactly; the target is in it (hit=False: the targets
    are surfels that can never contribute -- in NO ray's list, fragile or not)."""
    g, v, ro, rd, tid, along, a = case
    old = tracing.KEEP_LISTS["on"]
    tracing.KEEP_LISTS["on"] = True
    try:
        _trace(nodes, g, ro, rd, True)
        ids, _, n_used, hit_cnt = [x.cpu().numpy() for x in tracing.last_hit_lists()]
    finally:
        tracing.KEEP_LISTS["on"] = old
    cap = ids.shape[1]
    assert (hit_cnt <= cap).all(), "a ray was not served by the list path"
    ok = ~a["fragile"]
    record_fragile(test, "fragile_rays", a["fragile"], FRAGILE_RAYS_MAX)
    np.testing.assert_array_equal(n_used[ok], a["nhit"][ok])
    w = int(a["nhit"][ok].max(initial=0))
    assert w <= cap
    valid = np.arange(w)[None] < a["nhit"][:, None]
    got = np.where(valid, ids[:, :w], -1); want = np.where(valid, a["ids"][:, :w], -1)
    np.testing.assert_array_equal(got[ok], want[ok])
    aimed = ok & along
    if hit:
        assert ((got == tid[:, None]) & valid).any(axis=1)[aimed].all(), "a ray aimed inside the contribution boundary lost its target"
    else:
        listed = np.where(np.arange(cap)[None] < n_used[:, None], ids, -1)
        assert not np.isin(listed, np.unique(tid)).any(), "a surfel that can never contribute was composited"
    record(test, "hit_lists_bit_exact", 0.0, "(%d rays, %d composited ids compared, %d aimed targets found)" % (int(ok.sum()), int(a["nhit"][ok].sum()), int(aimed.sum())))


@pytest.mark.parametrize("delta", [1e-2, 3e-3])
def test_boundary_hits_list_path(delta):
    case = _ray_case("boundary", delta)
    g, v = case[0], case[1]
    _check_lists("bvh_tightened.boundary_lists.delta%g" % delta, _build(v, g["opacities"]), case)


@pytest.mark.parametrize("delta", [1e-2, 3e-3])
def test_boundary_hits_refitted_tree(delta):
    """The tree most training steps trace: built over OTHER vertices and opacities, refitted to the scene's."""
    case = _ray_case("boundary", delta)
    g, v = case[0], case[1]
    g0, v0 = _moved(g, SEED + 3)
    nodes = _build(v, g["opacities"], refit=_build(v0, g0["opacities"]))
    _check_lists("bvh_tightened.boundary_lists_refit.delta%g" % delta, nodes, case)


@pytest.mark.parametrize("delta", [1e-2, 3e-3])
def test_boundary_hits_kbuffer_path(delta):
    """use_lists=False walks the BINARY nodes: colour and accumulated alpha against the oracle on the non-fragile rays, at the suite's tolerance.

    The needles of the scene, seen from 2 to 6 units away, are what this is sensitive to: v = b.(o + t d - mu) / s_v with s_v ~ 2e-4 magnifies one ulp
    of |t d| to 1e-3 of alpha.  While hit_surfel left o + t d to FMA contraction and the oracle did not, this check failed on the MI355X (rgb / acc
    2.13e-4 / 2.20e-4 at delta = 1e-2, 1.12e-4 / 9.95e-5 at 3e-3, one or two single needle hits each; a host emulation of both orders reproduces
    2.20e-4 and 3.7e-7).  The hit point is now evaluated in the oracle's order, like the hit distance: 5.6e-7 / 4.7e-7 at both deltas."""
    from oracle import trace as otr
    g, v, ro, rd, tid, along, a = _ray_case("boundary", delta)
    outs = _trace(_build(v, g["opacities"]), g, ro, rd, False)
    ref = otr.trace_forward(ro, rd, g["means3D"], g["scales"], g["rotations"], g["opacities"], colors_precomp=g["colors_precomp"], bg=np.zeros(3, np.float32),
                            start_from_first=False)
    ok = ~a["fragile"]
    test = "bvh_tightened.boundary_kbuffer.delta%g" % delta
    record_fragile(test, "fragile_rays", a["fragile"], FRAGILE_RAYS_MAX)
    nfr = int(a["fragile"].sum())
    failed = []
    for name, got, want in (("rgb", outs[0].cpu().numpy(), ref["rgb"]), ("acc", outs[2].cpu().numpy().reshape(-1), ref["acc"])):
        try:                                                          # (both tensors are measured and recorded before the first one fails the test)
            check_close(test, name, got[ok], want[ok], tol=TOL, excluded=nfr)
        except AssertionError as e:
            print(e)
            failed.append(str(e))
    assert not failed, "\n".join(failed)


def test_rays_through_collapsed_leaves_composite_nothing_of_them():
    """Rays through the centres of the surfels whose leaves are collapsed (opacity at or below 1/255, zero, negative, NaN): the traversal reaches
    them, so their hit test runs, and it must refuse them -- over the tightened tree and over the plain one, where the whole quad is reachable.
    (A NaN opacity used to pass the hit test's clamp `a < 0.99 ? a : 0.99` as alpha = 0.99: composited on the few rays through a collapsed leaf,
    and on every ray through the quad without tightening or in the oracle; it is now culled where the surfel records are built.)"""
    case = _ray_case("centre", 0.0)
    g, v, tid = case[0], case[1], case[4]
    assert np.isnan(g["opacities"][tid]).any() and (g["opacities"][tid] < 0).any() and len(tid) >= 4 * 8
    _check_lists("bvh_tightened.centre_lists", _build(v, g["opacities"]), case, hit=False)
    _check_lists("bvh_tightened.centre_lists_plain", tracing.build_bvh(torch.from_numpy(v).cuda())[0], case, hit=False)


def _outputs(nodes, case, use_lists):
    g, v, ro, rd = case[:4]
    old = tracing.KEEP_LISTS["on"]
    tracing.KEEP_LISTS["on"] = True
    try:
        outs = _trace(nodes, g, ro, rd, use_lists)
        res = [outs[0].cpu().numpy(), outs[2].cpu().numpy()]
        if use_lists:
            ids, _, n_used, hit_cnt = [x.cpu().numpy() for x in tracing.last_hit_lists()]
            res += [np.where(np.arange(ids.shape[1])[None] < n_used[:, None], ids, -1), n_used, hit_cnt]
    finally:
        tracing.KEEP_LISTS["on"] = old
    return res


@pytest.mark.parametrize("kind,delta", [("boundary", 1e-2), ("boundary", 3e-3), ("axis", 1e-2), ("centre", 0.0)])
def test_tightening_changes_no_output(kind, delta):
    """"Tighter boxes, identical results": over the tightened tree, and over a tree refitted to it, BOTH paths return bit for bit what they return
    over the untightened tree (build_bvh without opacities) -- every ray, the fragile ones included, colour, accumulated alpha and the composited
    lists.  (The same kernels evaluate the same hits, so nothing is rounded differently: any difference is a hit the boxes lost -- or one that only some trees let through: the
    NaN-opacity surfel, collapsed by quad_box but accepted by the hit test at alpha = 0.99 until it was culled from the surfel records, put one
    ray of 1416 off by 0.92 between the two trees.)"""
    case = _ray_case(kind, delta)
    g, v = case[0], case[1]
    plain, n = tracing.build_bvh(torch.from_numpy(v).cuda())
    g0, v0 = _moved(g, SEED + 3)
    trees = dict(tightened=_build(v, g["opacities"]), refitted=_build(v, g["opacities"], refit=_build(v0, g0["opacities"])))
    for use_lists in (True, False):
        want = _outputs(plain, case, use_lists)
        for name, nodes in trees.items():
            got = _outputs(nodes, case, use_lists)
            for x, y in zip(got, want):
                assert np.array_equal(x.view(np.int32), y.view(np.int32)), (name, use_lists)


def test_axis_parallel_rays_list_path():
    """Directions exactly along +-x, +-y, +-z (an infinite inverse direction on two axes of the slab test) through the boundary targets of the
    axis-aligned surfels, whose leaf boxes have zero thickness before the pad."""
    case = _ray_case("axis", 1e-2)
    g, v = case[0], case[1]
    assert len(case[4]) >= 6 * 4 * 20
    _check_lists("bvh_tightened.axis_parallel_lists", _build(v, g["opacities"]), case)
