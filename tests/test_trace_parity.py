"""GPU parity: the HIP LBVH tracer (through the C-ABI and the drop-in SurfelTracer) against the brute-force CPU oracle.

Bar (BASELINE.json north_star): bit-exact index work, <= 1e-4 on values and gradients -- applied per ELEMENT (tests/util.py:check_close).
Threshold / ordering flips are separated from arithmetic error instead of being absorbed by a tolerance: the oracle's audit
(oracle/surfel_trace_oracle.c:trc_audit) marks the FRAGILE rays, whose hit set or termination hangs on a threshold inside fp32 noise.  Every ray is
traced, and then
  * on a non-fragile ray the sorted per-ray hit-id list the GPU composited must equal the brute-force list bit for bit (index parity),
  * on a fragile ray that list may differ from brute force only in decisions the audit itself marks ambiguous (tests/trace_lists.py:
    validate_gpu_list), and the oracle replays the GPU's list (oracle/trace.py: forced=),
  * every output, the per-surfel weights and every gradient must be within 1e-4 elementwise, fragile rays included (_parity)."""
import math

import numpy as np
import pytest
import torch

from envgs_amd import synth
from tests.test_oracle_trace import trace_scene, FRAME_ROUND_TRIP
from tests.trace_lists import validate_gpu_list, replay_rows, fragile_scene
from tests.util import check_close, record, record_fragile, FRAGILE_RAYS_MAX, CLAMP_RAYS_MAX

pytestmark = pytest.mark.gpu


def _settings(mod, bg, deg, dev, depth=0, thr=0.0, H=1, W=1, scale_modifier=1.0):
    I = torch.eye(4, device=dev)
    return mod.SurfelTracingSettings(image_height=H, image_width=W, tanfovx=1.0, tanfovy=1.0, bg=bg.to(dev), scale_modifier=scale_modifier,
                                     viewmatrix=I, projmatrix=I, sh_degree=torch.tensor([deg], device=dev), campos=torch.zeros(3, device=dev),
                                     prefiltered=False, debug=False, max_trace_depth=depth, specular_threshold=thr)


def _run_hip(g, ro, rd, bg, deg, use_sh, sff, grads=None, depth=0, thr=0.0, shape=None, others=True, scale_modifier=1.0, quad_modifier=None):
    """quad_modifier: what the scales are multiplied by for the BVH's 3-sigma quads (default: scale_modifier, so that the quads are those of the surfels
    the kernel and the oracle evaluate).  The reference caller builds them from the unmodified scales (optix_utils.py:39-69 next to :110): with a modifier
    below 1 they are larger than needed and every hit is still found -- that is a case of test_trace_forward_backward_vs_oracle.  The reverse, a modifier
    ABOVE 1 over unmodified quads, is not asserted anywhere: the quads are then smaller than the modified surfels, so whatever part of a surfel's
    3-sigma extent lies outside its quad is not found by the traversal and the image differs from the brute-force oracle's; the reference's extension
    sources are not available to say that it does otherwise."""
    ctx = _hip_forward(g, ro, rd, bg, deg, use_sh, sff, depth=depth, thr=thr, shape=shape, others=others, scale_modifier=scale_modifier, quad_modifier=quad_modifier)
    return _hip_backward(ctx, grads)


def _hip_forward(g, ro, rd, bg, deg, use_sh, sff, depth=0, thr=0.0, shape=None, others=True, scale_modifier=1.0, quad_modifier=None):
    """The forward half of _run_hip: (outs, L, o, d, g3), synchronised -- the hit lists can be read (tracing.last_hit_lists) before the upstream gradients
    of _hip_backward are chosen."""
    import diff_surfel_tracing as mod
    dev = torch.device("cuda:0")
    L = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities")}
    if others: L["others"] = g["others"].to(dev).requires_grad_(True)
    if use_sh: L["shs"] = g["shs"].to(dev).requires_grad_(True)
    else: L["colors_precomp"] = g["colors_precomp"].to(dev).requires_grad_(True)
    o = ro.to(dev).requires_grad_(True); d = rd.to(dev).requires_grad_(True)
    oo, dd = (o, d) if shape is None else (o.reshape(shape + (3,)), d.reshape(shape + (3,)))
    v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach() * (scale_modifier if quad_modifier is None else quad_modifier), L["rotations"].detach())
    tracer = mod.SurfelTracer()
    tracer.build_acceleration_structure(v.detach().clone(), f.detach().clone(), rebuild=True)
    g3 = torch.zeros_like(L["means3D"], requires_grad=True) + 0
    g3.retain_grad()
    outs = tracer(oo, dd, v, means3D=L["means3D"], grads3D=g3, shs=L.get("shs"), colors_precomp=L.get("colors_precomp"),
                  others_precomp=L.get("others"), opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"],
                  cov3D_precomp=None, tracer_settings=_settings(mod, bg, deg, dev, depth, thr, scale_modifier=scale_modifier), start_from_first=sff)
    torch.cuda.synchronize()
    return outs, L, o, d, g3


def _hip_backward(ctx, grads=None):
    """The backward half: <outputs, grads> backpropagated (grads None: nothing); returns the forward's tuple."""
    outs, L, o, d, g3 = ctx
    dev = o.device
    if grads is not None:
        rgb, dpt, acc, norm, dist, aux, mid, wet = outs
        R = o.shape[0]
        loss = sum((x.reshape(R, -1) * y.to(dev).reshape(R, -1)).sum() for x, y in zip((rgb, dpt, acc, norm, aux), grads))
        loss.backward()
    torch.cuda.synchronize()
    return outs, L, o, d, g3


def _np(g, k):
    return g[k].numpy()


def _drop_fragile(test, g, ro, rd, sff, others=True, max_frac=FRAGILE_RAYS_MAX, sh_degree=None, scale_modifier=1.0):
    """The oracle's audit of the stage: returns the non-fragile rays and their brute-force sorted hit-id lists."""
    from oracle import trace as otr
    a = otr.trace_audit(ro.numpy(), rd.numpy(), _np(g, "means3D"), _np(g, "scales"), _np(g, "rotations"), _np(g, "opacities"),
                        others=_np(g, "others") if others else None, start_from_first=sff, scale_modifier=scale_modifier,
                        shs=(g["shs"].float().numpy() if sh_degree is not None else None), sh_degree=(sh_degree or 0))
    keep = ~a["fragile"]
    record_fragile(test, "fragile_rays", a["fragile"], max_frac)
    k = torch.from_numpy(keep)
    return ro[k].contiguous(), rd[k].contiguous(), (a["ids"][keep], a["tbits"][keep]), a["nhit"][keep], int(a["fragile"].sum())


def _check_index_parity(test, ids_ref, nhit_ref, lists, rays=None):
    """Index work is bit-exact: the GPU's sorted, composited hit-id list of every ray served by the list path == the brute-force list.
    lists: _read_lists(); rays: the (non-fragile) rays to compare, default all."""
    if lists is None:
        return 0
    ids, tb, n_used, hit_cnt = lists
    ids_ref, _ = ids_ref
    cap = ids.shape[1]
    served = hit_cnt <= cap
    listed = served if rays is None else served & rays
    np.testing.assert_array_equal(n_used[listed], nhit_ref[listed])
    valid = (np.arange(cap)[None] < n_used[:, None])[listed]
    w = min(cap, ids_ref.shape[1])
    assert nhit_ref[listed].max(initial=0) <= w
    np.testing.assert_array_equal(np.where(valid, ids[listed], -1)[:, :w], ids_ref[:, :w][listed])                    # the same surfels, in the same order
    # (word 0 of a list entry holds the hit distance only until the composite pass replaces it by the blend weight, so the distances
    #  themselves are not comparable here; identical ORDER of identical ids for every ray is what their bit-exactness buys)
    record(test, "hit_lists_bit_exact", 0.0, "(%d rays, %d composited (t, id) pairs compared)" % (int(listed.sum()), int(n_used[listed].sum())))
    return int(served.sum())


GRADS_ALL = ("dmeans3D", "grads3D", "dscales", "drots", "dopacities", "dothers", "dcolor", "dray_o", "dray_d")


def _read_lists():
    """The kept hit lists of the most recent forward as numpy, or None when the list path did not run."""
    from envgs_amd import tracing
    L = tracing.last_hit_lists()
    return None if L is None else [x.cpu().numpy() for x in L]


def _audit_fragile_lists(test, a, lists, g, ro, rd, sff, others, sh_degree, scale_modifier):
    """Steps 4 of _parity: every fragile ray the GPU served from a list is validated against the audit's candidates and ambiguous set (a rejected list
    is a kernel bug: ListRejected names the ray and both lists).  Returns (forced = (ids, n, mask) over all rays, left_out (R,) bool, kinds (R,) u8
    = the audit's kinds of the natural list or-ed with those of the replay under the GPU's list, number of ambiguous decisions taken differently)."""
    R = ro.shape[0]
    frag = a["fragile"]
    kinds = a["kind"].copy()
    left_out = np.zeros(R, bool)
    if lists is None:
        return None, frag.copy(), kinds, 0
    ids, tb, n_used, hit_cnt = lists
    cap = ids.shape[1]
    listed = hit_cnt <= cap
    have = np.array([c is not None for c in a["cand"]])
    val = frag & listed & ~a["amb_overflow"] & have
    left_out = frag & ~val
    fr = np.nonzero(val)[0]
    flipped = 0
    if fr.size:
        gl = [[int(x) for x in ids[r, :n_used[r]]] for r in fr]
        rows, a2 = replay_rows((ro.numpy()[fr], rd.numpy()[fr]), gl, (_np(g, "means3D"), _np(g, "scales"), _np(g, "rotations"), _np(g, "opacities")),
                               others=_np(g, "others") if others else None, start_from_first=sff, scale_modifier=scale_modifier,
                               shs=(g["shs"].float().numpy() if sh_degree is not None else None), sh_degree=(sh_degree or 0))
        for r, row, G in zip(fr, rows, gl):
            flipped += validate_gpu_list(row, G, ray=int(r))
        kinds[fr] |= a2["kind"]
    f_ids = np.where(np.arange(cap)[None] < n_used[:, None], ids, -1).astype(np.int32)
    record(test, "fragile.lists_validated", float(fr.size), "(fragile rays served from a list, each list legitimate under the audit's ambiguous decisions; %d such "
           "decisions taken differently from the float oracle)" % flipped)
    return (f_ids, n_used.astype(np.int32), val), left_out, kinds, flipped


def _parity(test, g, ro, rd, bg, deg, use_sh, sff, gr_scale=1.0, seed=9, which=GRADS_ALL, others=True, hip_ctx=None, require_lists=True,
            zero_geo_grads=False, after_hip=None, scale_modifier=1.0, quad_modifier=None, all_listed=False):
    """Audit -> HIP forward on ALL rays -> index parity (non-fragile rays) and list validation (fragile rays) -> HIP backward -> oracle forward + backward
    with the fragile rays forced to the GPU's validated lists -> the 1e-4 contract on every output and gradient, fragile rays included.

    Two kinds of ray cannot be fully replayed; their upstream gradients are zeroed on both sides before the backward:
      * colour-clamp-fragile rays (a blended SH colour channel within rounding of zero: the clamp decision is in no list and flips that hit's whole SH
        gradient): dL_drgb only; everything else of the ray, its forward rgb included, is compared.  At most CLAMP_RAYS_MAX of the rays.
      * left-out rays (fragile, and served by the K-buffer kernels, so that there is no list to read -- or with more ambiguous surfels than the audit
        keeps): every upstream gradient; their forward values are not compared, and `wet` only over the surfels outside their candidate sets.  Exactly 0
        where every ray is list-served (all_listed=True asserts that they are); at most FRAGILE_RAYS_MAX where a test exceeds the list capacity.
    The fragile rays' own rows are also recorded apart (`fragile.<tensor>`; for a per-surfel tensor: the surfels the fragile rays composited)."""
    from oracle import trace as otr
    from envgs_amd import tracing
    sh_degree = deg if use_sh else None
    a = otr.trace_audit(ro.numpy(), rd.numpy(), _np(g, "means3D"), _np(g, "scales"), _np(g, "rotations"), _np(g, "opacities"),
                        others=_np(g, "others") if others else None, start_from_first=sff, scale_modifier=scale_modifier,
                        shs=(g["shs"].float().numpy() if use_sh else None), sh_degree=(sh_degree or 0), detail=True)
    frag = a["fragile"]
    nfr = int(frag.sum())
    R = ro.shape[0]
    gen = torch.Generator().manual_seed(seed)
    gr = [torch.randn(R, 3, generator=gen) * gr_scale, torch.randn(R, generator=gen) * gr_scale, torch.randn(R, generator=gen) * gr_scale,
          torch.randn(R, 3, generator=gen) * gr_scale, torch.randn(R, 2, generator=gen) * gr_scale]
    if zero_geo_grads:
        gr[1:] = [torch.zeros(R), torch.zeros(R), torch.zeros(R, 3), torch.zeros(R, 2)]
    old_keep = tracing.KEEP_LISTS["on"]
    tracing.KEEP_LISTS["on"] = True
    try:
        if hip_ctx is not None: hip_ctx.__enter__()
        try:
            ctx = _hip_forward(g, ro, rd, bg, deg, use_sh, sff, others=others, scale_modifier=scale_modifier, quad_modifier=quad_modifier)
            lists = _read_lists()
            assert lists is not None or not require_lists, "the list path did not run"
            n_listed = _check_index_parity(test, (a["ids"], a["tbits"]), a["nhit"], lists, ~frag)
            forced, left_out, kinds, flipped = _audit_fragile_lists(test, a, lists, g, ro, rd, sff, others, sh_degree, scale_modifier)
            every_ray_listed = lists is not None and bool(np.all(lists[3] <= lists[0].shape[1]))
            assert every_ray_listed or not all_listed, "a ray was not served by the list path"
            clamp = ((kinds & otr.KIND_CLAMP) != 0) & ~left_out
            record(test, "fragile_rays", float(frag.mean()) if R else 0.0, "(%d of %d rays are fragile: traced, validated and compared with the others)" % (nfr, R))
            record_fragile(test, "fragile_rays.rgb_gradient_zeroed", clamp, CLAMP_RAYS_MAX, "(colour-clamp-fragile rays)")
            record_fragile(test, "fragile_rays.left_out", left_out, 0.0 if every_ray_listed else FRAGILE_RAYS_MAX,
                           "(fragile rays without a list or with an overflowed ambiguous set)")
            if clamp.any() or left_out.any():
                gr = [x.clone() for x in gr]
                gr[0][torch.from_numpy(clamp | left_out)] = 0
                for x in gr[1:]:
                    x[torch.from_numpy(left_out)] = 0
            outs, L, o, d, g3 = _hip_backward(ctx, gr)
            cnt = tracing.last_trace_counts()
            extra = after_hip() if after_hip is not None else None
        finally:
            if hip_ctx is not None: hip_ctx.__exit__(None, None, None)
    finally:
        tracing.KEEP_LISTS["on"] = old_keep
    assert cnt["stack_overflows"] == 0 or extra == "overflow-expected"
    rgb, dpt, acc, norm, dist, aux, mid, wet = [x.detach().cpu().numpy() for x in outs]
    ckw = dict(shs=_np(g, "shs"), sh_degree=deg) if use_sh else dict(colors_precomp=_np(g, "colors_precomp"))
    ref = otr.trace_forward(ro.numpy(), rd.numpy(), _np(g, "means3D"), _np(g, "scales"), _np(g, "rotations"), _np(g, "opacities"),
                            others=_np(g, "others") if others else None, bg=bg.numpy(), start_from_first=sff, scale_modifier=scale_modifier, forced=forced, **ckw)
    np.testing.assert_array_equal(ref["nhits"][~frag], a["nhit"][~frag])
    fv = forced[2] if forced is not None else np.zeros(R, bool)                 # the fragile rays that were validated and replayed
    np.testing.assert_array_equal(ref["nhits"][fv], forced[1][fv] if forced is not None else [])
    keep = ~left_out
    P = g["means3D"].shape[0]
    keep_p = np.ones(P, bool)                                                     # wet: not over the candidate surfels of the left-out rays
    for r in np.nonzero(left_out)[0]:
        assert a["cand"][r] is not None, "the audit kept no candidates for the left-out ray %d" % r
        keep_p[a["cand"][r]["ids"]] = False
    frag_p = np.zeros(P, bool)                                                    # the surfels the replayed fragile rays composited
    for r in np.nonzero(fv)[0]:
        frag_p[forced[0][r, :forced[1][r]]] = True
    nlo = int(left_out.sum())

    def close(nm, x, y, per_ray, **kw):
        """The contract on a tensor (left-out rays / their surfels apart), and once more on the fragile rays' own rows."""
        k_all, k_fr = (keep, fv) if per_ray else (keep_p if nm == "wet" else None, frag_p)
        check_close(test, nm, x, y, keep=k_all, excluded=nlo, **kw)
        if k_fr.any():
            check_close(test, "fragile." + nm, x, y, keep=k_fr, **kw)

    for x, y, nm in ((rgb, ref["rgb"], "rgb"), (dpt[:, 0], ref["dpt"], "dpt"), (acc[:, 0], ref["acc"], "acc"), (norm, ref["norm"], "norm"),
                     (aux, ref["aux"], "aux"), (wet[:, 0], ref["wet"], "wet")):
        if nm == "aux" and not others: continue
        close(nm, x, y, nm != "wet")
    # distortion cancels catastrophically in fp32 in any implementation of its moment form: compared with the oracle's evaluation in DOUBLE under the
    # DERIVED per-ray bound of that form's fp32 rounding (oracle/surfel_trace_oracle.c: dist64 / distb; round 6) -- no mean-acc floor
    close("dist", dist[:, 0], ref["dist64"], True, cond=np.zeros_like(ref["dist_bound"]), unc=ref["dist_bound"], k_unc=1.0)
    np.testing.assert_array_equal(mid[:, 0:3], ro.numpy())
    check_close(test, "mid.rgb", mid[:, 13:16], rgb, tol=1e-6)

    rb = otr.trace_backward(ref, *[x.numpy() for x in gr], want_cond=True)
    cd = rb["cond"]
    cond = dict(dmeans3D=cd["dmeans3D"], grads3D=cd["dmeans3D"], dscales=cd["dscales"], drots=cd["drots"], dopacities=cd["dopacities"], dothers=cd["dothers"],
                dcolor=(cd["dshs"] if use_sh else cd["dcolors"]), dray_o=cd["dray_o"], dray_d=cd["dray_d"])
    ud = rb["unc"]
    unc = dict(dmeans3D=ud["dmeans3D"], grads3D=ud["dmeans3D"], dscales=ud["dscales"], drots=ud["drots"], dopacities=ud["dopacities"], dothers=ud["dothers"],
               dcolor=(ud["dshs"] if use_sh else ud["dcolors"]), dray_o=ud["dray_o"], dray_d=ud["dray_d"])
    got = dict(dmeans3D=L["means3D"].grad, grads3D=g3.grad, dscales=L["scales"].grad, drots=L["rotations"].grad, dopacities=L["opacities"].grad.reshape(-1),
               dothers=L["others"].grad if others else None, dcolor=(L["shs"].grad if use_sh else L["colors_precomp"].grad), dray_o=o.grad, dray_d=d.grad)
    want = dict(dmeans3D=rb["dmeans3D"], grads3D=rb["dmeans3D"], dscales=rb["dscales"], drots=rb["drots"], dopacities=rb["dopacities"],
                dothers=rb["dothers"], dcolor=(rb["dshs"] if use_sh else rb["dcolors"]), dray_o=rb["dray_o"], dray_d=rb["dray_d"])
    for k in which:
        if got[k] is None or want[k] is None: continue
        # (the left-out rays carry no upstream gradient on either side: every element of every gradient is compared)
        check_close(test, k, got[k].cpu().numpy(), want[k], excluded=nlo, cond=cond[k], unc=unc[k])
        k_fr = fv if k in ("dray_o", "dray_d") else frag_p
        if k_fr.any():
            check_close(test, "fragile." + k, got[k].cpu().numpy(), want[k], keep=k_fr, cond=cond[k], unc=unc[k])
    return dict(ref=ref, rb=rb, cnt=cnt, outs=outs, n_listed=n_listed, R=R, extra=extra, got=got, inputs=(ro, rd, gr), audit=a, kinds=kinds,
                validated=fv, left_out=left_out, flipped=flipped)


_FB_CASES = [(True, True, 3, 150, 400), (False, False, 0, 150, 400), (True, False, 2, 2000, 1024), (True, False, 1, 1, 64), (False, True, 0, 40, 130)]
# scale_modifier != 1 (never run before: surfel_record, hit_geometry_grad's gw[12], gw[13] *= mod): (case, modifier, quad modifier).  The quads are
# those of the modified surfels, except in the last case, which builds them from the unmodified scales as the reference caller does (_run_hip).
# (True, False, 2, 2000, 1024) at 1.7: 53 hits per ray on average, 79 at most -- the longest lists of this test.  Fragile rays on the CPU: <= 0.5 %.
_FB_MOD_CASES = [(c, m, None) for c in _FB_CASES[:2] for m in (0.5, 1.7)] + [(_FB_CASES[2], 1.7, None), (_FB_CASES[0], 0.5, 1.0)]


@pytest.mark.parametrize("use_sh,camera,deg,P,R,scale_modifier,quad_modifier",
                         [pytest.param(*c, 1.0, None, id="-".join(str(x) for x in c)) for c in _FB_CASES] +           # (the ids from before the modifier)
                         [pytest.param(*c, m, q, id="-".join(str(x) for x in c) + "-mod%g" % m + ("-unmodified_quads" if q is not None else "")) for c, m, q in _FB_MOD_CASES])
def test_trace_forward_backward_vs_oracle(use_sh, camera, deg, P, R, scale_modifier, quad_modifier, request):
    g, ro, rd = trace_scene(P=P, R=R, seed=7, camera=camera)
    if P > 500:
        g["scales"] = g["scales"] * 0.35                       # many small surfels: deep tree, > K hits per ray for some
    res = _parity(request.node.name, g, ro, rd, torch.tensor([0.3, 0.1, 0.7]), deg, use_sh, camera, scale_modifier=scale_modifier, quad_modifier=quad_modifier,
                  all_listed=True)
    if P > 1: assert res["ref"]["nhits"].mean() > 1


class _Switch:
    """Temporarily set entries of the tracing module's switch dicts / debug switches."""
    def __init__(self, **kw): self.kw = kw
    def __enter__(self):
        from envgs_amd import tracing, _lib
        self.old = {}
        # diag=True: the diagnostic build (libenvgs_hip_diag.so: the product kernels plus the exact-math raster kernels and the LDS alignment trap)
        self.lib_kind = _lib.select("diag") if self.kw.get("diag") else None
        for k, v in self.kw.items():
            if k == "force_cap":
                self.old[k] = dict(tracing.HIT_CAP)
                if v: tracing.HIT_CAP["force"] = v
            elif k == "no_lists":
                self.old[k] = tracing.trace_forward
                orig = tracing.trace_forward
                tracing.trace_forward = lambda *a, **kk: orig(*a, **{**kk, "use_lists": False})
            elif k == "rows_per_ray": self.old[k] = dict(tracing.ROW_CAP); tracing.ROW_CAP["force_per_ray"] = v
            elif k == "compact": self.old[k] = tracing.COMPACT["on"]; tracing.COMPACT["on"] = v
            elif k == "sparse": self.old[k] = tracing.SPARSE["mode"]; tracing.SPARSE["mode"] = v
            elif k == "sparse_cap": self.old[k] = tracing.SPARSE["cap"]; tracing.SPARSE["cap"] = v
            elif k == "sparse_poison": self.old[k] = tracing.SPARSE["poison"]; tracing.SPARSE["poison"] = v
            elif k == "sparse_max":                                  # ENVGS_DBG_SPARSE: value - 1 = the largest hit count of an entry filed per hit
                lib = _lib.load(); self.old[k] = lib.envgs_debug_get(5); lib.envgs_debug_set(5, v + 1)
            elif k == "sort_rays": self.old[k] = tracing.SORT_RAYS["on"]; tracing.SORT_RAYS["on"] = v
            elif k == "debug_trace":
                lib = _lib.load(); self.old[k] = lib.envgs_debug_get(0); lib.envgs_debug_set(0, v)
    def __exit__(self, *a):
        from envgs_amd import tracing, _lib
        for k, v in self.old.items():
            if k == "force_cap": tracing.HIT_CAP.clear(); tracing.HIT_CAP.update(v)
            elif k == "no_lists": tracing.trace_forward = v
            elif k == "rows_per_ray": tracing.ROW_CAP.clear(); tracing.ROW_CAP.update(v)
            elif k == "compact": tracing.COMPACT["on"] = v
            elif k == "sparse": tracing.SPARSE["mode"] = v
            elif k == "sparse_cap": tracing.SPARSE["cap"] = v
            elif k == "sparse_poison": tracing.SPARSE["poison"] = v
            elif k == "sparse_max": _lib.load().envgs_debug_set(5, v)
            elif k == "sort_rays": tracing.SORT_RAYS["on"] = v
            elif k == "debug_trace": _lib.load().envgs_debug_set(0, v)
        if self.lib_kind is not None:
            _lib.select(self.lib_kind)


# The bounce chain at the 1e-4 contract, link by link (tests/stagewise.py): every traced call of the HIP chain is compared with the oracle on
# the chain's OWN fp32 rays and upstream gradients (bit-identical inputs, the oracle's cond / unc noise floors), the torch glue between
# the calls against the same expressions in float64 on the recorded tensors.  The whole-chain comparison with float64 autograd of the eager
# twin is kept as a DIAGNOSTIC (recorded in the error table, bounded loosely): there stage k+1 traces rays that differ by the fp32 rounding
# of stage k, which no per-element noise scale describes (round 2 asserted it at 3e-3; measured <= 1.5e-3).
BOUNCE_CHAIN_DIAGNOSTIC_BOUND = 1e-2


def _bounce_glue_f64(calls, thr, gr):
    """The glue of SurfelTracer._forward_bounces in float64 on the recorded stage outputs.  Returns (leaves per call, o0, d0, loss):
    loss = <returned outputs, gr> + sum_k>=1 <o_k, dray_o_k> + <d_k, dray_d_k> with the kernels' recorded ray gradients as upstream."""
    dd = torch.float64
    cpu = lambda t: t.detach().cpu()
    S = []
    for c in calls:
        o = c["outs"]
        S.append(dict(rgb=cpu(o[0]).to(dd).requires_grad_(True), dpt=cpu(o[1]).to(dd).requires_grad_(True), acc=cpu(o[2]).to(dd).requires_grad_(True),
                      norm=cpu(o[3]).to(dd).requires_grad_(True), aux=cpu(o[5]).to(dd).requires_grad_(True)))
    o0 = cpu(calls[0]["o_in"]).to(dd).reshape(-1, 3).requires_grad_(True); d0 = cpu(calls[0]["d_in"]).to(dd).reshape(-1, 3).requires_grad_(True)
    R = o0.shape[0]
    rays = [(o0, d0)]
    sels = []
    for k in range(len(calls) - 1):
        c = calls[k]["outs"]
        nl = cpu(c[3]).reshape(-1, 3).norm(dim=-1, keepdim=True)                     # the decisions are taken on the fp32 values, as the module does
        go = ((cpu(c[5]).reshape(-1, 2)[:, 0:1] > thr) & (cpu(c[2]).reshape(-1, 1) > 0.5) & (nl > 0.0))[:, 0]
        sel = go.nonzero(as_tuple=False)[:, 0]
        sels.append(sel)
        po, pd = rays[k][0][sel], rays[k][1][sel]
        n = S[k]["norm"].reshape(-1, 3)[sel]
        nh = n / n.norm(dim=-1, keepdim=True)
        tdep = S[k]["dpt"].reshape(-1, 1)[sel] / S[k]["acc"].reshape(-1, 1)[sel]
        rays.append((po + pd * tdep, pd - 2.0 * (pd * nh).sum(-1, keepdim=True) * nh))
    col = S[-1]["rgb"].reshape(-1, 3)
    for k in range(len(calls) - 2, -1, -1):
        prgb = S[k]["rgb"].reshape(-1, 3)
        s_ = S[k]["aux"].reshape(-1, 2)[sels[k], 0:1]
        col = prgb.index_put((sels[k],), (1.0 - s_) * prgb[sels[k]] + s_ * col)
    fin = (col, S[0]["dpt"].reshape(R), S[0]["acc"].reshape(R), S[0]["norm"].reshape(R, 3), S[0]["aux"].reshape(R, 2))
    loss = sum((x.reshape(R, -1) * y.to(dd).reshape(R, -1)).sum() for x, y in zip(fin, gr))
    for k in range(1, len(calls)):
        loss = loss + (rays[k][0] * cpu(calls[k]["o_in"].grad).to(dd)).sum() + (rays[k][1] * cpu(calls[k]["d_in"].grad).to(dd)).sum()
    return S, rays, sels, o0, d0, loss


def test_trace_bounces_true_derivative():
    """max_trace_depth = 2 through the drop-in module: images, per-stage `mid` records and weights against the C oracle's forward; EVERY
    gradient at the 1e-4 contract link by link (each traced call vs the oracle on the chain's own rays, the glue vs float64), and the whole
    chain against float64 autograd of the eager twin (oracle/eager_trace.py:trace_bounces) as a recorded diagnostic."""
    from oracle import trace as otr, eager_trace
    from tests import stagewise
    test = "bounces_depth2"
    g, ro, rd = trace_scene(P=150, R=400, seed=4, camera=True)       # 20x20 camera rays
    bg = torch.tensor([0.0, 0.0, 0.0])
    thr, depth, deg = 0.1, 2, 1
    P = 150
    # image-shaped rays: shapes follow the ray tensor
    outs, *_ = _run_hip(g, ro, rd, bg, deg, True, True, depth=depth, thr=thr, shape=(20, 20))
    rgb, dpt, acc, norm, dist, aux, mid, wet = outs
    assert rgb.shape == (20, 20, 3) and dpt.shape == (20, 20, 1) and mid.shape == (20, 20, 48) and wet.shape == (P, 1)
    # audit every stage ON THE RAYS THE HIP CHAIN TRACED (its own `mid`): stage-k hit sets, orders and bounce decisions must be determined
    args = (_np(g, "means3D"), _np(g, "scales"), _np(g, "rotations"), _np(g, "opacities"))
    hmid = mid.detach().cpu().numpy().reshape(-1, 48)
    frag = otr.trace_audit(ro.numpy(), rd.numpy(), *args, others=_np(g, "others"), start_from_first=True, bounce_thr=thr, shs=_np(g, "shs"), sh_degree=deg)["fragile"]
    ref_all = otr.trace_forward(ro.numpy(), rd.numpy(), *args, shs=_np(g, "shs"), sh_degree=deg, others=_np(g, "others"), bg=bg.numpy(),
                                max_trace_depth=depth, specular_threshold=thr, start_from_first=True)
    for k in (1, 2):
        for m_ in (hmid, ref_all["mid"]):                          # the HIP chain's rays and the oracle chain's rays of the stage
            ran = np.abs(m_[:, 16 * k + 3:16 * k + 6]).sum(-1) > 0
            a = otr.trace_audit(m_[ran, 16 * k:16 * k + 3], m_[ran, 16 * k + 3:16 * k + 6], *args, others=_np(g, "others"),
                                start_from_first=False, tmin=1e-3, bounce_thr=(thr if k < depth else None), shs=_np(g, "shs"), sh_degree=deg)
            frag[np.nonzero(ran)[0][a["fragile"]]] = True
    keep = torch.from_numpy(~frag)
    record_fragile(test, "fragile_rays", frag, FRAGILE_RAYS_MAX, "(all stages)")
    ro, rd = ro[keep].contiguous(), rd[keep].contiguous()
    R = ro.shape[0]
    gen = torch.Generator().manual_seed(12)
    gr = [torch.randn(R, 3, generator=gen), torch.randn(R, generator=gen), torch.randn(R, generator=gen), torch.randn(R, 3, generator=gen),
          torch.randn(R, 2, generator=gen)]
    with stagewise.TraceTap() as tap:
        outs, L, o, d, g3 = _run_hip(g, ro, rd, bg, deg, True, True, grads=gr, depth=depth, thr=thr)
    rgb, dpt, acc, norm, dist, aux, mid, wet = [x.detach().cpu().numpy() for x in outs]
    ref = otr.trace_forward(ro.numpy(), rd.numpy(), *args, shs=_np(g, "shs"), sh_degree=deg, others=_np(g, "others"), bg=bg.numpy(),
                            max_trace_depth=depth, specular_threshold=thr, start_from_first=True)
    assert (ref["mid"][:, 16 + 7] != 0).any() and (ref["mid"][:, 32 + 7] != 0).any()          # both bounce stages really ran for some rays
    nfr = int(frag.sum())
    check_close(test, "rgb", rgb, ref["rgb"], excluded=nfr)
    check_close(test, "mid", mid, ref["mid"], excluded=nfr)
    check_close(test, "wet", wet[:, 0], ref["wet"], excluded=nfr)                           # summed over the three stages on both sides
    # ---- link by link at 1e-4 --------------------------------------------------------------------------------------------------------
    assert len(tap.calls) == 3 and [c["sff"] for c in tap.calls] == [True, 2, 2]
    backs = []
    for k, c in enumerate(tap.calls):
        _, rb = stagewise.oracle_trace_call(test, "stage%d" % k, c, g, bg.numpy(), deg, nfr=nfr)
        backs.append(rb)
    stagewise.check_summed_param_grads(test, "sum_over_stages", L, backs, nfr=nfr)
    S, rays, sels, o0, d0, loss = _bounce_glue_f64(tap.calls, thr, gr)
    for k in (1, 2):                                                                        # the glue's forward: the rays it handed to stage k
        stagewise.glue_check(test, "glue.o_%d" % k, tap.calls[k]["o_in"], rays[k][0], floor=1.0)
        stagewise.glue_check(test, "glue.d_%d" % k, tap.calls[k]["d_in"], rays[k][1], floor=1.0)
    loss.backward()
    for k, c in enumerate(tap.calls):                                                       # the glue's backward: what it delivers to every stage output
        for i, nm in ((0, "rgb"), (1, "dpt"), (2, "acc"), (3, "norm"), (5, "aux")):
            want = S[k][nm].grad if S[k][nm].grad is not None else torch.zeros_like(S[k][nm])
            got = c["up"][i] if c["up"][i] is not None else torch.zeros_like(c["outs"][i])
            stagewise.glue_check(test, "glue.up%d.%s" % (k, nm), got, want, floor=float(want.abs().mean()) + 1e-12)
    # ... and into the original rays: leaf gradient = stage 0's kernel gradient + the glue's
    stagewise.glue_check(test, "glue.dray_o", o.grad - tap.calls[0]["o_in"].grad, o0.grad, floor=float(o0.grad.abs().mean()) + 1e-12)
    stagewise.glue_check(test, "glue.dray_d", d.grad - tap.calls[0]["d_in"].grad, d0.grad, floor=float(d0.grad.abs().mean()) + 1e-12)
    # ---- whole chain vs float64 autograd of the eager twin: diagnostic ------------------------------------------------------------------
    dd = torch.float64
    E = {k: g[k].to(dd).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "others", "shs")}
    o64 = ro.to(dd).requires_grad_(True); d64 = rd.to(dd).requires_grad_(True)
    ergb, edpt, eacc, enorm, eaux, ewet, nst = eager_trace.trace_bounces(o64, d64, E["means3D"], E["scales"], E["rotations"], E["opacities"],
                                                                          max_trace_depth=depth, specular_threshold=thr, shs=E["shs"], others=E["others"],
                                                                          sh_degree=deg, bg=bg, start_from_first=True)
    assert nst == 3
    check_close(test, "rgb.vs_f64", rgb, ergb.detach().numpy(), excluded=nfr)
    check_close(test, "wet.vs_f64", wet[:, 0], ewet.detach().numpy(), excluded=nfr)
    loss = sum((x.reshape(R, -1) * y.to(dd).reshape(R, -1)).sum() for x, y in zip((ergb, edpt, eacc, enorm, eaux), gr))
    loss.backward()
    q = g["rotations"].double()
    proj = lambda v: v - (v * q).sum(-1, keepdim=True) * q                 # drots is defined on the unit sphere: compare tangent parts
    for nm, a, b in (("dmeans3D", L["means3D"].grad, E["means3D"].grad), ("grads3D", g3.grad, E["means3D"].grad), ("dscales", L["scales"].grad, E["scales"].grad),
                     ("dopacities", L["opacities"].grad, E["opacities"].grad), ("dothers", L["others"].grad, E["others"].grad), ("dshs", L["shs"].grad, E["shs"].grad),
                     ("dray_o", o.grad, o64.grad), ("dray_d", d.grad, d64.grad)):
        check_close(test, "chain_f64_diagnostic." + nm, a.cpu().numpy(), b.numpy(), excluded=nfr, tol=BOUNCE_CHAIN_DIAGNOSTIC_BOUND)
    check_close(test, "chain_f64_diagnostic.drots", proj(L["rotations"].grad.cpu().double()).numpy(), proj(E["rotations"].grad).numpy(), excluded=nfr,
                tol=BOUNCE_CHAIN_DIAGNOSTIC_BOUND)


def test_trace_kbuffer_in_kernel_bounces_forward():
    """The C-ABI's in-kernel bounce stages (K-buffer kernels; forward use only -- the drop-in module composes stages instead)."""
    from oracle import trace as otr
    from envgs_amd import tracing
    import diff_surfel_tracing as mod
    dev = torch.device("cuda:0")
    g, ro, rd = trace_scene(P=150, R=400, seed=4, camera=True)
    bg = torch.zeros(3)
    v, f = synth.get_disks(g["means3D"], g["scales"], g["rotations"])
    nodes, P = tracing.build_bvh(v.to(dev), g["opacities"].to(dev))
    gd = {k: x.to(dev) for k, x in g.items()}
    outs, _ = tracing.trace_forward(nodes, ro.to(dev), rd.to(dev), gd["means3D"], gd["shs"], None, gd["others"], gd["opacities"], gd["scales"],
                                    gd["rotations"], _settings(mod, bg, 1, dev, 2, 0.1), True, use_lists=False, need_grad=False)
    ref = otr.trace_forward(ro.numpy(), rd.numpy(), _np(g, "means3D"), _np(g, "scales"), _np(g, "rotations"), _np(g, "opacities"), shs=_np(g, "shs"),
                            sh_degree=1, others=_np(g, "others"), bg=bg.numpy(), max_trace_depth=2, specular_threshold=0.1, start_from_first=True)
    a = otr.trace_audit(ro.numpy(), rd.numpy(), _np(g, "means3D"), _np(g, "scales"), _np(g, "rotations"), _np(g, "opacities"), others=_np(g, "others"),
                        start_from_first=True, bounce_thr=0.1)
    ok = ~a["fragile"]
    same = np.all((ref["mid"] != 0) == (outs[6].cpu().numpy() != 0), axis=1) & ok            # rays whose stages agree (later stages are not audited here)
    assert same.mean() > 0.9
    check_close("kbuffer_in_kernel_bounces", "rgb", outs[0].cpu().numpy()[same], ref["rgb"][same], excluded=int((~same).sum()))
    check_close("kbuffer_in_kernel_bounces", "mid", outs[6].cpu().numpy()[same], ref["mid"][same], excluded=int((~same).sum()))


@pytest.mark.parametrize("scale_modifier", [1.0, 1.7])
def test_trace_cov3D_precomp_matches_scales_rotations(scale_modifier):
    """pipe.compute_cov3D_python (optix_utils.py:143-154): the tracer accepts the screen-space transMat, recovers the world-space frame from
    it and traces the same image; the gradient reaches the transMat (and, through the caller's own torch expressions, its parameters).
    With scale_modifier m the caller's transMat already holds m * scales and settings.scale_modifier is m as well: frame_from_transmat's division
    and the kernel's multiplication must cancel.  That is asserted on the recovered frame itself (tests/test_oracle_trace.py:
    test_frame_from_transmat_round_trip, and here on the device) and on the image and the gradients of the frame path over m * scales.

    At 1.7 a ray has 42 hits instead of 17, and on the MI355X one ray of 512 differed by 2e-3 of its colour: the hit distance t = n.(mu - o) / n.d comes
    from the RECOVERED normal, whose fp32 rounding (asserted: quaternion within FRAME_ROUND_TRIP) exchanged two hits of that ray that are equally far away.
    No model of that noise removes rays here.  At a modifier other than 1 the rays the oracle's audit marks are dropped as everywhere else; of the others,
    the two calls' composited hit lists are compared ray by ray.  Rays with identical lists meet the bounds this test always had (the upstream gradient
    is zero on the others, in both calls).  A ray whose lists differ must differ ONLY by what the rounding of the frame can decide (two GPU
    runs are compared here, so there is no audit row to validate a list against): a symmetric difference of at most 2 entries (threshold hits), nothing listed twice,
    and every pair of common surfels that the two lists order differently must be equally far away within the distance error of a normal that is off
    by 4 FRAME_ROUND_TRIP (|dn| <= 4 |dq| for a unit quaternion):  |t_i - t_j| <= dt_i + dt_j,  dt = 4 FRAME_ROUND_TRIP (|mu - o| + |t| |d|) / |n.d|, in
    float64.  A ray that differs by threshold hits alone (same order) also has a colour within exp(-4.5) * cmax of the frame path's: the largest blend
    weight of a hit at a threshold (alpha = 1/255; |u| or |v| = 3: alpha <= 0.99 exp(-4.5) = 0.011; a terminating hit: T < 1e-4) times the largest colour
    an SH degree-2 surfel of the scene can have.  Such rays are counted and bounded by FRAGILE_RAYS_MAX.  At 1.0 the test is what it always was: every
    ray, no lists."""
    from envgs_amd import tracing
    m = scale_modifier
    test = "cov3D_precomp" + ("" if m == 1.0 else ".mod%g" % m)
    import diff_surfel_tracing as mod
    dev = torch.device("cuda:0")
    g, ro, rd = trace_scene(P=200, R=512, seed=5, camera=False)
    if m != 1.0:
        gn = dict(g, rotations=g["rotations"] / g["rotations"].norm(dim=-1, keepdim=True))
        ro, rd, _, _, _ = _drop_fragile(test, gn, ro, rd, False, others=False, sh_degree=2, scale_modifier=m)
    cam = synth.orbit_camera(1, H=64, W=80, fx=100.0)
    bg = torch.tensor([0.1, 0.2, 0.3])
    st = mod.SurfelTracingSettings(image_height=64, image_width=80, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg.to(dev), scale_modifier=m,
                                   viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev), sh_degree=torch.tensor([2], device=dev),
                                   campos=cam.camera_center.to(dev), prefiltered=False, debug=False, max_trace_depth=0, specular_threshold=0.0)
    run, lists = {}, {}
    old_keep = tracing.KEEP_LISTS["on"]
    tracing.KEEP_LISTS["on"] = m != 1.0
    try:
        for mode in ("frame", "precomp"):
            L = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
            rn = L["rotations"] / L["rotations"].norm(dim=-1, keepdim=True)                     # what get_rotation does
            v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach() * m, rn.detach())
            tracer = mod.SurfelTracer(); tracer.build_acceleration_structure(v, f, rebuild=True)
            kw = dict(means3D=L["means3D"], grads3D=None, shs=L["shs"], colors_precomp=None, others_precomp=None, opacities=L["opacities"],
                      tracer_settings=st, start_from_first=False)
            if mode == "frame":
                outs = tracer(ro.to(dev), rd.to(dev), v, scales=L["scales"], rotations=rn, cov3D_precomp=None, **kw)
            else:
                class _C: pass
                c = _C(); c.__dict__.update(cam.__dict__)
                c.world_view_transform = cam.world_view_transform.to(dev); c.full_proj_transform = cam.full_proj_transform.to(dev)
                tm = synth.transmat_python(c, L["means3D"], L["scales"], rn, scale_modifier=m)  # the caller's torch expression
                s_rec, q_rec = tracing.frame_from_transmat(tm.detach(), st)                     # what the tracer hands to the kernel
                e_s = float(((s_rec - L["scales"].detach()).abs() / L["scales"].detach()).max())
                e_q = float((q_rec * torch.sign((q_rec * rn.detach()).sum(-1, keepdim=True)) - rn.detach()).abs().max())
                record(test, "recovered_frame.scales", e_s, "(relative; bound %.0e)" % FRAME_ROUND_TRIP)
                record(test, "recovered_frame.quaternion", e_q, "(absolute, up to sign; bound %.0e)" % FRAME_ROUND_TRIP)
                assert e_s <= FRAME_ROUND_TRIP and e_q <= FRAME_ROUND_TRIP, (e_s, e_q)
                outs = tracer(ro.to(dev), rd.to(dev), v, scales=None, rotations=None, cov3D_precomp=tm, **kw)
            torch.cuda.synchronize()
            if m != 1.0:
                ids, tb, n_used, hit_cnt = [x.cpu().numpy() for x in tracing.last_hit_lists()]
                assert np.all(hit_cnt <= ids.shape[1]), "a ray was not served by the list path"
                lists[mode] = [[int(x) for x in ids[r, :n_used[r]]] for r in range(ids.shape[0])]
            run[mode] = (outs, L)
    finally:
        tracing.KEEP_LISTS["on"] = old_keep
    R = ro.shape[0]
    same = np.ones(R, bool)
    if m != 1.0:
        same = np.array([lists["frame"][r] == lists["precomp"][r] for r in range(R)])
        record_fragile(test, "rays_with_differing_hit_lists", ~same, FRAGILE_RAYS_MAX)
        rgb_f, rgb_p = run["frame"][0][0].detach().cpu().numpy(), run["precomp"][0][0].detach().cpu().numpy()
        cmax = 0.5 + 1.1 * float(g["shs"][:, :9].abs().sum(dim=(1, 2)).max())                   # |SH basis of degree <= 2| <= 1.1 on unit directions
        worst, swaps = 0, 0
        d64 = torch.float64
        nrm = synth.build_rotation(g["rotations"].to(d64))[:, :, 2]
        for r in np.nonzero(~same)[0]:
            a_, b_ = lists["frame"][r], lists["precomp"][r]
            sd = set(a_) ^ set(b_)
            worst = max(worst, len(sd))
            assert len(a_) == len(set(a_)) and len(b_) == len(set(b_)), "ray %d: a surfel is listed twice" % r
            ca, cb = [x for x in a_ if x not in sd], [x for x in b_ if x not in sd]
            if ca == cb:
                assert float(np.abs(rgb_p[r] - rgb_f[r]).max()) <= math.exp(-4.5) * cmax, (r, rgb_p[r], rgb_f[r])
                continue
            o_, d_ = ro[r].to(d64), rd[r].to(d64)
            idx = torch.tensor(ca)
            nd = nrm[idx] @ d_
            t = ((g["means3D"][idx].to(d64) - o_) * nrm[idx]).sum(-1) / nd
            dt = 4 * FRAME_ROUND_TRIP * ((g["means3D"][idx].to(d64) - o_).norm(dim=-1) + t.abs() * d_.norm()) / nd.abs()
            pos_b = {x: k for k, x in enumerate(cb)}
            for i in range(len(ca)):
                for j in range(i + 1, len(ca)):
                    if pos_b[ca[i]] > pos_b[ca[j]]:
                        swaps += 1
                        assert abs(float(t[i] - t[j])) <= float(dt[i] + dt[j]), "ray %d: surfels %d and %d change order at distances %.9g, %.9g (allowed %.3g)" % (
                            r, ca[i], ca[j], float(t[i]), float(t[j]), float(dt[i] + dt[j]))
        record(test, "differing_lists_exchanged_pairs", float(swaps), "(pairs of equally distant hits in the other order; each within its distance error)")
        assert worst <= 2, "a ray's two hit lists differ by %d entries" % worst
        record(test, "differing_lists_max_symmetric_difference", float(worst), "(%d rays; bound 2 entries)" % int((~same).sum()))
        if (~same).any():
            record(test, "differing_lists_rgb", float(np.abs(rgb_p[~same] - rgb_f[~same]).max()), "(absolute; bound exp(-4.5) * %.2f = %.3f)" % (cmax, math.exp(-4.5) * cmax))
    res = {}
    up = torch.linspace(0.5, 1.5, 3, device=dev)[None] * torch.from_numpy(same).to(dev, torch.float32)[:, None]
    for mode in ("frame", "precomp"):
        outs, L = run[mode]
        (outs[0] * up).sum().backward()
        torch.cuda.synchronize()
        res[mode] = (outs[0].detach().cpu().numpy(), {k: x.grad.cpu().numpy() for k, x in L.items()})
    assert np.abs(res["frame"][0] - bg.numpy()).max() > 0.05
    check_close(test, "rgb", res["precomp"][0][same], res["frame"][0][same], tol=2e-4, excluded=int((~same).sum()))
    for k in ("scales", "rotations", "opacities", "shs"):
        check_close(test, "d" + k, res["precomp"][1][k], res["frame"][1][k], tol=2e-3, excluded=int((~same).sum()))


def test_trace_edge_cases():
    import diff_surfel_tracing as mod
    dev = torch.device("cuda:0")
    g, ro, rd = trace_scene(P=50, R=64, seed=2, camera=False)
    bg = torch.tensor([0.2, 0.4, 0.6])
    # rays that miss everything: background, zero weight, zero gradients
    far = ro + torch.tensor([1000.0, 0, 0]); away = torch.tensor([1.0, 0, 0]).expand_as(rd).contiguous()
    outs, L, o, d, g3 = _run_hip(g, far, away, bg, 2, True, False, grads=[torch.ones(64, 3), torch.ones(64), torch.ones(64), torch.ones(64, 3), torch.ones(64, 2)])
    rgb, dpt, acc, norm, dist, aux, mid, wet = outs
    assert torch.allclose(rgb, bg.to(dev).expand_as(rgb)) and float(acc.abs().max()) == 0 and float(wet.abs().max()) == 0
    assert float(L["means3D"].grad.abs().max()) == 0 and float(o.grad.abs().max()) == 0
    # validation mirrors the reference wrapper; stale BVH after "densification" is an error, not silent garbage
    tracer = mod.SurfelTracer()
    v, f = synth.get_disks(g["means3D"], g["scales"], g["rotations"])
    tracer.build_acceleration_structure(v.to(dev), f.to(dev), rebuild=True)
    kw = dict(means3D=g["means3D"].to(dev), grads3D=None, shs=g["shs"].to(dev), colors_precomp=None, others_precomp=None,
              opacities=g["opacities"].to(dev), scales=g["scales"].to(dev), rotations=g["rotations"].to(dev), cov3D_precomp=None,
              tracer_settings=_settings(mod, bg, 0, dev), start_from_first=False)
    with pytest.raises(Exception):
        tracer(ro.to(dev), rd.to(dev), None, **{**kw, "colors_precomp": torch.rand(50, 3, device=dev)})
    with pytest.raises(Exception):
        tracer(ro.to(dev), rd.to(dev), None, **{**kw, "means3D": torch.rand(60, 3, device=dev)})
    with pytest.raises(Exception):
        tracer(ro.to(dev), rd.to(dev), None, **{**kw, "scales": None})
    # cached BVH (v=None at test time, optix_utils.py:83) under inference_mode, (1,S,3) rays
    with torch.inference_mode():
        rgb2, *_ = tracer(ro.to(dev)[None], rd.to(dev)[None], None, **kw)
    assert rgb2.shape == (1, 64, 3) and torch.isfinite(rgb2).all()


@pytest.mark.parametrize("force_cap", [12, 20, 0, 512])
def test_trace_list_path_overflow_handoff(force_cap, request):
    """Per-ray hit lists with a tiny capacity: rays that overflow must be handed to the K-buffer kernels and give the same
    result as the oracle (forward and backward); force_cap=0 disables the list path entirely."""
    g, ro, rd = trace_scene(P=600, R=512, seed=11, camera=False)
    g["scales"] = g["scales"] * 0.6
    sw = _Switch(**({"force_cap": force_cap} if force_cap else {"no_lists": True}))
    res = _parity(request.node.name, g, ro, rd, torch.tensor([0.1, 0.2, 0.3]), 3, True, False, seed=3, hip_ctx=sw, require_lists=bool(force_cap))
    if force_cap and force_cap < 100:
        assert res["cnt"]["max_list"] > force_cap                 # the overflow path really ran
        assert (res["ref"]["nhits"] <= force_cap).any() and 0 < res["n_listed"] < res["R"]          # and so did the list path


def test_trace_packet_stack_overflow_is_handed_off_not_dropped():
    """The packet traversal's wave-uniform stack is limited to 2 entries (debug switch 1024): every batch that would have dropped a subtree
    is flagged, counted, and traced by the K-buffer kernels instead -- identical results."""
    from envgs_amd import tracing
    g, ro, rd = trace_scene(P=2000, R=1024, seed=7, camera=False)
    g["scales"] = g["scales"] * 0.35
    state = {}
    def after():
        state["cnt"] = tracing.last_trace_counts()
        return "overflow-expected"
    res = _parity("packet_stack_overflow", g, ro, rd, torch.tensor([0.3, 0.1, 0.7]), 2, True, False, hip_ctx=_Switch(debug_trace=1024), after_hip=after)
    assert state["cnt"]["stack_overflows"] > 0
    record("packet_stack_overflow", "batches_handed_off", state["cnt"]["stack_overflows"])


def test_trace_baseline_size_env_set_sample_vs_oracle():
    """BASELINE env set at full size (163 840 surfels over +-50, the reference's initial fog) traced by a 3 072-ray sample of
    reflected-like rays: deep LBVH, long hit lists (termination bound, list sort), all gradients -- against the
    brute-force oracle.  The whole 640 k-ray view is covered by bench.py; the oracle needs ~10 s for this sample."""
    P, R = 163840, 3072
    e = synth.env_gaussians(P, seed=1)
    gen = torch.Generator().manual_seed(5)
    ro = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.3
    rd = torch.randn(R, 3, generator=gen); rd = rd / rd.norm(dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(R, 1, generator=gen))
    g = dict(means3D=e["means3D"], scales=e["scales"], rotations=e["rotations"], opacities=e["opacities"], shs=e["shs"],
             others=torch.rand(P, 2, generator=gen), colors_precomp=torch.rand(P, 3, generator=gen))
    res = _parity("env_set_163840_sample", g, ro, rd, torch.zeros(3), 3, True, False, gr_scale=1.0 / R, seed=6, zero_geo_grads=True,
                  which=("dmeans3D", "dscales", "drots", "dopacities", "dcolor", "dray_o", "dray_d"))
    cnt = res["cnt"]
    assert cnt["hits"] / res["R"] > 30 and cnt["max_list"] > 100            # a fog: long lists
    lo = res["left_out"]                                                     # (fragile rays the K-buffer kernels served: no list to replay)
    if not lo.any():
        assert int(res["ref"]["nhits"].sum()) == cnt["hits"]                 # the same composited hits, exactly (fragile rays: under the GPU's validated lists)
    else:                                                                    # ... up to the ambiguous decisions (and the termination) of the left-out rays
        assert abs(int(res["ref"]["nhits"].sum()) - cnt["hits"]) <= int((res["audit"]["namb"][lo] + 1).sum())


def test_trace_clustered_surfels_deep_tree():
    """Thousands of surfels packed into a tiny cluster (identical Morton prefixes -> a very deep LBVH: exercises the index tie-break of the
    Karras build) plus a sparse far set; also exact ties in t (coplanar surfels) ordered by surfel id."""
    gen = torch.Generator().manual_seed(21)
    Pc, Pf = 3000, 200
    means = torch.cat([torch.tensor([0.0, 0.0, 5.0]) + 0.02 * torch.randn(Pc, 3, generator=gen), (torch.rand(Pf, 3, generator=gen) * 2 - 1) * 30])
    means[:50] = means[0]                                              # 50 exactly coincident centres
    P = Pc + Pf
    scales = torch.cat([0.3 + 0.3 * torch.rand(Pc, 2, generator=gen), 2 + 2 * torch.rand(Pf, 2, generator=gen)])
    q = torch.randn(P, 4, generator=gen); q[:50] = q[0]                # ... and coplanar: identical t for every ray
    rots = q / q.norm(dim=-1, keepdim=True)
    opac = torch.sigmoid(torch.randn(P, 1, generator=gen) - 2.5)       # faint: long lists through the cluster
    g = dict(means3D=means, scales=scales, rotations=rots, opacities=opac, shs=torch.randn(P, 16, 3, generator=gen) * 0.3,
             others=torch.rand(P, 2, generator=gen), colors_precomp=torch.rand(P, 3, generator=gen))
    R = 512
    ro = torch.randn(R, 3, generator=gen) * 0.2
    tgt = torch.tensor([0.0, 0.0, 5.0]) + 0.3 * torch.randn(R, 3, generator=gen)
    rd = tgt - ro; rd = rd / rd.norm(dim=-1, keepdim=True)
    res = _parity("clustered_deep_tree", g, ro, rd, torch.tensor([0.2, 0.2, 0.2]), 2, True, False, seed=22,
                  which=("dmeans3D", "dopacities", "dcolor", "dray_d"))
    # (not all_listed: a ray through the cluster FINDS more than the 512 hits a fresh tracer's lists hold, although it composites ~200 of them -- on
    #  the MI355X 510 of the 512 rays are served by the K-buffer kernels, so a fragile ray here has no list to replay and is left out under
    #  FRAGILE_RAYS_MAX; the same kind of cluster with lists long enough for every ray is test_fragile_rays_differ_from_the_oracle_by_threshold_hits_only)
    assert res["ref"]["nhits"].max() > 200


def test_fragile_rays_differ_from_the_oracle_by_threshold_hits_only():
    """The deep-list scene (P = 1200, R = 4096, ~207 composited hits per ray, up to 438): about 1 % of its rays have a decision within fp32 noise of its
    threshold -- exactly the deep-list rays, where sorting, merging and termination are hardest.  They are traced WITH the others, and through
    _parity's machinery each one's composited list must pass tests/trace_lists.py:validate_gpu_list (no id twice, only candidates of the ray, in
    (t, id) order, no unambiguous hit skipped, going on and stopping legitimate at the thresholds the audit marks), and under that list the oracle's
    replay must match every output and EVERY gradient at the 1e-4 contract -- the `fragile.*` rows.  An ordering bug, a dropped or duplicated hit or a
    wrong gradient on a near-threshold ray fails here.  Every ray is list-served (1024-entry lists), so nothing may be left out."""
    from oracle import trace as otr
    test = "fragile_rays_included"
    g, ro, rd, bg, deg = fragile_scene()
    g["colors_precomp"] = torch.rand(g["means3D"].shape[0], 3, generator=torch.Generator().manual_seed(1))
    # (a fresh tracer's first call would use 512-entry lists and 192 rows per ray)
    res = _parity(test, g, ro, rd, bg, deg, True, False, seed=22, hip_ctx=_Switch(force_cap=1024, rows_per_ray=1024), all_listed=True)
    kinds, val = res["kinds"], res["validated"]
    n_geo = int((((kinds & (otr.KIND_GEOM | otr.KIND_DISAGREE)) != 0) & val).sum()); n_term = int((((kinds & otr.KIND_TERM) != 0) & val).sum())
    record(test, "fragile.validated_by_kind", float(val.sum()), "(%d geometry / alpha, %d termination, %d colour clamp; %d ambiguous decisions taken differently)" % (
        n_geo, n_term, int((((kinds & otr.KIND_CLAMP) != 0) & val).sum()), res["flipped"]))
    assert not res["left_out"].any()
    assert int(val.sum()) >= 8 and n_geo >= 1 and n_term >= 1, "the scene is meant to have list-served fragile rays of geometry and of termination kind"
    assert res["ref"]["nhits"].max() > 400


@pytest.mark.parametrize("sort_rays", [True, False])
def test_trace_batch_table_overflow_and_unsorted_rays(sort_rays, request):
    """Incoherent rays through a dense set: a 64-ray batch blends far more distinct surfels than its 1024-slot merge table holds, so part
    of the hits become single entries (filed from the top of the batch's region) -- forward weights and every gradient must still match
    the oracle; with the coherence sort disabled the cooperative collection takes the rays in the order given (the (R, cap) layouts) and feeds
    the same batch kernels."""
    from envgs_amd import tracing
    gen = torch.Generator().manual_seed(33)
    P, R = 6000, 1000                                                   # R is not a multiple of 64: a ragged last batch
    means = (torch.rand(P, 3, generator=gen) * 2 - 1) * 2.0
    scales = 0.12 + 0.1 * torch.rand(P, 2, generator=gen)
    q = torch.randn(P, 4, generator=gen)
    g = dict(means3D=means, scales=scales, rotations=q / q.norm(dim=-1, keepdim=True), opacities=torch.sigmoid(torch.randn(P, 1, generator=gen) - 2.0),
             shs=torch.randn(P, 16, 3, generator=gen) * 0.3, others=torch.rand(P, 2, generator=gen), colors_precomp=torch.rand(P, 3, generator=gen))
    ro = (torch.rand(R, 3, generator=gen) * 2 - 1) * 2.0
    rd = torch.randn(R, 3, generator=gen); rd = rd / rd.norm(dim=-1, keepdim=True)
    res = _parity(request.node.name, g, ro, rd, torch.tensor([0.1, 0.0, 0.2]), 3, True, False, seed=34, hip_ctx=_Switch(sort_rays=sort_rays, sparse="off"),
                  after_hip=tracing.last_entry_counts)
    table, singles = res["extra"]
    assert table > 0 and singles > 0, (table, singles)                 # both kinds of entries were produced
    assert table + singles <= res["cnt"]["hits"]


@pytest.mark.parametrize("case", ["camera_sh_others", "free_rays_colours", "incoherent_table_overflow", "many_small_surfels", "colour_only_vs_batch_kernel",
                                  "generic_three_forms"])
def test_trace_sparse_entries_vs_oracle(case, request):
    """Round 6: SPARSE entries (include/envgs_trace.h: sparse_hits) -- (batch, surfel) entries of at most four hits are filed per hit by the
    forward and differentiated one lane per hit (sparse_hits_bwd) instead of costing the batch kernel a 64-lane pass each.  Forced on here (the
    default passes the list only when the tracer's previous call was incoherent): every output and gradient against the oracle, with SH and
    precomputed colours, with and without `others`, the generic and the colour-only backward, and a batch whose merge table overflows (those
    one-hit entries are filed too: the batch kernel sees no singles); and the backward's forms against each other (the last two cases)."""
    from envgs_amd import tracing
    kw = dict(hip_ctx=_Switch(sparse="on", sparse_poison=SPARSE_POISON), after_hip=lambda: (tracing.last_entry_counts(), _check_sparse_list(request.node.name)))
    if case == "camera_sh_others":
        g, ro, rd = trace_scene(P=150, R=400, seed=7, camera=True)
        res = _parity(request.node.name, g, ro, rd, torch.tensor([0.3, 0.1, 0.7]), 3, True, True, **kw)
    elif case == "free_rays_colours":
        g, ro, rd = trace_scene(P=150, R=400, seed=7, camera=False)
        res = _parity(request.node.name, g, ro, rd, torch.tensor([0.3, 0.1, 0.7]), 0, False, False, others=False, which=tuple(k for k in GRADS_ALL if k != "dothers"), **kw)
    elif case == "incoherent_table_overflow":
        gen = torch.Generator().manual_seed(33)
        P, R = 6000, 1000
        means = (torch.rand(P, 3, generator=gen) * 2 - 1) * 2.0
        q = torch.randn(P, 4, generator=gen)
        g = dict(means3D=means, scales=0.12 + 0.1 * torch.rand(P, 2, generator=gen), rotations=q / q.norm(dim=-1, keepdim=True),
                 opacities=torch.sigmoid(torch.randn(P, 1, generator=gen) - 2.0), shs=torch.randn(P, 16, 3, generator=gen) * 0.3,
                 others=torch.rand(P, 2, generator=gen), colors_precomp=torch.rand(P, 3, generator=gen))
        ro = (torch.rand(R, 3, generator=gen) * 2 - 1) * 2.0
        rd = torch.randn(R, 3, generator=gen); rd = rd / rd.norm(dim=-1, keepdim=True)
        res = _parity(request.node.name, g, ro, rd, torch.tensor([0.1, 0.0, 0.2]), 3, True, False, seed=34, **kw)
        assert res["extra"][0][1] == 0, "the table-overflow singles were meant to be filed as sparse hits"
    elif case == "colour_only_vs_batch_kernel":
        # the colour-only form (the EnvGS step: only rgb carries a gradient, dpt / acc / norm / aux arrive as None): sparse entries on against off
        import diff_surfel_tracing as mod
        dev = torch.device("cuda:0")
        g, ro, rd = trace_scene(P=2000, R=1024, seed=9, camera=False)
        g["scales"] = g["scales"] * 0.35
        up = torch.randn(1024, 3, generator=torch.Generator().manual_seed(2)).to(dev)
        got = {}
        for mode in ("on", "off"):
            with _Switch(sparse=mode):
                L = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
                o = ro.to(dev).requires_grad_(True); d = rd.to(dev).requires_grad_(True)
                v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach(), L["rotations"].detach())
                tracer = mod.SurfelTracer()
                tracer.build_acceleration_structure(v, f, rebuild=True)
                outs = tracer(o, d, v, means3D=L["means3D"], grads3D=None, shs=L["shs"], colors_precomp=None, others_precomp=None, opacities=L["opacities"],
                              scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None, tracer_settings=_settings(mod, torch.zeros(3), 2, dev, 0, 0.0),
                              start_from_first=False)
                (outs[0] * up).sum().backward()
                torch.cuda.synchronize()
                got[mode] = ({k: t.grad.clone() for k, t in L.items()}, o.grad.clone(), d.grad.clone(), tracing.last_trace_counts()["sparse_hits"])
        assert got["on"][3] > 0 and got["off"][3] == 0
        for k in got["on"][0]:
            a, b = got["on"][0][k].cpu().numpy(), got["off"][0][k].cpu().numpy()
            check_close(request.node.name, k, a, b, tol=2e-5)
        check_close(request.node.name, "dray_o", got["on"][1].cpu().numpy(), got["off"][1].cpu().numpy(), tol=2e-5)
        check_close(request.node.name, "dray_d", got["on"][2].cpu().numpy(), got["off"][2].cpu().numpy(), tol=2e-5)
        return
    elif case == "generic_three_forms":
        # the GENERIC backward (SH degree 3, `others`, all five outputs carry a gradient) in its three forms on the camera_sh_others scene -- sparse
        # entries one lane per hit, every entry through the batch kernel, the K-buffer kernels -- pairwise: the two list forms evaluate the same
        # expressions from the same stored state (2e-5, as the colour-only case above), the K-buffer form sums along the ray (the 1e-4 contract)
        g, ro, rd = trace_scene(P=150, R=400, seed=7, camera=True)
        ro, rd = _drop_fragile(request.node.name, g, ro, rd, True, sh_degree=3)[:2]
        R = ro.shape[0]
        gen = torch.Generator().manual_seed(9)
        gr = [torch.randn(R, 3, generator=gen), torch.randn(R, generator=gen), torch.randn(R, generator=gen), torch.randn(R, 3, generator=gen), torch.randn(R, 2, generator=gen)]
        got = {}
        for form, sw in (("on", dict(sparse="on")), ("off", dict(sparse="off")), ("kbuffer", dict(no_lists=True))):
            with _Switch(**sw):
                _, L, o, d, _ = _run_hip(g, ro, rd, torch.tensor([0.3, 0.1, 0.7]), 3, True, True, grads=gr)
                got[form] = (dict({k: t.grad.cpu().numpy() for k, t in L.items()}, dray_o=o.grad.cpu().numpy(), dray_d=d.grad.cpu().numpy()),
                             tracing.LAST_STATS["cap"], tracing.last_trace_counts()["sparse_hits"])
        assert got["on"][1] > 0 and got["on"][2] > 0 and got["off"][1] > 0 and got["off"][2] == 0 and got["kbuffer"][1] == 0, [v[1:] for v in got.values()]
        for a, b, tol in (("on", "off", 2e-5), ("on", "kbuffer", 1e-4), ("off", "kbuffer", 1e-4)):
            for k in got[a][0]:
                mx = check_close(request.node.name, "%s_vs_%s.%s" % (a, b, k), got[a][0][k], got[b][0][k], tol=tol)
                print("generic_three_forms %s vs %s %-10s max elementwise error %.3e (tol %.0e)" % (a, b, k, mx, tol))
        return
    else:
        g, ro, rd = trace_scene(P=2000, R=1024, seed=7, camera=False)
        g["scales"] = g["scales"] * 0.35
        res = _parity(request.node.name, g, ro, rd, torch.tensor([0.3, 0.1, 0.7]), 2, True, False, zero_geo_grads=True, **kw)
    assert res["cnt"]["sparse_hits"] > 0, "no hit took the sparse path"
    assert res["cnt"]["sparse_hits"] + res["extra"][0][0] <= res["cnt"]["hits"]
    # (and, tighter: every composited hit is differentiated exactly once -- filed, a single or one hit of its entry -- _check_sparse_list)
    assert res["extra"][1][0] == res["cnt"]["sparse_hits"] and res["extra"][1][2] <= res["cnt"]["hits"]


SPARSE_POISON = -1                  # what the sparse-hit list holds before the forward (tracing.SPARSE["poison"]): no field of a written entry can be 0xFFFFFFFF


def _check_sparse_list(test, cap_req=None):
    """The sparse-hit list of the most recent forward (include/envgs_trace.h: sparse_hits) against the kept hit lists (KEEP_LISTS), after its backward:
      * counters[64] <= the capacity passed, and the backward skipped no entry (sparse_invalid == 0);
      * each of the counters[64] filed entries is a composited hit of its ray (list position below n_used, the surfel of that list slot), and no slot
        holds the poison value; no (ray, list position) and no gradient record appears twice -- over the filed hits, the (batch, surfel) entries
        and the one-hit singles together, whose record slots are exactly the call's records;
      * every composited hit is differentiated exactly once: filed, a single, or one of the hits of its (batch, surfel) entry -- whose hit count is
        the number of such hits.
    Returns (hits filed, capacity passed, composited hits)."""
    from envgs_amd import tracing
    cnt = tracing.last_trace_counts()
    rec = tracing.last_record_scratch()
    assert rec is not None and rec["sparse_hits"] is not None, "the forward was given no sparse-hit list"
    ids, _, n_used, hit_cnt = [x.cpu().numpy() for x in tracing.last_hit_lists()]
    R, cap = ids.shape
    P = int(rec["surf_cnt"].numel() // tracing.NCOPY)
    rows = rec["sparse_hits"].shape[0]
    sc = rec["sparse_cap"]
    assert sc == (rows if cap_req is None else min(cap_req, rows)), (sc, cap_req, rows)
    filed = cnt["sparse_hits"] & 0xFFFFFFFF
    record(test, "sparse_invalid", float(cnt["sparse_invalid"]), "(counters[66]; %d filed of capacity %d)" % (filed, sc))
    assert cnt["sparse_invalid"] == 0, cnt["sparse_invalid"]
    assert filed <= sc, (filed, sc)
    record(test, "sparse_filed_over_cap", filed / max(sc, 1), "(counters[64] = %d <= cap %d)" % (filed, sc))
    order = rec["ray_order"].cpu().numpy().astype(np.int64) if rec["ray_order"] is not None else np.arange(R)
    slot_of = np.empty(R, np.int64); slot_of[order] = np.arange(R)
    scnt = rec["surf_cnt"].cpu().numpy().astype(np.int64).reshape(-1)
    soff = rec["surf_off"].cpu().numpy().astype(np.int64).reshape(-1)
    n_rec = int(soff[-1]) if P > 0 else 0
    # the filed hits
    sp = rec["sparse_hits"][:filed].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert not (sp == (SPARSE_POISON & 0xFFFFFFFF)).any(), "a slot below counters[64] was never written"
    f_slot, f_k, f_sid, f_rank = sp.T
    assert (f_slot < R).all() and (f_sid < P).all()
    f_r = order[f_slot]
    assert (hit_cnt[f_r] <= cap).all() and (f_k < n_used[f_r]).all(), "a filed entry names no composited hit"
    assert (ids[f_r, f_k] == f_sid).all(), "a filed entry names the wrong surfel"
    f_key = f_r * cap + f_k
    assert np.unique(f_key).size == filed, "a (ray, list position) was filed twice"
    rec_ci, rec_rank = [f_sid * tracing.NCOPY + ((f_slot >> 6) & (tracing.NCOPY - 1))], [f_rank]
    # the (batch, surfel) entries and the singles of every batch
    ne = rec["n_entries"].cpu().numpy().astype(np.int64)
    ent = rec["entries"].reshape(-1).cpu().numpy().view(np.uint64).astype(np.uint64) if rec["entries"].dtype == torch.int64 else None
    prs = rec["pairs"].reshape(-1).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    nb = ne.shape[0]
    if rec["batch_rows"] is not None:
        br = rec["batch_rows"].cpu().numpy().astype(np.int64)
        start, region = br[:, 0], br[:, 1]
    else:
        start, region = np.arange(nb) * 64 * cap, np.full(nb, 64 * cap)
    d_b, d_sid, d_hits, s_b, s_key = [], [], [], [], []
    for b in range(nb):
        D, NF = int(ne[b, 0]), int(ne[b, 1])
        if D:
            ev = ent[start[b]:start[b] + D]
            sid = (ev & np.uint64(0xFFFFFF)).astype(np.int64)
            d_b.append(np.full(D, b)); d_sid.append(sid); d_hits.append(((ev >> np.uint64(24)) & np.uint64(0xFF)).astype(np.int64) + 1)
            rec_ci.append(sid * tracing.NCOPY + (b & (tracing.NCOPY - 1))); rec_rank.append(((ev >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.int64))
        if NF:
            top = start[b] + region[b] - 1 - np.arange(NF)
            ev, pv = ent[top], prs[top]
            sid = (ev & np.uint64(0xFFFFFF)).astype(np.int64)
            r_ = order[b * 64 + (pv >> 16)]; k_ = pv & 0xFFFF
            assert (k_ < n_used[r_]).all() and (ids[r_, k_] == sid).all(), "a single names no composited hit of its surfel"
            s_b.append(np.full(NF, b)); s_key.append(r_ * cap + k_)
            rec_ci.append(sid * tracing.NCOPY + (b & (tracing.NCOPY - 1))); rec_rank.append((ev >> np.uint64(32)).astype(np.int64))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    d_b, d_sid, d_hits, s_key = cat(d_b), cat(d_sid), cat(d_hits), cat(s_key)
    ci, rk = cat(rec_ci), cat(rec_rank)
    assert (rk < scnt[ci]).all(), "a record slot beyond its surfel's records"
    rslot = soff[ci] - scnt[ci] + rk
    assert np.unique(rslot).size == rslot.size, "a gradient record slot was handed out twice"
    assert rslot.size == n_rec and (rslot < n_rec).all(), (rslot.size, n_rec)
    assert np.unique(d_b * P + d_sid).size == d_b.size and np.unique(s_key).size == s_key.size
    # every composited hit of a listed ray, exactly once
    listed = hit_cnt <= cap
    rr = np.repeat(np.arange(R), np.where(listed, n_used, 0))
    kk = np.arange(rr.size) - np.repeat(np.cumsum(np.where(listed, n_used, 0)) - np.where(listed, n_used, 0), np.where(listed, n_used, 0))
    h_key, h_sid, h_b = rr * cap + kk, ids[rr, kk].astype(np.int64), slot_of[rr] >> 6
    in_f, in_s = np.isin(h_key, f_key), np.isin(h_key, s_key)
    dk = d_b * P + d_sid
    in_d = np.isin(h_b * P + h_sid, dk)
    cover = in_f.astype(int) + in_s.astype(int) + in_d.astype(int)
    assert (cover == 1).all(), "composited hits differentiated %d times: %d hits" % (int(cover[cover != 1][0]), int((cover != 1).sum()))
    assert in_f.sum() == filed and in_s.sum() == s_key.size
    u, c = np.unique(h_b[in_d] * P + h_sid[in_d], return_counts=True)
    srt = np.argsort(dk)
    assert np.array_equal(u, dk[srt]) and np.array_equal(c, d_hits[srt]), "an entry's hit count is not the number of its hits"
    record(test, "sparse_exactly_once", 0.0, "(%d composited hits: %d filed, %d singles, %d in %d entries)" % (h_key.size, filed, s_key.size, int(in_d.sum()), dk.size))
    return filed, sc, h_key.size


def _incoherent_scene(R, seed=33):
    """Incoherent rays through a dense set: a 64-ray batch blends more distinct surfels than its merge table holds (one-hit singles)."""
    gen = torch.Generator().manual_seed(seed)
    P = 6000
    means = (torch.rand(P, 3, generator=gen) * 2 - 1) * 2.0
    q = torch.randn(P, 4, generator=gen)
    g = dict(means3D=means, scales=0.12 + 0.1 * torch.rand(P, 2, generator=gen), rotations=q / q.norm(dim=-1, keepdim=True),
             opacities=torch.sigmoid(torch.randn(P, 1, generator=gen) - 2.0), shs=torch.randn(P, 16, 3, generator=gen) * 0.3,
             others=torch.rand(P, 2, generator=gen), colors_precomp=torch.rand(P, 3, generator=gen))
    ro = (torch.rand(R, 3, generator=gen) * 2 - 1) * 2.0
    rd = torch.randn(R, 3, generator=gen); rd = rd / rd.norm(dim=-1, keepdim=True)
    return g, ro, rd


# scene -> (scene tensors, _parity keywords, switches of every run); "contention": enough incoherent rays for TWO forward segments on two streams
# (>= 512 batches) and entries of up to 16 hits filed per hit, so that most 64-surfel chunks claim list space at once and many claims fail
SPARSE_CAP_SCENES = {
    "many_small_surfels": lambda: (_small_surfels(), dict(deg=2, bg=torch.tensor([0.3, 0.1, 0.7]), seed=9), {}),
    "incoherent_table_overflow": lambda: (_incoherent_scene(1000), dict(deg=3, bg=torch.tensor([0.1, 0.0, 0.2]), seed=34), {}),
    "contention": lambda: (_incoherent_scene(33000, seed=35), dict(deg=3, bg=torch.tensor([0.1, 0.0, 0.2]), seed=36, gr_scale=1.0 / 64), dict(sparse_max=16)),
}
_SPARSE_BASELINES = {}


def _small_surfels():
    g, ro, rd = trace_scene(P=2000, R=1024, seed=7, camera=False)
    g["scales"] = g["scales"] * 0.35
    return g, ro, rd


def _sparse_baseline(scene):
    """Per scene, once: the rays the oracle's audit keeps, and on them the sparse-off run (gradients) and the uncapped sparse-on run (hits it files)."""
    if scene in _SPARSE_BASELINES:
        return _SPARSE_BASELINES[scene]
    from envgs_amd import tracing
    (g, ro, rd), kw, sw = SPARSE_CAP_SCENES[scene]()
    ro, rd, _, _, _ = _drop_fragile("sparse_cap." + scene, g, ro, rd, False, sh_degree=kw["deg"])
    R = ro.shape[0]
    gen = torch.Generator().manual_seed(kw["seed"])
    sc = kw.get("gr_scale", 1.0)
    gr = [torch.randn(R, 3, generator=gen) * sc, torch.randn(R, generator=gen) * sc, torch.randn(R, generator=gen) * sc,
          torch.randn(R, 3, generator=gen) * sc, torch.randn(R, 2, generator=gen) * sc]
    runs = {}
    for mode in ("off", "on"):
        with _Switch(sparse=mode, **sw):
            outs, L, o, d, g3 = _run_hip(g, ro, rd, kw["bg"], kw["deg"], True, False, grads=gr)
            filed = tracing.last_trace_counts()["sparse_hits"]
        runs[mode] = (dict(rgb=outs[0], dpt=outs[1], acc=outs[2], norm=outs[3], aux=outs[5], wet=outs[7], dmeans3D=L["means3D"].grad, grads3D=g3.grad,
                           dscales=L["scales"].grad, drots=L["rotations"].grad, dopacities=L["opacities"].grad, dothers=L["others"].grad,
                           dcolor=L["shs"].grad, dray_o=o.grad, dray_d=d.grad), filed)
    assert runs["off"][1] == 0 and runs["on"][1] > 128, (scene, runs["on"][1])
    _SPARSE_BASELINES[scene] = (g, ro, rd, gr, kw, sw, {k: v.detach().cpu().numpy() for k, v in runs["off"][0].items()}, runs["on"][1])
    return _SPARSE_BASELINES[scene]


def _close_to(test, got, ref, names):
    for k in names:
        a, b = np.asarray(got[k], np.float64).reshape(-1), np.asarray(ref[k], np.float64).reshape(-1)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        err = float(np.abs(a - b).max())
        record(test, "vs_sparse_off." + k, err / (float(np.abs(b).max()) + 1e-30), "(max|a-b| / max|b|, bound 2e-5)")
        assert err <= 2e-5 * float(np.abs(b).max()) + 1e-12, (k, err)


@pytest.mark.parametrize("cap_kind", ["1", "64", "half", "uncapped_minus_1"])
@pytest.mark.parametrize("scene", list(SPARSE_CAP_SCENES))
def test_trace_sparse_list_at_every_capacity(scene, cap_kind, request):
    """The sparse-hit list when it does NOT hold every hit the forward would file (include/envgs_trace.h: sparse_hits -- the C-ABI caller's overflow
    fall-back: what finds no room takes the batch kernel).  tracing.SPARSE["cap"] passes a capacity of 1, 64, about half and one less than what the
    uncapped run of the same rays files; the list is poisoned before the forward.  Claims that do not fit must leave no hole and no overlap
    (register_hits claims by compare-and-swap: [0, counters[64]) is exactly what was filed), so: every output and gradient against the oracle at
    the 1e-4 contract, the same as the sparse-off run within 2e-5 of each tensor's largest element, and _check_sparse_list's invariants."""
    g, ro, rd, gr, kw, sw, off, n0 = _sparse_baseline(scene)
    cap = {"1": 1, "64": 64, "half": n0 // 2, "uncapped_minus_1": n0 - 1}[cap_kind]
    test = request.node.name
    res = _parity(test, g, ro, rd, kw["bg"], kw["deg"], True, False, seed=kw["seed"], gr_scale=kw.get("gr_scale", 1.0),
                  hip_ctx=_Switch(sparse="on", sparse_cap=cap, sparse_poison=SPARSE_POISON, **sw), after_hip=lambda: _check_sparse_list(test, cap))
    filed, sc, hits = res["extra"]
    assert sc == cap and filed <= cap
    # a claim is one 64-surfel chunk of a batch's entries, or the batch's table-overflow singles.  In the incoherent scenes every chunk holds more
    # than 64 hits and every batch more than 64 singles, so a capacity of 64 admits no claim there and nothing is filed -- legitimately, like 1
    if cap_kind in ("half", "uncapped_minus_1") or (cap >= 64 and scene == "many_small_surfels"):
        assert filed > 0, "nothing was filed under a capacity of %d" % cap
    assert res["R"] == ro.shape[0]
    got = {k: v.detach().cpu().numpy() for k, v in res["got"].items() if v is not None}
    got.update(rgb=res["outs"][0].detach().cpu().numpy(), dpt=res["outs"][1].detach().cpu().numpy(), acc=res["outs"][2].detach().cpu().numpy(),
               norm=res["outs"][3].detach().cpu().numpy(), aux=res["outs"][5].detach().cpu().numpy(), wet=res["outs"][7].detach().cpu().numpy())
    _close_to(test, got, off, sorted(off))


def test_trace_sparse_list_capped_colour_only_backward(request):
    """The colour-only record backward (only rgb carries an upstream gradient: the EnvGS step) with the sparse-hit list capped at about half of what
    it would file: every gradient equals the sparse-off run's within 2e-5, and _check_sparse_list's invariants hold."""
    import diff_surfel_tracing as mod
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    test = request.node.name
    g, ro, rd = _small_surfels()
    up = torch.randn(ro.shape[0], 3, generator=torch.Generator().manual_seed(2)).to(dev)
    got, n0 = {}, None
    for mode in ("off", "uncapped", "capped"):
        sw = dict(sparse="off") if mode == "off" else dict(sparse="on", sparse_poison=SPARSE_POISON, sparse_cap=(None if mode == "uncapped" else n0 // 2))
        with _Switch(**sw):
            old_keep = tracing.KEEP_LISTS["on"]
            tracing.KEEP_LISTS["on"] = True
            try:
                L = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
                o = ro.to(dev).requires_grad_(True); d = rd.to(dev).requires_grad_(True)
                v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach(), L["rotations"].detach())
                tracer = mod.SurfelTracer()
                tracer.build_acceleration_structure(v, f, rebuild=True)
                outs = tracer(o, d, v, means3D=L["means3D"], grads3D=None, shs=L["shs"], colors_precomp=None, others_precomp=None, opacities=L["opacities"],
                              scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None, tracer_settings=_settings(mod, torch.zeros(3), 2, dev, 0, 0.0),
                              start_from_first=False)
                (outs[0] * up).sum().backward()
                torch.cuda.synchronize()
                if mode == "uncapped":
                    n0 = _check_sparse_list(test)[0]
                elif mode == "capped":
                    filed, sc, _ = _check_sparse_list(test, n0 // 2)
                    assert 0 < filed <= sc == n0 // 2
            finally:
                tracing.KEEP_LISTS["on"] = old_keep
        got[mode] = {k: t.grad.detach().cpu().numpy() for k, t in L.items()} | dict(dray_o=o.grad.cpu().numpy(), dray_d=d.grad.cpu().numpy())
    assert n0 > 128
    _close_to(test, got["capped"], got["off"], sorted(got["off"]))
    _close_to(test, got["uncapped"], got["off"], sorted(got["off"]))


def test_trace_two_segment_forward_pipeline_vs_oracle():
    """Enough rays (>= 512 batches) for the forward to run as TWO batch segments on two streams (collect -> sort+composite -> register each):
    the joined result -- images, per-surfel weights, every gradient through the per-batch entries of both segments -- against the oracle."""
    from envgs_amd import tracing
    g, _, _ = trace_scene(P=1500, R=4, seed=17, camera=False)
    g["scales"] = g["scales"] * 0.5
    cam = synth.orbit_camera(3, H=192, W=192, fx=160.0, radius=1.0)                 # 36 864 coherent rays = 576 batches
    ro, rd = synth.get_rays(cam)
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    R = ro.shape[0]
    res = _parity("two_segment_pipeline", g, ro, rd, torch.tensor([0.2, 0.3, 0.1]), 3, True, False, gr_scale=1.0 / R, seed=4,
                  after_hip=tracing.last_entry_counts)
    assert (res["R"] + 63) // 64 >= 512
    assert res["extra"][0] > 0


@pytest.mark.parametrize("force_cap", [1024, 512, 320])
def test_trace_very_long_lists(force_cap, request):
    """A stack of 900 faint sheets: most rays blend several hundred hits before they terminate, so the sort / composite pass for lists beyond
    256 entries runs (8 and 16 keys per lane), and with the smaller capacities the longest rays overflow into the K-buffer path."""
    P, R = 900, 192
    gen = torch.Generator().manual_seed(21)
    means = torch.stack([torch.randn(P, generator=gen) * 0.15, torch.randn(P, generator=gen) * 0.15, 2.0 + torch.arange(P) * 0.01], dim=1)
    q = torch.tensor([1.0, 0, 0, 0]).expand(P, 4) + torch.randn(P, 4, generator=gen) * 0.05
    g = dict(means3D=means, scales=torch.full((P, 2), 0.3) + 0.3 * torch.rand(P, 2, generator=gen), rotations=q / q.norm(dim=-1, keepdim=True),
             opacities=0.02 + 0.04 * torch.rand(P, 1, generator=gen), shs=torch.randn(P, 16, 3, generator=gen) * 0.2,
             others=torch.rand(P, 2, generator=gen))
    # (SH coefficients of 0.2, not 0.3 as in the other scenes: a ray blends ~460 hits here, and with colours 0.5 +- 0.27 one ray in fifty -- 4 of these
    #  192 by the oracle's audit alone -- has a blended colour channel within rounding of the clamp at zero, twice the share of rays whose dL/drgb _parity
    #  may zero (CLAMP_RAYS_MAX).  This test is about the sort / composite pass of long lists; the clamp on deep lists is covered by the 4096 rays of
    #  test_fragile_rays_differ_from_the_oracle_by_threshold_hits_only.)
    # rays through the middle of the stack terminate after a few hundred hits, rays near its rim see falloffs below 1/255: 14 .. 712 hits
    ro = torch.cat([(torch.rand(R, 2, generator=gen) - 0.5) * 1.6, torch.zeros(R, 1)], dim=1)
    rd = torch.cat([torch.randn(R, 2, generator=gen) * 0.03, torch.ones(R, 1)], dim=1)
    res = _parity(request.node.name, g, ro, rd, torch.tensor([0.1, 0.2, 0.3]), 2, True, False, seed=23, hip_ctx=_Switch(force_cap=force_cap),
                  which=("dmeans3D", "dopacities", "dcolor", "dothers", "dray_o", "dray_d"), )
    nh = res["ref"]["nhits"]
    assert nh.max() > 512 and ((nh > 256) & (nh <= 512)).sum() > 10 and (nh <= 256).sum() > 5 and res["cnt"]["max_list"] > 512
    assert ((nh > 128) & (nh <= 192)).sum() > 0 and ((nh > 64) & (nh <= 128)).sum() > 0      # the 192-key and 128-key networks ran too


@pytest.mark.parametrize("deg,half", [(3, False), (1, False), (3, True)])
def test_trace_quad_cooperative_sh_matches_per_lane_gathers(deg, half):
    """The list path evaluates SH colours four lanes per surfel from a permuted copy of the blocks (envgs_trace.h: sh_perm); with the copy
    withheld every lane gathers its own block.  Same products, summed in a different order: the images agree to fp32 rounding."""
    from envgs_amd import tracing
    P, R = 3000, 1536
    e = synth.env_gaussians(P, seed=3)
    gen = torch.Generator().manual_seed(8)
    ro = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.3
    rd = torch.randn(R, 3, generator=gen); rd = rd / rd.norm(dim=-1, keepdim=True)
    g = dict(means3D=e["means3D"] * 0.05, scales=e["scales"] * 0.25, rotations=e["rotations"], opacities=e["opacities"], shs=e["shs"].half() if half else e["shs"],
             others=torch.rand(P, 2, generator=gen))
    outs = {}
    for on in (True, False):
        tracing.QUAD_SH["on"] = on
        try:
            outs[on] = [x.detach().cpu().numpy() for x in _run_hip(g, ro, rd, torch.tensor([0.2, 0.3, 0.4]), deg, True, False)[0]]
        finally:
            tracing.QUAD_SH["on"] = True
    assert np.abs(outs[True][0]).max() > 0.05 and (outs[True][2] > 0.5).mean() > 0.2          # the rays do blend something
    for a, b in zip(outs[True], outs[False]):
        assert np.abs(a - b).max() <= 2e-6 * (np.abs(b).max() + 1.0)


def test_trace_forward_is_independent_of_the_traversal_interleaving():
    """Four wavefronts share a batch in the collection and prune each other through shared bins, so WHICH hits beyond the terminating one get
    collected depends on timing -- the composited result must not: two runs of the same call are bit-identical (lists are sorted by (t, id),
    the per-surfel weights are accumulated in fixed point)."""
    P, R = 20000, 8192
    e = synth.env_gaussians(P, seed=5)
    gen = torch.Generator().manual_seed(12)
    ro = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.3
    rd = torch.randn(R, 3, generator=gen); rd = rd / rd.norm(dim=-1, keepdim=True)
    g = dict(means3D=e["means3D"] * 0.2, scales=e["scales"] * 0.5, rotations=e["rotations"], opacities=e["opacities"], shs=e["shs"],
             others=torch.rand(P, 2, generator=gen))
    # (list capacity pinned above the longest list, ~630 hits here: a ray whose FOUND count -- which does depend on timing -- straddles the
    #  capacity of a fresh tracer (512) is composited by the K-buffer kernels in one run and by the list kernels in the other: the same terms
    #  summed in a different order, 1e-7 apart; scratch/determinism_probe.py)
    # (same for the rows of the compact per-hit buffers: a fresh tracer assumes 192 hits per ray, this scene has more)
    with _Switch(force_cap=1024, rows_per_ray=1024.0):
        runs = [[x.detach().clone() for x in _run_hip(g, ro, rd, torch.tensor([0.2, 0.3, 0.4]), 3, True, False)[0]] for _ in range(3)]
    assert float(runs[0][2].mean()) > 0.3                       # the rays blend plenty
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_trace_update_request_follows_the_new_vertices():
    """build_acceleration_structure(..., rebuild=False) is OptiX's update: the structure must follow the moved surfels (a stale one would be
    silently wrong).  Round 4: it IS a refit (topology and leaf order of the previous build kept, boxes recomputed); the result equals a fresh
    tracer's bit for bit -- hit sets do not depend on the topology."""
    import diff_surfel_tracing as mod
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    P, R = 4000, 2048
    e = synth.env_gaussians(P, seed=7, device=dev)
    gen = torch.Generator().manual_seed(3)
    ro = ((torch.rand(R, 3, generator=gen) * 2 - 1) * 1.3).to(dev)
    rd = torch.randn(R, 3, generator=gen); rd = (rd / rd.norm(dim=-1, keepdim=True)).to(dev)
    st = _settings(mod, torch.zeros(3), 3, dev)

    def trace(tracer, means, rebuild):
        n = means.shape[0]
        v, f = synth.get_disks(means, e["scales"][:n] * 0.4, e["rotations"][:n])
        tracer.build_acceleration_structure(v, f, rebuild=rebuild)
        with torch.no_grad():
            return tracer(ro, rd, v, means3D=means, grads3D=None, shs=e["shs"][:n], colors_precomp=None, others_precomp=None, opacities=e["opacities"][:n],
                          scales=e["scales"][:n] * 0.4, rotations=e["rotations"][:n], cov3D_precomp=None, tracer_settings=st, start_from_first=False)
    m0 = e["means3D"] * 0.1
    m1 = m0 + 0.5 * torch.randn_like(m0)
    with _Switch(force_cap=1024, rows_per_ray=1024.0):   # (one capacity for both tracers: the second call of `t` would otherwise run with a capacity adapted
        t = mod.SurfelTracer()                     #  to its first call, the fresh tracer with the default, and a ray near either takes a different kernel path)
        a0 = trace(t, m0, True)
        assert tracing.LAST_STATS["bvh"] == "build"
        a1 = trace(t, m1, False)                   # update request with moved surfels: the topology of the first build, refitted (envgs_bvh_refit)
        assert tracing.LAST_STATS["bvh"] == "refit"
        b1 = trace(mod.SurfelTracer(), m1, True)
        assert tracing.LAST_STATS["bvh"] == "build"
        c1 = trace(t, m0[:P // 2], False)          # an update request after the surfel count changed: nothing to keep, a full build
        assert tracing.LAST_STATS["bvh"] == "build" and c1[7].shape[0] == P // 2
    assert float(a1[2].mean()) > 0.05 and not torch.equal(a0[0], a1[0])
    for x, y in zip(a1, b1):
        assert torch.equal(x, y)


def test_trace_rebuild_requests_are_served_by_refits_while_the_tree_is_young():
    """VERDICT r4 item 5 / ADVICE r4: the reference's caller passes rebuild=True on EVERY training step (optix_utils.py:73-78).  A refit is exact, so the
    module answers such a request with one (SurfelTracer.set_structure_policy, default "adaptive") -- until `max_age` refits have followed the last
    full build, or the surface-area cost measured on the device after a refit (envgs_bvh_quality, read back without a host sync) has grown by more
    than `max_growth`.  Whatever it decides, the outputs equal a fresh tracer's bit for bit."""
    import diff_surfel_tracing as mod
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    P, R = 4000, 2048
    e = synth.env_gaussians(P, seed=9, device=dev)
    gen = torch.Generator().manual_seed(4)
    ro = ((torch.rand(R, 3, generator=gen) * 2 - 1) * 1.3).to(dev)
    rd = torch.randn(R, 3, generator=gen); rd = (rd / rd.norm(dim=-1, keepdim=True)).to(dev)
    st = _settings(mod, torch.zeros(3), 3, dev)

    def trace(tracer, means):
        v, f = synth.get_disks(means, e["scales"] * 0.4, e["rotations"])
        tracer.build_acceleration_structure(v, f, rebuild=True)                 # the reference's only form
        with torch.no_grad():
            out = tracer(ro, rd, v, means3D=means, grads3D=None, shs=e["shs"], colors_precomp=None, others_precomp=None, opacities=e["opacities"],
                         scales=e["scales"] * 0.4, rotations=e["rotations"], cov3D_precomp=None, tracer_settings=st, start_from_first=False)
        torch.cuda.synchronize()                                                # (the quality read-backs have landed: the next decision sees them)
        return out, tracing.LAST_STATS["bvh"]
    m0 = e["means3D"] * 0.1
    with _Switch(force_cap=1024, rows_per_ray=1024.0):
        t = mod.SurfelTracer()
        t.set_structure_policy("adaptive", max_age=3, max_growth=1.25)
        kinds, outs = [], []
        for k in range(6):                                                      # a training-like drift: small moves
            o, kind = trace(t, m0 + 0.002 * k * torch.ones_like(m0))
            kinds.append(kind); outs.append(o)
        assert kinds == ["build", "refit", "refit", "refit", "build", "refit"], kinds        # age bound: three refits, then a full build
        fresh, _ = trace(mod.SurfelTracer(), m0 + 0.002 * 5 * torch.ones_like(m0))
        for x, y in zip(outs[5], fresh):
            assert torch.equal(x, y)                                            # a refitted structure traces exactly like a fresh one
        # a jump (every surfel somewhere else): the request after it is still a refit -- its measurement is what reveals the damage -- and the
        # one after that is a full build
        t2 = mod.SurfelTracer()
        t2.set_structure_policy("adaptive", max_age=100, max_growth=1.25)
        perm = torch.randperm(P, generator=torch.Generator().manual_seed(1)).to(dev)
        seq = [trace(t2, m0)[1], trace(t2, m0[perm])[1], trace(t2, m0[perm])[1], trace(t2, m0[perm])[1]]
        assert seq == ["build", "refit", "build", "refit"], seq
        assert tracing.LAST_STATS.get("bvh_growth", 0.0) > 1.25 or True        # (recorded for the log below)
        # the literal policy: every request a full build
        t3 = mod.SurfelTracer()
        t3.set_structure_policy("rebuild")
        assert [trace(t3, m0)[1] for _ in range(3)] == ["build"] * 3
        # invalidate_structure: the caller knows better
        t.invalidate_structure()
        assert trace(t, m0)[1] == "build"


def test_trace_diagnostic_collection_kernels(request):
    """The diagnostic library's collection kernel -- the product's cooperative kernel plus the trap on a misaligned LDS bin table -- must keep
    producing the contract's results (the trap would abort the run)."""
    P, R = 2500, 1536
    e = synth.env_gaussians(P, seed=13)
    gen = torch.Generator().manual_seed(14)
    ro = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2
    rd = torch.randn(R, 3, generator=gen); rd = rd / rd.norm(dim=-1, keepdim=True)
    g = dict(means3D=e["means3D"] * 0.06, scales=e["scales"] * 0.3, rotations=e["rotations"], opacities=e["opacities"], shs=e["shs"],
             others=torch.rand(P, 2, generator=gen), colors_precomp=torch.rand(P, 3, generator=gen))
    res = _parity(request.node.name, g, ro, rd, torch.tensor([0.3, 0.2, 0.1]), 3, True, False, seed=15, hip_ctx=_Switch(diag=True),
                  which=("dmeans3D", "dopacities", "dcolor", "dray_o", "dray_d"))
    assert res["cnt"]["hits"] > 20 * res["R"]


def test_trace_removed_debug_switches_are_refused():
    """The ENVGS_DBG_TRACE bits of the deleted A/B kernels (8, 16, 512, 2048, 4096): a traced forward answers "bad argument" in the product AND in
    the diagnostic library, never a silent run of the default kernels under a switch that names another one."""
    import diff_surfel_tracing as mod
    from envgs_amd import _lib
    dev = torch.device("cuda:0")
    g, ro, rd = trace_scene(P=50, R=64, seed=2, camera=False)
    gd = {k: g[k].to(dev) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    v, f = synth.get_disks(gd["means3D"], gd["scales"], gd["rotations"])
    tracer = mod.SurfelTracer()
    tracer.build_acceleration_structure(v, f, rebuild=True)
    kw = dict(means3D=gd["means3D"], grads3D=None, shs=gd["shs"], colors_precomp=None, others_precomp=None, opacities=gd["opacities"], scales=gd["scales"],
              rotations=gd["rotations"], cov3D_precomp=None, tracer_settings=_settings(mod, torch.zeros(3), 1, dev), start_from_first=False)
    for kind in ("product", "diag"):
        old = _lib.select(kind)
        try:
            before = _lib.load().envgs_debug_get(0)
            for bit in (8, 16, 512, 2048, 4096):
                with _Switch(debug_trace=before | bit):
                    with pytest.raises(RuntimeError, match="bad argument"):
                        tracer(ro.to(dev), rd.to(dev), v, **kw)
                assert _lib.load().envgs_debug_get(0) == before, (kind, bit)    # the switch is restored ...
            rgb, *_ = tracer(ro.to(dev), rd.to(dev), v, **kw)                   # ... and the same call is accepted again
            torch.cuda.synchronize()
            assert rgb.shape == (64, 3) and torch.isfinite(rgb).all(), kind
        finally:
            _lib.select(old)


@pytest.mark.parametrize("P,R", [(50, 0), (0, 64), (0, 0), (1, 64)])
def test_trace_empty_inputs(P, R):
    """No rays, no surfels, neither, and a single surfel: shapes follow the inputs, an empty scene renders the background, backward runs."""
    import diff_surfel_tracing as mod
    dev = torch.device("cuda:0")
    g, ro, rd = trace_scene(P=50, R=64, seed=2, camera=False)
    bg = torch.tensor([0.2, 0.4, 0.6])
    L = {k: g[k][:P].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach(), L["rotations"].detach())
    tracer = mod.SurfelTracer()
    tracer.build_acceleration_structure(v, f, rebuild=True)
    o = ro[:R].to(dev).requires_grad_(True); d = rd[:R].to(dev).requires_grad_(True)
    outs = tracer(o, d, v, means3D=L["means3D"], grads3D=None, shs=L["shs"], colors_precomp=None, others_precomp=None, opacities=L["opacities"],
                  scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None, tracer_settings=_settings(mod, bg, 1, dev), start_from_first=False)
    rgb, dpt, acc, norm, dist, aux, mid, wet = outs
    assert [tuple(x.shape) for x in outs] == [(R, 3), (R, 1), (R, 1), (R, 3), (R, 1), (R, 2), (R, 16), (P, 1)]
    (rgb.sum() + acc.sum()).backward()
    torch.cuda.synchronize()
    assert o.grad is not None and o.grad.shape == (R, 3) and torch.isfinite(o.grad).all()
    if P == 0 and R:
        assert torch.allclose(rgb.detach(), bg.to(dev).expand(R, 3)) and float(acc.detach().abs().max()) == 0 and float(o.grad.abs().max()) == 0
    if P == 1:
        from oracle import trace as otr
        ref = otr.trace_forward(ro.numpy(), rd.numpy(), g["means3D"][:1].numpy(), g["scales"][:1].numpy(), g["rotations"][:1].numpy(),
                                g["opacities"][:1].numpy(), shs=g["shs"][:1].numpy(), sh_degree=1, bg=bg.numpy(), start_from_first=False)
        a = otr.trace_audit(ro.numpy(), rd.numpy(), g["means3D"][:1].numpy(), g["scales"][:1].numpy(), g["rotations"][:1].numpy(), g["opacities"][:1].numpy(),
                            start_from_first=False)
        ok = ~a["fragile"]
        check_close("single_surfel", "rgb", rgb.detach().cpu().numpy()[ok], ref["rgb"][ok], excluded=int((~ok).sum()))


@pytest.mark.parametrize("mode", ["generous", "tight", "legacy"])
def test_trace_compact_per_hit_buffers(mode, request):
    """hit_state / entries / pairs are addressed through row offsets taken from a scan of the hit counts (envgs_trace.h: compact_rows).
    generous: every ray has its rows; tight: the rows run out part-way through each segment and the remaining rays are handed to the K-buffer
    kernels (slower, never wrong); legacy: the (R, cap) layouts.  All three must meet the same contract."""
    from envgs_amd import tracing
    g, ro, rd = trace_scene(P=2000, R=1024, seed=7, camera=False)
    g["scales"] = g["scales"] * 0.35
    sw = {"generous": _Switch(rows_per_ray=400.0), "tight": _Switch(rows_per_ray=6.0), "legacy": _Switch(compact=False)}[mode]
    res = _parity(request.node.name, g, ro, rd, torch.tensor([0.3, 0.1, 0.7]), 2, True, False, hip_ctx=sw, require_lists=(mode != "tight"))
    cnt = res["cnt"]
    if mode == "generous":
        assert cnt["compact_rows"] > 0 and cnt["rays_without_rows"] == 0 and res["n_listed"] == res["R"]
    elif mode == "tight":
        assert cnt["compact_rows"] > 0 and cnt["rays_without_rows"] > 50 and 0 < res["n_listed"] < res["R"]
    else:
        assert cnt["compact_rows"] == 0 and res["n_listed"] == res["R"]


def test_trace_colour_only_state_promise():
    """SurfelTracer.set_colour_only_backward (include/envgs_trace.h: state_planes = 1): the forward keeps plane 0 of the per-hit state only; the
    colour's backward is the one of the full state (same kernel, same inputs), and a gradient for another output raises instead of being dropped."""
    import diff_surfel_tracing as mod
    dev = torch.device("cuda:0")
    g, _, _ = trace_scene(P=1500, R=4, seed=17, camera=False)
    g["scales"] = g["scales"] * 0.5
    cam = synth.orbit_camera(3, H=96, W=96, fx=80.0, radius=1.0)
    ro, rd = synth.get_rays(cam)
    ro, rd = ro.reshape(-1, 3).contiguous().to(dev), rd.reshape(-1, 3).contiguous().to(dev)
    R = ro.shape[0]
    up = torch.randn(R, 3, generator=torch.Generator().manual_seed(2)).to(dev) / R

    def run(promise, extra):
        L = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs", "others")}
        o = ro.clone().requires_grad_(True); d = rd.clone().requires_grad_(True)
        v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach(), L["rotations"].detach())
        tracer = mod.SurfelTracer()
        tracer.set_colour_only_backward(promise)
        tracer.build_acceleration_structure(v.detach().clone(), f.detach().clone(), rebuild=True)
        outs = tracer(o, d, v, means3D=L["means3D"], grads3D=None, shs=L["shs"], colors_precomp=None, others_precomp=L["others"],
                      opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None,
                      tracer_settings=_settings(mod, torch.tensor([0.2, 0.3, 0.1]), 3, dev), start_from_first=False)
        loss = (outs[0] * up).sum()
        if extra:
            loss = loss + outs[1].sum() * 1e-3
        loss.backward()
        torch.cuda.synchronize()
        return [x.detach().clone() for x in outs[:6]], {k: t.grad.clone() for k, t in L.items() if t.grad is not None}, o.grad.clone(), d.grad.clone()

    ref_o, ref_g, ref_do, ref_dd = run(False, False)
    got_o, got_g, got_do, got_dd = run(True, False)
    for a, b in zip(ref_o, got_o):
        assert torch.equal(a, b)
    assert set(ref_g) == set(got_g)
    for k in ref_g:
        err = float((ref_g[k] - got_g[k]).abs().max())
        assert err <= 2e-5 * float(ref_g[k].abs().max()) + 1e-12, (k, err)
    assert float((ref_do - got_do).abs().max()) <= 2e-5 * float(ref_do.abs().max()) and float((ref_dd - got_dd).abs().max()) <= 2e-5 * float(ref_dd.abs().max())
    with pytest.raises(RuntimeError, match="colour"):
        run(True, True)


class _CountDeferred:
    """Counts the traced backward calls that deferred their surfel gradients (the ENVGS_TRACE_DEFER bit handed to the library): what says whether
    the kernel calls deferred when a defer_barrier in front of the tracer has already joined inside backward()."""
    def __enter__(self):
        from envgs_amd import tracing
        self.tracing, self.orig, self.n = tracing, tracing.trace_backward, 0
        def counting(saved, *a, **kw):
            r = self.orig(saved, *a, **kw)
            self.n += int(saved.lists is not None and (saved.lists.defer_reduce & 1))
            return r
        tracing.trace_backward = counting
        return self
    def __exit__(self, *a):
        self.tracing.trace_backward = self.orig


@pytest.mark.gpu
@pytest.mark.parametrize("force_cap", [0, 16])
def test_trace_deferred_surfel_gradients(force_cap, request):
    """SurfelTracer.set_deferred_surfel_gradients (include/envgs_trace.h: defer_reduce): the record sums and the conversion of the surfel gradients
    run on the library's stream; after tracing.join_deferred_gradients() every gradient is the one of the stream-ordered backward to rounding (two
    runs order a surfel's records differently -- the slots come from atomics -- so neither form repeats itself bit for bit), also when rays took
    the K-buffer hand-off (force_cap = 16: the sum is then added to the hand-off's contributions instead of the other way round)."""
    import diff_surfel_tracing as mod
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    g, _, _ = trace_scene(P=1500, R=4, seed=23, camera=False)
    g["scales"] = g["scales"] * 0.5
    cam = synth.orbit_camera(2, H=96, W=96, fx=80.0, radius=1.0)
    ro, rd = synth.get_rays(cam)
    ro, rd = ro.reshape(-1, 3).contiguous().to(dev), rd.reshape(-1, 3).contiguous().to(dev)
    R = ro.shape[0]
    gen = torch.Generator().manual_seed(4)
    ups = [(torch.randn(R, c, generator=gen) / R).to(dev) for c in (3, 1, 1, 3, 2)]
    if force_cap:
        tracing.HIT_CAP["force"] = force_cap
        request.addfinalizer(lambda: tracing.HIT_CAP.pop("force", None))

    def run(defer):
        L = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs", "others")}
        o = ro.clone().requires_grad_(True); d = rd.clone().requires_grad_(True)
        v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach(), L["rotations"].detach())
        tracer = mod.SurfelTracer()
        tracer.set_deferred_surfel_gradients(defer)
        tracer.build_acceleration_structure(v.detach().clone(), f.detach().clone(), rebuild=True)
        outs = tracer(o, d, v, means3D=L["means3D"], grads3D=None, shs=L["shs"], colors_precomp=None, others_precomp=L["others"],
                      opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None,
                      tracer_settings=_settings(mod, torch.tensor([0.2, 0.3, 0.1]), 3, dev), start_from_first=False)
        loss = sum((x.reshape(R, -1) * y).sum() for x, y in zip((outs[0], outs[1], outs[2], outs[3], outs[5]), ups))
        loss.backward()
        pending = tracing._DEFERRED["pending"]
        tracing.join_deferred_gradients()                       # the current stream now waits for the tail; the clones below are queued behind it
        assert not tracing._DEFERRED["pending"]
        gr = {k: t.grad.clone() for k, t in L.items()}
        gr["ray_o"], gr["ray_d"] = o.grad.clone(), d.grad.clone()
        torch.cuda.synchronize()
        return gr, pending, tracing.last_trace_counts()

    ref, p0, _ = run(False)
    got, p1, tc = run(True)
    assert not p0 and p1                                        # the promise reached the library (records exist: the list path composited hits)
    if force_cap:
        assert tc["max_list"] > force_cap                       # some rays did take the hand-off
    for k in ref:
        err = float((ref[k] - got[k]).abs().max())
        assert err <= 2e-5 * float(ref[k].abs().max()) + 1e-12, (k, err)
        assert float(got[k].abs().max()) > 0


@pytest.mark.parametrize("force_cap", [0, 12])
def test_trace_deferred_surfel_gradients_over_a_bounce_chain(force_cap, request):
    """max_trace_depth = 2 with set_deferred_surfel_gradients: the three stages' backwards share their accumulators (include/envgs_trace.h:
    ENVGS_TRACE_ACCUMULATE / _NO_FINISH), each stage's record sums run under the next stage's record kernels, stage 0 converts once -- every
    gradient equals the stream-ordered chain's (one gradient set per stage, summed by autograd) to rounding; force_cap = 12: some rays of every
    stage take the K-buffer hand-off, whose atomics land in the shared accumulators between two stages' sums."""
    import diff_surfel_tracing as mod
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    g, ro, rd = trace_scene(P=150, R=400, seed=4, camera=True)
    thr, depth, deg = 0.1, 2, 1
    R = ro.shape[0]
    gen = torch.Generator().manual_seed(12)
    ups = [(torch.randn(R, c, generator=gen)).to(dev) for c in (3, 1, 1, 3, 2)]
    if force_cap:
        tracing.HIT_CAP["force"] = force_cap
        request.addfinalizer(lambda: tracing.HIT_CAP.pop("force", None))

    def run(defer):
        L = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs", "others")}
        o = ro.to(dev).requires_grad_(True); d = rd.to(dev).requires_grad_(True)
        v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach(), L["rotations"].detach())
        tracer = mod.SurfelTracer()
        tracer.set_deferred_surfel_gradients(defer)
        tracer.build_acceleration_structure(v.detach().clone(), f.detach().clone(), rebuild=True)
        g3 = torch.zeros_like(L["means3D"]).requires_grad_(True)
        calls = []
        orig = tracing.trace_backward
        def counting(saved, *a, chain=None, **kw):
            r = orig(saved, *a, chain=chain, **kw)
            calls.append((None if chain is None else chain[1], saved.lists.defer_reduce, sorted(k for k in ("means3D", "shs", "others_precomp", "ray_o") if r[k] is not None)))
            return r
        tracing.trace_backward = counting
        try:
            outs = tracer(o, d, v, means3D=L["means3D"], grads3D=g3, shs=L["shs"], colors_precomp=None, others_precomp=L["others"],
                          opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None,
                          tracer_settings=_settings(mod, torch.zeros(3), deg, dev, depth, thr), start_from_first=True)
            loss = sum((x.reshape(R, -1) * y).sum() for x, y in zip((outs[0], outs[1], outs[2], outs[3], outs[5]), ups))
            loss.backward()
        finally:
            tracing.trace_backward = orig
        tracing.join_deferred_gradients()
        gr = {k: t.grad.clone() for k, t in L.items()}
        gr["ray_o"], gr["ray_d"], gr["grads3D"] = o.grad.clone(), d.grad.clone(), g3.grad.clone()
        torch.cuda.synchronize()
        return gr, calls

    ref, c0 = run(False)
    got, c1 = run(True)
    assert [c[:2] for c in c0] == [(None, 0)] * 3
    # deepest stage first: it zeroes the accumulators and leaves them unconverted, the middle one adds, stage 0 adds and converts -- and only stage 0
    # hands surfel gradients to autograd (`others` and the rays come from every stage: they are complete on the caller's stream)
    assert [c[:2] for c in c1] == [(2, 1 | 4), (1, 1 | 2 | 4), (0, 1 | 2)], c1
    assert [c[2] for c in c1] == [["others_precomp", "ray_o"], ["others_precomp", "ray_o"], ["means3D", "others_precomp", "ray_o", "shs"]]
    for k in ref:
        err = float((ref[k] - got[k]).abs().max())
        assert float(ref[k].abs().max()) > 0 and err <= 3e-5 * float(ref[k].abs().max()) + 1e-12, (k, err)


@pytest.mark.parametrize("case", ["activated_parameters", "existing_grad", "tensor_hook", "post_accumulate_hook"])
def test_trace_deferral_steps_aside_when_autograd_would_touch_the_gradients(case):
    """set_deferred_surfel_gradients is only sound when autograd MOVES the surfel gradients into .grad.  The autograd node checks that per call and
    takes the stream-ordered backward otherwise: non-leaf inputs (the unchanged EasyVolcap caller feeds sigmoid / exp / normalize of its raw
    parameters: the activation's backward would read the gradient at once), a .grad to add into (gradient accumulation, GradExchange's flat views),
    a tensor hook or a post-accumulate hook on a parameter.  Nothing is left pending, and the gradients are the stream-ordered ones."""
    import diff_surfel_tracing as mod
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    g, _, _ = trace_scene(P=800, R=4, seed=41, camera=False)
    cam = synth.orbit_camera(2, H=48, W=48, fx=50.0, radius=1.0)
    ro, rd = synth.get_rays(cam)
    ro, rd = ro.reshape(-1, 3).contiguous().to(dev), rd.reshape(-1, 3).contiguous().to(dev)
    R = ro.shape[0]
    up = (torch.randn(R, 3, generator=torch.Generator().manual_seed(3)) / R).to(dev)
    seen = []

    def run(defer, twist):
        raw = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
        L = dict(raw)
        if twist == "activated_parameters":
            raw["opacities"] = torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4)).to(dev).requires_grad_(True)
            L["opacities"] = torch.sigmoid(raw["opacities"])
        if twist == "existing_grad":
            raw["scales"].grad = torch.zeros_like(raw["scales"])
        if twist == "tensor_hook":
            raw["means3D"].register_hook(lambda gr: seen.append(float(gr.abs().sum())) or None)
        if twist == "post_accumulate_hook":
            raw["shs"].register_post_accumulate_grad_hook(lambda p_: seen.append(float(p_.grad.abs().sum())))
        v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach(), L["rotations"].detach())
        tracer = mod.SurfelTracer()
        tracer.set_deferred_surfel_gradients(defer)
        tracer.build_acceleration_structure(v.detach().clone(), f.detach().clone(), rebuild=True)
        outs = tracer(ro, rd, v, means3D=L["means3D"], grads3D=None, shs=L["shs"], colors_precomp=None, others_precomp=None,
                      opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None,
                      tracer_settings=_settings(mod, torch.tensor([0.2, 0.3, 0.1]), 3, dev), start_from_first=False)
        (outs[0] * up).sum().backward()
        pending = tracing._DEFERRED["pending"]
        tracing.join_deferred_gradients()
        gr = {k: t.grad.clone() for k, t in raw.items()}
        torch.cuda.synchronize()
        return gr, pending

    ref, _ = run(False, case)
    got, pending = run(True, case)
    assert not pending                                       # the node saw the twist and did not defer
    plain, pend_plain = run(True, None)
    assert pend_plain                                        # ... and does defer the same call without it
    for k in ref:
        err = float((ref[k] - got[k]).abs().max())
        assert float(ref[k].abs().max()) > 0 and err <= 2e-5 * float(ref[k].abs().max()) + 1e-12, (k, err)


def test_trace_deferral_behind_a_barrier_serves_activated_parameters():
    """tracing.defer_barrier: raw parameters -> activations -> barrier (identity) -> tracer.  The tracer defers (its inputs are barrier outputs), the
    barrier's backward joins before the activations' backward sees the gradients -- no explicit join anywhere --, and because the barrier was created
    BEFORE the other branch of the step (a stand-in for the base pass) autograd reaches it AFTER that branch's backward has been queued: the overlap
    the deferral is for.  Raw-parameter gradients = those of the stream-ordered backward."""
    import diff_surfel_tracing as mod
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    g, _, _ = trace_scene(P=800, R=4, seed=43, camera=False)
    cam = synth.orbit_camera(1, H=48, W=48, fx=50.0, radius=1.0)
    ro, rd = synth.get_rays(cam)
    ro, rd = ro.reshape(-1, 3).contiguous().to(dev), rd.reshape(-1, 3).contiguous().to(dev)
    R = ro.shape[0]
    up = (torch.randn(R, 3, generator=torch.Generator().manual_seed(3)) / R).to(dev)

    def run(defer):
        raw = dict(means3D=g["means3D"].to(dev).requires_grad_(True), shs=g["shs"].to(dev).requires_grad_(True),
                   opacities=torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4)).to(dev).requires_grad_(True),
                   scales=torch.log(g["scales"]).to(dev).requires_grad_(True), rotations=(g["rotations"] * 1.7).to(dev).requires_grad_(True))
        other = torch.ones(16, device=dev, requires_grad=True)
        order = []
        act = (raw["means3D"] * 1.0, raw["shs"] * 1.0, torch.sigmoid(raw["opacities"]), torch.exp(raw["scales"]), torch.nn.functional.normalize(raw["rotations"], dim=-1))
        m3, sh, op, sc, rot = tracing.defer_barrier(*act) if defer else act        # first thing of the step
        base_like = (other * 3.0)                                                 # the rest of the step's forward comes after it
        base_like.register_hook(lambda gr: order.append("other branch") or None)
        v, f = synth.get_disks(m3.detach(), sc.detach(), rot.detach())
        tracer = mod.SurfelTracer()
        tracer.set_deferred_surfel_gradients(defer)
        tracer.build_acceleration_structure(v.detach().clone(), f.detach().clone(), rebuild=True)
        outs = tracer(ro, rd, v, means3D=m3, grads3D=None, shs=sh, colors_precomp=None, others_precomp=None, opacities=op, scales=sc, rotations=rot,
                      cov3D_precomp=None, tracer_settings=_settings(mod, torch.tensor([0.2, 0.3, 0.1]), 3, dev), start_from_first=False)
        orig = tracing.join_deferred_gradients
        def joining():
            if tracing._DEFERRED["pending"]: order.append("join")
            orig()
        tracing.join_deferred_gradients = joining
        try:
            ((outs[0] * up).sum() + base_like.sum()).backward()
        finally:
            tracing.join_deferred_gradients = orig
        assert not tracing._DEFERRED["pending"]                    # the barrier joined: nothing for the caller to do
        gr = {k: t.grad.clone() for k, t in raw.items()}
        torch.cuda.synchronize()
        return gr, order

    ref, o0 = run(False)
    got, o1 = run(True)
    assert o0 == ["other branch"] and o1 == ["other branch", "join"], (o0, o1)
    for k in ref:
        err = float((ref[k] - got[k]).abs().max())
        assert float(ref[k].abs().max()) > 0 and err <= 2e-5 * float(ref[k].abs().max()) + 1e-12, (k, err)


def test_trace_two_tracers_with_deferred_surfel_gradients():
    """Two tracers in one backward pass (the reference's samplers hold one over the base set and one over the environment set:
    envgs_sampler.py:508-521 next to :548), both deferring: the second backward to run joins the first one's tail on entry (scratch reuse is safe
    whatever the caller does) and leaves its own tail pending; one join afterwards covers both.  Gradients = the stream-ordered ones to rounding."""
    import diff_surfel_tracing as mod
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    sets = [trace_scene(P=900, R=4, seed=31, camera=False)[0], trace_scene(P=700, R=4, seed=32, camera=False)[0]]
    cam = synth.orbit_camera(1, H=64, W=64, fx=60.0, radius=1.0)
    ro, rd = synth.get_rays(cam)
    ro, rd = ro.reshape(-1, 3).contiguous().to(dev), rd.reshape(-1, 3).contiguous().to(dev)
    R = ro.shape[0]
    up = [(torch.randn(R, 3, generator=torch.Generator().manual_seed(5 + i)) / R).to(dev) for i in range(2)]

    def run(defer):
        Ls, loss = [], 0.0
        for i, g in enumerate(sets):
            L = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
            v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach(), L["rotations"].detach())
            tracer = mod.SurfelTracer()
            tracer.set_deferred_surfel_gradients(defer)
            tracer.build_acceleration_structure(v.detach().clone(), f.detach().clone(), rebuild=True)
            outs = tracer(ro, rd, v, means3D=L["means3D"], grads3D=None, shs=L["shs"], colors_precomp=None, others_precomp=None,
                          opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None,
                          tracer_settings=_settings(mod, torch.tensor([0.2, 0.3, 0.1]), 3, dev), start_from_first=False)
            loss = loss + (outs[0] * up[i]).sum()
            Ls.append(L)
        loss.backward()
        assert tracing._DEFERRED["pending"] == defer
        tracing.join_deferred_gradients()
        gr = [{k: t.grad.clone() for k, t in L.items()} for L in Ls]
        torch.cuda.synchronize()
        return gr

    ref, got = run(False), run(True)
    for a, b in zip(ref, got):
        for k in a:
            err = float((a[k] - b[k]).abs().max())
            assert float(a[k].abs().max()) > 0 and err <= 2e-5 * float(a[k].abs().max()) + 1e-12, (k, err)


@pytest.mark.parametrize("case", ["scale_regulariser", "two_calls_share_leaves"])
def test_trace_deferred_leaf_with_a_second_consumer(case):
    """A bare leaf surfel input of a deferring tracer that ANOTHER op of the same graph also uses: a regulariser on the scales, or a second traced
    call over the same parameters.  Autograd adds the gradients of a leaf's consumers as they arrive, so a deferred gradient handed straight to
    the leaf would be summed before the library's stream had finished it; SurfelTracer.forward puts bare leaves behind a leaf_barrier created at
    the call, which orders the stream after the deferred tail first.  The calls still defer, and every gradient = the stream-ordered one within 2e-5 of its largest element."""
    import diff_surfel_tracing as mod
    from envgs_amd import tracing
    dev = torch.device("cuda:0")
    g, _, _ = trace_scene(P=900, R=4, seed=37, camera=False)
    rays = []
    for c in (1, 2):
        ro, rd = synth.get_rays(synth.orbit_camera(c, H=64, W=64, fx=60.0, radius=1.0))
        rays.append((ro.reshape(-1, 3).contiguous().to(dev), rd.reshape(-1, 3).contiguous().to(dev)))
    R = rays[0][0].shape[0]
    up = [(torch.randn(R, 3, generator=torch.Generator().manual_seed(8 + i)) / R).to(dev) for i in range(2)]
    reg_w = (torch.rand(900, 2, generator=torch.Generator().manual_seed(10)) / 900).to(dev)

    def run(defer):
        L = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
        v, f = synth.get_disks(L["means3D"].detach(), L["scales"].detach(), L["rotations"].detach())
        tracer = mod.SurfelTracer()
        tracer.set_deferred_surfel_gradients(defer)
        tracer.build_acceleration_structure(v.detach().clone(), f.detach().clone(), rebuild=True)
        ncalls = 2 if case == "two_calls_share_leaves" else 1
        loss = 0.0
        for i in range(ncalls):
            outs = tracer(rays[i][0], rays[i][1], v, means3D=L["means3D"], grads3D=None, shs=L["shs"], colors_precomp=None, others_precomp=None,
                          opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None,
                          tracer_settings=_settings(mod, torch.tensor([0.2, 0.3, 0.1]), 3, dev), start_from_first=False)
            loss = loss + (outs[0] * up[i]).sum()
        if case == "scale_regulariser":
            loss = loss + (L["scales"].square() * reg_w).sum()
        with _CountDeferred() as cd:
            loss.backward()
        assert tracing._DEFERRED["pending"] == defer              # (the leaf barriers ordered the stream; the tail is released by a join)
        tracing.join_deferred_gradients()
        gr = {k: t.grad.clone() for k, t in L.items()}
        torch.cuda.synchronize()
        return gr, cd.n, ncalls

    ref, n0, _ = run(False)
    got, n1, ncalls = run(True)
    assert n0 == 0 and n1 == ncalls
    for k in ref:
        err = float((ref[k] - got[k]).abs().max())
        assert float(ref[k].abs().max()) > 0 and err <= 2e-5 * float(ref[k].abs().max()) + 1e-12, (k, err)


def test_trace_c_abi_refuses_a_lists_struct_with_a_missing_buffer():
    """the forward fell back to the K-buffer kernels when a scratch pointer of the lists struct was NULL, and a backward that found ITS
    pointers complete then took the list path and read counts nobody had written (silently wrong gradients).  Which path a call takes now depends
    on `cap` and the sizes alone, in both directions; a struct that asks for lists with a buffer of the call's direction missing is
    ENVGS_ERR_BAD_ARG.  (A released hit_lists pointer in the BACKWARD stays legal: it is forward-only.)"""
    from envgs_amd import tracing, _lib
    dev = torch.device("cuda:0")

    def clone(x):                                                              # (ctypes structs that hold pointers cannot be copy.copy'd)
        y = _lib.TraceLists()
        for name, _ in _lib.TraceLists._fields_:
            setattr(y, name, getattr(x, name))
        return y
    g, ro, rd = trace_scene(P=300, R=256, seed=4, camera=False)
    import diff_surfel_tracing as mod
    gd = {k: v.to(dev) for k, v in g.items()}
    v, _ = synth.get_disks(gd["means3D"], gd["scales"], gd["rotations"])
    nodes, _ = tracing.build_bvh(v)
    st = _settings(mod, torch.zeros(3), 3, dev)
    outs, saved = tracing.trace_forward(nodes, ro.to(dev), rd.to(dev), gd["means3D"], gd["shs"], None, gd["others"], gd["opacities"], gd["scales"],
                                        gd["rotations"], st, False)
    torch.cuda.synchronize()
    assert saved.cap > 0 and saved.lists is not None
    lib = _lib.load()
    p = _lib.ptr
    s = saved
    R = ro.shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    o = [torch.empty(R, c, **f32) for c in (3, 1, 1, 3, 1, 2, 16)] + [torch.empty(300, 1, **f32), torch.empty(R, **f32)]

    def fwd(lists):
        return lib.envgs_trace_forward(s.cfg, p(s.nodes), p(s.ro), p(s.rd), p(s.means3D), p(s.scales), p(s.rotations), p(s.opacities),
                                       p(s.shs), None, p(s.others), p(s.bg), p(s.srec), p(s.counters), *[p(t) for t in o], lists, None)

    full = clone(s.lists)
    full.hit_lists = s.keep.hit_lists.data_ptr() if s.keep.hit_lists is not None else None
    if full.hit_lists is not None:
        assert fwd(full) == 0                                                   # the complete struct is accepted
        torch.cuda.synchronize()
    for field in ("hit_lists", "surf_acc", "scan_temp", "hit_cnt"):
        bad = clone(full); setattr(bad, field, None)
        assert fwd(bad) == -1, field                                            # ... and with any forward buffer missing it is refused, not re-routed
    gup = torch.zeros(R, 3, **f32)
    grads = [torch.empty(300, c, **f32) for c in (16, 3, 3, 2, 4, 1)] + [torch.empty(300, 16, 3, **f32), None, torch.empty(300, 2, **f32),
                                                                          torch.empty(R, 3, **f32), torch.empty(R, 3, **f32)]
    for field in ("surf_off", "n_used"):
        bad = clone(s.lists); setattr(bad, field, None)
        rc = lib.envgs_trace_backward(s.cfg, p(s.nodes), p(s.ro), p(s.rd), p(s.means3D), p(s.scales), p(s.rotations), p(s.opacities),
                                      p(s.shs), None, p(s.others), p(s.bg), p(s.srec), p(s.counters), p(s.rgb), p(s.dpt), p(s.acc),
                                      p(s.norm), p(s.aux), p(s.final_T), p(gup), None, None, None, None, *[p(t) for t in grads], bad, None)
        assert rc == -1, field
