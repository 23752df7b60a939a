"""GPU parity on opaque, surface-aligned scenes (tests/saturated_scenes.py): the HIP rasterizer and tracer against the CPU oracles where blends take the
alpha cap (opacity * G > 0.99), pixels and rays end after two or three hits, tiles leave the forward compositing before their last batch and the
collection's optical-depth bound engages after a handful of hits -- none of which the random-initialisation clouds of the other parity files reach.

The machinery is that of tests/test_raster_parity.py and tests/test_trace_parity.py (same contract: bit-exact index work, 1e-4 per element with the
oracle's cond / unc, K_UNC = 1; fragile pixels masked, fragile rays compared through their validated lists).  That the scenes DO reach those regimes, in
the references alone, is asserted without a GPU by tests/test_saturated_scenes_cpu.py."""
import numpy as np
import pytest
import torch

from tests import saturated_scenes as S
from tests.test_raster_parity import _settings as _raster_settings, _oracle, _mod_for, _compare_forward, _masked_upstream, _sh_clamp_fragile, GRAD_NAMES
from tests.test_saturated_scenes_cpu import RASTER_BG, plates_tiles, stack_closed_form, oracle_trace
from tests.test_trace_parity import _parity, _Switch, _hip_forward, _hip_backward, _read_lists
from tests.util import check_close, record, record_fragile, FRAGILE_PX_MAX

pytestmark = pytest.mark.gpu

SPHERES = ["sphere600", "sphere1500", "sphere300_17x15"]
TRACE_BG = torch.tensor([0.3, 0.1, 0.7])          # test_trace_parity's


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# rasterizer
@pytest.mark.parametrize("name", SPHERES)
def test_surface_object_forward_stages_vs_oracle(name, request):
    from envgs_amd import raster
    from oracle import raster as orc
    dev = torch.device("cuda:0")
    g, cam, c = S.raster_scene(name)
    st = _raster_settings(_mod_for(c["C"]), cam, RASTER_BG, c["deg"], dev)
    gd = {k: v.to(dev) for k, v in g.items()}
    outs, saved = raster.rasterize_forward(c["C"], gd["means3D"], gd["shs"] if c["sh"] else None, None if c["sh"] else gd["colors_precomp"], gd["opacities"],
                                           gd["scales"], gd["rotations"], None, st, keep_binning=True)
    torch.cuda.synchronize()
    ref = _oracle(g, cam, RASTER_BG, c["deg"], c["C"], c["sh"])
    aud = orc.raster_audit(ref, want_contrib=True)
    _compare_forward(request.node.name, outs, saved, ref, aud, c["sh"], check_sets=True)


@pytest.mark.parametrize("name", SPHERES)
def test_surface_object_backward_vs_oracle(name, request):
    from oracle import raster as orc
    dev = torch.device("cuda:0")
    g, cam, c = S.raster_scene(name)
    C, H, W = c["C"], c["H"], c["W"]
    mod = _mod_for(C)
    st = _raster_settings(mod, cam, RASTER_BG, c["deg"], dev)
    ref = _oracle(g, cam, RASTER_BG, c["deg"], C, c["sh"])
    aud = orc.raster_audit(ref)
    test = request.node.name
    record_fragile(test, "fragile_px", aud["fragile"], FRAGILE_PX_MAX)
    dcol, dall = _masked_upstream(C, H, W, c["seed"] + 100, aud["fragile"])
    leaves = {k: g[k].to(dev).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs" if c["sh"] else "colors_precomp")}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True) + 0
    means2D.retain_grad()
    color, radii, allmap, weight = mod.GaussianRasterizer(raster_settings=st)(
        means3D=leaves["means3D"], means2D=means2D, shs=leaves.get("shs"), colors_precomp=leaves.get("colors_precomp"),
        opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"], cov3D_precomp=None)
    ((color * dcol.to(dev)).sum() + (allmap * dall.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    rb = orc.raster_backward(ref, dcol.numpy(), dall.numpy(), want_cond=True)
    nfr = int(aud["fragile"].sum())
    grads = dict(leaves, means2D=means2D)
    clampfrag = _sh_clamp_fragile(ref) if c["sh"] else None
    for k_hip, k_ref in GRAD_NAMES + ((("shs", "dshs"),) if c["sh"] else (("colors_precomp", "dcolors"),)):
        check_close(test, k_ref, grads[k_hip].grad.cpu().numpy().reshape(rb[k_ref].shape), rb[k_ref], excluded=nfr, cond=rb["cond"][k_ref], unc=rb["unc"][k_ref],
                    keep=(~clampfrag if k_ref == "dshs" else None))


def test_plates_and_crowd_raster_tiles_leave_early(request):
    """Every pixel stops at the third plate, so 12 of the 16 tiles leave the forward compositing (__syncthreads_and(done)) batches before their list ends: the
    later batches' contrib_mask and tile_cost are never written, and the backward starts from the tile's deepest last contributor.  The surfels never
    reached keep EXACTLY zero weight and gradient, with and without the forward's contrib_mask."""
    from envgs_amd import raster
    from oracle import raster as orc
    dev = torch.device("cuda:0")
    test = request.node.name
    g, cam = S.plates_and_crowd_raster()
    P = g["means3D"].shape[0]
    H, W = cam.image_height, cam.image_width
    st = _raster_settings(_mod_for(3), cam, RASTER_BG, 3, dev)
    gd = {k: v.to(dev) for k, v in g.items()}
    args = (3, gd["means3D"], gd["shs"], None, gd["opacities"], gd["scales"], gd["rotations"], None, st)
    outs, saved = raster.rasterize_forward(*args, keep_binning=True)
    torch.cuda.synchronize()
    ref = _oracle(g, cam, RASTER_BG, 3, 3, True)
    aud = orc.raster_audit(ref, want_contrib=True)
    assert not aud["fragile"].any() and len(plates_tiles(ref, P)) >= 4
    _compare_forward(test, outs, saved, ref, aud, True, check_sets=True)
    zero = ref["weight"] == 0
    assert zero[:P - 3].sum() > 2000 and not zero[P - 3:P - 1].any()             # (the third plate stops every pixel and is itself never blended)
    weight = outs[3].cpu().numpy()[:, 0]
    assert np.all(weight[zero] == 0)
    # the backward with the forward's masks and with the geometric fallback
    dcol, dall = _masked_upstream(3, H, W, 104, aud["fragile"])
    rb = orc.raster_backward(ref, dcol.numpy(), dall.numpy(), want_cond=True)
    clampfrag = _sh_clamp_fragile(ref)
    saved2 = dict(saved); saved2["contrib_mask"] = None
    got = {}
    for form, sv in (("masks", saved), ("no_masks", saved2)):
        gr = raster.rasterize_backward(sv, dcol.to(dev), dall.to(dev))
        torch.cuda.synchronize()
        got[form] = {k: v.cpu().numpy() for k, v in gr.items() if v is not None}
        for k_hip, k_ref in GRAD_NAMES + (("shs", "dshs"),):
            a = got[form][k_hip].reshape(rb[k_ref].shape)
            check_close(test + "." + form, k_ref, a, rb[k_ref], cond=rb["cond"][k_ref], unc=rb["unc"][k_ref], keep=(~clampfrag if k_ref == "dshs" else None))
            assert np.all(a[zero] == 0), (form, k_hip)                              # never reached: not one term
    for k_hip, _ in GRAD_NAMES + (("shs", "dshs"),):
        a, b = got["masks"][k_hip], got["no_masks"][k_hip]
        assert np.abs(a - b).max() <= 2e-5 * (np.abs(b).max() + 1e-30), k_hip      # same terms, summed by LDS / L2 atomics in a different order
    # a second forward (and the tile queues it builds) gives the identical image
    outs2, saved2nd = raster.rasterize_forward(*args, keep_binning=True)
    torch.cuda.synchronize()
    assert torch.equal(outs2[0], outs[0]) and torch.equal(outs2[2], outs[2])
    assert torch.equal(saved2nd["n_contrib"], saved["n_contrib"]) and torch.equal(saved2nd["final_T"], saved["final_T"])
    assert np.all(outs2[3].cpu().numpy()[:, 0][zero] == 0)


def test_stack_raster_doubly_capped_stop(request):
    """Opacities (1, 1, 1): on the four central pixels the first blend is capped and the second stops the pixel, T (1 - 0.99f) = 9.99998e-5 against
    T_EPS = 1e-4f -- a relative margin of 1.9e-6, decided by ONE rounded multiply.  The audit marks these pixels fragile (its margin does not know that);
    they are asserted here directly, by bits."""
    from envgs_amd import raster
    from oracle import raster as orc
    dev = torch.device("cuda:0")
    test = request.node.name
    g, cam, central = S.stack_raster((1.0, 1.0, 1.0))
    H, W = cam.image_height, cam.image_width
    m = central.numpy()
    st = _raster_settings(_mod_for(3), cam, S.STACK_BG, 0, dev)
    gd = {k: v.to(dev) for k, v in g.items()}
    outs, saved = raster.rasterize_forward(3, gd["means3D"], None, gd["colors_precomp"], gd["opacities"], gd["scales"], gd["rotations"], None, st, keep_binning=True)
    torch.cuda.synchronize()
    ref = _oracle(g, cam, S.STACK_BG, 0, 3, False)
    cf = stack_closed_form()
    nc = saved["n_contrib"].cpu().numpy()
    fT = saved["final_T"].cpu().numpy()
    color, _, allmap, weight = [o.cpu().numpy() for o in outs]
    np.testing.assert_array_equal(nc[0][m], np.ones(4, np.int32))
    np.testing.assert_array_equal(nc[0][m], ref["n_contrib"][0][m])
    np.testing.assert_array_equal(_bits(fT[0][m]), _bits(np.full(4, cf["final_T"])))
    np.testing.assert_array_equal(_bits(allmap[1][m]), _bits(np.full(4, cf["alpha"])))
    assert np.abs(color[:, m] - cf["rgb"][:, None]).max() <= 1e-6
    # gradients for an upstream that lives on the central pixels alone: nothing for the second and third surfel, the oracle's for the first
    gen = torch.Generator().manual_seed(5)
    cm = central.to(torch.float32)
    dcol = torch.randn(3, H, W, generator=gen) * cm
    dall = torch.randn(7, H, W, generator=gen) * cm
    gr = raster.rasterize_backward(saved, dcol.to(dev), dall.to(dev))
    torch.cuda.synchronize()
    rb = orc.raster_backward(ref, dcol.numpy(), dall.numpy(), want_cond=True)
    for k_hip, k_ref in GRAD_NAMES + (("colors_precomp", "dcolors"),):
        a = gr[k_hip].cpu().numpy().reshape(rb[k_ref].shape)
        assert np.all(rb[k_ref][1:] == 0) and np.all(a[1:] == 0), k_hip
        check_close(test, k_ref, a[:1], rb[k_ref][:1], cond=np.asarray(rb["cond"][k_ref])[:1], unc=np.asarray(rb["unc"][k_ref])[:1])
    assert np.abs(rb["dopacities"][0]) > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# tracer
_PATHS = {"lists": lambda: dict(all_listed=True), "kbuffer": lambda: dict(hip_ctx=_Switch(no_lists=True), require_lists=False),
          "sparse": lambda: dict(hip_ctx=_Switch(sparse="on"), all_listed=True)}


@pytest.mark.parametrize("path", list(_PATHS))
def test_room_forward_backward_vs_oracle(path, request):
    g, ro, rd, c = S.trace_scene_of("room600")
    res = _parity(request.node.name, g, ro, rd, TRACE_BG, 3, True, c["camera"], **_PATHS[path]())
    assert res["ref"]["nhits"].mean() > 2
    if path == "kbuffer":
        assert res["n_listed"] == 0
    if path == "sparse":
        assert res["cnt"]["sparse_hits"] > 0


def test_room_camera_rays_vs_oracle(request):
    g, ro, rd, c = S.trace_scene_of("room200")
    _parity(request.node.name, g, ro, rd, TRACE_BG, 3, True, c["camera"], all_listed=True)


def test_plates_and_crowd_trace_collects_a_superset(request):
    """Three plates of opacity 0.97 exhaust the rays that meet them: the collection's optical-depth bound (KILL_OD) may cut what lies behind, but never
    what the compositing needs -- composited <= found <= accepted."""
    g, ro, rd = S.plates_and_crowd_trace()
    test = request.node.name
    res = _parity(test, g, ro, rd, TRACE_BG, 3, True, False, all_listed=True)
    cen = S.census_trace(g, ro, rd, False)
    cnt = res["cnt"]
    record(test, "found_over_accepted", cnt["found"] / cen["accepted"], "(%d hits composited, %d found by the collection, %d accepted by the float64 twin with termination ignored)"
           % (cnt["hits"], cnt["found"], cen["accepted"]))
    assert cnt["hits"] <= cnt["found"] <= cen["accepted"], (cnt["hits"], cnt["found"], cen["accepted"])
    assert cnt["hits"] == int(res["ref"]["nhits"].sum())


_STACK_FORWARDS = {}


def _stack_run(opac, path):
    """One stack on one path: (forward outputs as numpy, lists or None, gradients as numpy)."""
    from envgs_amd import tracing
    g, ro, rd = S.stack_trace(opac)
    R = ro.shape[0]
    gen = torch.Generator().manual_seed(3)
    gr = [torch.randn(R, 3, generator=gen), torch.randn(R, generator=gen), torch.randn(R, generator=gen), torch.randn(R, 3, generator=gen), torch.randn(R, 2, generator=gen)]
    sw = {"lists": _Switch(), "kbuffer": _Switch(no_lists=True), "sparse": _Switch(sparse="on")}[path]
    old = tracing.KEEP_LISTS["on"]
    tracing.KEEP_LISTS["on"] = True
    try:
        with sw:
            ctx = _hip_forward(g, ro, rd, S.STACK_BG, 0, False, False)
            lists = _read_lists()
            outs, L, o, d, _ = _hip_backward(ctx, gr)
    finally:
        tracing.KEEP_LISTS["on"] = old
    fwd = {k: outs[i].detach().cpu().numpy() for k, i in (("rgb", 0), ("dpt", 1), ("acc", 2), ("norm", 3), ("aux", 5), ("wet", 7))}
    grads = {k: L[k].grad.cpu().numpy() for k in ("means3D", "scales", "rotations", "opacities", "others", "colors_precomp")}
    return (g, ro, rd, gr), fwd, lists, grads


@pytest.mark.parametrize("path", list(_PATHS))
@pytest.mark.parametrize("opac", S.STACKS, ids=lambda o: "-".join("%g" % x for x in o))
def test_stack_trace_stop_decisions(opac, path, request):
    """(1, 1, 1): one hit, the second is the doubly-capped stop; (1, 0.5, 1) and (1, 0.98, 1): two hits.  On the list path, the K-buffer path and in sparse
    mode: acc and wet by bits, rgb and dpt to 1e-6, the kept lists hold exactly the composited ids, nothing behind the stop gets a gradient, and the
    three paths give bit-identical forwards."""
    from oracle import trace as otr
    test = request.node.name
    (g, ro, rd, gr), fwd, lists, grads = _stack_run(opac, path)
    R = ro.shape[0]
    ref = oracle_trace(g, ro, rd, False, S.STACK_BG)
    nh = 1 if opac == (1.0, 1.0, 1.0) else 2
    np.testing.assert_array_equal(ref["nhits"], np.full(R, nh))
    np.testing.assert_array_equal(_bits(fwd["acc"][:, 0]), _bits(ref["acc"]))
    one = oracle_trace(g, ro[:1], rd[:1], False, S.STACK_BG)["wet"].astype(np.float32)      # the fp32 blend weights of one ray; every ray has the same
    wet = np.zeros(3, np.float32)
    for _ in range(R):
        wet = (wet + one).astype(np.float32)                                                 # equal addends: the sum does not depend on the order
    np.testing.assert_array_equal(_bits(fwd["wet"][:, 0]), _bits(wet))
    assert np.abs(fwd["rgb"] - ref["rgb"]).max() <= 1e-6
    assert (np.abs(fwd["dpt"][:, 0] - ref["dpt"]) / ref["dpt"]).max() <= 1e-6
    if opac == (1.0, 1.0, 1.0):
        cf = stack_closed_form()
        np.testing.assert_array_equal(_bits(fwd["acc"][:, 0]), _bits(np.full(R, cf["alpha"])))
        assert np.abs(fwd["rgb"] - cf["rgb"][None]).max() <= 1e-6
    if path == "kbuffer":
        assert lists is None
    else:
        ids, tb, n_used, hit_cnt = lists
        np.testing.assert_array_equal(n_used, np.full(R, nh))
        np.testing.assert_array_equal(ids[:, :nh], np.tile(np.arange(nh, dtype=ids.dtype), (R, 1)))
        assert np.all(hit_cnt >= n_used) and np.all(hit_cnt <= 3)
    # gradients: exactly nothing behind the stop (the surfel whose test stops the ray is not blended either); the composited rows against the oracle
    rb = otr.trace_backward(ref, *[x.numpy() for x in gr], want_cond=True)
    for k, a in grads.items():
        assert np.all(a[nh:] == 0), (k, a)
    for k_hip, k_ref in (("opacities", "dopacities"), ("others", "dothers"), ("colors_precomp", "dcolors")):      # (u = v = 0 exactly: the geometric gradients vanish)
        assert np.all(np.asarray(rb[k_ref])[nh:] == 0)
        check_close(test, k_ref, grads[k_hip].reshape(np.asarray(rb[k_ref]).shape)[:nh], np.asarray(rb[k_ref])[:nh], cond=np.asarray(rb["cond"][k_ref])[:nh],
                    unc=np.asarray(rb["unc"][k_ref])[:nh])
    # the three paths agree bit for bit on the forward (each case compares itself with the first path that ran for these opacities)
    first = _STACK_FORWARDS.setdefault(opac, (path, fwd))
    for k in fwd:
        np.testing.assert_array_equal(_bits(fwd[k]), _bits(first[1][k]), err_msg="%s: path %s against path %s" % (k, path, first[0]))
