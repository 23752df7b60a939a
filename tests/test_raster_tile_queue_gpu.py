"""GPU: R6 / R7 as persistent grids over per-call tile queues (include/envgs_raster.h: tile_queue) against the fixed mapping, one workgroup per
tile over the eight bands (ENVGS_DBG_BALANCE bit 2), inside one process.  Which workgroup composites a tile changes no arithmetic, so

  * everything a pixel or a list entry owns alone -- colour, allmap, final_T, n_contrib, contrib_mask, radii -- is equal bit for bit;
  * what is summed over tiles with float atomics (`weight`, every gradient) agrees as two runs of the fixed mapping agree.  That bound is
    measured here by running the fixed mapping twice; one pair of runs is a sample, not a bound (on a small image two runs often agree to the
    last bit), so it is never taken below RUN_TO_RUN, the bound the suite already uses between two runs of such sums (tests/test_raster_parity.py,
    tests/test_bwd_batch_order_gpu.py): 2e-5 of the tensor's largest magnitude, far inside tests/util.py's TOL.

The default is ONE queue over all tiles, heaviest class first; ENVGS_DBG_BALANCE value 4 selects a queue per band (the eight contiguous eighths of
the image) with a workgroup taking from its own XCD's queue first and then from the next ones -- the form that was measured against it
(profiles/r09_ab_raster_persistent.txt).  Both run here.
ENVGS_DBG_TILE_GRID sets the persistent grid: 1 and 3 workgroups loop over every tile and take from every queue; 1000 is more than there are tiles
(the surplus workgroups find every queue dry and leave).  The queues themselves are read back: a permutation of the tiles (with band queues: each
tile in its own band's row), classes of the cost non-ascending, tile index ascending inside a class; R7's cost is the popcount of contrib_mask
over the tile's list."""
import importlib

import numpy as np
import pytest
import torch

from envgs_amd import synth
from tests.util import TOL

pytestmark = pytest.mark.gpu

RUN_TO_RUN = 2e-5
assert RUN_TO_RUN < TOL
BALANCE, TILE_GRID = 6, 7            # ENVGS_DBG_BALANCE, ENVGS_DBG_TILE_GRID
FIXED, BANDS = 2, 4                  # values of ENVGS_DBG_BALANCE
PKG = {3: "diff_surfel_rasterization_wet", 5: "diff_surfel_rasterization_wet_ch05", 7: "diff_surfel_rasterization_wet_ch07"}
BITWISE = ("color", "allmap", "final_T", "n_contrib", "contrib_mask", "radii", "ranges")
# (W, H): 1, 7, 8, 9, 63 and 65 tiles, and one image ragged against both tile borders (4 x 3 tiles)
SIZES = [(16, 16), (112, 16), (128, 16), (144, 16), (144, 112), (208, 80), (50, 37)]


def _scene(P, W, H, C, seed, fx=None, spread=1.0, scale_mul=4.0, shift_px=(0.0, 0.0), behind=False):
    """synth.base_gaussians x scale_mul seen by orbit camera 1; shift_px moves the cloud's centre on the screen (the offset is perpendicular to
    the viewing axis: the depth stays 4, so pixels = fx * world / 4); behind = the whole cloud behind the camera (nothing visible)."""
    g = synth.base_gaussians(P, seed=seed)
    fx = 1111.1 * max(W, 16) / 800.0 if fx is None else fx
    cam = synth.orbit_camera(1, H=H, W=W, fx=fx)
    Rt = cam.world_view_transform[:3, :3]                  # columns = camera right, down, forward in world coordinates
    g["means3D"] = g["means3D"] * spread + Rt[:, 0] * (shift_px[0] * 4.0 / fx) + Rt[:, 1] * (shift_px[1] * 4.0 / fx)
    if behind:
        g["means3D"] = g["means3D"] - Rt[:, 2] * 8.0
    g["scales"] = g["scales"] * scale_mul
    g["colors_precomp"] = torch.rand(P, C, generator=torch.Generator().manual_seed(seed + 7))
    return g, cam


def _settings(C, cam, W, H, dev):
    mod = importlib.import_module(PKG[C])
    return mod.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.full((C,), 0.25, device=dev), scale_modifier=1.0,
        viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev), sh_degree=torch.tensor([0], device=dev),
        campos=cam.camera_center.to(dev), prefiltered=False, debug=False)


def _upstream(C, W, H, dev, seed=3):
    gen = torch.Generator().manual_seed(seed)
    dall = torch.randn(7, H, W, generator=gen)
    dall[6] = 0.0
    dall[6, : H // 2] = torch.randn(H // 2, W, generator=gen)          # the distortion gradient in some tiles only: both DIST forms of R7
    return torch.randn(C, H, W, generator=gen).to(dev), dall.to(dev)


def _forward(g, cam, W, H, C, dev):
    from envgs_amd import raster
    gd = {k: v.to(dev) for k, v in g.items()}
    outs, saved = raster.rasterize_forward(C, gd["means3D"], None, gd["colors_precomp"], gd["opacities"], gd["scales"], gd["rotations"], None,
                                           _settings(C, cam, W, H, dev))
    return outs, saved


def _walked(saved):
    """Per tile: the entries R6 walks, the deepest last contributor of its pixels.  R6 stops flushing contrib_mask once every pixel of a tile has
    stopped, so entries behind that are not written (and R7 never reads them)."""
    H, W = saved["n_contrib"].shape[1:]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    last = torch.zeros(gy * 16, gx * 16, dtype=torch.int32, device=saved["n_contrib"].device)
    last[:H, :W] = saved["n_contrib"][0]
    return last.view(gy, 16, gx, 16).amax(dim=(1, 3)).reshape(-1).long().cpu().numpy()


def _contrib_mask(saved):
    """contrib_mask as far as it is defined: entries behind their tile's deepest last contributor read 0."""
    rg = saved["ranges"].view(-1, 2).long().cpu().numpy()
    cm = saved["contrib_mask"][:saved["N"]].cpu().numpy().copy()
    for t, w in enumerate(_walked(saved)):
        cm[rg[t, 0] + min(w, rg[t, 1] - rg[t, 0]):rg[t, 1]] = 0
    return cm


def _collect(outs, saved, grads):
    r = dict(color=outs[0], radii=outs[1], allmap=outs[2], weight=outs[3], final_T=saved["final_T"], n_contrib=saved["n_contrib"],
             ranges=saved["ranges"])
    r.update({"d_" + k: v for k, v in grads.items() if v is not None})
    r = {k: v.detach().cpu().numpy() for k, v in r.items()}
    r["contrib_mask"] = _contrib_mask(saved)
    return r


def _run(g, cam, W, H, C, balance=0, grid=0):
    """One forward and backward under the given switches; every output and gradient as numpy, and the saved state."""
    from envgs_amd import raster, _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    lib.envgs_debug_set(BALANCE, balance); lib.envgs_debug_set(TILE_GRID, grid)
    try:
        outs, saved = _forward(g, cam, W, H, C, dev)
        grads = raster.rasterize_backward(saved, *_upstream(C, W, H, dev))
        torch.cuda.synchronize()
    finally:
        lib.envgs_debug_set(BALANCE, 0); lib.envgs_debug_set(TILE_GRID, 0)
    return _collect(outs, saved, grads), saved


def _compare(ref, ref2, got, what):
    for k in ref:
        a, b, c = ref[k], ref2[k], got[k]
        if k in BITWISE:
            assert np.array_equal(a, c), (what, k)
            continue
        assert np.isfinite(c).all(), (what, k)
        sample = float(np.abs(a.astype(np.float64) - b).max()) if a.size else 0.0
        bound = max(sample, RUN_TO_RUN * (float(np.abs(a).max()) if a.size else 0.0))
        d = float(np.abs(a.astype(np.float64) - c).max()) if a.size else 0.0
        print("%s %s: fixed twice %.3e  bound %.3e  against the fixed mapping %.3e" % (what, k, sample, bound, d))
        assert d <= bound, (what, k, d, bound)


def _ab(g, cam, W, H, C, what=""):
    """The fixed mapping twice, then every queue form under every grid; the queues of each run are read back.  Returns the fixed mapping's
    results and the costs (R6's, R7's) per tile."""
    ref, _ = _run(g, cam, W, H, C, balance=FIXED)
    ref2, _ = _run(g, cam, W, H, C, balance=FIXED)
    for k in BITWISE:
        assert np.array_equal(ref[k], ref2[k]), k
    costs = None
    for balance in (0, BANDS):
        for grid in (0, 1, 3, 1000):
            got, saved = _run(g, cam, W, H, C, balance=balance, grid=grid)
            _compare(ref, ref2, got, "%s balance %d grid %d" % (what, balance, grid))
            costs = _check_orders(saved, W, H, banded=balance != 0)
    return ref, costs


def _check_orders(saved, W, H, banded=False):
    """The queues of the last forward and backward of `saved`, read back."""
    from envgs_amd import raster
    v = {k: t.cpu().numpy().astype(np.int64) for k, t in raster.tile_queue_views(saved).items()}
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    per = (ntiles + 7) // 8
    rg = saved["ranges"].view(-1, 2).long().cpu().numpy()
    cm = _contrib_mask(saved)
    pas = np.concatenate([[0], np.cumsum(np.unpackbits(cm[:, None], axis=1).sum(1))])
    cost6 = rg[:, 1] - rg[:, 0]
    cost7 = pas[rg[:, 1]] - pas[rg[:, 0]]
    assert v["tile_cost"].shape == (ntiles,) and np.array_equal(v["tile_cost"], cost7)
    for order, heads, cost in ((v["order6"], v["heads6"], cost6), (v["order7"], v["heads7"], cost7)):
        assert np.array_equal(np.sort(order), np.arange(ntiles))                    # every tile exactly once
        if banded:
            assert np.array_equal(order // per, np.arange(ntiles) // per)          # in its own band's row
        cls = (cost * 32) // (cost.max() + 1)
        for x in range(8 if banded else 1):
            row = order[x * per:(x + 1) * per] if banded else order
            step = np.diff(cls[row])
            assert (step <= 0).all()                                               # heaviest class first
            assert (np.diff(row)[step == 0] > 0).all()                             # tile index ascending inside a class
            assert heads[x] >= len(row)                                            # the queue was emptied
    return cost6, cost7


@pytest.mark.parametrize("C", [3, 5, 7])
@pytest.mark.parametrize("W, H", SIZES)
def test_persistent_grid_equals_fixed_mapping(W, H, C):
    P = 200 + 300 * ((W * H) // 4096)            # 200 .. 2000 surfels
    g, cam = _scene(P, W, H, C, seed=W + H + C)
    ref, _ = _ab(g, cam, W, H, C, what="%dx%d C%d" % (W, H, C))
    assert ref["n_contrib"].max() > 0 and np.abs(ref["d_grad_rec"]).max() > 0      # something was composited and differentiated


def test_every_surfel_in_the_first_band():
    """A 1 x 32 column of tiles with the cloud in its top 64 pixels: queue 0 holds every non-empty tile, seven queues hold empty ones only."""
    W, H, C = 16, 512, 5
    g, cam = _scene(600, W, H, C, seed=11, fx=100.0, spread=0.3, scale_mul=1.0, shift_px=(0.0, 32.0 - H / 2))
    ref, (cost6, _) = _ab(g, cam, W, H, C, what="first band")
    assert cost6[:4].sum() > 0 and cost6[4:].sum() == 0


def test_one_tile_holds_every_instance():
    W, H, C = 16, 512, 3
    g, cam = _scene(300, W, H, C, seed=12, fx=100.0, spread=0.02, scale_mul=0.3, shift_px=(0.0, 40.0 - H / 2))
    ref, (cost6, cost7) = _ab(g, cam, W, H, C, what="one tile")
    assert (cost6 > 0).sum() == 1 and cost6[2] > 0 and cost7[2] > 0


def test_nothing_visible():
    W, H, C = 144, 112, 3
    g, cam = _scene(200, W, H, C, seed=13, behind=True)
    ref, (cost6, _) = _ab(g, cam, W, H, C, what="N = 0")
    assert cost6.sum() == 0 and ref["n_contrib"][0].max() == 0 and np.all(ref["color"] == 0.25)
    assert np.abs(ref["d_grad_rec"]).max() == 0


def test_two_calls_outstanding_and_two_streams():
    """Two forwards outstanding, their backwards in reverse order; then the two calls on two streams.  Each backward uses the order, the heads and
    the costs of its own forward."""
    from envgs_amd import raster
    dev = torch.device("cuda:0")
    cases = [(144, 112, 5, 21, 1200), (208, 80, 5, 22, 700)]
    scenes = [_scene(P, W, H, C, seed=s) for W, H, C, s, P in cases]
    alone = []
    for (W, H, C, _, _), (g, cam) in zip(cases, scenes):
        a, _ = _run(g, cam, W, H, C, balance=FIXED)
        b, _ = _run(g, cam, W, H, C, balance=FIXED)
        alone.append((a, b))

    def check(outs, saveds, grads, what):
        for i, (W, H, C, _, _) in enumerate(cases):
            _compare(alone[i][0], alone[i][1], _collect(outs[i], saveds[i], grads[i]), "%s call %d" % (what, i))
            _check_orders(saveds[i], W, H)

    fw = [_forward(g, cam, W, H, C, dev) for (W, H, C, _, _), (g, cam) in zip(cases, scenes)]
    assert fw[0][1]["tile_queue"].data_ptr() != fw[1][1]["tile_queue"].data_ptr()
    grads = [None, None]
    for i in (1, 0):
        W, H, C = cases[i][:3]
        grads[i] = raster.rasterize_backward(fw[i][1], *_upstream(C, W, H, dev))
    torch.cuda.synchronize()
    check([f[0] for f in fw], [f[1] for f in fw], grads, "reverse order")

    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    ups = [_upstream(C, W, H, dev) for W, H, C, _, _ in cases]
    torch.cuda.synchronize()
    fw, grads = [None, None], [None, None]
    for i in (0, 1):
        with torch.cuda.stream(streams[i]):
            W, H, C = cases[i][:3]
            fw[i] = _forward(*scenes[i], W, H, C, dev)
    for i in (1, 0):
        with torch.cuda.stream(streams[i]):
            grads[i] = raster.rasterize_backward(fw[i][1], *ups[i])
    torch.cuda.synchronize()
    check([f[0] for f in fw], [f[1] for f in fw], grads, "two streams")
