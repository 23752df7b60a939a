"""The reflect, blend, bounce, quad and acc-filter glue (envgs_amd.fused, envgs_amd/csrc/glue.hip) at the sizes, upstream sets, leaf sets and layouts
the product step uses: partly filled workgroups, NULL upstream pointers, leaves without a gradient, converted inputs, guarded buffers at the C ABI.

Ground truth: the float64 twins of tests/glue_twins.py.  Rule (tests/test_fused_glue.py, the surface normals): every output and gradient tensor is
compared elementwise (tests/util.py:check_close) under  max(1e-4, K_F32 * e_twin32),  e_twin32 = the float32 twin on the CPU against the float64
twin -- what one float32 evaluation of the expressions loses.  Only elements whose float64 twin is not finite are left out (torch's 0 * inf at
alpha == 0); there the kernel must give exactly 0.  Where the twin is exactly zero, so must the kernel be.
The tests without the gpu mark (the twin pins, the e_twin32 table, the argument checks of the front ends) launch nothing."""
import functools

import numpy as np
import pytest
import torch

from envgs_amd import synth
from tests import glue_twins as T
from tests.test_fused_glue import K_F32
from tests.util import check_close, floor_rel_err, record

# HW = 1, 63, 64, 65, 255, 256, 257, 513, 1961: one lane per pixel, 256 per workgroup
PIXEL_SHAPES = [(1, 1), (1, 63), (8, 8), (5, 13), (3, 85), (16, 16), (1, 257), (19, 27), (37, 53)]
# (R, n, how the n rows are chosen): one lane per row of sel
ROW_CASES = [(1, 1, "all"), (7, 0, "none"), (300, 255, "random"), (300, 256, "random"), (300, 257, "random"), (600, 600, "all"), (600, 1, "first"),
             (600, 1, "last"), (600, 350, "reversed")]
QUAD_P = [1, 255, 256, 257, 1000]
ALL4 = (True, True, True, True)
LEAVES = ("o", "d", "dpt", "acc", "norm", "aux", "rgb", "col_next")
ALL8 = (True,) * 8
RATIO = 0.3


def _np(t):
    return t.detach().cpu().numpy()


def _twin_error(t32, t64, only=None):
    """-> (keep, e_twin32): the elements compared (the float64 twin is finite; `only` narrows further) and the float32 twin's error on them;
    e_twin32 is None when the float64 twin is zero on all of them."""
    t32, t64 = _np(t32), _np(t64)
    assert t32.shape == t64.shape and t32.dtype == np.float32 and t64.dtype == np.float64
    keep = np.isfinite(t64)
    if only is not None:
        keep = keep & np.broadcast_to(_np(only), t64.shape)
    b = t64[keep]
    if not b.any():
        return keep, None
    assert np.isfinite(t32[keep]).all()
    return keep, float(floor_rel_err(t32[keep], b)[0].max())


def _compare(test, what, hip, t32, t64, only=None):
    """The comparison rule of this file (see the module docstring)."""
    keep, e_twin = _twin_error(t32, t64, only)
    hip, t64 = _np(hip), _np(t64)
    assert hip.shape == t64.shape and hip.dtype == np.float32, (what, hip.shape, t64.shape, hip.dtype)
    assert np.isfinite(hip).all(), "%s / %s: not finite" % (test, what)
    assert not hip[~np.isfinite(t64)].any(), "%s / %s: must be exactly 0 where the twin's own gradient is not finite" % (test, what)
    if e_twin is None:
        assert not hip[keep].any(), "%s / %s: must be exactly 0 (the float64 twin is)" % (test, what)
        return
    e_hip = float(floor_rel_err(hip[keep], t64[keep])[0].max())
    print("%s %s: e_hip %.3e  e_twin32 %.3e  ratio %.3f" % (test, what, e_hip, e_twin, e_hip / max(e_twin, 1e-30)))
    record(test, what + " e_twin32", e_twin, note="float32 twin (CPU) vs float64 twin")
    record(test, what + " ratio", e_hip / max(e_twin, 1e-30), note="e_hip / e_twin32")
    check_close(test, what, hip, t64, tol=max(1e-4, K_F32 * e_twin), keep=keep)


def _bits(a, b):
    """Bit for bit."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


# ---- reflect ------------------------------------------------------------------------------------------------------------------------------------
_reflect_case = functools.lru_cache(maxsize=None)(T.reflect_input)
NAMES4 = ("normal_world", "depth", "ref_o", "ref_d")


def _reflect_run(fn, H, W, ratio, dtype, device, use, need):
    """fn = the twin or fused.reflect, same signature.  -> the four outputs, [dallmap, dray_o, dray_d] (None: that ray needs no gradient)."""
    cam, allmap, ro, rd, _, ws = _reflect_case(H, W)
    mk = lambda t, g=False: t.to(device=device, dtype=dtype).clone().requires_grad_(g)
    a, o, d = mk(allmap, True), mk(ro, need[0]), mk(rd, need[1])
    outs = fn(a, o, d, mk(cam.world_view_transform), ratio)
    assert [tuple(x.shape) for x in outs] == [(3, H, W), (1, H, W), (H, W, 3), (H, W, 3)] and all(x.dtype == dtype for x in outs)
    sum((x * mk(w)).sum() for x, w, u in zip(outs, ws, use) if u).backward()
    grads = [t.grad if t.grad is not None else torch.zeros_like(t) for t in (a, o, d)]
    assert o.grad is None or need[0]
    assert d.grad is None or need[1]
    return [x.detach().cpu() for x in outs], [g.cpu() if (i == 0 or need[i - 1]) else None for i, g in enumerate(grads)]


@functools.lru_cache(maxsize=None)
def _reflect_twin(H, W, ratio, dtype, use=ALL4, need=(True, True)):
    return _reflect_run(T.twin_reflect, H, W, ratio, dtype, "cpu", use, need)


def _reflect_pairs(H, W, ratio, use=ALL4, need=(True, True)):
    """-> [(what, float32 twin, float64 twin, only, picker)]: every tensor the rule compares, `picker` taking it out of a run's (outs, grads)."""
    px = _reflect_case(H, W)[4]
    (o32, g32), (o64, g64) = _reflect_twin(H, W, ratio, torch.float32, use, need), _reflect_twin(H, W, ratio, torch.float64, use, need)
    pairs = [(nm, o32[i], o64[i], None, (lambda r, i=i: r[0][i])) for i, nm in enumerate(NAMES4)]
    for what, sl in (("dallmap[0]", slice(0, 1)), ("dallmap[1]", slice(1, 2)), ("dallmap[2:5]", slice(2, 5)), ("dallmap[5]", slice(5, 6))):
        pairs.append((what, g32[0][sl], g64[0][sl], None, (lambda r, sl=sl: r[1][0][sl])))
    # the tiny normals carry gradients 1e6 times the others' and so set the floor of the comparison above: the other pixels once more, by themselves
    pairs.append(("dallmap[2:5] but tiny", g32[0][2:5], g64[0][2:5], ~px["tiny"][None], (lambda r: r[1][0][2:5])))
    for i, nm in ((1, "dray_o"), (2, "dray_d")):
        if need[i - 1]:
            pairs.append((nm, g32[i], g64[i], None, (lambda r, i=i: r[1][i])))
    return pairs


def _reflect_check(test, H, W, ratio, use=ALL4, need=(True, True)):
    from envgs_amd import fused
    run = _reflect_run(fused.reflect, H, W, ratio, torch.float32, torch.device("cuda:0"), use, need)
    for what, t32, t64, only, pick in _reflect_pairs(H, W, ratio, use, need):
        _compare(test, what, pick(run), t32, t64, only)
    px = _reflect_case(H, W)[4]
    dall = run[1][0]
    assert dall.shape == (7, H, W) and not dall[6].any()
    dead = px["empty"] | px["inf"]
    assert not dall[:2][:, dead].any() and not dall[5][px["nan"]].any()
    for i in (0, 1):
        assert (run[1][i + 1] is None) == (not need[i])
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", PIXEL_SHAPES)
def test_reflect_shape_ladder(H, W):
    _reflect_check("glue_reflect[%d-%d]" % (H, W), H, W, RATIO)


REFLECT_ALONE = [("normal_world_only", RATIO, (True, False, False, False), (True, True)), ("depth_only", RATIO, (False, True, False, False), (True, True)),
                 ("ref_o_only", RATIO, (False, False, True, False), (True, True)), ("ref_d_only", RATIO, (False, False, False, True), (True, True)),
                 ("no_ray_gradient", RATIO, ALL4, (False, False)), ("ray_d_gradient_only", RATIO, ALL4, (False, True)),
                 ("ratio_0", 0.0, ALL4, (True, True)), ("ratio_1", 1.0, ALL4, (True, True))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", REFLECT_ALONE, ids=[c[0] for c in REFLECT_ALONE])
def test_reflect_one_upstream_one_leaf_at_a_time(case):
    """An output the loss does not use reaches the kernel as a NULL upstream pointer, a ray that needs no gradient as a NULL output pointer (the
    product step: camera rays need none)."""
    name, ratio, use, need = case
    _reflect_check("glue_reflect_alone[%s]" % name, 19, 27, ratio, use, need)


@pytest.mark.gpu
def test_reflect_sends_minus_infinity_to_zero():
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    H, W = 5, 6
    cam = T.reflect_cam(H, W, device=dev)
    ro, rd = synth.get_rays(cam)
    allmap = torch.rand(7, H, W, generator=torch.Generator().manual_seed(2)) + 0.5
    allmap[5, 2, 3] = float("-inf")                       # a -inf median
    allmap[0, 3, 2] = -1.0; allmap[1, 3, 2] = 0.0         # -1 / 0: a -inf expected depth
    grads = {}
    for ratio in (1.0, 0.0):
        a = allmap.to(dev).requires_grad_(True)
        outs = fused.reflect(a, ro, rd, cam.world_view_transform, ratio)
        sum(x.sum() for x in outs).backward()
        assert all(torch.isfinite(x).all() for x in outs) and torch.isfinite(a.grad).all()
        grads[ratio] = (outs[1].detach().cpu(), a.grad.cpu())
    # The kernels send -inf to 0, like NaN and +inf.  The reference's nan_to_num(x, 0, 0) leaves neginf at its default and sends -inf to the lowest
    # finite float (-3.4e38), and so does the twin; the rasterizer cannot produce it (depths are >= 0.2), so the difference is pinned here and not
    # reproduced (include/envgs_glue.h).
    assert float(grads[1.0][0][0, 2, 3]) == 0.0 and float(grads[0.0][0][0, 3, 2]) == 0.0
    assert float(grads[1.0][1][5, 2, 3]) == 0.0 and not grads[0.0][1][:2, 3, 2].any()
    twin = T.twin_reflect(allmap, ro.cpu(), rd.cpu(), cam.world_view_transform.cpu(), 1.0)[1]
    assert float(twin[0, 2, 3]) < -3e38 and float(T.twin_reflect(allmap, ro.cpu(), rd.cpu(), cam.world_view_transform.cpu(), 0.0)[1][0, 3, 2]) < -3e38


# ---- blend ---------------------------------------------------------------------------------------------------------------------------------------
_blend_case = functools.lru_cache(maxsize=None)(T.blend_input)


def _blend_run(fn, H, W, C, dtype, device, need_env=True):
    img, env, up = _blend_case(H, W, C)
    mk = lambda t, g=False: t.to(device=device, dtype=dtype).clone().requires_grad_(g)
    i, e = mk(img, True), mk(env, need_env)
    out = fn(i, e)
    assert out.shape == (H, W, 3) and out.dtype == dtype
    (out * mk(up)).sum().backward()
    assert e.grad is None or need_env
    return out.detach().cpu(), i.grad.cpu(), (e.grad.cpu() if need_env else None)


@functools.lru_cache(maxsize=None)
def _blend_twin(H, W, C, dtype, need_env=True):
    return _blend_run(T.twin_blend, H, W, C, dtype, "cpu", need_env)


def _blend_pairs(H, W, C, need_env=True):
    t32, t64 = _blend_twin(H, W, C, torch.float32, need_env), _blend_twin(H, W, C, torch.float64, need_env)
    pairs = [("rgb", t32[0], t64[0], None, lambda r: r[0]), ("dimg[:3]", t32[1][:3], t64[1][:3], None, lambda r: r[1][:3]),
             ("dimg[3:C-1]", t32[1][3:C - 1], t64[1][3:C - 1], None, lambda r: r[1][3:C - 1])]
    if need_env:
        pairs.append(("drgb_env", t32[2], t64[2], None, lambda r: r[2]))
    return pairs


BLEND_CASES = ([(H, W, C, True) for H, W in PIXEL_SHAPES for C in (5, 7)]
               + [(H, W, C, False) for H, W in PIXEL_SHAPES if H * W in (255, 256, 257) for C in (5, 7)])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,need_env", BLEND_CASES, ids=["%d-%d-%d%s" % (c[0], c[1], c[2], "" if c[3] else "-no_env_gradient") for c in BLEND_CASES])
def test_blend_shape_ladder(H, W, C, need_env):
    """need_env False: drgb_env is a NULL pointer (at the three sizes around one workgroup)."""
    from envgs_amd import fused
    test = "glue_blend[%d-%d-%d]" % (H, W, C)
    run = _blend_run(fused.blend, H, W, C, torch.float32, torch.device("cuda:0"), need_env)
    for what, t32, t64, only, pick in _blend_pairs(H, W, C, need_env):
        _compare(test, what, pick(run), t32, t64, only)
    assert run[1].shape == (C, H, W) and not run[1][C - 1].any()
    assert (run[2] is None) == (not need_env)


# ---- the acc filter ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.75, 0.3])
@pytest.mark.parametrize("H,W", PIXEL_SHAPES)
def test_select_acc_keeps_exactly_alpha_above_the_threshold(H, W, thr):
    """keep = alpha > thr, strictly, in float32: pixels with alpha equal to the float32 threshold bit for bit and one float32 step on either side."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    allmap = _reflect_case(H, W)[1].clone()
    HW = H * W
    t32 = np.float32(thr)
    alpha = allmap[1].reshape(-1)                           # (a view)
    planted = [(HW - 1, t32)] + ([(0, np.nextafter(t32, np.float32(2.0))), (HW // 2, np.nextafter(t32, np.float32(-1.0)))] if HW >= 3 else [])
    for p, v in planted:
        alpha[p] = float(v)
    assert alpha[HW - 1].numpy().tobytes() == t32.tobytes()
    want = allmap[1].numpy() > t32
    assert not want.reshape(-1)[HW - 1] and (HW < 3 or (want.reshape(-1)[0] and not want.reshape(-1)[HW // 2]))
    sel = fused.select_pixels(allmap=allmap.to(dev), acc_threshold=thr)
    assert sel.mask.shape == (H, W) and sel.mask.dtype == torch.bool and np.array_equal(sel.mask.cpu().numpy(), want)
    assert np.array_equal(sel.keep.cpu().numpy(), want.reshape(-1).astype(np.uint8))
    assert sel.count == int(want.sum())
    assert np.array_equal(sel.positions.cpu().numpy()[:HW][want.reshape(-1)], np.arange(sel.count))


# ---- the bounce stage ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bounce_case(R, n, kind):
    return T.bounce_input(R, kind, seed=11 + R + n, n=(n if kind in ("random", "reversed") else None))


def _twin_bounce(o, d, dpt, acc, norm, aux, rgb, col_next, sel):
    return (*T.twin_bounce_rays(o, d, dpt, acc, norm, sel), T.twin_bounce_blend(rgb, aux, col_next, sel))


def _fused_bounce(o, d, dpt, acc, norm, aux, rgb, col_next, sel):
    from envgs_amd import fused
    return (*fused.bounce_rays(o, d, dpt, acc, norm, sel), fused.bounce_blend(rgb, aux, col_next, sel))


def _bounce_run(fn, R, n, kind, dtype, device, need, use):
    """-> (o2, d2, col), the eight gradients (None: that leaf needs none; zeros: nothing reached it)."""
    inp = _bounce_case(R, n, kind)
    mk = lambda t, g=False: t.to(device=device, dtype=dtype).clone().requires_grad_(g)
    L = [mk(inp[k], g) for k, g in zip(LEAVES, need)]
    outs = fn(*L, inp["sel"].to(device))
    assert [tuple(x.shape) for x in outs] == [(n, 3), (n, 3), (R, 3)] and all(x.dtype == dtype for x in outs)
    loss = sum((x * mk(inp[w])).sum() for x, w, u in zip(outs, ("up_o", "up_d", "up_c"), use) if u)
    if loss.requires_grad:
        loss.backward()
    for t, g in zip(L, need):
        assert t.grad is None or (g and t.grad.shape == t.shape and t.grad.dtype == dtype)
    grads = [((t.grad if t.grad is not None else torch.zeros_like(t)).cpu() if g else None) for t, g in zip(L, need)]
    return [x.detach().cpu() for x in outs], grads


@functools.lru_cache(maxsize=None)
def _bounce_twin(R, n, kind, dtype, need=ALL8, use=(True, True, True)):
    return _bounce_run(_twin_bounce, R, n, kind, dtype, "cpu", need, use)


def _bounce_pairs(R, n, kind, need=ALL8, use=(True, True, True)):
    inp = _bounce_case(R, n, kind)
    (o32, g32), (o64, g64) = _bounce_twin(R, n, kind, torch.float32, need, use), _bounce_twin(R, n, kind, torch.float64, need, use)
    pairs = [(nm, o32[i], o64[i], None, (lambda r, i=i: r[0][i])) for i, nm in enumerate(("o2", "d2", "col"))]
    for i, nm in enumerate(LEAVES):
        if need[i]:
            pairs.append(("g_" + nm, g32[i], g64[i], None, (lambda r, i=i: r[1][i])))
    if need[4] and "norm_tiny" in inp["planted"]:
        # the row with |norm| = 1e-12 carries a gradient 1e12 times the others' and sets the floor above: the other rows once more, by themselves
        rows = torch.ones(R, 1, dtype=torch.bool); rows[inp["planted"]["norm_tiny"]] = False
        pairs.append(("g_norm but tiny", g32[4], g64[4], rows, (lambda r: r[1][4])))
    return pairs


def _bounce_check(test, R, n, kind, need=ALL8, use=(True, True, True)):
    run = _bounce_run(_fused_bounce, R, n, kind, torch.float32, torch.device("cuda:0"), need, use)
    for what, t32, t64, only, pick in _bounce_pairs(R, n, kind, need, use):
        _compare(test, what, pick(run), t32, t64, only)
    inp = _bounce_case(R, n, kind)
    out = torch.ones(R, dtype=torch.bool); out[inp["sel"]] = False
    (o2, d2, col), g = run
    assert _bits(col[out], inp["rgb"][out])                                   # rows that do not bounce: the colour itself
    for i in range(5):                                                        # ... and exactly nothing for the ray side
        assert g[i] is None or not g[i][out].any(), LEAVES[i]
    assert g[5] is None or (not g[5][out].any() and not g[5][:, 1].any())
    if g[6] is not None:                                                      # the colour gradient passes through bit for bit
        assert _bits(g[6][out], inp["up_c"][out]) if use[2] else not g[6].any()
    if n == 0:
        assert _bits(col, inp["rgb"]) and o2.shape == d2.shape == (0, 3) and (g[7] is None or g[7].shape == (0, 3))
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("R,n,kind", ROW_CASES, ids=["%d-%d-%s" % c for c in ROW_CASES])
def test_bounce_row_ladder(R, n, kind):
    _bounce_check("glue_bounce[%d-%d-%s]" % (R, n, kind), R, n, kind)


_only = lambda *names: tuple(k in names for k in LEAVES)
BOUNCE_ALONE = ([("%s_alone" % k, _only(k), (True, True, True)) for k in LEAVES]
                + [("o2_only", ALL8, (True, False, False)), ("d2_only", ALL8, (False, True, False)),
                   ("col_next_without_gradient", _only(*LEAVES[:7]), (True, True, True)),
                   ("camera_rays_without_gradient", _only(*LEAVES[2:]), (True, True, True))])


@pytest.mark.gpu
@pytest.mark.parametrize("case", BOUNCE_ALONE, ids=[c[0] for c in BOUNCE_ALONE])
def test_bounce_one_leaf_one_upstream_at_a_time(case):
    """A leaf that needs no gradient reaches the backward kernels as a NULL pointer (the product step: stage 0's camera rays)."""
    name, need, use = case
    _bounce_check("glue_bounce_alone[%s]" % name, 300, 257, "random", need, use)


def _stage_rows(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, w, generator=gen) for w in (3, 3, 1, 1, 3, 2, 3)]


@pytest.mark.gpu
def test_bounce_pack_mid_is_the_cat_form():
    """Stage 0 at every row (idx = None), stage 1 at the rows of a descending sel, stage 2 at every other of those: bit for bit torch.cat, and the
    columns and rows no call names still hold what they held."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    R = 300
    sel = _bounce_case(R, 257, "reversed")["sel"]
    sel2 = sel[::2]
    assert sel.numel() == 257 and sel2.numel() == 129
    before = torch.randn(R, 48, generator=torch.Generator().manual_seed(5))
    st = [_stage_rows(R, 1), _stage_rows(257, 2), _stage_rows(129, 3)]
    mid = before.to(dev)
    want = before.clone()
    for k, (rows, idx) in enumerate(zip(st, (None, sel, sel2))):
        fused.bounce_pack_mid(mid, k, 3, None if idx is None else idx.to(dev), *[t.to(dev) for t in rows])
        want[torch.arange(R) if idx is None else idx, 16 * k:16 * k + 16] = torch.cat(rows, 1)
        assert _bits(mid, want), k
    untouched = torch.ones(R, dtype=torch.bool); untouched[sel] = False
    assert _bits(mid.cpu()[untouched, 16:], before[untouched, 16:]) and int(untouched.sum()) == 43


# ---- the quads -----------------------------------------------------------------------------------------------------------------------------------
_quads_case = functools.lru_cache(maxsize=None)(T.quads_input)


@functools.lru_cache(maxsize=None)
def _quads_twin(P, dtype):
    v, f = synth.get_disks(*[t.to(dtype) for t in _quads_case(P)])
    assert v.dtype == dtype
    return v, f


@pytest.mark.gpu
@pytest.mark.parametrize("P", QUAD_P)
def test_surfel_quads_ladder(P):
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    m, s, q = [t.to(dev) for t in _quads_case(P)]
    v, f = fused.surfel_quads(m, s, q)
    (v32, f32), (v64, _) = _quads_twin(P, torch.float32), _quads_twin(P, torch.float64)
    assert v.shape == (4 * P, 3) and f.shape == (2 * P, 3) and f.dtype == torch.int32
    assert _bits(f, f32)                                                      # faces are exact
    _compare("glue_quads[%d]" % P, "vertices", v, v32, v64)
    v2, f2 = fused.surfel_quads(m, s, q)
    assert f2 is f and _bits(v2, v)                                           # the cached table, the same vertices


@pytest.mark.gpu
def test_surfel_quads_cache_evicts_but_a_held_table_keeps_its_values():
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    call = lambda P: fused.surfel_quads(*[t.to(dev) for t in _quads_case(P)])[1]
    held = call(33)
    for P in range(2, 12):                                                    # ten other sizes: more than the cache keeps
        assert _bits(call(P), _quads_twin(P, torch.float32)[1])
    assert (dev.index, 33) not in fused._FACES and len(fused._FACES) <= 8
    assert _bits(held, _quads_twin(33, torch.float32)[1])
    again = call(33)
    assert again is not held and _bits(again, held)


# ---- nothing is written beyond the size, everything below it: the C ABI on guarded buffers --------------------------------------------------------
CANARY = 0x7FA5A5A5          # a NaN no arithmetic here produces
MARK = 123.25                # a finite value no result here equals: buffers a kernel writes only some rows of
GUARD = 4096


class _Guarded:
    """n float32 (or int32) elements followed by GUARD canary words.  head: None = the NaN canary; a float = that value."""

    def __init__(self, n, dev, head=None):
        self.n = n
        self.raw = torch.full((n + GUARD,), CANARY, dtype=torch.int32, device=dev)
        if head is not None:
            self.raw[:n].view(torch.float32).fill_(head)

    def ptr(self):
        return self.raw.data_ptr()

    def head(self, shape, dtype=torch.float32):
        """The tail must be untouched -> the n elements, on the host."""
        host = self.raw.cpu()
        assert bool((host[self.n:] == CANARY).all()), "written beyond its %d elements" % self.n
        return host[:self.n].view(dtype).reshape(shape)


def _written(t):
    assert bool(torch.isfinite(t).all()), "elements left unwritten"
    return t


@pytest.fixture
def abi():
    from envgs_amd import _lib
    dev = torch.device("cuda:0")
    return _lib.load(), dev, _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream), (lambda t: None if t is None else _lib.c_void_p(t.data_ptr()))


@pytest.mark.gpu
def test_c_abi_reflect_on_guarded_buffers(abi):
    from envgs_amd import fused
    lib, dev, st, p = abi
    H, W = 1, 257
    cam, allmap, ro, rd, _, ws = _reflect_case(H, W)
    a, o, d, V = allmap.to(dev), ro.to(dev), rd.to(dev), cam.world_view_transform.to(dev)
    front = _reflect_run(fused.reflect, H, W, RATIO, torch.float32, dev, ALL4, (True, True))
    shapes = [(3, H, W), (1, H, W), (H, W, 3), (H, W, 3)]
    bufs = [_Guarded(int(np.prod(s)), dev) for s in shapes]
    assert lib.envgs_reflect_forward(H, W, RATIO, p(a), p(o), p(d), p(V), *[b.ptr() for b in bufs], st) == 0
    torch.cuda.synchronize()
    for b, s, ref in zip(bufs, shapes, front[0]):
        assert _bits(_written(b.head(s)), ref)
    up = [w.to(dev) for w in ws]
    gshapes = [(7, H, W), (H, W, 3), (H, W, 3)]
    g = [_Guarded(int(np.prod(s)), dev) for s in gshapes]
    assert lib.envgs_reflect_backward(H, W, RATIO, p(a), p(o), p(d), p(V), *[p(u) for u in up], *[b.ptr() for b in g], st) == 0
    torch.cuda.synchronize()
    for b, s, ref in zip(g, gshapes, front[1]):
        assert _bits(_written(b.head(s)), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [5, 7])
def test_c_abi_blend_on_guarded_buffers(abi, C):
    from envgs_amd import fused
    lib, dev, st, p = abi
    H, W = 1, 257
    img, env, up = [t.to(dev) for t in _blend_case(H, W, C)]
    front = _blend_run(fused.blend, H, W, C, torch.float32, dev)
    rgb = _Guarded(3 * H * W, dev)
    assert lib.envgs_blend_forward(H, W, C, p(img), p(env), rgb.ptr(), st) == 0
    dimg, denv = _Guarded(C * H * W, dev), _Guarded(3 * H * W, dev)
    assert lib.envgs_blend_backward(H, W, C, p(img), p(env), p(up), dimg.ptr(), denv.ptr(), st) == 0
    torch.cuda.synchronize()
    assert _bits(_written(rgb.head((H, W, 3))), front[0])
    assert _bits(_written(dimg.head((C, H, W))), front[1]) and _bits(_written(denv.head((H, W, 3))), front[2])


@pytest.mark.gpu
def test_c_abi_select_acc_on_a_guarded_buffer(abi):
    lib, dev, st, p = abi
    H, W = 1, 257
    allmap = _reflect_case(H, W)[1]
    keep = torch.full((H * W + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    a = allmap.to(dev)
    assert lib.envgs_select_acc(H, W, 0.75, p(a), p(keep), st) == 0
    host = keep.cpu().numpy()
    assert (host[H * W:] == 0xA5).all() and np.array_equal(host[:H * W], (allmap[1].numpy().reshape(-1) > np.float32(0.75)).astype(np.uint8))


@pytest.mark.gpu
def test_c_abi_bounce_on_guarded_buffers(abi):
    """The forward entries write their n rows (o2, d2) or the rows of sel (col); the backward entries write ONLY the rows of sel: buffers filled
    with a mark, not zeros, still hold it everywhere else."""
    lib, dev, st, p = abi
    R, n, kind = 300, 257, "random"
    inp = _bounce_case(R, n, kind)
    front = _bounce_run(_fused_bounce, R, n, kind, torch.float32, dev, ALL8, (True, True, True))
    t = {k: inp[k].to(dev) for k in LEAVES + ("sel", "up_o", "up_d", "up_c")}
    sel = inp["sel"]
    out = torch.ones(R, dtype=torch.bool); out[sel] = False
    o2, d2, col = _Guarded(3 * n, dev), _Guarded(3 * n, dev), _Guarded(3 * R, dev, head=MARK)
    ray = [p(t[k]) for k in ("o", "d", "dpt", "acc", "norm")]
    assert lib.envgs_bounce_rays_forward(n, p(t["sel"]), *ray, o2.ptr(), d2.ptr(), st) == 0
    assert lib.envgs_bounce_blend_forward(n, p(t["sel"]), p(t["rgb"]), p(t["aux"]), p(t["col_next"]), col.ptr(), st) == 0
    widths = (3, 3, 1, 1, 3)
    g = [_Guarded(R * w, dev, head=MARK) for w in widths]
    assert lib.envgs_bounce_rays_backward(n, p(t["sel"]), *ray, p(t["up_o"]), p(t["up_d"]), *[b.ptr() for b in g], st) == 0
    g_rgb, g_aux, g_next = _Guarded(3 * R, dev, head=MARK), _Guarded(2 * R, dev, head=MARK), _Guarded(3 * n, dev)
    assert lib.envgs_bounce_blend_backward(n, p(t["sel"]), p(t["rgb"]), p(t["aux"]), p(t["col_next"]), p(t["up_c"]), g_rgb.ptr(), g_aux.ptr(),
                                           g_next.ptr(), st) == 0
    torch.cuda.synchronize()
    assert _bits(_written(o2.head((n, 3))), front[0][0]) and _bits(_written(d2.head((n, 3))), front[0][1])
    c = col.head((R, 3))
    assert _bits(c[sel], front[0][2][sel]) and bool((c[out] == MARK).all())
    for b, w, ref, nm in zip(g, widths, front[1][:5], LEAVES):
        h = b.head((R, w))
        assert _bits(h[sel], ref[sel]) and bool((h[out] == MARK).all()), nm
    h = g_rgb.head((R, 3))
    assert _bits(h[sel], front[1][6][sel]) and bool((h[out] == MARK).all())
    h = g_aux.head((R, 2))
    assert _bits(h[sel, 0], front[1][5][sel, 0]) and bool((h[out] == MARK).all()) and bool((h[:, 1] == MARK).all())
    assert _bits(_written(g_next.head((n, 3))), front[1][7])


@pytest.mark.gpu
def test_c_abi_pack_mid_and_quads_on_guarded_buffers(abi):
    from envgs_amd import fused
    lib, dev, st, p = abi
    R, n = 300, 257
    sel = _bounce_case(R, n, "random")["sel"]
    rows = _stage_rows(n, 7)
    mid = _Guarded(R * 32, dev, head=MARK)
    idx, on_dev = sel.to(dev), [t.to(dev) for t in rows]                       # (held: the call takes bare addresses)
    assert lib.envgs_bounce_pack_mid(n, p(idx), 2, 1, *[p(t) for t in on_dev], mid.ptr(), st) == 0
    torch.cuda.synchronize()
    want = torch.full((R, 32), MARK)
    want[sel, 16:] = torch.cat(rows, 1)
    assert _bits(mid.head((R, 32)), want)
    P = 257
    m, s, q = [t.to(dev) for t in _quads_case(P)]
    v, f = _Guarded(12 * P, dev), _Guarded(6 * P, dev)
    assert lib.envgs_surfel_quads(P, p(m), p(s), p(q), v.ptr(), f.ptr(), st) == 0
    torch.cuda.synchronize()
    v2, f2 = fused.surfel_quads(m, s, q)
    assert _bits(_written(v.head((4 * P, 3))), v2) and _bits(f.head((2 * P, 3), torch.int32), f2)


# ---- layouts and dtypes through the front ends -----------------------------------------------------------------------------------------------------
def _inside(t, pad=(1, 0, 2), tail=(1, 0, 3)):
    """t as a strided view with a storage offset of a larger tensor (same values)."""
    big = torch.full([a + s + b for a, s, b in zip(pad, t.shape, tail)], 7.5, dtype=t.dtype, device=t.device)
    view = big[tuple(slice(a, a + s) for a, s in zip(pad, t.shape))]
    view.copy_(t)
    assert not view.is_contiguous() and view.storage_offset() > 0
    return view


@pytest.mark.gpu
def test_reflect_converts_layouts_and_dtypes():
    """allmap as a strided view with a storage offset, the rays in float64: bit for bit the contiguous float32 call, gradients in the inputs' dtype
    and shape."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    H, W = 19, 27
    cam, allmap, ro, rd, _, ws = _reflect_case(H, W)
    plain = _reflect_run(fused.reflect, H, W, RATIO, torch.float32, dev, ALL4, (True, True))
    a = _inside(allmap.to(dev)).requires_grad_(True)
    o, d = ro.to(dev).double().requires_grad_(True), rd.to(dev).double().requires_grad_(True)
    outs = fused.reflect(a, o, d, cam.world_view_transform.to(dev).double().T.contiguous().T, RATIO)
    sum((x * w.to(dev)).sum() for x, w in zip(outs, ws)).backward()
    for x, ref in zip(outs, plain[0]):
        assert x.dtype == torch.float32 and _bits(x, ref)
    assert a.grad.dtype == torch.float32 and _bits(a.grad, plain[1][0])
    for t, ref in ((o, plain[1][1]), (d, plain[1][2])):
        assert t.grad.dtype == torch.float64 and t.grad.shape == (H, W, 3) and _bits(t.grad, ref.double())


@pytest.mark.gpu
@pytest.mark.parametrize("C", [5, 7])
def test_blend_converts_layouts_and_shapes(C):
    """img as a strided view with a storage offset, rgb_env as (1, HW, 3)."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    H, W = 3, 85
    img, env, up = _blend_case(H, W, C)
    plain = _blend_run(fused.blend, H, W, C, torch.float32, dev)
    i = _inside(img.to(dev)).requires_grad_(True)
    e = env.to(dev).reshape(1, H * W, 3).clone().requires_grad_(True)
    out = fused.blend(i, e)
    (out * up.to(dev)).sum().backward()
    assert _bits(out, plain[0]) and _bits(i.grad, plain[1])
    assert e.grad.shape == (1, H * W, 3) and _bits(e.grad.reshape(H, W, 3), plain[2])


@pytest.mark.gpu
def test_bounce_rays_converts_layouts_and_dtypes():
    """sel as a non-contiguous view, the rays in float64, norm as a strided view."""
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    R, n, kind = 300, 257, "random"
    inp = _bounce_case(R, n, kind)
    plain = _bounce_run(_fused_bounce, R, n, kind, torch.float32, dev, ALL8, (True, True, False))
    sel = torch.stack([inp["sel"], inp["sel"] + 1], 1).to(dev)[:, 0]
    assert not sel.is_contiguous() and sel.dim() == 1
    o, d = inp["o"].to(dev).double().requires_grad_(True), inp["d"].to(dev).double().requires_grad_(True)
    dpt, acc = inp["dpt"].to(dev).requires_grad_(True), inp["acc"].to(dev).requires_grad_(True)
    norm = _inside(inp["norm"].to(dev), (2, 1), (0, 2)).requires_grad_(True)
    o2, d2 = fused.bounce_rays(o, d, dpt, acc, norm, sel)
    ((o2 * inp["up_o"].to(dev)).sum() + (d2 * inp["up_d"].to(dev)).sum()).backward()
    assert o2.dtype == torch.float32 and _bits(o2, plain[0][0]) and _bits(d2, plain[0][1])
    for t, ref, dt in ((o, plain[1][0], torch.float64), (d, plain[1][1], torch.float64), (dpt, plain[1][2], torch.float32),
                       (acc, plain[1][3], torch.float32), (norm, plain[1][4], torch.float32)):
        assert t.grad.dtype == dt and t.grad.shape == t.shape and _bits(t.grad, ref.to(dt))


@pytest.mark.gpu
def test_bounce_rays_takes_upstreams_that_are_not_contiguous():
    """2 sum(o2) + 3 sum(d2): both upstream gradients arrive as expanded scalars and are converted inside the backward.  Bit for bit the call whose
    upstreams are contiguous tensors of 2 and 3.  (The two converted copies used to be temporaries of the argument list: the first was freed
    before the second was made, the second took its block, and the kernel read 3 through both pointers.)"""
    dev = torch.device("cuda:0")
    R, n, kind = 300, 257, "random"
    inp = _bounce_case(R, n, kind)
    grads = []
    for expanded in (False, True):
        L = [inp[k].to(dev).requires_grad_(True) for k in LEAVES[:5]]
        o2, d2 = _fused_bounce(*L, *[inp[k].to(dev) for k in LEAVES[5:]], inp["sel"].to(dev))[:2]
        if expanded:
            (2.0 * o2.sum() + 3.0 * d2.sum()).backward()
        else:
            ((o2 * torch.full_like(o2, 2.0)).sum() + (d2 * torch.full_like(d2, 3.0)).sum()).backward()
        grads.append([t.grad.cpu() for t in L])
    for nm, a, b in zip(LEAVES, *grads):
        assert _bits(a, b), nm
    assert bool((grads[1][0][inp["sel"]] == 2.0).all())                        # g_o is g_o2 itself


# ---- without a GPU: the twins, their float32 errors, the argument checks ---------------------------------------------------------------------------
def test_twins_are_the_restated_expressions_in_float32():
    """Each twin, in float32 on the CPU, bit for bit the expressions tests/test_fused_glue.py (test_reflect_matches_torch, test_blend_matches_torch,
    test_bounce_stage_glue_matches_torch_f64) compare the kernels with: values and autograd gradients (NaN where torch's own backward of
    nan_to_num(0 / 0) is NaN).  float64 inputs give float64 outputs."""
    same = lambda x, y: x.dtype == y.dtype and torch.allclose(x, y, rtol=0, atol=0, equal_nan=True)
    for H, W in ((19, 27), (5, 13), (1, 1)):
        cam, allmap, ro, rd, px, ws = _reflect_case(H, W)
        for ratio in (0.0, 0.3, 1.0):
            a2 = allmap.clone().requires_grad_(True); o2 = ro.clone().requires_grad_(True); d2 = rd.clone().requires_grad_(True)
            alpha = a2[1:2]
            nw2 = (a2[2:5].permute(1, 2, 0) @ cam.world_view_transform[:3, :3].T).permute(2, 0, 1)
            de = torch.nan_to_num(a2[0:1] / alpha, 0, 0); dm = torch.nan_to_num(a2[5:6], 0, 0)
            dep2 = de * (1 - ratio) + dm * ratio
            n = nw2.permute(1, 2, 0); n = n / (n.norm(dim=-1, keepdim=True) + 1e-8)
            ref_d2 = d2 - 2 * (d2 * n).sum(-1, keepdim=True) * n
            ref_o2 = o2 + d2 * dep2.permute(1, 2, 0)
            sum((x * w).sum() for x, w in zip((nw2, dep2, ref_o2, ref_d2), ws)).backward()
            outs, grads = _reflect_twin(H, W, ratio, torch.float32)
            assert all(same(x, y.detach()) for x, y in zip(outs, (nw2, dep2, ref_o2, ref_d2)))
            assert all(same(x, y.grad) for x, y in zip(grads, (a2, o2, d2)))
            if H * W >= 70:                                 # every planted kind is there, and torch's NaN sits where the docstrings say
                assert all(bool(m.any()) for m in px.values())
                assert bool(torch.isnan(grads[0][:2][:, px["empty"] | px["inf"]]).all()) and bool(torch.isfinite(grads[0][2:]).all())
        assert all(x.dtype == torch.float64 for x in _reflect_twin(H, W, 0.3, torch.float64)[0] + _reflect_twin(H, W, 0.3, torch.float64)[1])
    for C in (5, 7):
        H, W, S = 5, 13, C - 4
        img0, env0, up = _blend_case(H, W, C)
        img = img0.clone().requires_grad_(True); env = env0.clone().requires_grad_(True)
        spec = img[3:3 + S].permute(1, 2, 0)
        ref = (1 - spec) * img[:3].permute(1, 2, 0) + spec * env
        (ref * up).sum().backward()
        out, gi, ge = _blend_twin(H, W, C, torch.float32)
        assert same(out, ref.detach()) and same(gi, img.grad) and same(ge, env.grad)
        assert all(x.dtype == torch.float64 for x in _blend_twin(H, W, C, torch.float64))
    for R, n, kind in ((300, 257, "random"), (600, 350, "reversed"), (7, 0, "none")):
        inp = _bounce_case(R, n, kind)
        o_, d_, dpt_, acc_, norm_, aux_, rgb_, cn_ = L = [inp[k].clone().requires_grad_(True) for k in LEAVES]
        s_ = inp["sel"]
        nh = norm_[s_] / norm_[s_].norm(dim=-1, keepdim=True)
        o2 = o_[s_] + d_[s_] * (dpt_[s_] / acc_[s_])
        d2 = d_[s_] - 2.0 * (d_[s_] * nh).sum(-1, keepdim=True) * nh
        sp = aux_[s_, 0:1]
        col = rgb_.index_put((s_,), (1.0 - sp) * rgb_[s_] + sp * cn_)
        ((o2 * inp["up_o"]).sum() + (d2 * inp["up_d"]).sum() + (col * inp["up_c"]).sum()).backward()
        outs, grads = _bounce_twin(R, n, kind, torch.float32)
        assert all(same(x, y.detach()) for x, y in zip(outs, (o2, d2, col)))
        assert all(same(x, y.grad) for x, y in zip(grads, L))
        assert all(x.dtype == torch.float64 for x in _bounce_twin(R, n, kind, torch.float64)[0] + _bounce_twin(R, n, kind, torch.float64)[1])
    assert _quads_twin(257, torch.float64)[0].dtype == torch.float64 and _quads_twin(257, torch.float32)[1].dtype == torch.int32


def test_every_bound_is_known_without_a_gpu(capsys):
    """Builds every input of the ladders (the planted-row budgets are asserted inside the helpers) and evaluates e_twin32 for every compared
    tensor: the bound  max(1e-4, K_F32 * e_twin32)  of every GPU comparison above is fixed here, on the CPU.  Printed: the tensors whose
    e_twin32 exceeds 1e-4 / K_F32, for which the bound leaves 1e-4."""
    table = {}

    def note(entry, pairs):
        for what, t32, t64, only, _ in pairs:
            e = _twin_error(t32, t64, only)[1]
            if e is not None:
                assert np.isfinite(e)
                table[(entry, what)] = max(table.get((entry, what), 0.0), e)

    for H, W in PIXEL_SHAPES:
        note("reflect", _reflect_pairs(H, W, RATIO))
        for C in (5, 7):
            note("blend", _blend_pairs(H, W, C))
    for _, ratio, use, need in REFLECT_ALONE:
        note("reflect", _reflect_pairs(19, 27, ratio, use, need))
    for R, n, kind in ROW_CASES:
        note("bounce", _bounce_pairs(R, n, kind))
    for _, need, use in BOUNCE_ALONE:
        note("bounce", _bounce_pairs(300, 257, "random", need, use))
    for P in QUAD_P:
        note("quads", [("vertices", _quads_twin(P, torch.float32)[0], _quads_twin(P, torch.float64)[0], None, None)])
    with capsys.disabled():
        for (entry, what), e in sorted(table.items()):
            print("e_twin32  %-8s %-22s %.3e%s" % (entry, what, e, "   -> bound %.3e" % (K_F32 * e) if K_F32 * e > 1e-4 else ""))
    assert {"reflect", "blend", "bounce", "quads"} == {k[0] for k in table}


class _NoLibrary:
    def __getattr__(self, name):
        pytest.fail("the front end reached the library (%s) with arguments it should have refused" % name)


def test_front_ends_refuse_bad_arguments_before_the_library(monkeypatch):
    """CPU tensors only, and the library replaced by a stub that fails the test when touched: every malformed call raises ValueError, a well-formed
    one RuntimeError (no CPU path); nothing here could launch a kernel even if a check were missing."""
    from envgs_amd import _lib, fused
    monkeypatch.setattr(_lib, "load", lambda: _NoLibrary())
    H, W, R, n = 4, 6, 10, 5
    z = lambda *s: torch.zeros(*s)
    V = torch.eye(4)
    sel = torch.arange(n)
    meta_sel = torch.empty(n, dtype=torch.int64, device="meta")
    ray = lambda R=R: dict(ray_o=z(R, 3), ray_d=z(R, 3), dpt=z(R, 1), acc=z(R, 1), norm=z(R, 3))
    stage = lambda n=n: dict(ray_o=z(n, 3), ray_d=z(n, 3), dpt=z(n, 1), acc=z(n, 1), norm=z(n, 3), aux=z(n, 2), rgb=z(n, 3))
    good = {
        "reflect": lambda: fused.reflect(z(7, H, W), z(H, W, 3), z(H, W, 3), V),
        "blend": lambda: fused.blend(z(5, H, W), z(H, W, 3)),
        "blend7": lambda: fused.blend(z(7, H, W), z(1, H * W, 3)),
        "bounce_rays": lambda: fused.bounce_rays(sel=sel, **ray()),
        "bounce_blend": lambda: fused.bounce_blend(z(R, 3), z(R, 2), z(n, 3), sel),
        "bounce_pack_mid": lambda: fused.bounce_pack_mid(z(R, 32), 1, 2, sel, **stage()),
        "bounce_pack_mid0": lambda: fused.bounce_pack_mid(z(R, 32), 0, 2, None, **stage(R)),
        "surfel_quads": lambda: fused.surfel_quads(z(R, 3), z(R, 2), z(R, 4)),
    }
    for name, call in good.items():
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    bad = {
        "reflect: (6,H,W) allmap": lambda: fused.reflect(z(6, H, W), z(H, W, 3), z(H, W, 3), V),
        "reflect: 2-D allmap": lambda: fused.reflect(z(7, H * W), z(H, W, 3), z(H, W, 3), V),
        "reflect: short ray_o": lambda: fused.reflect(z(7, H, W), z(H, W - 1, 3), z(H, W, 3), V),
        "reflect: short ray_d": lambda: fused.reflect(z(7, H, W), z(H, W, 3), z(H * W, 2), V),
        "reflect: 3x3 view matrix": lambda: fused.reflect(z(7, H, W), z(H, W, 3), z(H, W, 3), torch.eye(3)),
        "reflect: rays on another device": lambda: fused.reflect(z(7, H, W), torch.empty(H, W, 3, device="meta"), z(H, W, 3), V),
        "blend: 6 channels": lambda: fused.blend(z(6, H, W), z(H, W, 3)),
        "blend: 3 channels": lambda: fused.blend(z(3, H, W), z(H, W, 3)),
        "blend: short rgb_env": lambda: fused.blend(z(5, H, W), z(H * W - 1, 3)),
        "blend: (H,W) img": lambda: fused.blend(z(H, W), z(H, W, 3)),
        "bounce_rays: row counts": lambda: fused.bounce_rays(sel=sel, **dict(ray(), acc=z(R - 1, 1))),
        "bounce_rays: norm rows": lambda: fused.bounce_rays(sel=sel, **dict(ray(), norm=z(R + 1, 3))),
        "bounce_rays: dpt width": lambda: fused.bounce_rays(sel=sel, **dict(ray(), dpt=z(R, 3))),
        "bounce_rays: 1-D acc": lambda: fused.bounce_rays(sel=sel, **dict(ray(), acc=z(R))),
        "bounce_rays: ray_d width": lambda: fused.bounce_rays(sel=sel, **dict(ray(), ray_d=z(R, 4))),
        "bounce_rays: int32 sel": lambda: fused.bounce_rays(sel=sel.int(), **ray()),
        "bounce_rays: bool sel": lambda: fused.bounce_rays(sel=torch.ones(R, dtype=torch.bool), **ray()),
        "bounce_rays: 2-D sel": lambda: fused.bounce_rays(sel=sel[:, None], **ray()),
        "bounce_rays: sel on another device": lambda: fused.bounce_rays(sel=meta_sel, **ray()),
        "bounce_blend: col_next rows": lambda: fused.bounce_blend(z(R, 3), z(R, 2), z(n + 1, 3), sel),
        "bounce_blend: col_next width": lambda: fused.bounce_blend(z(R, 3), z(R, 2), z(n, 2), sel),
        "bounce_blend: aux width": lambda: fused.bounce_blend(z(R, 3), z(R, 1), z(n, 3), sel),
        "bounce_blend: aux rows": lambda: fused.bounce_blend(z(R, 3), z(R - 1, 2), z(n, 3), sel),
        "bounce_blend: int32 sel": lambda: fused.bounce_blend(z(R, 3), z(R, 2), z(n, 3), sel.int()),
        "bounce_blend: 2-D sel": lambda: fused.bounce_blend(z(R, 3), z(R, 2), z(n, 3), sel[None]),
        "bounce_blend: sel on another device": lambda: fused.bounce_blend(z(R, 3), z(R, 2), z(n, 3), meta_sel),
        "pack_mid: mid a column slice": lambda: fused.bounce_pack_mid(z(R, 48)[:, :32], 1, 2, sel, **stage()),
        "pack_mid: mid float64": lambda: fused.bounce_pack_mid(z(R, 32).double(), 1, 2, sel, **stage()),
        "pack_mid: mid of another width": lambda: fused.bounce_pack_mid(z(R, 16), 1, 2, sel, **stage()),
        "pack_mid: mid 1-D": lambda: fused.bounce_pack_mid(z(R * 32), 1, 2, sel, **stage()),
        "pack_mid: mid transposed": lambda: fused.bounce_pack_mid(z(32, 32).T, 1, 2, torch.arange(n), **stage()),
        "pack_mid: k = stages": lambda: fused.bounce_pack_mid(z(R, 32), 2, 2, sel, **stage()),
        "pack_mid: k = -1": lambda: fused.bounce_pack_mid(z(R, 32), -1, 2, sel, **stage()),
        "pack_mid: stages = 0": lambda: fused.bounce_pack_mid(z(R, 0), 0, 0, sel, **stage()),
        "pack_mid: int32 idx": lambda: fused.bounce_pack_mid(z(R, 32), 1, 2, sel.int(), **stage()),
        "pack_mid: 2-D idx": lambda: fused.bounce_pack_mid(z(R, 32), 1, 2, sel[:, None], **stage()),
        "pack_mid: idx on another device": lambda: fused.bounce_pack_mid(z(R, 32), 1, 2, meta_sel, **stage()),
        "pack_mid: idx count": lambda: fused.bounce_pack_mid(z(R, 32), 1, 2, torch.arange(n + 1), **stage()),
        "pack_mid: aux width": lambda: fused.bounce_pack_mid(z(R, 32), 1, 2, sel, **dict(stage(), aux=z(n, 3))),
        "pack_mid: rgb rows": lambda: fused.bounce_pack_mid(z(R, 32), 1, 2, sel, **dict(stage(), rgb=z(n - 1, 3))),
        "pack_mid: more rows than mid": lambda: fused.bounce_pack_mid(z(R, 32), 0, 2, None, **stage(R + 1)),
        "surfel_quads: scales width": lambda: fused.surfel_quads(z(R, 3), z(R, 3), z(R, 4)),
        "surfel_quads: rotations rows": lambda: fused.surfel_quads(z(R, 3), z(R, 2), z(R - 1, 4)),
    }
    for name, call in bad.items():
        try:
            call()
        except ValueError:
            continue
        except Exception as e:
            pytest.fail("%s: %s instead of ValueError: %s" % (name, type(e).__name__, e))
        pytest.fail("%s: accepted" % name)
