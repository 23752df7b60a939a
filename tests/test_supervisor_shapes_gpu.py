"""The fused geometry loss (envgs_amd/csrc/supervisor.hip, envgs_amd.loss.EnvGSGeometryLoss) where its pixel count is no multiple of the 256-thread
workgroup, term by term.  tests/test_supervisor_loss.py compares it at 3072 and 640 000 pixels, both whole numbers of workgroups; here the last
workgroup is partly empty (the `i < N` guard, the zero lanes of the wave sums, the short block's partial row, the gradient stores next to row N),
a term or a leaf runs alone (NULL input pointers, NULL gradient maps), the maps arrive strided, and the two depth percentiles coincide.

Inputs: tests/test_supervisor_loss.py:_full_inputs cut to (N, P), plus planted rows (_inputs).  What makes a float32 answer differ from the float64
twin by a DECISION rather than by rounding is kept out of the inputs and asserted on them (test_inputs_have_stated_margins), not allowed for
afterwards: outside the planted rows no component of a - g is within 1e-5 of 0 (the sign in the L1 part), | |norm| - 0.25 | > 1e-4 (the mask),
far > near, and no opacity within 1e-6 of a clamp bound.  The planted rows sit EXACTLY on those decisions, where float32 and float64 agree
because nothing is rounded: norm_map == 0, norm == 0.5 (a zero prior), msk == 0.5, norm == (0.25, 0, 0), env_opacity in {0, 1, float32(1e-3),
float32(0.999)} and, under R = identity, norm_map.x == 0 with norm.x == 0.5 (a.x - g.x == 0 exactly).  No pixel is left out of a comparison.

Bars: the loss and the term means 1e-4 relative (the bar of tests/test_supervisor_loss.py); gradients on the pixels with norm_map != 0 and on
env_opacity tests/util.py:check_close at its TOL (elementwise, floored at the tensor's mean magnitude); the pixels with norm_map == 0, whose
gradient is amplified by 1e8 three times, the max-norm rule _check_grads applies at full size; wherever the twin's gradient is exactly 0 the
device's is; two runs agree bit for bit.  test_float32_twin_stays_inside_the_bar shows that float32 arithmetic itself -- the twin evaluated in
float32 -- uses about a hundredth of these bars."""
import functools

import numpy as np
import pytest
import torch

from tests import reference_supervisor as twin
from tests.test_supervisor_loss import _check_grads, _full_inputs, _to_dev
from tests.util import check_close, record

F32 = np.float32
IT = 5
TERMS = ("norm_loss", "gs_norm_loss", "msk_loss", "gs_dist_loss", "env_opacity_loss")              # the columns of envgs_supervisor_finish's output
LEAVES = ("norm_map", "surf_norm_map", "acc_map", "dist_map", "env_opacity")
ENV_PLANTED = np.array([0.0, 1.0, F32(1e-3), F32(0.999)], F32)

# (N, P, seed, depth scale, R = identity).  N in 100..199 has n = int(0.01 N) = 1; 255 / 256 / 257 straddle one workgroup; 3073 = 12 workgroups + 1 pixel.
# Without the depth scale N < 100 is legal: one pixel, two, and one wavefront - 1 / exactly / + 1.  The seeds are those for which the margins of
# test_inputs_have_stated_margins hold (seed = N does for every entry).
LADDER = [(100, 1, 100, True, False), (101, 255, 101, True, False), (199, 63, 199, True, False), (255, 256, 255, True, False),
          (256, 257, 256, True, False), (257, 1000, 257, True, True), (319, 7, 319, True, False), (3073, 300, 3073, True, False)]
SMALL = [(N, 1, N, False, False) for N in (1, 2, 63, 64, 65, 99)]
ENTRIES = LADDER + SMALL
ALONE_ENTRY = (319, 257, 7, True, False)                # test_each_term_alone, test_each_leaf_alone_...: 11 x 29 pixels
COINCIDING_ENTRY = (300, 1, 300, True, False)           # test_coinciding_percentiles_...: the depths are replaced there
_ids = lambda e: "N%d-P%d%s" % (e[0], e[1], "-identity" if e[4] else "")


@functools.lru_cache(maxsize=None)
def _inputs(N, P, seed, identity=False):
    """-> (inputs as the twin's rows, planted: (N,) bool, env_planted: (P,) bool).  _full_inputs needs N >= 100 and P >= 100 (its percentile ties,
    its opacity blocks): it is drawn at least that large and cut."""
    full = _full_inputs(1, max(N, 100), P + 100, seed)
    inp = {k: full[k][:N].copy() for k in ("norm_map", "surf_norm_map", "acc_map", "dpt_map", "dist_map", "norm", "msk")}
    env = full["env_opacity"][100:].copy()                                      # P interior values ...
    env_planted = np.zeros(P, bool)
    if P >= 4:
        env[0:4] = ENV_PLANTED
        env_planted[0:4] = True
    if P >= 12:
        env[4:8], env[8:12] = full["env_opacity"][0:4], full["env_opacity"][50:54]      # ... and some below / above the clamp of the 'sparse' form
    inp["env_opacity"] = env
    inp["R"] = np.eye(3, dtype=F32) if identity else full["R"]
    nm, sn, prior, acc, msk = inp["norm_map"], inp["surf_norm_map"], inp["norm"], inp["acc_map"], inp["msk"]
    rows = lambda a, b: slice(a, min(b, max(N - 1, 0)))                         # the last row is set below
    nm[rows(3, 8)] = 0.0                                                        # background
    prior[rows(6, 11)] = 0.5                                                    # a zero prior; rows 6, 7 have neither a normal nor a prior
    msk[rows(12, 15)] = 0.5                                                     # not > 0.5 ...
    prior[rows(12, 15)] = (0.9, 0.2, 0.6)                                       # ... under a prior that would pass
    prior[rows(15, 18)] = (0.25, 0.0, 0.0)                                      # |norm| == 0.25 exactly: not > 0.25
    msk[rows(15, 18)], acc[rows(15, 18)] = 1.0, 0.75
    prior[rows(18, 21)] = (0.03, 0.1, 0.05)                                     # a short prior
    planted = np.zeros(N, bool)
    planted[rows(3, 21)] = True
    if identity:
        j = np.arange(6, dtype=F32)[: max(0, min(27, N - 1) - 21)]
        nm[rows(21, 27)] = np.stack([0 * j, 0.3 + 0.05 * j, -0.4 + 0.03 * j], -1)          # a.x == 0 ...
        prior[rows(21, 27)] = np.stack([0.5 + 0 * j, 0.9 - 0.02 * j, 0.2 + 0.01 * j], -1)  # ... and g.x == 0
        sn[rows(24, 27), 0] = 0.0                                               # no x-gradient from the gs_norm term either
        acc[rows(21, 27)] = 0.5
        planted[rows(21, 27)] = True
    planted |= (nm == 0).all(-1) | (prior == 0.5).all(-1)                       # _full_inputs' own background pixels and zero priors
    # the last row always carries weight in every term, so a sum that loses it is outside the 1e-4 bar at every N of the ladder
    last = N - 1
    if (nm[last] == 0).all():
        nm[last] = (0.3, -0.5, 0.4)
    if (prior[last] == 0.5).all():
        prior[last] = (0.9, 0.2, 0.6)
    planted[last] = False
    acc[last], inp["dpt_map"][last], inp["dist_map"][last], msk[last] = 0.75, 3.5, 0.05, 0.0
    for v in inp.values():
        v.setflags(write=False)
    return inp, planted, env_planted


def _opts(kind="sparse", dpt=True, acc=True):
    return dict(norm_loss_weight=0.01, norm_loss_start_iter=0, gs_norm_loss_weight=0.04, gs_norm_loss_start_iter=0, use_acc_scale_norm_loss=acc,
                use_acc_scale_gs_norm_loss=acc, use_dpt_scale_norm_loss=dpt, use_dpt_scale_gs_norm_loss=dpt, msk_loss_weight=0.1, msk_loss_start_iter=0,
                gs_dist_loss_weight=100.0, gs_dist_loss_start_iter=0, env_opacity_loss_weight=0.01, env_opacity_loss_type=kind)


@functools.lru_cache(maxsize=None)
def _reference(entry, kind, dtype=np.float64):
    """The twin on one ladder entry, computed once and shared."""
    N, P, seed, dpt, identity = entry
    loss, stats, grads = twin.geometry_loss(_inputs(N, P, seed, identity)[0], _opts(kind, dpt), IT, dtype=dtype)
    for g in grads.values():
        g.setflags(write=False)
    return loss, stats, grads


def _compare(test, what, got, ref, zero):
    """got / ref: (loss, stats, grads), the gradients as arrays shaped like the twin's; zero: (N,) bool, the pixels with norm_map == 0.
    -> the largest elementwise error check_close measured."""
    (gl, gs, gg), (rl, rs, rg) = got, ref
    print("%s loss %.9g ref %.9g" % (what, gl, rl))
    assert np.isfinite(gl) and abs(gl - rl) <= 1e-4 * abs(rl), (what, gl, rl)
    record(test, "loss", abs(gl - rl) / abs(rl) if rl else abs(gl), "relative; bar 1e-4")
    assert sorted(gs) == sorted(rs)
    for k, r in rs.items():
        assert abs(float(gs[k]) - r) <= 1e-4 * abs(r), (what, k, float(gs[k]), r)
    assert sorted(gg) == sorted(rg)
    gg = {k: np.asarray(gg[k], np.float64).reshape(rg[k].shape) for k in rg}
    _check_grads(gg, rg, zero, what=what)                                       # every pixel, the pixels with norm_map == 0 under their own rule
    worst = 0.0
    for k, r in rg.items():
        keep = None if k == "env_opacity" else ~zero
        if keep is None or keep.any():
            worst = max(worst, check_close(test, "d " + k, gg[k], r, keep=keep))
        assert (gg[k][r == 0] == 0).all(), (what, k)                            # an exact zero of the twin is an exact zero here
    return worst


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES + [ALONE_ENTRY, COINCIDING_ENTRY], ids=_ids)
def test_inputs_have_stated_margins(entry):
    N, P, seed, dpt, identity = entry
    inp, planted, env_planted = _inputs(N, P, seed, identity)
    for k, v in inp.items():
        assert v.dtype == F32 and np.isfinite(v).all(), k
    nm, prior, msk, env, R = (inp[k].astype(np.float64) for k in ("norm_map", "norm", "msk", "env_opacity", "R"))
    a = twin._unit(twin._unit(nm)[0] @ R.T)[0]
    g = twin._unit(2.0 * prior - 1.0)[0]
    free = ~planted
    assert not planted[N - 1]
    assert (np.abs(a - g)[free] > 1e-5).all(), np.abs(a - g)[free].min()
    assert (np.abs(np.sqrt((prior * prior).sum(-1)) - 0.25)[free] > 1e-4).all()
    assert np.isin(msk[free], (0.0, 1.0)).all()
    e = env[~env_planted]
    assert (np.abs(e - 1e-3) > 1e-6).all() and (np.abs(e - (1 - 1e-3)) > 1e-6).all() and (e > 1e-6).all() and (e < 1 - 1e-6).all()
    if dpt:
        near, far = twin.percentiles(inp["dpt_map"])
        assert far > near and N >= 100
    if N >= 63:                                                                 # every planted row is there
        assert (nm[3:8] == 0).all() and (prior[6:11] == 0.5).all() and (msk[12:15] == 0.5).all() and (msk[15:18] == 1).all()
        assert (np.sqrt((inp["norm"][15:18] ** 2).sum(-1, dtype=F32)) == F32(0.25)).all() and (inp["norm"][15:18] == (0.25, 0, 0)).all()
        assert (np.sqrt((prior[18:21] ** 2).sum(-1)) < 0.25 - 1e-4).all() and (inp["acc_map"][15:18] > 0.5).all()
    if P >= 4:
        assert env[:4].astype(F32).tobytes() == ENV_PLANTED.tobytes()
    if P >= 12:
        assert (env[4:8] < 1e-3 - 1e-6).all() and (env[8:12] > 1 - 1e-3 + 1e-6).all()
    if identity:
        assert (a[21:27, 0] == 0).all() and (g[21:27, 0] == 0).all() and (np.abs(a - g)[21:27, 1:] > 1e-5).all() and (inp["surf_norm_map"][24:27, 0] == 0).all()
        for kind in ("sparse", "l1"):                                           # the twin states an exact zero there
            gr = _reference(entry, kind)[2]
            assert (gr["norm_map"][24:27, 0] == 0).all() and (gr["surf_norm_map"][21:27, 0] == 0).all() and (gr["norm_map"][21:24, 0] != 0).all()


@pytest.mark.parametrize("entry", ENTRIES, ids=_ids)
def test_float32_twin_stays_inside_the_bar(entry):
    """The twin's own arithmetic in float32 against itself in float64, under the bars of the GPU ladder: what any float32 evaluation loses."""
    N, P, seed, dpt, identity = entry
    zero = (_inputs(N, P, seed, identity)[0]["norm_map"] == 0).all(-1)
    for kind in ("sparse", "l1"):
        l32, s32, g32 = _reference(entry, kind, np.float32)
        assert all(g.dtype == np.float32 for g in g32.values())
        worst = _compare("float32_twin_vs_float64_twin", "%s %s" % (_ids(entry), kind), (float(l32), s32, g32), _reference(entry, kind), zero)
        record("float32_twin_vs_float64_twin", "worst/TOL", worst / 1e-4, "%s %s" % (_ids(entry), kind))


def test_twin_at_float64_is_what_it_was():
    """dtype and dpt_scale default to the float64 statement pinned by the fixtures: float64 inputs and explicit defaults change no bit."""
    inp = _inputs(319, 257, 319)[0]
    for kind in ("sparse", "l1"):
        a = twin.geometry_loss(inp, _opts(kind), IT)
        b = twin.geometry_loss({k: v.astype(np.float64) for k, v in inp.items()}, _opts(kind), IT, dtype=np.float64, dpt_scale=None)
        assert np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and a[1] == b[1]
        assert all(a[2][k].dtype == np.float64 and a[2][k].tobytes() == b[2][k].tobytes() for k in LEAVES)
        ds = twin.depth_scale(inp["dpt_map"].astype(np.float64), *twin.percentiles(inp["dpt_map"]))
        c = twin.geometry_loss(inp, _opts(kind), IT, dpt_scale=ds)             # the override with the formula's own values
        assert np.float64(a[0]).tobytes() == np.float64(c[0]).tobytes() and all(a[2][k].tobytes() == c[2][k].tobytes() for k in LEAVES)


def _coinciding_depths():
    d = np.full(300, 2.5, F32)
    d[[100, 200]] = (1.0, 1.5)
    d[[150, 250]] = (4.0, 5.0)
    return d


def _coinciding_rule(d, near):
    """The depth scale this project means when far == near: 0 at d == near and beyond it, 1 in front of it."""
    return np.where(d < near, 1.0, 0.0)


def test_coinciding_percentiles_on_the_cpu():
    """far == near: the reference's formula and the twin give NaN at d == near; float32 min / max, which return their other operand when one is
    NaN (IEEE 754 minNum / maxNum; fminf / fmaxf on the device), give the rule pinned by test_coinciding_percentiles_follow_the_stated_rule."""
    d = _coinciding_depths()
    near, far = twin.percentiles(d)
    assert near == far == F32(2.5) and (d == near).sum() == 296
    with np.errstate(divide="ignore", invalid="ignore"):
        s = twin.depth_scale(d, near, far)
        x = F32(1.0) - (d - near) / (far - near)
        dev = np.fmin(np.fmax(x, F32(0.0)), F32(1.0))
    assert np.isnan(s[d == near]).all() and (s[d < near] == 1).all() and (s[d > near] == 0).all()
    assert np.isnan(x[d == near]).all() and np.array_equal(dev, _coinciding_rule(d, near))


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------------
def _shaped(inp):
    """The twin's rows in the reference's shapes: (1,N,3), (1,N,1), (P,1), (1,3,3)."""
    out = {}
    for k, v in inp.items():
        out[k] = np.array(v[None] if k in ("norm_map", "surf_norm_map", "norm", "R") else v[:, None] if k == "env_opacity" else v[None, :, None])
    return out


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _device(inp, opts, up=3.0, leaves=LEAVES, out_keys=None, batch_keys=None):
    """One front-end run -> (loss: 0-d float32 array, stats: name -> float, grads: leaf -> float32 array or None, the output dict)."""
    from envgs_amd.loss import EnvGSGeometryLoss
    dev = torch.device("cuda", 0)
    out, batch = _to_dev(_shaped(inp), dev, grad=False)
    for k in leaves:
        out[k].requires_grad_(True)
    sub_out = {k: v for k, v in out.items() if out_keys is None or k in out_keys}
    sub_batch = {k: v for k, v in batch.items() if batch_keys is None or k in batch_keys}
    loss, stats = EnvGSGeometryLoss(**opts)(sub_out, sub_batch, IT)
    if up is not None and loss.requires_grad:
        (loss * up).backward()
    grads = {k: None if out[k].grad is None else out[k].grad.cpu().numpy() for k in LEAVES}
    return loss.detach().cpu().numpy(), {k: float(v) for k, v in stats.items()}, grads, loss.requires_grad


def _against_twin(test, what, run, ref, zero, up=3.0):
    loss, stats, grads, _ = run
    assert loss.dtype == np.float32 and loss.shape == ()
    assert sorted(k for k in LEAVES if grads[k] is not None) == sorted(ref[2]), what
    got = {k: grads[k].astype(np.float64) / up for k in ref[2]}
    return _compare(test, what, (float(loss), stats, got), ref, zero)


def _same_bits(a, b, what):
    assert a[0].tobytes() == b[0].tobytes(), what
    for k in LEAVES:
        assert (a[2][k] is None) == (b[2][k] is None) and (a[2][k] is None or a[2][k].tobytes() == b[2][k].tobytes()), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES, ids=_ids)
def test_size_ladder_against_the_twin(entry):
    """All five terms, both normal terms under the acc scale and (N >= 100) the depth scale, 'sparse' and 'l1', upstream gradient 3."""
    N, P, seed, dpt, identity = entry
    inp = _inputs(N, P, seed, identity)[0]
    zero = (inp["norm_map"] == 0).all(-1)
    for kind in ("sparse", "l1"):
        what = "%s %s" % (_ids(entry), kind)
        run = _device(inp, _opts(kind, dpt))
        assert sorted(run[1]) == sorted(TERMS)
        _against_twin("supervisor_size_ladder", what, run, _reference(entry, kind), zero)
        _same_bits(run, _device(inp, _opts(kind, dpt)), what)                   # the sums have a fixed order


# ---- nothing is written at or beyond row N: the C-ABI with guarded buffers ----
CANARY = 0x7FA5A5A5          # a NaN no arithmetic here produces
GUARD = 4096


def _guarded(n, dev):
    return torch.full((n + GUARD,), CANARY, dtype=torch.int32, device=dev)


@pytest.mark.gpu
@pytest.mark.parametrize("N,P", [(257, 257), (1, 1)])
def test_c_abi_writes_every_row_below_n_and_none_beyond(N, P):
    from envgs_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    dpt = N >= 100
    inp = _inputs(N, P, N + P)[0]
    opts = _opts("sparse", dpt)
    t = {k: torch.from_numpy(np.array(inp[k])).to(dev) for k in inp}
    a = _lib.SupervisorArgs()
    a.N, a.P = N, P
    a.flags = (1 << 0) | (1 << 1) | (1 << 2) | (1 << 3) | (1 << 4) | (1 << 6) | (1 << 8) | (((1 << 7) | (1 << 9)) if dpt else 0)
    a.weight[:] = [opts["norm_loss_weight"], opts["gs_norm_loss_weight"], opts["msk_loss_weight"], opts["gs_dist_loss_weight"], opts["env_opacity_loss_weight"]]
    for name, key, ch in (("norm_map", "norm_map", 1), ("surf_norm_map", "surf_norm_map", 1), ("prior", "norm", 1), ("acc_map", "acc_map", 0),
                          ("dist_map", "dist_map", 0), ("env_opacity", "env_opacity", 0), ("msk", "msk", 0)) + ((("dpt_map", "dpt_map", 0),) if dpt else ()):
        setattr(a, name, t[key].data_ptr())
        setattr(a, name + "_row", 3 if ch else 1)
        if ch:
            setattr(a, name + "_ch", 1)
    a.R = t["R"].data_ptr()
    if dpt:
        near_far = torch.empty(2, device=dev)
        tb = lib.envgs_depth_percentiles_temp_bytes()
        temp = torch.empty((tb + 3) // 4, dtype=torch.int32, device=dev)
        assert lib.envgs_depth_percentiles(N, _lib.ptr(t["dpt_map"]), 1, _lib.ptr(near_far), _lib.ptr(temp), tb, st) == 0
        a.near_far = near_far.data_ptr()
    sizes = dict(g_norm_map=3 * N, g_surf_norm_map=3 * N, g_acc_map=N, g_dist_map=N, g_env_opacity=P)
    rows = lib.envgs_supervisor_partial_count(N, P)
    assert rows == (N + 255) // 256 + (P + 255) // 256
    bufs = {k: _guarded(n, dev) for k, n in sizes.items()}
    bufs["partial"], bufs["out"] = _guarded(5 * rows, dev), _guarded(6, dev)
    sizes.update(partial=5 * rows, out=6)
    for k in sizes:
        if k != "out":
            setattr(a, k, bufs[k].data_ptr())
    assert lib.envgs_supervisor_forward(a, st) == 0
    assert lib.envgs_supervisor_finish(a, _lib.ptr(bufs["out"]), st) == 0
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, n in sizes.items():
        assert (host[k][n:] == CANARY).all(), "%s: written beyond its %d elements" % (k, n)
        assert (host[k][:n] != CANARY).all(), "%s: rows left unwritten" % k
    # the front end on the same inputs (upstream gradient 1: scale_by_scalar multiplies by 1.0)
    loss, stats, grads, _ = _device(inp, opts, up=1.0)
    out = host["out"][:6].view(np.float32)
    assert out[5].tobytes() == loss.tobytes()
    assert [float(v) for v in out[:5]] == [stats[k] for k in TERMS]
    for k in LEAVES:
        assert host["g_" + k][:sizes["g_" + k]].tobytes() == grads[k].tobytes(), k


# ---- each term alone, each leaf alone ----
_NO, _ACC, _DPT, _BOTH = (False, False), (True, False), (False, True), (True, True)
ALONE = ([("norm_loss", s) for s in (_NO, _ACC, _DPT, _BOTH)] + [("gs_norm_loss", s) for s in (_NO, _ACC, _DPT, _BOTH)]
         + [("msk_loss", _NO), ("gs_dist_loss", _NO), ("env_opacity_loss", "sparse"), ("env_opacity_loss", "l1")])


def _alone(term, how):
    """-> (options with this term only, the output keys and the batch keys it reads)."""
    o = dict(env_opacity_loss_weight=0.0)
    if term == "norm_loss":
        o.update(norm_loss_weight=0.01, norm_loss_start_iter=0, use_acc_scale_norm_loss=how[0], use_dpt_scale_norm_loss=how[1])
        keys, bkeys = ["norm_map"], ["norm", "R"]
    elif term == "gs_norm_loss":
        o.update(gs_norm_loss_weight=0.04, gs_norm_loss_start_iter=0, use_acc_scale_gs_norm_loss=how[0], use_dpt_scale_gs_norm_loss=how[1])
        keys, bkeys = ["norm_map", "surf_norm_map"], []
    elif term == "msk_loss":
        o.update(msk_loss_weight=0.1, msk_loss_start_iter=0)
        keys, bkeys = ["acc_map"], ["msk", "norm"]
    elif term == "gs_dist_loss":
        o.update(gs_dist_loss_weight=100.0, gs_dist_loss_start_iter=0)
        keys, bkeys = ["dist_map"], []
    else:
        o.update(env_opacity_loss_weight=0.01, env_opacity_loss_type=how)
        keys, bkeys = ["env_opacity"], []
    if term in ("norm_loss", "gs_norm_loss"):
        keys += (["acc_map"] if how[0] else []) + (["dpt_map"] if how[1] else [])
    return o, keys, bkeys


@pytest.mark.gpu
@pytest.mark.parametrize("term,how", ALONE, ids=lambda v: v if isinstance(v, str) else "acc%d-dpt%d" % v)
def test_each_term_alone(term, how):
    """One term, the keys it does not read absent: their input pointers are NULL and their gradient maps do not exist."""
    inp = _inputs(*ALONE_ENTRY[:3])[0]
    zero = (inp["norm_map"] == 0).all(-1)
    opts, keys, bkeys = _alone(term, how)
    ref = twin.geometry_loss({k: inp[k] for k in keys + bkeys}, opts, IT)
    assert list(ref[1]) == [term]
    run = _device(inp, opts, out_keys=keys, batch_keys=bkeys)
    assert list(run[1]) == [term]
    _against_twin("supervisor_term_alone", "%s %s" % (term, how), run, ref, zero)


@pytest.mark.gpu
def test_only_the_opacity_term():
    """No pixel map at all: N defaults to 1, the one pixel workgroup runs empty and writes a zero row."""
    from envgs_amd.loss import _Geometry
    inp = _inputs(*ALONE_ENTRY[:3])[0]
    dev = torch.device("cuda", 0)
    for flag, kind in ((1 << 4, "sparse"), (1 << 5, "l1")):
        ref_loss, ref_stats, _ = twin.geometry_loss(dict(env_opacity=inp["env_opacity"]), dict(env_opacity_loss_weight=0.01, env_opacity_loss_type=kind), IT)
        env = torch.from_numpy(np.array(inp["env_opacity"])).to(dev)
        loss, vec = _Geometry.apply(flag, [0.0, 0.0, 0.0, 0.0, 0.01], None, None, None, None, env, None, None, None, None)
        vec = vec.cpu().numpy()
        assert (vec[:4] == 0).all() and abs(float(vec[4]) - ref_stats["env_opacity_loss"]) <= 1e-4 * abs(ref_stats["env_opacity_loss"])
        assert abs(float(loss) - ref_loss) <= 1e-4 * abs(ref_loss) and not loss.requires_grad


@pytest.mark.gpu
def test_each_leaf_alone_no_leaf_and_upstream_zero():
    """The gradient maps of leaves that do not require grad are NULL in the kernel: what is left is unchanged, bit for bit."""
    inp = _inputs(*ALONE_ENTRY[:3])[0]
    opts = _opts("sparse")
    full = _device(inp, opts)
    assert all(full[2][k] is not None for k in LEAVES) and full[3]
    for leaf in LEAVES:
        one = _device(inp, opts, leaves=(leaf,))
        assert one[0].tobytes() == full[0].tobytes() and one[1] == full[1], leaf
        assert [k for k in LEAVES if one[2][k] is not None] == [leaf]
        assert one[2][leaf].tobytes() == full[2][leaf].tobytes(), leaf
    none = _device(inp, opts, leaves=())
    assert not none[3] and none[0].tobytes() == full[0].tobytes() and none[1] == full[1] and all(none[2][k] is None for k in LEAVES)
    still = _device(inp, opts, up=0.0)
    assert still[0].tobytes() == full[0].tobytes()
    for k in LEAVES:
        assert still[2][k].shape == full[2][k].shape and (still[2][k] == 0).all(), k


# ---- layouts at a ragged size ----
@pytest.mark.gpu
def test_strided_layouts_at_a_ragged_size():
    """11 x 29 pixels: (3,H,W) planes viewed channel-last, single-channel maps (the depth the percentiles read among them) as column 2 of an
    interleaved (N,4) tensor at a non-zero storage offset, env_opacity as a column of (P,3), float64 inputs: the bits of the contiguous float32 run."""
    from envgs_amd.loss import EnvGSGeometryLoss
    H, W, P = 11, 29, 257
    N = H * W
    dev = torch.device("cuda", 0)
    inp = _inputs(N, P, 11)[0]
    opts = _opts("sparse")
    ref = _device(inp, opts)
    dv = lambda k: torch.from_numpy(np.array(inp[k])).to(dev)

    def planes(k, grad):
        return dv(k).reshape(H, W, 3).permute(2, 0, 1).contiguous().requires_grad_(grad)

    def interleaved(k, grad):
        base = torch.full((5 + 4 * N,), 7.25, device=dev)
        base[5:].view(N, 4)[:, 2] = dv(k)
        return base.requires_grad_(grad)

    col = lambda base: base[5:].view(N, 4)[:, 2:3][None]                        # (1,N,1), row stride 4, storage offset 7
    pl = {k: planes(k, k != "norm") for k in ("norm_map", "surf_norm_map", "norm")}
    il = {k: interleaved(k, k in ("acc_map", "dist_map")) for k in ("acc_map", "dist_map", "dpt_map", "msk")}
    env = torch.full((P, 3), 0.5, device=dev)
    env[:, 1] = dv("env_opacity")
    env.requires_grad_(True)
    out = dict(norm_map=pl["norm_map"].permute(1, 2, 0), surf_norm_map=pl["surf_norm_map"].permute(1, 2, 0), acc_map=col(il["acc_map"]),
               dist_map=col(il["dist_map"]), dpt_map=col(il["dpt_map"]), env_opacity=env[:, 1:2])
    batch = dict(norm=pl["norm"].permute(1, 2, 0), msk=col(il["msk"]), R=dv("R")[None])
    assert not out["norm_map"].is_contiguous() and out["dpt_map"].storage_offset() == 7 and out["dpt_map"].stride(1) == 4 and out["env_opacity"].stride(0) == 3
    loss, stats = EnvGSGeometryLoss(**opts)(out, batch, IT)
    (loss * 3.0).backward()
    assert _bits(loss) == ref[0].tobytes() and {k: float(v) for k, v in stats.items()} == ref[1]
    for k in ("norm_map", "surf_norm_map"):
        assert pl[k].grad.shape == (3, H, W) and _bits(pl[k].grad.permute(1, 2, 0).contiguous()) == ref[2][k].tobytes(), k
    for k in ("acc_map", "dist_map"):
        g = il[k].grad
        assert _bits(g[5:].view(N, 4)[:, 2].contiguous()) == ref[2][k].tobytes(), k
        rest = g.clone()
        rest[5:].view(N, 4)[:, 2] = 0
        assert not bool(rest.any()), k                                          # nothing lands beside the column
    assert _bits(env.grad[:, 1].contiguous()) == ref[2]["env_opacity"].tobytes() and not bool(env.grad[:, [0, 2]].any())
    assert il["dpt_map"].grad is None
    # float64 inputs (float32-representable, so rounding them changes nothing): the same loss, float64 gradients
    out64, batch64 = _to_dev(_shaped(inp), dev, grad=False)
    out64 = {k: v.double().requires_grad_(k in LEAVES) for k, v in out64.items()}
    batch64 = {k: v.double() for k, v in batch64.items()}
    loss, stats = EnvGSGeometryLoss(**opts)(out64, batch64, IT)
    (loss * 3.0).backward()
    assert loss.dtype == torch.float32 and _bits(loss) == ref[0].tobytes()
    for k in LEAVES:
        assert out64[k].grad.dtype == torch.float64 and out64[k].grad.shape == out64[k].shape
        assert np.array_equal(out64[k].grad.cpu().numpy().reshape(ref[2][k].shape), ref[2][k].astype(np.float64)), k
    assert out64["dpt_map"].grad is None


# ---- coinciding percentiles ----
@pytest.mark.gpu
def test_coinciding_percentiles_follow_the_stated_rule():
    """N = 300, 296 equal depths, two smaller, two larger: near == far.  The reference's normalize_depth divides 0 by 0 at every pixel with
    d == near and its loss is NaN, so there is nothing of the reference's to match, and the deviation is deliberate: this project's depth scale is
    then 0 where d == near, 0 where d > near and 1 where d < near (what fminf(fmaxf(x, 0), 1) makes of NaN, -inf and +inf), every output is
    finite, and the result is the twin's under exactly that scale (include/envgs_supervisor.h; EnvGSGeometryLoss)."""
    inp = dict(_inputs(*COINCIDING_ENTRY[:3])[0], dpt_map=_coinciding_depths())
    zero = (inp["norm_map"] == 0).all(-1)
    near, far = twin.percentiles(inp["dpt_map"])
    assert near == far
    opts = dict(norm_loss_weight=0.01, norm_loss_start_iter=0, gs_norm_loss_weight=0.04, gs_norm_loss_start_iter=0, use_dpt_scale_norm_loss=True,
                use_dpt_scale_gs_norm_loss=True)
    ref = twin.geometry_loss(inp, opts, IT, dpt_scale=_coinciding_rule(inp["dpt_map"], near))
    assert ref[0] > 0 and np.isfinite(ref[0])
    run = _device(inp, opts, out_keys=("norm_map", "surf_norm_map", "dpt_map"), batch_keys=("norm", "R"))
    assert np.isfinite(run[0]) and all(np.isfinite(v) for v in run[1].values())
    for k in ("norm_map", "surf_norm_map"):
        assert np.isfinite(run[2][k]).all(), k
        assert (run[2][k].reshape(-1, 3)[inp["dpt_map"] >= near] == 0).all(), k             # no gradient where the scale is 0
    _against_twin("supervisor_coinciding_percentiles", "far == near", run, ref, zero)
