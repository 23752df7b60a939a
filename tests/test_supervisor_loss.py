"""Geometry regularisers of the EnvGS supervisor (include/envgs_supervisor.h, envgs_amd.loss.EnvGSGeometryLoss).

CPU: the float64 twin (tests/reference_supervisor.py) against the reference's own outputs (tests/golden/supervisor_golden.npz and, at a pixel
count that is no multiple of the kernel's workgroup, supervisor_golden_ragged.npz; both written by tests/golden/make_supervisor_golden.py), its
percentile routine against np.partition, argument rejection of the C-ABI and of the front-end.
GPU: exact percentiles, the fixture cases, full-size option combinations and layouts against the twin, composition with the image loss
through the base pass, and the absence of host synchronisation.

Tolerances: scalars 1e-4 relative; gradients max|got - ref| / max|ref| < 1e-4 per tensor (the bar tests/test_loss.py applies), taken SEPARATELY
over the pixels with norm_map == 0 and over the rest.  On a pixel with norm_map == 0 both x / (|x| + 1e-8) steps and the cosine's clamp
multiply the gradient of norm_loss by 1e8.  For the 64 x 48 fixture (the magnitudes depend on N and on the inputs) the reference's float64
gradient reaches 3e18 there against 3e-5 elsewhere, and the reference's own float32 run deviates from its float64 run by 2.0e-5 / 4.0e-5 /
1.9e-5 elementwise (cases a / b / c); the fixture stores that deviation per case (f32_noise_zero_normal_*) and the bound there is 4x it,
elementwise, with every value finite.  No pixel is left out of a comparison."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import reference_supervisor as twin

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "supervisor_golden.npz")
RAGGED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "supervisor_golden_ragged.npz")     # 11 x 29 pixels (n = 3), P = 257
# (fixture, case): the 48 x 64 fixture keeps its test ids
FIXTURE_CASES = [pytest.param(GOLD, t, id=t) for t in "abcd"] + [pytest.param(RAGGED, t, id="ragged-" + t) for t in "ac"]
GRAD_KEYS = ("norm_map", "surf_norm_map", "acc_map", "dist_map", "env_opacity")
ENVGS_YAML = dict(gs_norm_loss_weight=0.04, gs_norm_loss_start_iter=0, use_dpt_scale_gs_norm_loss=True, norm_loss_weight=0.01, norm_loss_start_iter=0,
                  use_dpt_scale_norm_loss=True)


def _fixture(path=GOLD):
    z = np.load(path)
    inp = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    return z, inp


def _flat(inp):
    """The fixture's (1,N,C) / (P,1) arrays as the twin's rows."""
    out = {}
    for k, v in inp.items():
        v = np.asarray(v)
        if k == "R":
            out[k] = v.reshape(3, 3)
        elif k in ("norm_map", "surf_norm_map", "norm"):
            out[k] = v.reshape(-1, 3)
        else:
            out[k] = v.reshape(-1)
    return out


def _case(z, tag):
    return dict(ast.literal_eval(str(z["opts_" + tag]))), int(z["iter_" + tag])


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------------
@pytest.mark.parametrize("path,tag", FIXTURE_CASES)
def test_twin_matches_reference_golden(path, tag):
    z, inp = _fixture(path)
    opts, it = _case(z, tag)
    loss, stats, grads = twin.geometry_loss(_flat(inp), opts, it)
    assert abs(loss - float(z["loss_" + tag])) < 1e-12
    assert sorted(stats) == sorted(str(s) for s in z["stats_" + tag])
    for k, v in stats.items():
        assert abs(v - float(z["%s_%s" % (k, tag)])) < 1e-12, k
    assert sorted(grads) == sorted(k for k in GRAD_KEYS if "grad_%s_%s" % (k, tag) in z.files)
    for k, g in grads.items():
        ref = z["grad_%s_%s" % (k, tag)].reshape(g.shape)
        assert np.allclose(g, ref, rtol=1e-9, atol=1e-14), (k, float(np.abs(g - ref).max()))
    if tag == "d":
        assert loss == 0.0 and not stats and not grads


def test_fixture_holds_the_degenerate_inputs():
    z, inp = _fixture()
    f = _flat(inp)
    N = f["dpt_map"].size
    n = int(N * 0.01)
    assert N == int(z["H"]) * int(z["W"]) and n == 30 and f["env_opacity"].size == int(z["P"])
    assert (f["norm_map"] == 0).all(-1).sum() >= 100 and (f["norm"] == 0.5).all(-1).sum() >= 100 and (f["dpt_map"] == 0).sum() >= 10
    near, far = twin.percentiles(f["dpt_map"])
    assert (f["dpt_map"] == near).sum() >= 3 and (f["dpt_map"] == far).sum() >= 3                    # ties at both percentiles
    for tag in "abc":
        assert 0 < float(z["f32_noise_zero_normal_" + tag]) < 1e-3
    for k in inp:                                                                                    # float32-representable
        assert inp[k].dtype == np.float32


def _tie_inputs(N, seed):
    g = np.random.default_rng(seed)
    d = (g.random(N, dtype=np.float32) * 8 - 2).astype(np.float32)                                   # negative values too
    d[g.integers(0, N, N // 20)] = 0.0
    d[g.integers(0, N, N // 50)] = -0.0
    n = int(N * 0.01)
    s = np.sort(d)
    d[g.integers(0, N, 7)] = s[n - 1]                                                                # repeat both order statistics
    d[g.integers(0, N, 7)] = s[N - n]
    return d


@pytest.mark.parametrize("N", [100, 257, 7680, 100003])
def test_twin_percentiles_are_exact_order_statistics(N):
    d = _tie_inputs(N, N)
    n = int(N * 0.01)
    near, far = twin.percentiles(d)
    assert near.dtype == np.float32
    assert near.tobytes() == np.partition(d, n - 1)[n - 1].tobytes() or (near == 0 and np.partition(d, n - 1)[n - 1] == 0)
    assert far.tobytes() == np.partition(d, N - n)[N - n].tobytes() or (far == 0 and np.partition(d, N - n)[N - n] == 0)
    assert (d <= near).sum() >= n > (d < near).sum() and (d >= far).sum() >= n > (d > far).sum()
    assert all(int(m * 0.01) == m // 100 for m in range(100, 200000, 37))                            # the device side uses the integer form
    with pytest.raises(ValueError):
        twin.percentiles(d[:99])


@pytest.fixture(scope="module")
def lib():
    from envgs_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_abi_rejects_bad_arguments_before_any_gpu_work(lib):
    from envgs_amd import _lib
    one = ctypes.c_void_p(16)                                            # a non-null address that must never be dereferenced
    tb = lib.envgs_depth_percentiles_temp_bytes()
    assert tb >= 4 * (2048 + 2 * 2048 + 2 * 1024)
    assert lib.envgs_depth_percentiles(99, one, 1, one, one, tb, None) == -1
    assert lib.envgs_depth_percentiles(1 << 31, one, 1, one, one, tb, None) == -1
    assert lib.envgs_depth_percentiles(1000, None, 1, one, one, tb, None) == -1
    assert lib.envgs_depth_percentiles(1000, one, 1, None, one, tb, None) == -1
    assert lib.envgs_depth_percentiles(1000, one, 1, one, None, tb, None) == -1
    assert lib.envgs_depth_percentiles(1000, one, 1, one, one, tb - 1, None) == -2
    assert lib.envgs_supervisor_partial_count(0, 0) == 0 and lib.envgs_supervisor_partial_count(-5, 3) == 0
    assert lib.envgs_supervisor_partial_count(640000, 163840) == 2500 + 640 and lib.envgs_supervisor_partial_count(257, 0) == 2
    assert lib.envgs_supervisor_backward(0, one, one, one, None) == -1 and lib.envgs_supervisor_backward(8, one, None, one, None) == -1

    def args(**kw):
        a = _lib.SupervisorArgs()
        a.N, a.P, a.flags = 1000, 0, 0
        for k in ("norm_map", "surf_norm_map", "acc_map", "dpt_map", "dist_map", "prior", "msk", "R", "near_far", "partial"):
            setattr(a, k, 16)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    F_NORM, F_GS, F_MSK, F_DIST, F_SPARSE, F_L1, F_NORM_ACC, F_NORM_DPT, F_GS_ACC, F_GS_DPT = (1 << i for i in range(10))
    bad = [args(flags=0), args(flags=1 << 10), args(flags=F_NORM | (1 << 31)), args(flags=F_NORM, partial=None), args(flags=F_NORM, N=0),
           args(flags=F_NORM, norm_map=None), args(flags=F_NORM, prior=None), args(flags=F_NORM, R=None), args(flags=F_GS, surf_norm_map=None),
           args(flags=F_MSK, msk=None), args(flags=F_MSK, acc_map=None), args(flags=F_DIST, dist_map=None),
           args(flags=F_GS | F_GS_ACC, acc_map=None), args(flags=F_GS | F_GS_DPT, N=99), args(flags=F_NORM | F_NORM_DPT, near_far=None),
           args(flags=F_NORM | F_NORM_DPT, dpt_map=None), args(flags=F_SPARSE, P=10), args(flags=F_SPARSE | F_L1, P=10, env_opacity=16),
           args(flags=F_L1, P=0, env_opacity=16), args(flags=F_GS, P=10), args(flags=F_DIST, g_norm_map=16), args(flags=F_NORM, g_acc_map=16),
           args(flags=F_NORM, g_env_opacity=16)]
    for i, a in enumerate(bad):
        assert lib.envgs_supervisor_forward(a, None) == -1, i
        assert lib.envgs_supervisor_finish(a, one, None) == -1, i
    assert lib.envgs_supervisor_forward(None, None) == -1
    assert lib.envgs_supervisor_finish(args(flags=F_DIST), None, None) == -1


def test_front_end_rejects_what_is_out_of_scope():
    from envgs_amd.loss import EnvGSGeometryLoss
    reg = EnvGSGeometryLoss(**ENVGS_YAML, norm_smooth_loss_weight=0.0, res_norm_loss_weight=0.001, max_dpt_scale_percet=False)     # defaults pass
    assert reg.norm_loss_start_iter == 0 and EnvGSGeometryLoss().norm_loss_start_iter == 7000 and EnvGSGeometryLoss().gs_dist_loss_start_iter == 3000
    for kw in (dict(max_dpt_scale_percet=0.95), dict(norm_loss_weight_final=0.001), dict(gs_norm_loss_weight_final=0.1), dict(use_spec_scale_norm_loss=True),
               dict(use_spec_scale_gs_norm_loss=True), dict(norm_smooth_loss_weight=0.01), dict(res_norm_loss_weight=0.0), dict(specular_loss_weight=0.1),
               dict(ref_rgb_loss_weight=0.1), dict(use_edge_aware_smooth=False), dict(specular_target=0.5)):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            EnvGSGeometryLoss(**kw)
    with pytest.raises(TypeError, match="perc_loss_weight"):
        EnvGSGeometryLoss(perc_loss_weight=0.01)
    with pytest.raises(ValueError, match="env_opacity_loss_type"):
        EnvGSGeometryLoss(env_opacity_loss_type="l2")
    out = dict(norm_map=torch.zeros(1, 200, 3), surf_norm_map=torch.zeros(1, 200, 3), dpt_map=torch.ones(1, 200, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):          # CPU tensors: refuse, never fall back
        reg(out, dict(norm=torch.zeros(1, 200, 3), R=torch.eye(3)[None]), 10)
    flags, w = reg.active_terms(out, dict(R=torch.eye(3)[None]), 10)     # no batch.norm: the prior term is skipped, as in the reference
    assert flags == (1 << 1) | (1 << 9) and w == [0.0, 0.04, 0.0, 0.0, 0.0]
    assert EnvGSGeometryLoss(gs_norm_loss_weight=0.04).active_terms(out, {}, 6999)[0] == 0
    assert EnvGSGeometryLoss(gs_norm_loss_weight=0.04, gs_norm_loss_until_iter=8000).active_terms(out, {}, 8000)[0] == 0


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------------
def _to_dev(inp, dev, grad=True):
    out = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(dev) for k in ("norm_map", "surf_norm_map", "acc_map", "dpt_map", "dist_map", "env_opacity")}
    if grad:
        for k in out:
            out[k].requires_grad_(True)
    batch = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(dev) for k in ("norm", "msk", "R")}
    return out, batch


def _check_grads(got, ref, zero, noise=None, tol=1e-4, what=""):
    """got / ref: dict name -> (N,C) or (N,) arrays; zero: (N,) bool, the pixels with norm_map == 0.  Every comparison is measured and printed
    before the first one beyond its bound fails the test."""
    beyond = []
    for k, r in ref.items():
        g = got[k]
        assert g is not None, k
        g = g.reshape(r.shape).astype(np.float64)
        assert np.isfinite(g).all(), k
        if k == "env_opacity":
            parts = [("all", slice(None))]
        else:
            parts = [("norm_map != 0", ~zero), ("norm_map == 0", zero)]
        for name, sel in parts:
            rr, gg = r[sel], g[sel]
            if rr.size == 0:
                continue
            scale = np.abs(rr).max()
            err = np.abs(gg - rr).max() / scale if scale > 0 else np.abs(gg).max()
            print("%s d %-14s %-14s max|ref| %.3e  max|got - ref|/max|ref| %.3e" % (what, k, name, scale, err))
            if k == "norm_map" and name == "norm_map == 0" and noise is not None:
                nz = rr != 0
                el = (np.abs(gg[nz] - rr[nz]) / np.abs(rr[nz])).max()
                print("%s d %-14s %-14s elementwise rel %.3e (reference float32 noise %.3e)" % (what, k, name, el, noise))
                assert (gg[~nz] == 0).all()
                if not el <= 4.0 * noise:
                    beyond.append((k, name, el, noise))
            elif not err < tol:
                beyond.append((k, name, err))
    assert not beyond, beyond


@pytest.mark.gpu
@pytest.mark.parametrize("N", [100, 199, 257, 7680, 640000, 100003])
def test_device_percentiles_are_bit_exact(N):
    """N = 100 is the smallest legal count (n = 1: the ranks are 0 and N - 1), 199 the largest with n = 1, 257 one workgroup plus one element; at
    N = 100 an all-equal input too, whose two ranks share every prefix in all three passes of the select."""
    from envgs_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tb = lib.envgs_depth_percentiles_temp_bytes()
    for d in [_tie_inputs(N, N + 1)] + ([np.full(N, 1.5, np.float32)] if N == 100 else []):
        near, far = twin.percentiles(np.where(d == 0, np.float32(0.0), d))              # (-0 counts as +0 on the device)
        for stride in (1, 3):                                                           # contiguous, and one channel of an interleaved map
            buf = torch.full((N, stride), 1e30, device=dev)
            buf[:, 0] = torch.from_numpy(d).to(dev)
            nf = torch.full((2,), -1.0, device=dev)
            temp = torch.full(((tb + 3) // 4,), 0x55555555, dtype=torch.int32, device=dev)    # dirty scratch: the call clears what it uses
            assert lib.envgs_depth_percentiles(N, _lib.ptr(buf), stride, _lib.ptr(nf), _lib.ptr(temp), tb, st) == 0
            got = nf.cpu().numpy()
            assert got[0].tobytes() == np.float32(near).tobytes() and got[1].tobytes() == np.float32(far).tobytes(), (got, near, far)


@pytest.mark.gpu
@pytest.mark.parametrize("path,tag", FIXTURE_CASES)
def test_fused_geometry_loss_matches_golden(path, tag):
    """The fixture cases on the device.  On the pixels with norm_map == 0 the bound is 4 x the reference's own float32 deviation, elementwise; on
    the 11 x 29 fixture (45 non-zero elements there) that is 4 x 1.259e-06 for case a, and the element at row 1, x (-6.0e16 in a row of magnitude
    2.9e19: R^T gb cancels 480-fold) comes out 1.148e-05 off under plain float32 arithmetic, the float32 twin's included.  The kernel evaluates
    those rows in double (supervisor.hip:zero_normal_adjoint) and meets the bound."""
    from envgs_amd.loss import EnvGSGeometryLoss
    z, inp = _fixture(path)
    opts, it = _case(z, tag)
    dev = torch.device("cuda", 0)
    out, batch = _to_dev(inp, dev)
    loss, stats = EnvGSGeometryLoss(**opts)(out, batch, it)
    ref_loss = float(z["loss_" + tag])
    assert loss.shape == () and loss.device.type == "cuda" and loss.dtype == torch.float32
    assert sorted(stats) == sorted(str(s) for s in z["stats_" + tag])
    if tag == "d":
        assert float(loss) == 0.0 and not loss.requires_grad and not stats
        return
    loss.backward()
    loss = loss.detach()
    print("case %s loss %.9g ref %.9g" % (tag, float(loss), ref_loss))
    assert abs(float(loss) - ref_loss) < 1e-4 * abs(ref_loss)
    for k, v in stats.items():
        r = float(z["%s_%s" % (k, tag)])
        print("case %s %s %.9g ref %.9g" % (tag, k, float(v), r))
        assert abs(float(v) - r) < 1e-4 * abs(r), k
    assert out["dpt_map"].grad is None
    want = [k for k in GRAD_KEYS if "grad_%s_%s" % (k, tag) in z.files]
    for k in GRAD_KEYS:
        assert (out[k].grad is not None) == (k in want), k
    zero = (inp["norm_map"].reshape(-1, 3) == 0).all(-1)
    ref = {k: z["grad_%s_%s" % (k, tag)].reshape(-1, 3) if k.endswith("norm_map") else z["grad_%s_%s" % (k, tag)].reshape(-1) for k in want}
    got = {k: out[k].grad.cpu().numpy() for k in want}
    _check_grads(got, ref, zero, noise=float(z["f32_noise_zero_normal_" + tag]), what="case " + tag)


def _full_inputs(H, W, P, seed):
    g = np.random.default_rng(seed)
    N = H * W
    f32 = np.float32
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    nm = (unit(g.standard_normal((N, 3))) * (0.3 + 0.7 * g.random((N, 1)))).astype(f32)
    nm[g.random(N) < 0.1] = 0.0                                                          # background
    sn = (unit(g.standard_normal((N, 3))) * (0.3 + 0.7 * g.random((N, 1)))).astype(f32)
    prior = (unit(g.standard_normal((N, 3))) * 0.5 + 0.5).astype(f32)
    prior[g.random(N) < 0.05] = 0.5
    acc = g.random(N).astype(f32)
    acc[g.random(N) < 0.05] = 0.0
    dpt = (1.0 + 5.0 * g.random(N)).astype(f32)
    dpt[g.random(N) < 0.005] = 0.0
    n = int(N * 0.01)
    s = np.sort(dpt)
    dpt[g.integers(0, N, 5)] = s[n - 1]
    dpt[g.integers(0, N, 5)] = s[N - n]
    dist = (0.1 * g.random(N) ** 2).astype(f32)
    msk = (g.random(N) > 0.3).astype(f32)
    env = g.random(P).astype(f32)
    env[:50] = 0.0005 * g.random(50).astype(f32)
    env[50:100] = 1.0 - 0.0005 * g.random(50).astype(f32)
    R = np.linalg.qr(g.standard_normal((3, 3)))[0].astype(f32)
    return dict(norm_map=nm, surf_norm_map=sn, acc_map=acc, dpt_map=dpt, dist_map=dist, env_opacity=env, norm=prior, msk=msk, R=R)


@pytest.mark.gpu
def test_fused_geometry_loss_full_size_options_and_layouts():
    """800 x 800, P = 163 840: every combination of (acc scale, depth scale) x (sparse, l1), a non-unit upstream gradient, against the twin;
    channel-last contiguous maps and (3,H,W)-derived strided views give the same result."""
    from envgs_amd.loss import EnvGSGeometryLoss
    H, W, P = 800, 800, 163840
    dev = torch.device("cuda", 0)
    inp = _full_inputs(H, W, P, 11)
    zero = (inp["norm_map"] == 0).all(-1)
    shaped = dict(inp, norm_map=inp["norm_map"][None], surf_norm_map=inp["surf_norm_map"][None], acc_map=inp["acc_map"][None, :, None],
                  dpt_map=inp["dpt_map"][None, :, None], dist_map=inp["dist_map"][None, :, None], env_opacity=inp["env_opacity"][:, None],
                  norm=inp["norm"][None], msk=inp["msk"][None, :, None], R=inp["R"][None])
    first = None
    for use_acc in (False, True):
        for use_dpt in (False, True):
            for kind in ("sparse", "l1"):
                opts = dict(norm_loss_weight=0.01, norm_loss_start_iter=0, gs_norm_loss_weight=0.04, gs_norm_loss_start_iter=0, use_acc_scale_norm_loss=use_acc,
                            use_acc_scale_gs_norm_loss=use_acc, use_dpt_scale_norm_loss=use_dpt, use_dpt_scale_gs_norm_loss=use_dpt, msk_loss_weight=0.1,
                            msk_loss_start_iter=0, gs_dist_loss_weight=100.0, gs_dist_loss_start_iter=0, env_opacity_loss_weight=0.01, env_opacity_loss_type=kind)
                ref_loss, ref_stats, ref_grads = twin.geometry_loss(inp, opts, 5)
                out, batch = _to_dev(shaped, dev)
                loss, stats = EnvGSGeometryLoss(**opts)(out, batch, 5)
                (loss * 3.0).backward()
                what = "acc %d dpt %d %s" % (use_acc, use_dpt, kind)
                loss = loss.detach()
                print("%s loss %.9g ref %.9g" % (what, float(loss), ref_loss))
                assert abs(float(loss) - ref_loss) < 1e-4 * abs(ref_loss)
                assert sorted(stats) == sorted(ref_stats)
                for k, v in ref_stats.items():
                    assert abs(float(stats[k]) - v) < 1e-4 * abs(v), k
                got = {k: out[k].grad.cpu().numpy() / 3.0 for k in ref_grads}
                # (the twin is this project's own statement: there is no float32 run of the reference at this size, so the pixels with
                #  norm_map == 0 are held to the plain max-norm bound over their own set)
                _check_grads(got, ref_grads, zero, what=what)
                if use_acc and use_dpt and kind == "sparse":
                    first = (float(loss), {k: out[k].grad.clone() for k in ref_grads}, opts)
    # (3,H,W) planes viewed channel-last, as envgs_step hands them over; (H,W) single-channel maps
    ref_loss, ref_g, opts = first
    planes = {k: torch.from_numpy(inp[k].reshape(H, W, 3).transpose(2, 0, 1).copy()).to(dev).requires_grad_(True) for k in ("norm_map", "surf_norm_map")}
    singles = {k: torch.from_numpy(inp[k].reshape(H, W)).to(dev).requires_grad_(True) for k in ("acc_map", "dist_map")}
    env = torch.from_numpy(inp["env_opacity"]).to(dev).requires_grad_(True)
    out = dict(norm_map=planes["norm_map"].permute(1, 2, 0), surf_norm_map=planes["surf_norm_map"].permute(1, 2, 0), acc_map=singles["acc_map"],
               dist_map=singles["dist_map"][None], dpt_map=torch.from_numpy(inp["dpt_map"].reshape(1, H, W)).to(dev), env_opacity=env)
    prior_planes = torch.from_numpy(inp["norm"].reshape(H, W, 3).transpose(2, 0, 1).copy()).to(dev)
    batch = dict(norm=prior_planes.permute(1, 2, 0), msk=torch.from_numpy(inp["msk"].reshape(H, W, 1)).to(dev), R=torch.from_numpy(inp["R"]).to(dev))
    assert not out["norm_map"].is_contiguous()
    loss, _ = EnvGSGeometryLoss(**opts)(out, batch, 5)
    (loss * 3.0).backward()
    assert abs(float(loss.detach()) - ref_loss) <= 1e-6 * abs(ref_loss)
    for k in ("norm_map", "surf_norm_map"):
        assert planes[k].grad.shape == (3, H, W)
        assert torch.equal(planes[k].grad.permute(1, 2, 0).reshape(-1, 3), ref_g[k].reshape(-1, 3)), k
    for k in ("acc_map", "dist_map"):
        assert torch.equal(singles[k].grad.reshape(-1), ref_g[k].reshape(-1)), k
    assert torch.equal(env.grad.reshape(-1), ref_g["env_opacity"].reshape(-1))
    with pytest.raises(ValueError, match="one view per call"):
        EnvGSGeometryLoss(**opts)(out, dict(batch, R=torch.eye(3, device=dev).repeat(2, 1, 1)), 5)
    small = {k: v.reshape(-1, v.shape[-1])[:64] if v.dim() == 3 and v.shape[-1] == 3 else v.reshape(-1)[:64] for k, v in out.items() if k != "env_opacity"}
    with pytest.raises(ValueError, match="N >= 100"):
        EnvGSGeometryLoss(**opts)(small, dict(norm=batch["norm"].reshape(-1, 3)[:64], msk=batch["msk"].reshape(-1)[:64], R=batch["R"]), 5)


@pytest.mark.gpu
def test_geometry_loss_composes_with_the_image_loss_through_the_base_pass():
    import diff_surfel_rasterization_wet_ch05 as pkg
    from envgs_amd import envgs_step, fused, synth
    from envgs_amd.loss import EnvGSGeometryLoss, l1_ssim_loss
    dev = torch.device("cuda", 0)
    H = W = 96
    P = 3000
    base = synth.base_gaussians(P, seed=3, device=dev)
    base["scales"] = base["scales"] * 4.0
    for v in base.values():
        v.requires_grad_(True)
    cam = synth.orbit_camera(1, n_views=4, H=H, W=W, fx=1111.1 * W / 800.0, device=dev)
    g = torch.Generator().manual_seed(9)
    target = torch.rand(3, H, W, generator=g).to(dev)
    prior = torch.rand(1, H * W, 3, generator=g).to(dev)
    o = envgs_step.base_pass(pkg, cam, base, torch.zeros(3, device=dev), torch.tensor([2], device=dev))
    _, surf_normal = fused.surface_normal(o["allmap"], cam)
    output = dict(norm_map=o["normal"].permute(1, 2, 0), surf_norm_map=surf_normal.permute(1, 2, 0), acc_map=o["alpha"].permute(1, 2, 0),
                  dpt_map=o["depth"].permute(1, 2, 0), dist_map=o["allmap"][6:7].permute(1, 2, 0), env_opacity=torch.rand(500, 1, generator=g).to(dev).requires_grad_(True))
    batch = dict(norm=prior, msk=torch.ones(1, H * W, 1, device=dev), R=cam.world_view_transform[:3, :3].T[None])
    reg = EnvGSGeometryLoss(**ENVGS_YAML, msk_loss_weight=0.1, msk_loss_start_iter=0, gs_dist_loss_weight=100.0, gs_dist_loss_start_iter=0,
                            env_opacity_loss_weight=0.01)
    geo, stats = reg(output, batch, 100)
    assert sorted(stats) == ["env_opacity_loss", "gs_dist_loss", "gs_norm_loss", "msk_loss", "norm_loss"]
    img = l1_ssim_loss(o["rgb"], target)
    (img + geo).backward()
    assert np.isfinite(float(geo.detach())) and np.isfinite(float(img.detach())) and float(geo.detach()) != 0.0
    for k, v in base.items():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()), k
    keys = ("means3D", "scales", "rotations", "opacities")
    again = envgs_step.base_pass(pkg, cam, base, torch.zeros(3, device=dev), torch.tensor([2], device=dev))
    image_only = torch.autograd.grad(l1_ssim_loss(again["rgb"], target), [base[k] for k in keys])
    for k, ref in zip(keys, image_only):
        assert float((base[k].grad - ref).abs().max()) > 1e-3 * float(ref.abs().max()), k            # the geometry terms reach the geometry
    assert bool(torch.isfinite(output["env_opacity"].grad).all()) and float(output["env_opacity"].grad.abs().max()) > 0


@pytest.mark.gpu
def test_geometry_loss_never_synchronises_the_host():
    from envgs_amd.loss import EnvGSGeometryLoss
    z, inp = _fixture()
    dev = torch.device("cuda", 0)
    opts, it = _case(z, "c")
    reg = EnvGSGeometryLoss(**opts)
    out, batch = _to_dev(inp, dev)
    loss, _ = reg(out, batch, it)                                        # warm-up: library load, allocator
    loss.backward()
    out, batch = _to_dev(inp, dev)
    up = torch.full((), 2.0, device=dev)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, stats = reg(out, batch, it)
        (loss * up).backward()
        outside, none = EnvGSGeometryLoss(**_case(z, "d")[0])(out, batch, _case(z, "d")[1])        # outside every window
    finally:
        torch.cuda.set_sync_debug_mode(old)
    ref = float(z["loss_c"])
    assert abs(float(loss.detach()) - ref) < 1e-4 * abs(ref) and len(stats) == 5 and float(outside) == 0.0 and not none
    g = z["grad_dist_map_c"].reshape(-1)
    assert np.abs(out["dist_map"].grad.cpu().numpy().reshape(-1) / 2.0 - g).max() < 1e-4 * np.abs(g).max()
