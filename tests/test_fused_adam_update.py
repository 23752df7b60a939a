"""Sparse fused Adam (include/envgs_optim.h, envgs_amd/optim.py) by its UPDATE, in the project's usual triangle:

    float64 Adam written here from the formula  <-  oracle/adam_oracle.c (CPU, float)  <-  the HIP kernel

A measured step starts from p = 0, so that `p_after == -update` exactly and no rounding of `p - update` stands between the kernel and the
comparison; a second run from p ~ N(0, 1) must then equal `p - update` of the first, bit for bit.  The moments are compared with the oracle to
one float32 ulp (np.spacing: subnormals included, no atol), the update with float64 to 8 times the oracle's own error on the same case.

Every case is one step from a state installed by hand (step, exp_avg, exp_avg_sq), so that t = 30000 costs what t = 1 costs.

Measured (MI355X, 4099 elements per case, about 2450 of them updated).  e_ref, the oracle's largest relative update error against float64;
the kernel's own error against float64 was the same figure in all 75 cases, and not one element of exp_avg or exp_avg_sq differed from the
oracle's in any bit (the bound asserted is 8 * e_ref, at least 4.8e-7):

      t  betas         g=1,eps=1e-15  g=1e-6,eps=1e-15  g=1e-6,eps=1e-8  g=1e-18,eps=1e-15  g=1e-21,eps=1e-15
      1  (0.9, 0.999)  2.26e-07       2.37e-07          3.27e-07         2.27e-07           2.02e-07
      1  (0.5, 0.9)    2.01e-07       2.16e-07          2.14e-07         1.70e-07           1.80e-07
      1  (0, 0)        5.11e-13       6.46e-08          1.21e-07         1.30e-07           1.53e-07
      2  (0.9, 0.999)  3.62e-06       3.63e-06          3.65e-06         3.49e-07           2.71e-07
      2  (0.5, 0.9)    1.92e-07       1.97e-07          2.47e-07         1.85e-07           1.98e-07
      2  (0, 0)        6.38e-12       7.44e-08          1.20e-07         1.32e-07           1.37e-07
     10  (0.9, 0.999)  4.29e-07       4.04e-07          4.05e-07         2.02e-07           2.27e-07
     10  (0.5, 0.9)    2.21e-07       2.31e-07          2.33e-07         1.58e-07           1.54e-07
     10  (0, 0)        2.10e-12       6.47e-08          1.25e-07         1.31e-07           1.40e-07
   1000  (0.9, 0.999)  2.37e-07       2.90e-07          2.76e-07         2.13e-07           2.00e-07
   1000  (0.5, 0.9)    1.77e-07       2.13e-07          1.90e-07         1.57e-07           1.58e-07
   1000  (0, 0)        7.99e-13       5.96e-08          1.22e-07         1.35e-07           1.49e-07
  30000  (0.9, 0.999)  2.34e-07       2.49e-07          2.23e-07         2.12e-07           2.16e-07
  30000  (0.5, 0.9)    1.80e-07       1.83e-07          1.76e-07         1.75e-07           1.78e-07
  30000  (0, 0)        1.55e-12       5.92e-08          1.20e-07         1.32e-07           1.47e-07

Only t = 2 with beta2 = 0.999 shows the powf cancellation (1 - 0.999^2 = 0.002); at t = 1 powf returns beta itself on both sides and the
subtraction is exact.  Long run, 200 steps: d_ref 6.4e-8, the kernel 5.6e-8 from float64, at max |p| 0.14.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_fused_adam import oracle_adam
from tests.util import record

STEPS = [1, 2, 10, 1000, 30000]
SCALES = [(1.0, 1e-15), (1e-6, 1e-15), (1e-6, 1e-8), (1e-18, 1e-15), (1e-21, 1e-15)]       # (gradient scale, eps)
BETAS = [(0.9, 0.999), (0.5, 0.9), (0.0, 0.0)]
N = 4099                                      # five 1024-element chunks, the last one 3 elements: vector quads, whole zero quads and a scalar tail
LR = 1e-2
ULP4 = 4 * 2.0 ** -23                         # floor of the update bound: 4 float32 ulp (4.8e-7)
K_REF = 8.0                                   # kernel-vs-float64 bound in units of the oracle's error on the same case (the issue's reasoning:
                                              # both carry the powf rounding amplified by 1 / (1 - beta^t); device powf ~2 ulp against glibc's < 1,
                                              # sqrtf and the division about one each)


def f32(x):
    return np.float32(x)


def sparse_gradient(rng, n, scale):
    """g ~ N(0, 1) * scale with about 40 % exact zeros: random ones, whole zero quads, and some of them -0.0 (skipped like +0)."""
    g = (rng.standard_normal(n) * scale).astype(np.float32)
    g[rng.random(n) < 0.4] = 0.0
    if n >= 64:
        g[n // 8 // 4 * 4:n // 8 // 4 * 4 + 24] = 0.0                       # six whole quads
    zero = np.flatnonzero(g == 0)
    g[zero[::3]] = -0.0
    return g


def installed_state(rng, g, scale, beta1):
    """Moments of the gradient's scale.  m is drawn independently of g, except that where beta1 * m and (1 - beta1) * g would cancel to less than a
    quarter of their magnitudes the sign of m is flipped: the relative error of the update then speaks about the formula, not about a
    cancellation in m' whose amplified rounding both sides share (the 1-ulp state comparison covers m' whatever its conditioning)."""
    n = g.size
    m = (rng.standard_normal(n) * 0.3 * scale).astype(np.float32)
    a, b = np.float64(f32(beta1)) * m.astype(np.float64), (1.0 - np.float64(f32(beta1))) * g.astype(np.float64)
    flip = np.abs(a + b) < 0.25 * (np.abs(a) + np.abs(b))
    m[flip] = -m[flip]
    v = ((0.25 + rng.random(n)) * scale * scale).astype(np.float32)       # subnormal in float32 at scale 1e-21, partly at 1e-18
    return m, v


def adam_f64(g, m, v, t, beta1, beta2, lr, eps):
    """Adam in float64, from the formula.  Hyper-parameters are rounded to float32 first (the kernel receives floats); elements whose gradient is
    zero keep their moments and get no update.  Returns (update, m', v')."""
    b1, b2, lr, eps = (np.float64(f32(x)) for x in (beta1, beta2, lr, eps))
    g, m, v = (np.asarray(a, np.float64) for a in (g, m, v))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    update = lr / (1.0 - b1 ** t) * m1 / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** t) + eps)
    nz = g != 0
    return np.where(nz, update, 0.0), np.where(nz, m1, m), np.where(nz, v1, v)


@functools.lru_cache(maxsize=None)
def case(t, scale, eps, betas):
    """One case of the matrix: inputs, the float64 step and the oracle's step from p = 0 (computed once, shared by the CPU and the GPU test)."""
    rng = np.random.default_rng([t, int(-np.log10(scale)), int(-np.log10(eps)), int(betas[0] * 10)])
    g = sparse_gradient(rng, N, scale)
    m, v = installed_state(rng, g, scale, betas[0])
    p0 = rng.standard_normal(N).astype(np.float32)
    u64, m64, v64 = adam_f64(g, m, v, t, betas[0], betas[1], LR, eps)
    po, mo, vo = oracle_adam(np.zeros(N, np.float32), g, m, v, float(t), betas[0], betas[1], LR, eps)
    c = dict(g=g, m=m, v=v, p0=p0, u64=u64, m64=m64, v64=v64, u_orc=-po, m_orc=mo, v_orc=vo, nz=g != 0)
    for a in c.values():
        a.setflags(write=False)
    c["e_ref"] = rel_update_error(c["u_orc"], c)
    return c


def rel_update_error(u, c):
    nz = c["nz"]
    return float((np.abs(u[nz].astype(np.float64) - c["u64"][nz]) / np.abs(c["u64"][nz])).max())


def case_id(t, scale, eps, betas):
    return "t%d-g%g-eps%g-b%g_%g" % (t, scale, eps, betas[0], betas[1])


MATRIX = [(t, s, e, b) for t in STEPS for s, e in SCALES for b in BETAS]
MATRIX_IDS = [case_id(*c) for c in MATRIX]


def ulp_distance_exceeds(a, b, ulps=1):
    """Elementwise |a - b| > ulps * spacing(b) in float32 (np.spacing: the subnormal range has its own, constant, spacing)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) > ulps * np.spacing(np.abs(b)).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(a, b, what=""):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d of %d elements differ in bits, first at %d" % (what, bad.size, a.size, bad[0])


# ------------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the float64 formula, the oracle against it, the C-ABI's refusals
# ------------------------------------------------------------------------------------------------------------------------------------------------

def test_float64_adam_is_torch_adam_in_float64():
    """The module's float64 formula against torch.optim.Adam on float64 tensors (dense gradients, eight steps): an independent statement of Adam."""
    rng = np.random.default_rng(5)
    b1, b2, lr, eps = (float(f32(x)) for x in (0.9, 0.999, 1e-2, 1e-15))
    tp = torch.nn.Parameter(torch.zeros(257, dtype=torch.float64))
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = np.zeros(257), np.zeros(257), np.zeros(257)
    for t in range(1, 9):
        g = rng.standard_normal(257) * 1e-4 + 2e-4
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        u, m, v = adam_f64(g, m, v, t, b1, b2, lr, eps)
        p = p - u
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=0)


def test_float64_adam_leaves_zero_gradients_alone():
    g = np.array([0.0, -0.0, 1.0, -2.0], np.float32)
    m = np.array([1.0, 2.0, 3.0, 4.0], np.float32); v = np.array([5.0, 6.0, 7.0, 8.0], np.float32)
    u, m1, v1 = adam_f64(g, m, v, 3, 0.9, 0.999, 1e-2, 1e-15)
    assert (u[:2] == 0).all() and (m1[:2] == m[:2]).all() and (v1[:2] == v[:2]).all()
    assert (u[2:] != 0).all() and (m1[2:] != m[2:]).all() and (v1[2:] != v[2:]).all()


@pytest.mark.parametrize("t,scale,eps,betas", MATRIX, ids=MATRIX_IDS)
def test_oracle_update_matches_float64(t, scale, eps, betas):
    """Oracle against float64: e_ref, the largest relative error of the oracle's update, is recorded; it is the unit of the kernel's bound.  What is
    asserted here is what float arithmetic promises the oracle: moments within their two roundings of the float64 ones (one float multiply,
    double arithmetic, one rounding), skipped elements untouched, and an update whose relative error stays below the sum of
      - the powf rounding (one ulp, 2^-23 of beta^t) amplified by the cancellation beta^t / (1 - beta^t), halved under the square root for beta2;
      - sixteen float roundings of 2^-24: bc1, bc2, lr / bc1, sqrtf(bc2), sqrtf(v'), the division, + eps, m' / denom, * step_size, the rounding
        of m' and of beta1 * m (up to four times m' after `installed_state`), with three to spare;
      - the rounding of v' itself, half its spacing over v' and halved again by the square root, weighted by the share of sqrt(v') in the
        denominator: the only term that counts where v' is subnormal."""
    c = case(t, scale, eps, betas)
    name = "fused_adam_update[%s]" % case_id(t, scale, eps, betas)
    record(name, "e_ref", c["e_ref"], "oracle update vs float64, max relative")
    z = ~c["nz"]
    assert 0.35 < z.mean() < 0.5 and np.signbit(c["g"][z]).any() and not np.signbit(c["g"][z]).all()
    assert (c["u_orc"][z] == 0).all() and np.array_equal(bits(c["m_orc"][z]), bits(c["m"][z])) and np.array_equal(bits(c["v_orc"][z]), bits(c["v"][z]))
    b1, b2 = (float(f32(b)) for b in betas)
    for got, want, old, b in ((c["m_orc"], c["m64"], c["m"], b1), (c["v_orc"], c["v64"], c["v"], b2)):
        # two roundings to float: of beta * old (half its spacing) and of the result (half its own, a whole one for slack in the double sum)
        room = 0.5 * np.spacing(np.abs(b * old.astype(np.float64)).astype(np.float32)) + np.spacing(np.abs(want).astype(np.float32))
        assert (np.abs(got.astype(np.float64) - want) <= room.astype(np.float64)).all()
    nz = c["nz"]
    if scale == 1e-21:                                                                             # every v' subnormal, none flushed; m' normal
        assert (c["v_orc"][nz] < np.finfo(np.float32).tiny).all() and (c["v_orc"][nz & (c["v64"] > 1.5e-45)] > 0).all()
        assert (np.abs(c["m_orc"][nz]) >= np.finfo(np.float32).tiny).all()
    amp = sum(2.0 ** -23 * b ** t / (1.0 - b ** t) * w for b, w in ((b1, 1.0), (b2, 0.5)) if b > 0)
    root = np.sqrt(c["v64"][nz]) / np.sqrt(1.0 - b2 ** t)
    v_term = (root / (root + float(f32(eps))) * 0.25 * np.spacing(c["v64"][nz].astype(np.float32)) / np.maximum(c["v64"][nz], 1e-300)).max()
    assert c["e_ref"] <= amp + 16 * 2.0 ** -24 + v_term, (c["e_ref"], amp, v_term)


def _adam_tensor(_lib, param=0, grad=0, exp_avg=0, exp_avg_sq=0, numel=0, lr=1e-2, step=1.0):
    return _lib.AdamTensor(param, grad, exp_avg, exp_avg_sq, numel, lr, step)


def test_fused_adam_abi_refuses_bad_arguments_before_any_gpu_work():
    from envgs_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    one = (_lib.AdamTensor * 1)(_adam_tensor(_lib))
    assert lib.envgs_fused_adam(-1, one, 0.9, 0.999, 1e-15, None) == -1
    many = (_lib.AdamTensor * 25)(*[_adam_tensor(_lib) for _ in range(25)])
    assert lib.envgs_fused_adam(25, many, 0.9, 0.999, 1e-15, None) == -1
    assert lib.envgs_fused_adam(1, None, 0.9, 0.999, 1e-15, None) == -1
    fake = 0x1000                                                                               # never dereferenced: the refusal precedes the launch
    for missing in ("param", "grad", "exp_avg", "exp_avg_sq"):
        kw = dict(param=fake, grad=fake, exp_avg=fake, exp_avg_sq=fake, numel=8)
        kw[missing] = 0
        for arr in ((_lib.AdamTensor * 1)(_adam_tensor(_lib, **kw)),
                    (_lib.AdamTensor * 3)(_adam_tensor(_lib), _adam_tensor(_lib, **kw), _adam_tensor(_lib))):
            assert lib.envgs_fused_adam(len(arr), arr, 0.9, 0.999, 1e-15, None) == -1, missing
    assert lib.envgs_fused_adam(0, None, 0.9, 0.999, 1e-15, None) == 0
    assert lib.envgs_fused_adam(0, one, 0.9, 0.999, 1e-15, None) == 0
    empty = (_lib.AdamTensor * 24)(*[_adam_tensor(_lib) for _ in range(24)])                    # all numel == 0: nothing to do, pointers not looked at
    assert lib.envgs_fused_adam(24, empty, 0.9, 0.999, 1e-15, None) == 0


# ------------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------------------

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def abi_step(tensors, betas, eps):
    """One envgs_fused_adam call over `tensors`: dicts of device tensors p, g, m, v (updated in place) with lr and t.  At most 24."""
    from envgs_amd import _lib
    lib = _lib.load()
    arr = (_lib.AdamTensor * len(tensors))()
    for j, T in enumerate(tensors):
        arr[j] = _lib.AdamTensor(T["p"].data_ptr(), T["g"].data_ptr(), T["m"].data_ptr(), T["v"].data_ptr(), T["p"].numel(), T["lr"], float(T["t"]))
    stream = _lib.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(lib.envgs_fused_adam(len(tensors), arr, betas[0], betas[1], eps, stream), "envgs_fused_adam")
    torch.cuda.synchronize()


def abi_single(p, g, m, v, t, betas, lr, eps):
    """The single-tensor, freshly allocated (aligned) run every layout is compared with: numpy in, numpy (p', m', v') out."""
    T = dict(p=dev(p), g=dev(g), m=dev(m), v=dev(v), lr=lr, t=t)
    if T["p"].numel():
        assert all(T[k].data_ptr() % 16 == 0 for k in "pgmv")
    abi_step([T], betas, eps)
    return host(T["p"]), host(T["m"]), host(T["v"])


def optimizer_step(params, betas, eps):
    """One FusedAdam.step() over `params`: dicts with numpy p, g (or None), m, v, lr, t -- one param group each, the state installed by hand
    (t == 1 with m is None: no state, the optimizer creates it).  Returns the optimizer and the torch Parameters."""
    from envgs_amd.optim import FusedAdam
    ps = [torch.nn.Parameter(dev(P["p"]).reshape(P.get("shape", (-1,)))) for P in params]
    opt = FusedAdam([{"params": [p], "lr": P["lr"], "betas": P.get("betas", betas), "eps": P.get("eps", eps)} for p, P in zip(ps, params)], lr=0.0)
    for p, P in zip(ps, params):
        if P.get("m") is not None:
            opt.state[p] = {"step": torch.tensor(float(P["t"] - 1)), "exp_avg": dev(P["m"]).reshape(p.shape), "exp_avg_sq": dev(P["v"]).reshape(p.shape)}
        if P["g"] is not None:
            p.grad = P["g"] if torch.is_tensor(P["g"]) else dev(P["g"]).reshape(p.shape)
    opt.step()
    torch.cuda.synchronize()
    return opt, ps


def state_of(opt, p):
    st = opt.state[p]
    return host(p).reshape(-1), host(st["exp_avg"]).reshape(-1), host(st["exp_avg_sq"]).reshape(-1), float(st["step"])


@pytest.mark.gpu
@pytest.mark.parametrize("t,scale,eps,betas", MATRIX, ids=MATRIX_IDS)
def test_kernel_update_against_oracle_and_float64(t, scale, eps, betas):
    c = case(t, scale, eps, betas)
    name = "fused_adam_update[%s]" % case_id(t, scale, eps, betas)
    nz, z = c["nz"], ~c["nz"]
    opt, (q,) = optimizer_step([dict(p=np.zeros(N, np.float32), g=c["g"], m=c["m"], v=c["v"], lr=LR, t=t)], betas, eps)
    pk, mk, vk, step = state_of(opt, q)
    assert step == t
    # skipped elements (+0 and -0 gradients): nothing written
    assert_bits_equal(pk[z], np.zeros(int(z.sum()), np.float32), "p of skipped elements")
    assert_bits_equal(mk[z], c["m"][z], "exp_avg of skipped elements"); assert_bits_equal(vk[z], c["v"][z], "exp_avg_sq of skipped elements")
    # state against the oracle: one float32 ulp, no atol -- a flushed subnormal v (spacing 1.4e-45) is many ulps from the oracle's
    bad_m, bad_v = ulp_distance_exceeds(mk, c["m_orc"], 1), ulp_distance_exceeds(vk, c["v_orc"], 1)
    record(name, "m_ulp_diff", int((bits(mk) != bits(c["m_orc"])).sum()), "elements of exp_avg that differ from the oracle at all, of %d" % int(nz.sum()))
    record(name, "v_ulp_diff", int((bits(vk) != bits(c["v_orc"])).sum()), "elements of exp_avg_sq that differ from the oracle at all")
    e_k = rel_update_error(-pk, c)
    record(name, "e_ref", c["e_ref"], "oracle update vs float64, max relative")
    record(name, "e_kernel", e_k, "kernel update vs float64, max relative; e_ref %.3g, bound %.3g" % (c["e_ref"], max(K_REF * c["e_ref"], ULP4)))
    print("%s: e_ref %.3e e_kernel %.3e m_diff %d v_diff %d" % (name, c["e_ref"], e_k, (bits(mk) != bits(c["m_orc"])).sum(), (bits(vk) != bits(c["v_orc"])).sum()))
    assert not bad_m.any(), "exp_avg: %d elements beyond 1 ulp of the oracle, first %d" % (bad_m.sum(), np.flatnonzero(bad_m)[0])
    assert not bad_v.any(), "exp_avg_sq: %d elements beyond 1 ulp of the oracle, first %d" % (bad_v.sum(), np.flatnonzero(bad_v)[0])
    # elements that differ from the oracle AT ALL: a fused instead of an unfused double multiply-add moves the double sum by at most 2^-53 of
    # itself, which changes the float it rounds to only where the sum lies that close to a rounding boundary -- 2^-29 of the elements, 5e-6 of
    # one expected per case.  One is allowed; all-float moment arithmetic differs in the last bit of several to hundreds of them
    assert (bits(mk) != bits(c["m_orc"])).sum() <= 1 and (bits(vk) != bits(c["v_orc"])).sum() <= 1
    # update against float64
    assert e_k <= max(K_REF * c["e_ref"], ULP4), (e_k, c["e_ref"])
    # the same step from p ~ N(0, 1): p - update of the run from zero, bit for bit; the moments do not depend on p
    opt, (q,) = optimizer_step([dict(p=c["p0"], g=c["g"], m=c["m"], v=c["v"], lr=LR, t=t)], betas, eps)
    p1, m1, v1, _ = state_of(opt, q)
    assert_bits_equal(p1, c["p0"] - (-pk), "p - update")
    assert_bits_equal(p1[z], c["p0"][z], "p of skipped elements")
    assert_bits_equal(m1, mk, "exp_avg from p != 0"); assert_bits_equal(v1, vk, "exp_avg_sq from p != 0")


def _mixed(i, t, lr):
    rng = np.random.default_rng(100 + i)
    n = (1500, 1029, 2048)[i]
    g = sparse_gradient(rng, n, 1e-4)
    m, v = installed_state(rng, g, 1e-4, 0.9)
    return dict(p=rng.standard_normal(n).astype(np.float32), g=g, m=m, v=v, t=t, lr=lr)


@pytest.mark.gpu
def test_mixed_steps_and_rates_in_one_launch():
    """`step` and `lr` travel per tensor record: three tensors at t = 1, 10 and 30000 in one launch, each equal to its own single-tensor run."""
    betas, eps = (0.9, 0.999), 1e-15
    params = [_mixed(i, t, lr) for i, (t, lr) in enumerate([(1, 1e-2), (10, 3e-3), (30000, 1.6e-4)])]
    opt, ps = optimizer_step(params, betas, eps)
    singles = []
    for P, q in zip(params, ps):
        want = abi_single(P["p"], P["g"], P["m"], P["v"], P["t"], betas, P["lr"], eps)
        got = state_of(opt, q)
        assert got[3] == P["t"]
        for a, b, what in zip(got, want, ("p", "exp_avg", "exp_avg_sq")):
            assert_bits_equal(a, b, "%s of the tensor at t=%d" % (what, P["t"]))
        singles.append(want)
    # and the steps really matter: tensor 0 at the step of tensor 1 is another result
    tc = dict(p=dev(params[0]["p"]), g=dev(params[0]["g"]), m=dev(params[0]["m"]), v=dev(params[0]["v"]), lr=params[0]["lr"], t=10)
    abi_step([tc], betas, eps)
    assert (bits(host(tc["p"])) != bits(singles[0][0])).mean() > 0.3                               # tensor 0 at the step of tensor 1: another result


POISON = 7.25


def _window(values, n, k):
    """A device buffer of n + 4 floats filled with POISON, `values` written at [k, k + n); returns (buffer, view of the window)."""
    buf = torch.full((n + 4,), POISON, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[k:k + n] = dev(values)
    return buf, buf[k:k + n]


ALIGN_CASES = [("param", (1, 0, 0, 0)), ("grad", (0, 1, 0, 0)), ("exp_avg", (0, 0, 1, 0)), ("exp_avg_sq", (0, 0, 0, 1)),
               ("all+1", (1, 1, 1, 1)), ("all+2", (2, 2, 2, 2)), ("all+3", (3, 3, 3, 3))]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 7, 1024, 1029])
def test_misaligned_pointers_through_the_c_abi(n):
    """The float4 path needs all four pointers 16-byte aligned; base + k elements sends whole quads through the scalar loop.  Same bits as the
    aligned run, and not one float outside [k, k + n) written."""
    betas, eps, t, lr = (0.9, 0.999), 1e-15, 10, 1e-2
    rng = np.random.default_rng(n)
    g = sparse_gradient(rng, n, 1e-4)
    if n == 4:
        g[:] = (1e-4, 0.0, -2e-4, -0.0)
    m, v = installed_state(rng, g, 1e-4, betas[0])
    p = rng.standard_normal(n).astype(np.float32)
    want = abi_single(p, g, m, v, t, betas, lr, eps)
    assert (bits(want[0]) != bits(p)).any()
    for label, ks in ALIGN_CASES:
        bufs, views = zip(*[_window(a, n, k) for a, k in zip((p, g, m, v), ks)])
        for w, k in zip(views, ks):
            assert w.is_contiguous() and w.data_ptr() % 16 == 4 * k
        abi_step([dict(p=views[0], g=views[1], m=views[2], v=views[3], lr=lr, t=t)], betas, eps)
        for what, buf, k, ref in zip(("p", "g", "exp_avg", "exp_avg_sq"), bufs, ks, (want[0], g, want[1], want[2])):
            b = host(buf)
            assert_bits_equal(b[k:k + n], ref, "%s: %s of n=%d" % (label, what, n))
            outside = np.concatenate([b[:k], b[k + n:]])
            assert_bits_equal(outside, np.full(4, POISON, np.float32), "%s: floats around the window of %s" % (label, what))


@pytest.mark.gpu
def test_parameter_made_from_an_offset_view_steps():
    """torch.nn.Parameter(buf[1:]) is contiguous with a storage offset: the wrapper takes it, and the kernel's scalar path updates it."""
    from envgs_amd.optim import FusedAdam
    n = 1029
    rng = np.random.default_rng(77)
    g = sparse_gradient(rng, n, 1e-4)
    p = rng.standard_normal(n).astype(np.float32)
    buf, _ = _window(p, n, 1)
    q = torch.nn.Parameter(buf[1:1 + n])
    assert q.is_contiguous() and q.data_ptr() % 16 == 4
    opt = FusedAdam([q], lr=1e-2, betas=(0.9, 0.999), eps=1e-15)
    zeros = np.zeros(n, np.float32)
    want = (p, zeros, zeros)
    for t in (1, 2):
        q.grad = dev(g)
        opt.step()
        torch.cuda.synchronize()
        want = abi_single(want[0], g, want[1], want[2], t, (0.9, 0.999), 1e-2, 1e-15)
        got = state_of(opt, q)
        assert got[3] == t
        for a, b, what in zip(got, want, ("p", "exp_avg", "exp_avg_sq")):
            assert_bits_equal(a, b, "%s after step %d" % (what, t))
    b = host(buf)
    assert b[0] == POISON and (b[1 + n:] == POISON).all()


LAYOUT_SIZES = [0, 1, 3, 4, 1023, 1024, 1025, 2048, 4099]


def _layout_tensor(i, n, scale=1e-4):
    rng = np.random.default_rng(1000 + i)
    g = sparse_gradient(rng, n, scale)
    m, v = installed_state(rng, g, scale, 0.9)
    return dict(p=rng.standard_normal(n).astype(np.float32), g=g, m=m, v=v, t=1 + 3 * i, lr=1e-2 / (1 + i % 5))


@pytest.mark.gpu
def test_twenty_four_tensors_with_empty_ones_in_one_call():
    """The chunk-to-tensor scan: every size class around the 1024-element chunk, empty tensors first, in the middle and last."""
    betas, eps = (0.9, 0.999), 1e-15
    rng = np.random.default_rng(24)
    sizes = [0] + list(rng.permutation(LAYOUT_SIZES[1:])) + [0, 0] + list(rng.choice(LAYOUT_SIZES, 11)) + [1025, 0]
    assert len(sizes) == 24 and set(sizes) == set(LAYOUT_SIZES)
    params = [_layout_tensor(i, int(n)) for i, n in enumerate(sizes)]
    T = [dict(p=dev(P["p"]), g=dev(P["g"]), m=dev(P["m"]), v=dev(P["v"]), lr=P["lr"], t=P["t"]) for P in params]
    abi_step(T, betas, eps)
    for i, (P, d) in enumerate(zip(params, T)):
        want = abi_single(P["p"], P["g"], P["m"], P["v"], P["t"], betas, P["lr"], eps)
        for k, b in zip("pmv", want):
            assert_bits_equal(host(d[k]), b, "%s of tensor %d (n=%d)" % (k, i, sizes[i]))
        assert_bits_equal(host(d["g"]), P["g"], "grad of tensor %d" % i)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [25, 49])
def test_optimizer_splits_more_than_24_parameters_into_launches(count):
    betas, eps = (0.9, 0.999), 1e-15
    sizes = [(3, 1025, 4, 1, 64)[i % 5] for i in range(count)]
    params = [_layout_tensor(i, n) for i, n in enumerate(sizes)]
    opt, ps = optimizer_step(params, betas, eps)
    for i, (P, q) in enumerate(zip(params, ps)):
        want = abi_single(P["p"], P["g"], P["m"], P["v"], P["t"], betas, P["lr"], eps)
        got = state_of(opt, q)
        assert got[3] == P["t"]
        for a, b, what in zip(got, want, ("p", "exp_avg", "exp_avg_sq")):
            assert_bits_equal(a, b, "%s of parameter %d of %d" % (what, i, count))


@pytest.mark.gpu
def test_optimizer_groups_none_gradients_views_and_empty_parameters():
    """FusedAdam's own glue: param groups that differ in betas and eps go to separate launches with their own values; `grad is None` creates no
    state and advances no step; a transposed (non-contiguous) gradient is read in the parameter's order; an empty parameter is harmless."""
    groups = [((0.9, 0.999), 1e-15), ((0.5, 0.9), 1e-8), ((0.9, 0.999), 1e-8)]
    params = []
    for i in range(6):
        P = _layout_tensor(50 + i, (40, 1030, 7, 40, 1030, 7)[i])
        P["betas"], P["eps"] = groups[i % 3]
        params.append(P)
    rng = np.random.default_rng(9)
    gt = torch.from_numpy(rng.standard_normal((8, 5)).astype(np.float32) * 1e-4).to(DEV).t()      # (5, 8) view of an (8, 5) tensor
    assert not gt.is_contiguous()
    params[0]["shape"], params[0]["g"] = (5, 8), gt
    untouched = dict(_layout_tensor(60, 33), g=None)                                              # has state, gets no gradient
    fresh = dict(p=np.ones(9, np.float32), g=None, m=None, v=None, t=1, lr=1e-2)                  # no state, no gradient
    empty = dict(p=np.zeros(0, np.float32), g=np.zeros(0, np.float32), m=None, v=None, t=1, lr=1e-2)
    params += [untouched, fresh, empty]
    opt, ps = optimizer_step(params, (0.9, 0.999), 1e-15)
    for i, (P, q) in enumerate(zip(params[:6], ps[:6])):
        g = host(P["g"].contiguous()).reshape(-1) if torch.is_tensor(P["g"]) else P["g"]
        want = abi_single(P["p"], g, P["m"], P["v"], P["t"], P["betas"], P["lr"], P["eps"])
        got = state_of(opt, q)
        assert got[3] == P["t"]
        for a, b, what in zip(got, want, ("p", "exp_avg", "exp_avg_sq")):
            assert_bits_equal(a, b, "%s of parameter %d (betas %s eps %g)" % (what, i, P["betas"], P["eps"]))
    # the groups really differ: parameter 0 stepped with group 1's values is another result
    P = params[0]
    other = abi_single(P["p"], host(gt.contiguous()).reshape(-1), P["m"], P["v"], P["t"], groups[1][0], P["lr"], groups[1][1])
    assert (bits(other[0]) != bits(state_of(opt, ps[0])[0])).any()
    got = state_of(opt, ps[6])
    assert got[3] == untouched["t"] - 1
    for a, b, what in zip(got, (untouched["p"], untouched["m"], untouched["v"]), ("p", "exp_avg", "exp_avg_sq")):
        assert_bits_equal(a, b, "%s of the parameter without a gradient" % what)
    assert len(opt.state[ps[7]]) == 0 and (host(ps[7]) == 1).all()
    st = opt.state[ps[8]]
    assert float(st["step"]) == 1 and st["exp_avg"].numel() == 0 and st["exp_avg_sq"].numel() == 0


@pytest.mark.gpu
def test_non_finite_gradients_stay_in_their_element():
    """One NaN and one Inf gradient inside vector quads: that element's p, m, v turn non-finite as in the oracle, its three quad neighbours and
    everything else keep the bits of the run in which those two gradients are zero."""
    betas, eps, t, lr, n = (0.9, 0.999), 1e-15, 10, 1e-2, 1030
    rng = np.random.default_rng(31)
    g = sparse_gradient(rng, n, 1e-4)
    m, v = installed_state(rng, g, 1e-4, betas[0])
    p = rng.standard_normal(n).astype(np.float32)
    bad = {513: np.nan, 770: np.inf, 1029: -np.inf}                                               # two vector quads and the scalar tail
    g[[512, 514, 515, 768, 769, 771]] = 1e-4                                                      # live neighbours
    clean, dirty = g.copy(), g.copy()
    for i, x in bad.items():
        clean[i] = 0.0; dirty[i] = x
    want = abi_single(p, clean, m, v, t, betas, lr, eps)
    got = abi_single(p, dirty, m, v, t, betas, lr, eps)
    orc = oracle_adam(p, dirty, m, v, float(t), betas[0], betas[1], lr, eps)
    keep = np.ones(n, bool); keep[list(bad)] = False
    for a, b, what in zip(got, want, ("p", "exp_avg", "exp_avg_sq")):
        assert_bits_equal(a[keep], b[keep], "%s beside the non-finite gradients" % what)
    for i in bad:
        for a, o, what in zip(got, orc, ("p", "exp_avg", "exp_avg_sq")):
            assert not np.isfinite(a[i]) and not np.isfinite(o[i]), (what, i, a[i], o[i])
            assert np.isnan(a[i]) == np.isnan(o[i]) and (np.isnan(a[i]) or a[i] == o[i]), (what, i, a[i], o[i])


@pytest.mark.gpu
def test_two_hundred_steps_stay_with_float64():
    """A bias that each single step hides: 200 steps on 4096 elements, a fresh zero pattern each step, gradient scale 1e-4, eps 1e-15.  d_ref is
    the oracle trajectory's final distance from the float64 trajectory (measured here, recorded); the kernel's is at most 8 times that."""
    from envgs_amd.optim import FusedAdam
    n, steps, betas, eps, lr = 4096, 200, (0.9, 0.999), 1e-15, 1e-3
    rng = np.random.default_rng(200)
    G = np.stack([sparse_gradient(rng, n, 1e-4) for _ in range(steps)])
    b = (rng.standard_normal(n) * 5e-5).astype(np.float32)                                         # a per-element mean: the trajectories go somewhere
    G = np.where(G != 0, G + b, G).astype(np.float32)
    p64, m64, v64 = np.zeros(n), np.zeros(n), np.zeros(n)
    po, mo, vo = (np.zeros(n, np.float32) for _ in range(3))
    q = torch.nn.Parameter(torch.zeros(n, device=DEV))
    opt = FusedAdam([q], lr=lr, betas=betas, eps=eps)
    Gd = torch.from_numpy(G).to(DEV)
    for t in range(1, steps + 1):
        u, m64, v64 = adam_f64(G[t - 1], m64, v64, t, betas[0], betas[1], lr, eps)
        p64 = p64 - u
        po, mo, vo = oracle_adam(po, G[t - 1], mo, vo, float(t), betas[0], betas[1], lr, eps)
        q.grad = Gd[t - 1]
        opt.step()
    torch.cuda.synchronize()
    pk, mk, vk, step = state_of(opt, q)
    assert step == steps and np.abs(p64).max() > 50 * lr
    d_ref = float(np.abs(po - p64).max())
    d_k = float(np.abs(pk - p64).max())
    record("fused_adam_long_run", "d_ref", d_ref, "oracle vs float64 after %d steps, max |dp|; max |p| %.3g" % (steps, np.abs(p64).max()))
    record("fused_adam_long_run", "d_kernel", d_k, "kernel vs float64 after %d steps, max |dp|" % steps)
    print("long run: d_ref %.3e d_kernel %.3e max|p| %.3e" % (d_ref, d_k, np.abs(p64).max()))
    assert d_ref > 0
    assert d_k <= 8 * d_ref, (d_k, d_ref)
