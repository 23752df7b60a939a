"""CPU: the float64 reference the BVH tests hold the builder to (tests/bvh_reference.py), pinned against the surfel parameters and against the
brute-force oracle's audit before any GPU is involved: rays aimed just INSIDE the contribution boundary of a surfel (alpha = (1 + 1e-2) / 255 at
the point where the disc touches its own bounding box) hit it, rays aimed just outside never do."""
import numpy as np
import pytest
import torch

from envgs_amd import synth
from oracle import trace as otr
from tests import bvh_reference as br
from tests.util import FRAGILE_RAYS_MAX, record_fragile

SEED = 3


def _scene(P=256, seed=SEED):
    g = br.scene(P, seed)
    v, _ = synth.get_disks(*(torch.from_numpy(g[k]) for k in ("means3D", "scales", "rotations")))
    return g, v.numpy()


def test_frame_recovered_from_the_vertices():
    g, v = _scene()
    mu, a, b = br.frame(v)
    R = synth.build_rotation(torch.from_numpy(g["rotations"]).double()).numpy()
    s = g["scales"].astype(np.float64)
    eps = 2.0 ** -23
    # a corner is mu -+ 3a +- 3b in fp32: each coordinate carries a few roundings of magnitude |mu| + 3|a| + 3|b| (<= 1.4 here)
    assert np.abs(mu - g["means3D"]).max() <= 4 * eps * 1.4
    for vec, k in ((a, 0), (b, 1)):
        assert np.abs(vec - R[:, :, k] * s[:, k:k + 1]).max() <= 8 * eps * 1.4 / 6.0 + 4 * eps * s[:, k].max()
        ln = np.linalg.norm(vec, axis=1)
        big = s[:, k] > 0.004                                          # (a needle's short side is 1e-4 long: its direction is not recoverable to 1e-6)
        assert np.abs(ln / s[:, k] - 1.0)[big].max() <= 1e-4
        assert np.abs(vec / ln[:, None] - R[:, :, k])[big].max() <= 1e-4
    # the identity surfels are exactly axis-aligned: zero extent along their normal; the quarter turns are up to the rounding of sqrt(1/2)
    flat = ((a == 0.0) & (b == 0.0)).any(axis=1)
    lo, hi = br.quad_box(v)
    assert flat.sum() >= 24 and ((hi - lo)[flat].min(axis=1) == 0.0).all()
    assert ((hi - lo).min(axis=1) <= 1e-7).sum() == 32


def test_contributing_box_bounds_the_contributing_region():
    """Brute force in float64: points of the quad sampled on a fine (u, v) grid with alpha >= 1/255 lie inside contributing_box(delta=0), and the
    box is reached (tight) by the sampled points up to the grid spacing."""
    g, v = _scene()
    o = g["opacities"]
    mu, a, b = br.frame(v)
    lo, hi, mask = br.contributing_box(v, o, 0.0)
    assert mask.sum() > 200 and (~mask).sum() >= 8
    n = 601
    uu, vv = np.meshgrid(np.linspace(-3, 3, n), np.linspace(-3, 3, n), indexing="ij")
    h = 6.0 / (n - 1)
    r2, _ = br.radius2(o)
    tight = 0
    for i in np.nonzero(mask)[0][::3]:
        inside = 255.0 * float(o[i]) * np.exp(-0.5 * (uu * uu + vv * vv)) >= 1.0
        assert inside.any()
        p = mu[i] + uu[inside][:, None] * a[i] + vv[inside][:, None] * b[i]
        tol = 1e-12
        assert (p.min(axis=0) >= lo[i] - tol).all() and (p.max(axis=0) <= hi[i] + tol).all()
        if r2[i] <= 9.0:                                               # the disc lies inside the quad: the box is the disc's own, and exact
            slack = 2.0 * h * (np.abs(a[i]) + np.abs(b[i])) + tol
            assert (p.min(axis=0) - lo[i] <= slack).all() and (hi[i] - p.max(axis=0) <= slack).all()
            tight += 1
    assert tight > 30


@pytest.mark.parametrize("delta", [1e-2])
def test_boundary_rays_against_the_oracle_audit(delta):
    g, v = _scene()
    o = g["opacities"]
    test = "bvh_reference.boundary_rays.delta%g" % delta
    for sign, name in ((1.0, "inside"), (-1.0, "outside")):
        ro, rd, tid = br.boundary_rays(v, o, sign * delta, np.random.default_rng(SEED + 1))
        assert 1200 <= len(tid) <= 1536
        a = otr.trace_audit(ro, rd, g["means3D"], g["scales"], g["rotations"], o, start_from_first=False)
        record_fragile(test, "fragile_rays." + name, a["fragile"], FRAGILE_RAYS_MAX)
        listed = (a["ids"] == tid[:, None]) & (np.arange(a["ids"].shape[1])[None] < a["nhit"][:, None])
        ok = ~a["fragile"]
        if sign > 0:
            assert listed.any(axis=1)[ok].all(), "a ray aimed inside the contribution boundary misses its target"
        else:
            assert not listed.any(axis=1)[ok].any(), "a ray aimed outside the contribution boundary hits its target"


def test_oracle_composites_nothing_of_a_surfel_that_cannot_contribute():
    """Rays through the centres of the surfels at or below the threshold, zero, negative and NaN: none of them in any list of the audit, and the
    traced colour is that of the scene without them (a NaN opacity is culled, not clamped to alpha = 0.99)."""
    g, v = _scene()
    o = g["opacities"]
    _, contributes = br.radius2(o)
    dead = np.nonzero(~contributes)[0]
    assert np.isnan(o[dead]).any() and (o[dead] < 0).any() and (o[dead] == 0).any()
    ro, rd, tid = br.centre_rays(v, dead, np.random.default_rng(SEED + 1))
    a = otr.trace_audit(ro, rd, g["means3D"], g["scales"], g["rotations"], o, start_from_first=False)
    listed = np.where(np.arange(a["ids"].shape[1])[None] < a["nhit"][:, None], a["ids"], -1)
    assert not np.isin(listed, dead).any()
    col = np.random.default_rng(SEED + 5).uniform(0.0, 1.0, (256, 3)).astype(np.float32)
    keep = contributes
    full = otr.trace_forward(ro, rd, g["means3D"], g["scales"], g["rotations"], o, colors_precomp=col, start_from_first=False)
    rest = otr.trace_forward(ro, rd, g["means3D"][keep], g["scales"][keep], g["rotations"][keep], o[keep], colors_precomp=col[keep], start_from_first=False)
    assert np.isfinite(full["rgb"]).all() and np.array_equal(full["rgb"], rest["rgb"]) and np.array_equal(full["acc"], rest["acc"])
