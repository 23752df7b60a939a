"""NumPy float64 twin of the depth fusion (include/envgs_mesh.h, "depth fusion"; csrc/mesh_fuse.hip), with the AUDIT of its decisions.

Semantics, in this project's words.  All views share one size; the centre of pixel (x, y) is (x + 0.5, y + 0.5).  A reference pixel of depth d is
carried into a source image by one affine map, p = d (A (xc, yc, 1)) + b with A = K_s R_s R_r^T K_r^-1 and b = K_s (T_s - R_s R_r^T T_r); there the
source depth is sampled bilinearly under the border clip (torch's grid_sample defaults), and the sampled point is carried back by the map with the
roles exchanged.  The pair passes iff the pixel returns within geo_abs_thresh, the returned depth z is within geo_rel_thresh of d relative to d, and
the sample is positive; a reference depth that is not finite or not positive passes nothing.  depth_avg = (sum of the passing z + d) / (count + 1);
geo = count >= min_count; photo = d > pho_abs_thresh; final = both.  The kept pixels, in (view, row, column) order, are back-projected by
c_v + depth_avg (R_v^T K_v^-1 (xc, yc, 1)).

Audit.  The device rounds in fp32 in its own sequence, so a comparison whose two sides are closer than the rounding can go either way.  With `band`
the measured relative rounding ("Depth fusion"), a (pixel, source) pair is FRAGILE when a comparison it needs is inside the band while
the other comparisons pass:
  dist:      |dist - geo_abs_thresh| <= band max(dist, geo_abs_thresh)       the error of dist is that of a pixel coordinate: absolute at that scale
  relative:  |rel - geo_rel_thresh| <= band (|z| / d + rel)                  the error of rel = |z - d| / d is that of z, divided by d
  sample:    |sampled| <= band max(|ix|, |iy|, 1) max |tap|                  a bilinear weight is a difference of pixel coordinates; the sampled
             value is continuous across cell boundaries and under the clip, so which taps are chosen is no decision, only the sign of the sum is
A pixel is fragile if one of its pairs is (its count and its average depend on the pair).  Its geo / final bit is fragile only if flipping its
fragile pairs can cross min_count."""
import math
from types import SimpleNamespace

import numpy as np


def min_count(geo_sum_thresh, S):
    """The smallest integer n with n >= geo_sum_thresh * S, the product in Python float arithmetic."""
    need = float(geo_sum_thresh) * S
    n = 0
    while n < need:
        n += 1
    return n


def pair_maps(K, R, T, r, s):
    """(fwd, back): 12 float64 each, A row major then b."""
    def one(a, b):
        Rab = R[b] @ R[a].T
        return np.concatenate([(K[b] @ Rab @ np.linalg.inv(K[a])).reshape(-1), K[b] @ (T[b] - Rab @ T[a])])
    return one(r, s), one(s, r)


def view_maps(K, R, T):
    return np.stack([np.concatenate([(R[v].T @ np.linalg.inv(K[v])).reshape(-1), -R[v].T @ T[v]]) for v in range(len(K))])


def pixel_centres(H, W):
    yc, xc = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    return xc, yc


def bilinear_border(src, u, v):
    """grid_sample(bilinear, border, align_corners=False) of src (H,W) at pixel coordinates (u, v), both finite.
    -> (sampled, scale = max(|ix|, |iy|, 1), the largest |tap| among the finite taps inside the image)."""
    H, W = src.shape
    ix, iy = np.clip(u - 0.5, 0, W - 1), np.clip(v - 0.5, 0, H - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = (x0 + 1) - ix, (y0 + 1) - iy
    s = np.zeros_like(ix)
    big = np.zeros_like(ix)
    for yy, xx, w in ((y0, x0, wx0 * wy0), (y0, x0 + 1, wx1 * wy0), (y0 + 1, x0, wx0 * wy1), (y0 + 1, x0 + 1, wx1 * wy1)):
        inside = (xx < W) & (yy < H)
        tap = src[np.minimum(yy, H - 1), np.minimum(xx, W - 1)]
        s = s + np.where(inside, tap * w, 0.0)
        big = np.maximum(big, np.where(inside & np.isfinite(tap), np.abs(tap), 0.0))
    return s, np.maximum(np.maximum(np.abs(ix), np.abs(iy)), 1.0), big


def pair(dref, dsrc, fwd, back, geo_abs_thresh, geo_rel_thresh, band):
    """One (reference, source) pair over the whole reference map -> namespace of (H,W) arrays: passed, fragile, z (depth_reprojected, unmasked),
    dist, rel, sampled, u, v."""
    H, W = dref.shape
    xc, yc = pixel_centres(H, W)
    pix = np.stack([xc, yc, np.ones_like(xc)], axis=-1)
    A, b, B, bb = fwd[:9].reshape(3, 3), fwd[9:], back[:9].reshape(3, 3), back[9:]
    with np.errstate(all="ignore"):
        ref_ok = np.isfinite(dref) & (dref > 0)
        p = dref[..., None] * (pix @ A.T) + b
        u, v = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
        uv_ok = ref_ok & np.isfinite(u) & np.isfinite(v)
        us, vs = np.where(uv_ok, u, 0.0), np.where(uv_ok, v, 0.0)
        sampled, scale, big = bilinear_border(dsrc, us, vs)
        q = sampled[..., None] * (np.stack([us, vs, np.ones_like(us)], axis=-1) @ B.T) + bb
        z = q[..., 2]
        dist = np.sqrt((q[..., 0] / z - xc) ** 2 + (q[..., 1] / z - yc) ** 2)
        rel = np.abs(z - dref) / dref
        s_fin = uv_ok & np.isfinite(sampled)
        c1, c2, c3 = dist < geo_abs_thresh, rel < geo_rel_thresh, sampled > 0
        passed = s_fin & c1 & c2 & c3
        f1 = np.abs(dist - geo_abs_thresh) <= band * np.maximum(dist, geo_abs_thresh)
        f2 = np.abs(rel - geo_rel_thresh) <= band * (np.abs(z) / dref + rel)
        f3 = (np.abs(sampled) <= band * scale * big) & (big > 0)
        fragile = s_fin & (f1 | f2 | f3) & (c1 | f1) & (c2 | f2) & (c3 | f3)
    return SimpleNamespace(passed=passed, fragile=fragile, z=z, dist=dist, rel=rel, sampled=sampled, u=u, v=v)


def consistency(depth, K, R, T, sources, geo_abs_thresh=1.0, geo_rel_thresh=0.01, geo_sum_thresh=0.75, pho_abs_thresh=0.0, band=0.0):
    """depth (V,H,W); K, R (V,3,3), T (V,3); sources (V,S) -> namespace: pair_mask, pair_fragile, z, dist (V,S,H,W); count, total, depth_avg,
    photo_mask, geo_mask, final_mask, fragile (pixel), fragile_geo, fragile_final (V,H,W); min_count."""
    depth = np.asarray(depth, np.float64)
    K, R, T = (np.asarray(a, np.float64) for a in (K, R, T))
    sources = np.asarray(sources, np.int64).reshape(depth.shape[0], -1)
    V, H, W = depth.shape
    S = sources.shape[1]
    shape = (V, S, H, W)
    pm, pf, zz, dd = np.zeros(shape, bool), np.zeros(shape, bool), np.zeros(shape), np.zeros(shape)
    total = np.zeros((V, H, W))
    for r in range(V):
        for k in range(S):
            s = int(sources[r, k])
            fwd, back = pair_maps(K, R, T, r, s)
            o = pair(depth[r], depth[s], fwd, back, geo_abs_thresh, geo_rel_thresh, band)
            pm[r, k], pf[r, k], zz[r, k], dd[r, k] = o.passed, o.fragile, o.z, o.dist
            total[r] = total[r] + np.where(o.passed, o.z, 0.0)                  # source order
    count = pm.sum(1)
    n_min = min_count(geo_sum_thresh, S)
    with np.errstate(all="ignore"):
        depth_avg = (total + depth) / (count + 1)
        photo = depth > pho_abs_thresh
    geo = count >= n_min
    sure, loose = (pm & ~pf).sum(1), pf.sum(1)
    fragile_geo = (sure < n_min) & (n_min <= sure + loose)
    return SimpleNamespace(pair_mask=pm, pair_fragile=pf, z=zz, dist=dd, count=count, total=total, depth_avg=depth_avg, photo_mask=photo, geo_mask=geo,
                           final_mask=geo & photo, fragile=pf.any(1), fragile_geo=fragile_geo, fragile_final=fragile_geo & photo, min_count=n_min)


def points(depth_avg, K, R, T, index, band):
    """The back-projection of the pixels `index` (flat (view H + row) W + column) -> (points (N,3), bound (N,3)): the fp32 bound of the header's
    rule 5, 8 * 2^-24 (|c_k| + d sum_j |A_kj pix_j|) + (band d) |A_k pix|: eight roundings on the sum of magnitudes plus the depth's own band."""
    V, H, W = depth_avg.shape
    M = view_maps(np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(T, np.float64))
    index = np.asarray(index, np.int64)
    v, r = index // (H * W), index % (H * W)
    pix = np.stack([(r % W) + 0.5, (r // W) + 0.5, np.ones(len(index))], axis=-1)
    A, c = M[v, :9].reshape(-1, 3, 3), M[v, 9:]
    d = np.asarray(depth_avg, np.float64).reshape(-1)[index][:, None]
    ray = np.einsum("nkj,nj->nk", A, pix)
    mag = np.einsum("nkj,nj->nk", np.abs(A), np.abs(pix))
    return c + d * ray, 8 * 2.0 ** -24 * (np.abs(c) + np.abs(d) * mag) + band * np.abs(d) * np.abs(ray)


def check(got, want, band, what, depth_avg_ref=None):
    """`got` (depth_avg, count, geo_mask, final_mask, photo_mask as arrays) against the audited oracle `want`: the count and the masks exactly off
    the audited set, depth_avg within band relative off the fragile pixels (against depth_avg_ref when given -- the reference's recorded values --
    else the oracle's).  -> the figures, printed before anything is asserted."""
    keep = ~want.fragile
    ref = want.depth_avg if depth_avg_ref is None else np.asarray(depth_avg_ref, np.float64)
    a = np.asarray(got.depth_avg, np.float64)
    both_nan = np.isnan(a) & np.isnan(ref)
    with np.errstate(all="ignore"):
        err = np.where(both_nan | (a == ref), 0.0, np.abs(a - ref) / np.abs(ref))
    err = np.where(np.isnan(err), np.inf, err)
    fig = SimpleNamespace(share=float(want.fragile.mean()), fragile=int(want.fragile.sum()), pixels=want.fragile.size,
                          depth_err=float(err[keep].max()) if keep.any() else 0.0,
                          count_bad=int((np.asarray(got.count)[keep] != want.count[keep]).sum()),
                          geo_bad=int((np.asarray(got.geo_mask) != want.geo_mask)[~want.fragile_geo].sum()),
                          final_bad=int((np.asarray(got.final_mask) != want.final_mask)[~want.fragile_final].sum()),
                          photo_bad=int((np.asarray(got.photo_mask) != want.photo_mask).sum()))
    print("%s: fragile %d of %d pixels (%.3f %%), depth_avg error %.3g (band %.3g), count %d geo %d final %d photo %d mismatches off the audited set"
          % (what, fig.fragile, fig.pixels, 100 * fig.share, fig.depth_err, band, fig.count_bad, fig.geo_bad, fig.final_bad, fig.photo_bad))
    assert fig.share <= 0.01, "%s: %.3f %% of the pixels are fragile, above 1 %%" % (what, 100 * fig.share)
    assert fig.count_bad == 0 and fig.geo_bad == 0 and fig.final_bad == 0 and fig.photo_bad == 0, "%s: decisions differ off the audited set" % what
    assert fig.depth_err <= band, "%s: depth_avg differs by %.3g relative, measured band %.3g" % (what, fig.depth_err, band)
    return fig
