"""float64 reference of the opacity-tightened leaf boxes of the acceleration structure (csrc/trace_bvh.hip: quad_box), the seeded scene the BVH tests
share, rays aimed at the boundary of every surfel's contributing region, and a vectorised walk over a read-back tree.  Plain numpy, no GPU: the CPU
test (tests/test_bvh_reference_cpu.py) pins it against the oracle's audit, the GPU test (tests/test_bvh_tightened_gpu.py) holds the builder to it.

A hit contributes when alpha = o exp(-(u^2 + v^2) / 2) >= 1/255 and |u|, |v| <= 3: the contributing region of a surfel is its 3-sigma quad intersected
with the disc u^2 + v^2 <= 2 ln(255 o) of its own plane.  Everything here works from the float32 vertices synth.get_disks returns, taken to float64:
what the builder is given, not the parameters they came from."""
import numpy as np

ALPHA_MIN = float(np.float32(1.0) / np.float32(255.0))      # the compositing threshold as the kernels and the oracle hold it (fp32)
UV_MAX = 3.0
EDGE_OPACITIES = (0.0, 1.0 / 255.0, 0.0039, -0.5, float("nan"), 1e-30, 0.003, 0.00392, 0.0, 0.001)


# ---- the scene ----------------------------------------------------------------------------------------------------------------------------------
def _labels(rng, counts, P):
    """256 labels (0 = ordinary, k = the k-th special kind, counts[k - 1] of them), shuffled, repeated up to P."""
    lab = np.zeros(256, np.int64)
    at = 0
    for k, n in enumerate(counts):
        lab[at:at + n] = k + 1
        at += n
    return np.resize(rng.permutation(lab), P)


def scene(P=256, seed=0):
    """The seeded surfels of the BVH tests, float32 numpy: dict(means3D (P,3), scales (P,2), rotations (P,4), opacities (P,)).  Per 256 surfels:
    30 needles (one scale x 0.02), 24 identity rotations and 8 quarter turns about x (axis-aligned surfels: a box of zero thickness), and of the
    opacities 40 just above 1/255, 28 at the 0.01 reset value, 20 at 0.99, 10 at 1.0 and the ten EDGE_OPACITIES; the mix repeats beyond 256."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1.0, 1.0, (P, 3))
    scales = rng.uniform(0.005, 0.055, (P, 2))
    needle = _labels(rng, [30], P) == 1
    scales[needle, rng.integers(0, 2, P)[needle]] *= 0.02
    q = rng.standard_normal((P, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    kind = _labels(rng, [24, 8], P)
    q[kind == 1] = (1.0, 0.0, 0.0, 0.0)
    q[kind == 2] = (np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.0)
    opac = rng.uniform(0.01, 0.99, P)
    near = (1.0 / 255.0) * (1.0 + 10.0 ** rng.uniform(-2.0, 0.0, P))
    ok = _labels(rng, [40, 28, 20, 10] + [1] * len(EDGE_OPACITIES), P)
    opac[ok == 1] = near[ok == 1]
    opac[ok == 2] = 0.01
    opac[ok == 3] = 0.99
    opac[ok == 4] = 1.0
    for k, val in enumerate(EDGE_OPACITIES):
        opac[ok == 5 + k] = val
    with np.errstate(over="ignore", under="ignore"):
        return dict(means3D=means.astype(np.float32), scales=scales.astype(np.float32), rotations=q.astype(np.float32), opacities=opac.astype(np.float32))


# ---- the reference boxes ------------------------------------------------------------------------------------------------------------------------
def _quads(v):
    return np.asarray(v, np.float64).reshape(-1, 4, 3)


def frame(v):
    """(mu, a, b) of every quad, (P,3) float64 each: the corners are mu -+ 3a +- 3b in the order get_disks writes them."""
    q = _quads(v)
    return 0.5 * (q[:, 0] + q[:, 3]), (q[:, 2] - q[:, 0]) / 6.0, (q[:, 0] - q[:, 1]) / 6.0


def quad_box(v):
    q = _quads(v)
    return q.min(axis=1), q.max(axis=1)


def radius2(o, delta=0.0, thr=1.0 / 255.0):
    """r2 = 2 ln(o / (thr (1 + delta))) per surfel (float64; -inf / nan where the opacity is zero / negative / NaN) and the mask r2 > 0.
    A NaN opacity contributes nowhere: the tracer culls it when it builds the surfel records, the oracle when it sets its surfels up."""
    o = np.asarray(o, np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = 2.0 * np.log(o / (thr * (1.0 + delta)))
    return r2, r2 > 0.0


def contributing_box(v, o, delta=0.0):
    """(lo, hi, mask): per surfel and axis the exact AABB of (quad box) n (box of the disc alpha >= (1 + delta) / 255), and the surfels that have
    such a disc at all (r2 > 0; lo / hi of the others are the centre)."""
    mu, a, b = frame(v)
    qlo, qhi = quad_box(v)
    he, mask = disc_half_extent(v, o, delta)
    return np.maximum(qlo, mu - he), np.minimum(qhi, mu + he), mask


def disc_half_extent(v, o, delta=0.0):
    """(he (P,3), mask): sqrt(r2) sqrt(a_c^2 + b_c^2), the half extent of the disc's box about mu (0 where there is no disc, or no extent along c)."""
    _, a, b = frame(v)
    r2, mask = radius2(o, delta)
    h = np.sqrt(a * a + b * b)
    with np.errstate(invalid="ignore"):
        he = np.where(h > 0.0, np.sqrt(np.where(mask, r2, 0.0))[:, None] * h, 0.0)
    return he, mask


def pad(lo, hi):
    """The builder's documented outward pad of a leaf box, on reference values."""
    return 1e-5 * (np.abs(lo) + np.abs(hi) + (hi - lo)) + 1e-7


# ---- rays at the contribution boundary ----------------------------------------------------------------------------------------------------------
def boundary_targets(v, o, delta):
    """Per contributing surfel and axis c, sign s: the point of the disc alpha = ALPHA_MIN (1 + delta) that is extremal along c -- where the disc
    touches its own AABB, (u, v) = s r (a_c, b_c) / sqrt(a_c^2 + b_c^2) -- pulled back to |u|, |v| <= 3 (1 - delta) where the quad cuts the disc.
    Returns (points (N,3) float64, surfel ids (N,), axes (N,)); an axis along which the surfel has no extent (a_c = b_c = 0) has no such point."""
    mu, a, b = frame(v)
    r2, mask = radius2(o, delta, thr=ALPHA_MIN)
    pts, ids, axes = [], [], []
    for i in np.nonzero(mask)[0]:
        r = np.sqrt(r2[i])
        for c in range(3):
            h = np.hypot(a[i, c], b[i, c])
            if not h > 0.0:
                continue
            for s in (1.0, -1.0):
                uv = s * r * np.array([a[i, c], b[i, c]]) / h
                m = np.abs(uv).max()
                if m > UV_MAX * (1.0 - delta):
                    uv *= UV_MAX * (1.0 - delta) / m
                pts.append(mu[i] + uv[0] * a[i] + uv[1] * b[i]); ids.append(i); axes.append(c)
    return np.array(pts).reshape(-1, 3), np.array(ids, np.int64), np.array(axes, np.int64)


def _rays_through(pts, ids, v, rng):
    _, a, b = frame(v)
    n = np.cross(a[ids], b[ids]); n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = n * rng.choice([-1.0, 1.0], (len(ids), 1)) + 0.7 * rng.standard_normal((len(ids), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    org = pts - d * rng.uniform(2.0, 6.0, (len(ids), 1))
    return org.astype(np.float32), d.astype(np.float32), ids


def centre_rays(v, ids, rng, per_surfel=4):
    """Rays through the CENTRES of the surfels `ids` (directions and origins as boundary_rays'): where a surfel that can never contribute keeps its
    collapsed leaf box, so these are the rays on which its hit test still runs.  Returns (ray_o, ray_d, target surfel id)."""
    mu, _, _ = frame(v)
    ids = np.repeat(np.asarray(ids, np.int64), per_surfel)
    return _rays_through(mu[ids], ids, v, rng)


def boundary_rays(v, o, delta, rng):
    """Rays through boundary_targets: direction = the surfel's normal with a random sign + 0.7 N(0,1) noise, normalised; origin 2 to 6 units back.
    Returns (ray_o (N,3) f32, ray_d (N,3) f32, target surfel id (N,))."""
    pts, ids, _ = boundary_targets(v, o, delta)
    return _rays_through(pts, ids, v, rng)


def axis_rays(v, o, delta, rng):
    """Rays exactly along +-x, +-y, +-z through the boundary targets of the AXIS-ALIGNED surfels (a box of zero thickness along their normal): all six
    directions per target -- along the normal they meet the target, across it they run inside the plane of the flat box.
    Returns (ray_o, ray_d, target id, along (N,) bool: the ray runs along the target's normal)."""
    pts, ids, _ = boundary_targets(v, o, delta)
    _, a, b = frame(v)
    flat = ((a == 0.0) & (b == 0.0)).any(axis=1)
    sel = flat[ids]
    pts, ids = pts[sel], ids[sel]
    n = np.cross(a[ids], b[ids])
    dirs = np.concatenate([np.eye(3), -np.eye(3)])
    P_ = np.repeat(pts, 6, axis=0); I_ = np.repeat(ids, 6); D_ = np.tile(dirs, (len(ids), 1)); N_ = np.repeat(n, 6, axis=0)
    org = P_ - D_ * rng.uniform(2.0, 6.0, (len(I_), 1))
    return org.astype(np.float32), D_.astype(np.float32), I_, (N_ * D_).sum(axis=1) != 0.0


# ---- a read-back tree ---------------------------------------------------------------------------------------------------------------------------
FAR = np.float32(1e30)


def split_tree(flat, P):
    """The node buffer of envgs_bvh_build as (refs (ni,2) int32, boxes (ni, side, lo/hi, xyz) f32, wide (ni,4,8) f32, order (P,) int32)."""
    ni = max(P - 1, 1)
    assert flat.size == 48 * ni + P                                  # binary nodes, wide nodes, sorted leaf order
    nodes = flat[:16 * ni].reshape(ni, 16)
    return (nodes[:, 12:14].copy().view(np.int32), nodes[:, :12].reshape(ni, 2, 2, 3), flat[16 * ni:48 * ni].reshape(ni, 4, 8),
            flat[48 * ni:].copy().view(np.int32))


def topology_words(flat, P):
    """What a refit must carry over unchanged: the four topology words of every binary node and the sorted leaf order."""
    ni = max(P - 1, 1)
    return flat[:16 * ni].reshape(ni, 16)[:, 12:].copy().view(np.int32), flat[48 * ni:].copy().view(np.int32)


def leaf_boxes(flat, P):
    """(lo, hi) (P,3) f32: the stored box of every surfel's leaf, found through the child references (ref < 0 = ~surfel id)."""
    refs, boxes, _, _ = split_tree(flat, P)
    if P == 1:
        return boxes[:1, 0, 0].copy(), boxes[:1, 0, 1].copy()
    m = refs < 0
    sid = ~refs[m]
    lo = np.empty((P, 3), np.float32); hi = np.empty((P, 3), np.float32)
    lo[sid] = boxes[m][:, 0]; hi[sid] = boxes[m][:, 1]
    return lo, hi


def check_tree(flat, P):
    """The structural invariants tests/test_bvh_structure.py asserts node by node, vectorised: the leaf order is a permutation; the binary nodes
    reach every surfel and every node exactly once; an inner child's stored box is bit-equal to the union of the two boxes stored in that child (by
    induction: of all the leaf boxes below it); the 4-wide node of a binary node holds its grandchildren (a leaf child stays), unused slots are
    far points; the wide nodes reach every surfel exactly once too."""
    refs, boxes, w8, order = split_tree(flat, P)
    ni = refs.shape[0]
    assert np.array_equal(np.sort(order), np.arange(P))
    assert not np.isnan(boxes).any()
    used2 = np.ones((ni, 2), bool)
    if P == 1:
        used2[0, 1] = False                                          # the single-surfel tree: the right child is an unreachable far point
        assert (boxes[0, 1] == FAR).all()
    # binary reach counts, level by level
    seen_leaf = np.zeros(P, np.int64); seen_node = np.zeros(ni, np.int64)
    front = np.array([0], np.int64)
    depth = 0
    while front.size:
        np.add.at(seen_node, front, 1)
        r = refs[front][used2[front]]
        assert (r >= -P).all() and (r < ni).all()
        np.add.at(seen_leaf, ~r[r < 0], 1)
        front = r[r >= 0].astype(np.int64)
        depth += 1
        assert depth <= P + 1
    assert (seen_leaf == 1).all() and (seen_node == 1).all()
    # inner boxes: exactly the union of what is stored below
    i, s = np.nonzero((refs >= 0) & used2)
    c = refs[i, s]
    assert np.array_equal(boxes[i, s, 0], np.minimum(boxes[c, 0, 0], boxes[c, 1, 0]))
    assert np.array_equal(boxes[i, s, 1], np.maximum(boxes[c, 0, 1], boxes[c, 1, 1]))
    # wide nodes: per slot [lo.x hi.x lo.y hi.y lo.z hi.z ref 0]
    wl = w8[:, :, 0:6:2]; wh = w8[:, :, 1:6:2]                        # (node, slot, axis)
    wr = np.ascontiguousarray(w8[:, :, 6]).view(np.int32)
    assert (w8[:, :, 7] == 0).all()
    e_lo = np.full((ni, 4, 3), FAR, np.float32); e_hi = np.full((ni, 4, 3), FAR, np.float32)
    e_ref = np.zeros((ni, 4), np.int32); e_on = np.zeros((ni, 4), bool)
    at = np.zeros(ni, np.int64)
    all_i = np.arange(ni)
    for side in range(2):
        leaf = refs[:, side] < 0
        j = all_i[leaf]
        e_lo[j, at[j]] = boxes[j, side, 0]; e_hi[j, at[j]] = boxes[j, side, 1]; e_ref[j, at[j]] = refs[j, side]; e_on[j, at[j]] = True
        j = all_i[~leaf]
        cj = refs[j, side]
        for s2 in range(2):
            e_lo[j, at[j] + s2] = boxes[cj, s2, 0]; e_hi[j, at[j] + s2] = boxes[cj, s2, 1]; e_ref[j, at[j] + s2] = refs[cj, s2]; e_on[j, at[j] + s2] = True
        at += np.where(leaf, 1, 2)
    assert np.array_equal(wl, e_lo) and np.array_equal(wh, e_hi)
    assert np.array_equal(wr[e_on], e_ref[e_on])
    used4 = ~((wl[:, :, 0] == FAR) & (wh[:, :, 0] == FAR))
    seen = np.zeros(P, np.int64)
    front = np.array([0], np.int64)
    depth = 0
    while front.size:
        r = wr[front][used4[front]]
        np.add.at(seen, ~r[r < 0], 1)
        front = r[r >= 0].astype(np.int64)
        depth += 1
        assert depth <= P + 1
    assert (seen == 1).all()
