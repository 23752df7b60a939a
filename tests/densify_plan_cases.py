"""Inputs for the tests of the one-pass densification plan (`SurfelSet.grow_and_prune`; include/envgs_densify.h, `envgs_densify_plan`), built on the
CPU with NumPy / torch only, and a NumPy float32 restatement of the plan written from the header.

  * `plan_reference`      class bits, the six flag arrays [A|B|D|E|S1|S2], their scan and the counters, from the statistics and ACTIVATED values;
  * `threshold_case`      P = 320 rows that sit exactly on, one step below and one step above each of the plan's six comparisons;
  * `mixed_state`         a random state for any P and any parameter layout; `uniform_state` / `one_of_each`: empty segments of the scan;
  * `flag_state`, `weight_state`, `special_rows`, `oversize_case`: the rest.

A `before` state has the layout of tests/golden/densify_golden.pt: {"params", "stats", "m", "v"}, CPU tensors.
Statistics are free inputs, so rows are put on a gradient / radius threshold by choosing the statistics.  Scale and opacity thresholds go the other
way: the threshold is the activated value of one chosen row as the device computes it (`data_thresholds`), and the neighbours are raw values a few
steps of the raw float apart, so equality never depends on the bits of some `exp` or `sigmoid`.
"""
import math

import numpy as np
import torch

F = np.float32
NAMES8 = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_specular", "_roughness")
NAMES6 = NAMES8[:6]                                                    # the environment set: no _specular, no _roughness
CLS_CLONE, CLS_SPLIT, CLS_PRUNE_1, CLS_PRUNE_S = 1, 2, 4, 8          # ENVGS_GROW_CLS_*: the bits of envgs_densify_plan's `cls`
FLAG_MIN_OPACITY, FLAG_MIN_GRADIENT, FLAG_SPLIT_SCREEN = 1, 2, 4      # ENVGS_PLAN_*

MIXED_ARGS = dict(min_opacity=0.05, min_gradient=0.15, grad_threshold=0.1, size_threshold=0.03, split_screen_threshold=20.0)
# grad_threshold above min_gradient: a surfel can be "not high" and still survive the gradient prune (needed for "nothing selected")
UNIFORM_ARGS = dict(min_opacity=0.05, min_gradient=0.15, grad_threshold=0.2, size_threshold=0.03, split_screen_threshold=20.0)


# ---- floats ----------------------------------------------------------------------------------------------------------------------------------
def ulp_step(x, k):
    """The float32 `k` representable values above (k < 0: below) the finite non-zero float32 `x`, without crossing zero."""
    i = int(np.array(x, F).view(np.int32))
    j = i + k if i >= 0 else i - k                                     # (negative floats: the larger the word, the smaller the value)
    assert (i >= 0) == (j >= 0) and j != 0 and j != -2 ** 31
    return np.array(j, np.int32).view(F)[()]


def float_of_key(k):
    """`float_of_key` of envgs_amd/csrc/float_key.h: the float whose ordered uint32 key is `k`."""
    k = int(k) & 0xFFFFFFFF
    b = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return np.array(b, np.uint32).view(F)[()]


def stat_avg(x, dn):
    """IEEE float32 division, NaN -> 0 (`get_xyz_gradient_avg`)."""
    with np.errstate(all="ignore"):
        q = np.asarray(x, F) / np.asarray(dn, F)
    q = np.array(q, F, ndmin=1)
    q[np.isnan(q)] = 0.0
    return q


def split_r(N, ratio=0.8):
    return 1.0 / (ratio * N)


def scaled_avg(ga, dn, r):
    """fl(fl(ga * r) / dn): what the gradient prune sees of a split child."""
    with np.errstate(all="ignore"):
        return stat_avg(np.asarray(ga, F) * F(r), dn)


# ---- the plan, restated ------------------------------------------------------------------------------------------------------------------------
def plan_reference(ga, dn, mr, wa, scal, opac, thr, N, ratio=0.8):
    """include/envgs_densify.h in NumPy float32.  thr: grad_threshold, size_limit (= size_threshold * spatial_scale), and split_screen_threshold /
    min_opacity / min_gradient or None (flag off).  scal (P,2), opac (P): activated values."""
    ga, dn, mr, wa, opac = (np.asarray(t, F).reshape(-1) for t in (ga, dn, mr, wa, opac))
    scal = np.asarray(scal, F).reshape(-1, 2)
    P = ga.shape[0]
    r = F(split_r(N, ratio))
    a1, a_s = stat_avg(ga, dn), scaled_avg(ga, dn, r)
    high = a1 >= F(thr["grad_threshold"])
    small = np.maximum(scal[:, 0], scal[:, 1]) <= F(thr["size_limit"])
    clone = small & high
    big = ~small
    if thr.get("split_screen_threshold") is not None:
        big = big | (mr > F(thr["split_screen_threshold"]))
    split = high & big
    occ = opac < F(thr["min_opacity"]) if thr.get("min_opacity") is not None else np.zeros(P, bool)
    pr_1, pr_s = occ.copy(), occ.copy()
    if thr.get("min_gradient") is not None:
        pr_1 |= (a1 <= F(thr["min_gradient"])) & (dn != 0)
        pr_s |= (a_s <= F(thr["min_gradient"])) & (dn != 0)
    cls = (clone * CLS_CLONE + split * CLS_SPLIT + pr_1 * CLS_PRUNE_1 + pr_s * CLS_PRUNE_S).astype(np.uint8)
    flags = np.stack([~split & ~pr_1, clone & ~split & ~pr_1, split & ~pr_s, clone & split & ~pr_s, split, clone & split]).astype(np.uint32)
    scan = np.cumsum(flags.reshape(-1), dtype=np.uint64).astype(np.uint32)
    nA, nB, nD, nE, nS1, nS2 = (int(v) for v in flags.sum(axis=1))
    n_clone, nS = int(clone.sum()), nS1 + nS2
    total = nA + nB + N * (nD + nE)
    return dict(cls=cls, flags=flags, scan=scan, counters=[nA, nB, nD, nE, nS1, nS2, n_clone], clone=clone, split=split, pr_1=pr_1, pr_s=pr_s,
                high=high, small=small, total=total, w_all=wa.max() if P else None, w_clone_max=wa[clone].max() if n_clone else None,
                w_clone_min=wa[clone].min() if n_clone else None,
                log=[("clone", n_clone), ("split", nS), ("prune_occ_grad", P + n_clone + (N - 1) * nS - total)])


def plan_flags(thr):
    return ((FLAG_MIN_OPACITY if thr.get("min_opacity") is not None else 0) | (FLAG_MIN_GRADIENT if thr.get("min_gradient") is not None else 0)
            | (FLAG_SPLIT_SCREEN if thr.get("split_screen_threshold") is not None else 0))


def activated(before, dev="cpu"):
    """exp / sigmoid of the raw scales / opacities as `dev` computes them: (scal (P,2), opac (P)) float32 NumPy."""
    scal = torch.exp(before["params"]["_scaling"].to(dev))
    opac = torch.sigmoid(before["params"]["_opacity"].to(dev))[:, 0]
    return scal.cpu().numpy(), opac.cpu().numpy()


def plan_of(before, cfg, args, N=2, ratio=0.8, dev="cpu"):
    """`plan_reference` of a `before` state under grow_and_prune's arguments, activations from `dev`."""
    scal, opac = activated(before, dev)
    st = before["stats"]
    thr = dict(args, size_limit=float(F(args["size_threshold"] * cfg.get("spatial_scale", 1.0))))
    return plan_reference(st["xyz_gradient_accum"].numpy(), st["denom"].numpy(), st["max_radii2D"].numpy(), st["xyz_weight_accum"].numpy(), scal, opac,
                          thr, N, ratio)


# ---- states ------------------------------------------------------------------------------------------------------------------------------------
def _param_shapes(P, names, rest):
    shapes = {"_xyz": (P, 3), "_features_dc": (P, 1, 3), "_features_rest": (P,) + tuple(rest), "_scaling": (P, 2), "_rotation": (P, 4), "_opacity": (P, 1),
              "_specular": (P, 1), "_roughness": (P, 1)}
    return {k: shapes[k] for k in names}


def state_from_rows(scaling_raw, opacity_raw, ga, dn, mr, wa, seed=0, names=NAMES8, rest=(3, 3)):
    """A `before` state whose decisive columns are given (NumPy float32) and whose other parameters and Adam moments are seeded noise."""
    P = len(ga)
    g = torch.Generator().manual_seed(seed)
    params = {}
    for k, shape in _param_shapes(P, names, rest).items():
        params[k] = torch.rand(*shape, generator=g) * 2 - 1 if k == "_xyz" else torch.randn(*shape, generator=g)
    params["_scaling"] = torch.from_numpy(np.array(scaling_raw, F).reshape(P, 2))
    params["_opacity"] = torch.from_numpy(np.array(opacity_raw, F).reshape(P, 1))
    col = lambda x: torch.from_numpy(np.array(x, F).reshape(P, 1))
    stats = {"xyz_gradient_accum": col(ga), "denom": col(dn), "max_radii2D": torch.from_numpy(np.array(mr, F).reshape(P)), "xyz_weight_accum": col(wa)}
    return {"params": params, "stats": stats, "m": {k: torch.randn(*v.shape, generator=g) * 0.1 for k, v in params.items()},
            "v": {k: torch.rand(*v.shape, generator=g) * 0.01 for k, v in params.items()}}


def mixed_state(P, seed=11, names=NAMES8, rest=(3, 3)):
    """Every class at random (for MIXED_ARGS): scales on both sides of 0.03, denominators 0 .. 4 with 0 / 0 and x / 0 averages, radii on both sides
    of 20, opacities on both sides of 0.05, weights >= 0."""
    rng = np.random.default_rng(seed)
    dn = rng.integers(0, 5, P).astype(F)
    ga = (rng.random(P).astype(F) * F(0.5) * dn).astype(F)
    inf = (np.arange(P) % 7 == 3) & (dn == 0)
    ga[inf] = rng.random(P).astype(F)[inf] + F(0.01)                  # x / 0 = inf
    return state_from_rows(np.log(rng.random((P, 2)).astype(F) * F(0.095) + F(0.005)), rng.standard_normal(P).astype(F) * 2, ga, dn,
                           rng.random(P).astype(F) * 50, rng.random(P).astype(F) * 3 * dn, seed, names, rest)


SMALL, LARGE = F(math.log(0.01)), F(math.log(0.06))                   # raw scales far from a limit of 0.03
OPAQUE, FAINT = F(2.0), F(-5.0)                                        # raw opacities far from 0.05
UNIFORM_KINDS = ("all_clone", "all_split", "all_clone_split", "all_pruned", "prune_only", "nothing")


def _class_row(kind, i=0):
    """(ga, dn, mr, raw scale, raw opacity) of one row of a class under UNIFORM_ARGS; `i` varies the values without moving a decision."""
    e = F(i % 5) * F(0.01)
    rows = {"plain": (F(0.17), 1, 3.0, SMALL, OPAQUE),                            # not high, survives: A
            "clone": (F(0.5) + e, 1, 3.0, SMALL, OPAQUE),                         # A + B
            "split": (F(0.6) + e, 1, 3.0, LARGE, OPAQUE),                         # D
            "clone_split": (F(0.7) + e, 1, 30.0, SMALL, OPAQUE),                  # D + E
            "pruned": (F(0.17), 1, 3.0, LARGE, FAINT),                            # not high, low opacity
            "clone_pruned": (F(0.5) + e, 1, 3.0, SMALL, FAINT),                   # cloned, then both pruned
            "split_pruned": (F(0.22), 1, 3.0, LARGE, OPAQUE),                     # avg 0.22 >= 0.2: split; children 0.1375 (N = 2) <= 0.15: pruned
            "clone_split_pruned": (F(0.7) + e, 1, 30.0, SMALL, FAINT)}
    ga, dn, mr, s, o = rows[kind]
    return ga, F(dn), F(mr), s, o


def _rows_state(kinds, seed, names=NAMES8, rest=(3, 3)):
    cols = list(zip(*[_class_row(k, i) for i, k in enumerate(kinds)]))
    ga, dn, mr, s, o = (np.array(c, F) for c in cols)
    P = len(kinds)
    rng = np.random.default_rng(seed)
    scal = np.stack([s, s + F(-0.5) * rng.random(P).astype(F)], axis=1)           # the second column is never the maximum's rival
    flip = rng.random(P) < 0.5
    scal[flip] = scal[flip][:, ::-1]
    return state_from_rows(scal, o, ga, dn, mr, rng.random(P).astype(F) * 3 + F(0.1), seed, names, rest)


def uniform_state(P, kind, seed=5):
    """Every row of one fate (UNIFORM_ARGS)."""
    if kind == "all_pruned":
        kinds = [("clone_pruned", "pruned", "clone_split_pruned", "split_pruned")[i % 4] for i in range(P)]
    elif kind == "prune_only":
        kinds = [("pruned", "plain")[i % 2] for i in range(P)]
    else:
        kinds = [{"all_clone": "clone", "all_split": "split", "all_clone_split": "clone_split", "nothing": "plain"}[kind]] * P
    return _rows_state(kinds, seed)


ONE_OF_EACH = ("clone", "split", "clone_split", "pruned", "clone_pruned", "split_pruned", "clone_split_pruned")


def one_of_each(P, edge_kind, at_end, seed=9):
    """One row of each class of ONE_OF_EACH among plain rows; the row of `edge_kind` at index 0 (or P - 1 with at_end), the others inside."""
    assert P >= 4 * len(ONE_OF_EACH)
    kinds = ["plain"] * P
    inner = [k for k in ONE_OF_EACH if k != edge_kind]
    for j, k in enumerate(inner):
        kinds[1 + (j + 1) * (P - 2) // (len(inner) + 1)] = k
    kinds[P - 1 if at_end else 0] = edge_kind
    assert all(kinds.count(k) == 1 for k in ONE_OF_EACH)
    return _rows_state(kinds, seed)


# ---- rows on every threshold -------------------------------------------------------------------------------------------------------------------
T_GRAD = F(F(0.6) / F(3.0))                                            # fl(0.6f / 3): reachable with denominators 1, 2 and 3
T_MING = F(0.15)
T_SCREEN = F(20.0)
RAW_SIZE, RAW_OPAC = F(math.log(0.03)), F(math.log(0.05 / 0.95))      # the rows whose activated values become the size / opacity thresholds
NEIGHBOURS = (-60, -2, -1, 0, 1, 2, 60)                                # steps of the raw float around them


def hits(fn, centre, target, window=64):
    """The float32 values within `window` steps of `centre` where fn(x) == target, ascending."""
    out = []
    for k in range(-window, window + 1):
        x = ulp_step(centre, k)
        if fn(x) == F(target):
            out.append(x)
    return out


def around(fn, centre, target, window=64):
    """(below, at, above): the largest x with fn(x) < target, one x with fn(x) == target, the smallest x with fn(x) > target (fn nondecreasing)."""
    h = hits(fn, centre, target, window)
    assert h, "no float near %r reaches %r" % (centre, target)
    lo, hi = ulp_step(h[0], -1), ulp_step(h[-1], 1)
    assert fn(lo) < F(target) < fn(hi)
    return lo, h[len(h) // 2], hi


def quotient_rows(target, dn):
    return around(lambda x: stat_avg(x, F(dn))[0], F(F(target) * F(dn)), target)


def scaled_rows(target, dn, N, ratio=0.8):
    r = F(split_r(N, ratio))
    return around(lambda x: scaled_avg(x, F(dn), r)[0], F(float(target) * dn / float(r)), target)


def threshold_case(P=320, seed=3):
    """-> (before, tags, picks).  tags: {name: row indices}; picks: the rows whose activated scale / opacity become the thresholds.
    Arguments: grad_threshold T_GRAD, min_gradient T_MING, split_screen_threshold T_SCREEN, size_threshold and min_opacity from `data_thresholds`."""
    rows, tags = [], {}

    def add(tag, ga, dn, mr, s0, s1, op):
        tags.setdefault(tag, []).append(len(rows))
        rows.append((F(ga), F(dn), F(mr), F(s0), F(s1), F(op)))

    for dn in (1, 2, 3):
        for ga in quotient_rows(T_GRAD, dn):
            add("grad_small", ga, dn, 0.0, SMALL, SMALL - F(1), OPAQUE)                   # clone (and keep: avg > T_MING) or nothing
            add("grad_large", ga, dn, 0.0, LARGE - F(1), LARGE, OPAQUE)                   # split (children pruned by gradient) or keep the original
        for ga in quotient_rows(T_MING, dn):
            add("mingrad_1", ga, dn, 0.0, SMALL if dn % 2 else LARGE, SMALL, OPAQUE)      # not high: never split; kept or pruned
    for j in NEIGHBOURS:
        s = ulp_step(RAW_SIZE, j) if j else RAW_SIZE
        add("size_c0", 0.5, 1, 0.0, s, SMALL, OPAQUE)                                     # high: clone (<=) or split (>)
        add("size_c1", 0.5, 1, 0.0, SMALL, s, OPAQUE)
        o = ulp_step(RAW_OPAC, j) if j else RAW_OPAC
        add("opac_1", 0.17, 1, 0.0, SMALL, SMALL, o)                                      # neither high nor pruned by gradient: opacity decides
        add("opac_s", 0.5, 1, 0.0, LARGE, SMALL, o)                                       # split: the children go or stay by opacity
    for mr in (ulp_step(T_SCREEN, -1), T_SCREEN, ulp_step(T_SCREEN, 1)):
        for ga in (0.5, 0.75):
            add("screen", ga, 1, mr, SMALL, SMALL - F(1), OPAQUE)                         # clone only, or clone and both split
    for N in (2, 3):
        for dn in (1, 2, 3, 4):
            try:
                trio = scaled_rows(T_MING, dn, N)
            except AssertionError:
                continue                                                                  # (no hit with this denominator: the CPU test counts the hits)
            for ga in trio:
                add("mingrad_s%d" % N, ga, dn, 0.0, LARGE, SMALL, OPAQUE)                 # split; children pruned or not (D)
                add("mingrad_s%d" % N, ga, dn, 30.0, SMALL, SMALL, OPAQUE)                # cloned and both split (D and E)
    add("dn0", 0.0, 0, 0.0, SMALL, SMALL, OPAQUE)                                         # 0 / 0 = 0 <= min_gradient, but never counted: stays
    add("dn0", 0.0, 0, 0.0, LARGE, SMALL, OPAQUE)
    add("dn0", 0.3, 0, 0.0, LARGE, SMALL, OPAQUE)                                         # x / 0 = inf: high, split, not pruned
    add("dn0", 0.3, 0, 0.0, SMALL, SMALL, OPAQUE)
    assert len(rows) <= P
    rng = np.random.default_rng(seed)
    n_fill = P - len(rows)
    dn = rng.integers(0, 5, n_fill).astype(F)
    fill = np.stack([rng.random(n_fill).astype(F) * F(0.6) * dn, dn, rng.random(n_fill).astype(F) * 50,
                     np.log(rng.random(n_fill).astype(F) * F(0.04) + F(0.035)), np.log(rng.random(n_fill).astype(F) * F(0.02) + F(0.005)),
                     rng.standard_normal(n_fill).astype(F) * 2 + F(1.0)], axis=1)         # (raw scales and opacities off the two data thresholds)
    fill[:, 3][rng.random(n_fill) < 0.5] = SMALL
    table = np.concatenate([np.array(rows, F).reshape(-1, 6), fill.astype(F)])
    perm = rng.permutation(P)                                                             # table row i goes to index place[i]
    place = np.empty(P, np.int64)
    place[perm] = np.arange(P)
    table = table[perm]
    tags = {k: np.sort(place[np.array(v)]) for k, v in tags.items()}
    picks = dict(size=int(place[rows.index(next(r for r in rows if r[3] == RAW_SIZE))]), opac=int(place[next(i for i, r in enumerate(rows) if r[5] == RAW_OPAC)]))
    before = state_from_rows(table[:, 3:5], table[:, 5], table[:, 0], table[:, 1], table[:, 2], rng.random(P).astype(F) * 3 * np.maximum(table[:, 1], 1), seed)
    return before, tags, picks


def data_thresholds(before, picks, spatial_scale=1.0, dev="cpu"):
    """grow_and_prune's arguments for `threshold_case`: the size and opacity thresholds are the picked rows' activated values on `dev`.
    spatial_scale must be a power of two: size_threshold * spatial_scale is then that value again, exactly."""
    assert math.frexp(spatial_scale)[0] == 0.5
    scal, opac = activated(before, dev)
    return dict(min_opacity=float(opac[picks["opac"]]), min_gradient=float(T_MING), grad_threshold=float(T_GRAD),
                size_threshold=float(scal[picks["size"]].max()) / spatial_scale, split_screen_threshold=float(T_SCREEN))


def _sides(values, t):
    values = np.asarray(values, F)
    return int((values < F(t)).sum()), int((values == F(t)).sum()), int((values > F(t)).sum())


def threshold_witness(before, tags, args, cfg, N, scal, opac):
    """{comparison: (rows below, rows equal, rows above)} over the tagged rows, from the activated values given.  A zero anywhere: vacuous."""
    st = {k: v.numpy().reshape(-1) for k, v in before["stats"].items()}
    ga, dn, mr = st["xyz_gradient_accum"], st["denom"], st["max_radii2D"]
    limit = F(args["size_threshold"] * cfg.get("spatial_scale", 1.0))
    r = F(split_r(N))
    out = {}
    for tag in ("grad_small", "grad_large"):
        out[tag] = _sides(stat_avg(ga[tags[tag]], dn[tags[tag]]), args["grad_threshold"])
    for tag, col in (("size_c0", 0), ("size_c1", 1)):
        i = tags[tag]
        assert bool((scal[i].argmax(axis=1) == col).all())                                # the maximum sits in the column the tag names
        out[tag] = _sides(scal[i].max(axis=1), limit)
    out["screen"] = _sides(mr[tags["screen"]], args["split_screen_threshold"])
    for tag in ("opac_1", "opac_s"):
        out[tag] = _sides(opac[tags[tag]], args["min_opacity"])
    out["mingrad_1"] = _sides(stat_avg(ga[tags["mingrad_1"]], dn[tags["mingrad_1"]]), args["min_gradient"])
    i = tags["mingrad_s%d" % N]
    out["mingrad_s"] = _sides(scaled_avg(ga[i], dn[i], r), args["min_gradient"])
    return out


# ---- flags, weights, special rows -----------------------------------------------------------------------------------------------------------------
ZERO_ROWS = 12


def flag_state(P=257, seed=21):
    """`mixed_state` whose first rows make a threshold of exactly 0.0 decide: max_radii2D == 0 and a tiny positive one, an average of
    exactly 0 with a non-zero denominator, and an opacity that saturates to 0 (sigmoid(-200) == 0 in float32)."""
    b = mixed_state(P, seed)
    st, pr = b["stats"], b["params"]
    z = slice(0, ZERO_ROWS)
    st["xyz_gradient_accum"][z, 0] = torch.tensor([0.0, 0.0, 0.3, 0.3, 0.3, 0.3, 0.0, 1e-30, 0.3, 0.3, 0.0, 0.3])
    st["denom"][z, 0] = torch.tensor([1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 3.0, 1.0])
    st["max_radii2D"][z] = torch.tensor([0.0, 5.0, 0.0, 1e-30, 0.0, 1e-30, 0.0, 0.0, 30.0, 0.0, 0.0, 0.0])
    pr["_scaling"][z] = torch.tensor(float(SMALL))
    pr["_scaling"][9] = torch.tensor(float(LARGE))
    pr["_opacity"][z, 0] = torch.tensor([2.0, 2.0, 2.0, 2.0, -200.0, -200.0, 2.0, 2.0, -200.0, 2.0, -200.0, -100.0])
    return b


FLAG_VARIANTS = {"no_min_opacity": dict(min_opacity=None), "no_min_gradient": dict(min_gradient=None), "no_split_screen": dict(split_screen_threshold=None),
                 "none_of_the_three": dict(min_opacity=None, min_gradient=None, split_screen_threshold=None),
                 "min_opacity_zero": dict(min_opacity=0.0), "min_gradient_zero": dict(min_gradient=0.0), "split_screen_zero": dict(split_screen_threshold=0.0)}
WEIGHT_KINDS = ("zeros", "negative", "mixed_sign", "cloned_negative")


def weight_state(kind, P=257, seed=31):
    """`mixed_state` with other accumulated weights.  A clone child gets weight * wmax0 and a split child weight * wmax1, wmax1 the maximum once
    the clone children are appended: with wmax0 < 0 ("negative") the largest product comes from the SMALLEST cloned weight."""
    b = mixed_state(P, seed)
    rng = np.random.default_rng(seed)
    w = rng.random(P).astype(F) * 3 + F(0.25)
    if kind == "zeros":
        w[:] = 0.0
    elif kind == "negative":
        w = -w
    elif kind == "mixed_sign":
        w[::2] = -w[::2]
    else:                                                                  # "cloned_negative": every cloned weight below zero, the maximum above
        clone = plan_of(b, {}, MIXED_ARGS)["clone"]
        w[clone] = -w[clone]
    b["stats"]["xyz_weight_accum"] = torch.from_numpy(w.reshape(P, 1))
    return b


def special_rows():
    """Statistics no finite training run produces, for the plan-level check only: (ga, dn, mr, wa, scal, opac) NumPy, activated values given directly."""
    nan, inf = F("nan"), F("inf")
    ga = np.array([nan, nan, inf, inf, 0.3, 0.3, 0.0, 0.0, nan, inf, -1.0, -inf, 0.05, 0.05, -0.0, 0.3], F)
    dn = np.array([1.0, 2.0, 1.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, -0.0], F)
    P = ga.shape[0]
    scal = np.where((np.arange(P) % 2 == 0)[:, None], F(0.01), F(0.06)) * np.array([[1.0, 0.5]], F)
    scal[3] = scal[3][::-1]
    mr = np.where(np.arange(P) % 4 < 2, F(3.0), F(30.0)).astype(F)
    return ga, dn, mr, (np.arange(P, dtype=F) - F(4.5)), scal.astype(F), np.full(P, 0.9, F)


# ---- the oversize masks ----------------------------------------------------------------------------------------------------------------------------
T_MAX_SCREEN = F(45.0)
RAW_SCENE = F(math.log(0.09))


def oversize_case(P=65, seed=41):
    """-> (before, tags, pick) for `prune_max_scene_and_screen`: rows at max_radii2D == T_MAX_SCREEN and one step either side (small scales), rows
    whose larger scale is the picked row's and a few raw steps either side (small radii), the maximum once in each column."""
    b = mixed_state(P, seed)
    b["params"]["_scaling"] = torch.log(torch.exp(b["params"]["_scaling"]) * 0.5)         # every other scale well below 0.09
    b["stats"]["max_radii2D"] = b["stats"]["max_radii2D"] * 0.8                            # every other radius below 45
    rng = np.random.default_rng(seed)
    free = list(rng.permutation(P))
    tags = {"screen": [], "scene_c0": [], "scene_c1": []}
    for mr in (ulp_step(T_MAX_SCREEN, -1), T_MAX_SCREEN, ulp_step(T_MAX_SCREEN, 1)) * 2:
        i = int(free.pop())
        tags["screen"].append(i)
        b["stats"]["max_radii2D"][i] = float(mr)
    for j in NEIGHBOURS:
        s = float(ulp_step(RAW_SCENE, j) if j else RAW_SCENE)
        for tag, pair in (("scene_c0", (s, float(SMALL))), ("scene_c1", (float(SMALL), s))):
            i = int(free.pop())
            tags[tag].append(i)
            b["params"]["_scaling"][i] = torch.tensor(pair)
            b["stats"]["max_radii2D"][i] = 1.0
    pick = next(i for i in tags["scene_c0"] if float(b["params"]["_scaling"][i, 0]) == float(RAW_SCENE))
    b["stats"]["xyz_weight_accum"] = (torch.randperm(P, generator=torch.Generator().manual_seed(seed)).float()[:, None] + 1) * 0.25   # distinct averages
    b["stats"]["denom"][:] = 1.0
    return b, {k: np.array(sorted(v)) for k, v in tags.items()}, pick


def oversize_witness(before, tags, scal, scene_limit):
    mr = before["stats"]["max_radii2D"].numpy()
    out = {"screen": _sides(mr[tags["screen"]], T_MAX_SCREEN)}
    for tag, col in (("scene_c0", 0), ("scene_c1", 1)):
        i = tags[tag]
        assert bool((scal[i].argmax(axis=1) == col).all())
        out[tag] = _sides(scal[i].max(axis=1), scene_limit)
    return out


# ---- the end-to-end cases ----------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 170, 171, 255, 256, 257, 1025)           # wavefront and workgroup borders; 6 P = 1020 / 1026 around the scan's 1024 counters
EDGE_SIZES = (1, 2, 257)


def _case(before, args, cfg=None, N=2, names=NAMES8, optimizer="state"):
    fixed = args if callable(args) else (lambda dev: args)
    return dict(before=before, cfg=cfg or {}, args=fixed, N=N, names=names, optimizer=optimizer)


def _threshold_grow_case(N, spatial_scale):
    before, tags, picks = threshold_case()
    c = _case(before, lambda dev: data_thresholds(before, picks, spatial_scale, dev), {"spatial_scale": spatial_scale}, N)
    c["tags"] = tags
    return c


def _registry():
    reg = {}
    for N, s in ((2, 1.0), (2, 2.0), (2, 0.5), (3, 1.0)):
        reg["thresholds-N%d-scale%g" % (N, s)] = lambda N=N, s=s: _threshold_grow_case(N, s)
    for P in SIZES:
        reg["mixed-P%d" % P] = lambda P=P: _case(mixed_state(P, seed=P), MIXED_ARGS)
    for P in EDGE_SIZES:
        for kind in UNIFORM_KINDS:
            reg["%s-P%d" % (kind, P)] = lambda P=P, kind=kind: _case(uniform_state(P, kind), UNIFORM_ARGS)
    for kind in ONE_OF_EACH:
        for at_end in (False, True):
            reg["one_%s_%s" % (kind, "last" if at_end else "first")] = lambda kind=kind, at_end=at_end: _case(one_of_each(65, kind, at_end), UNIFORM_ARGS)
    reg["layout-six_parameters"] = lambda: _case(mixed_state(257, 13, NAMES6), MIXED_ARGS, names=NAMES6)
    reg["layout-features_rest_15x3"] = lambda: _case(mixed_state(257, 14, rest=(15, 3)), MIXED_ARGS)
    reg["layout-no_optimizer"] = lambda: _case(mixed_state(257, 15), MIXED_ARGS, optimizer=None)
    reg["layout-empty_optimizer"] = lambda: _case(mixed_state(257, 16), MIXED_ARGS, optimizer="empty")
    reg["children-N1"] = lambda: _case(mixed_state(65, 17), MIXED_ARGS, N=1)
    reg["children-N16"] = lambda: _case(mixed_state(65, 18), MIXED_ARGS, N=16)
    for name, change in FLAG_VARIANTS.items():
        reg["flags-" + name] = lambda change=change: _case(flag_state(), dict(MIXED_ARGS, **change))
    for kind in WEIGHT_KINDS:
        reg["weights-" + kind] = lambda kind=kind: _case(weight_state(kind), MIXED_ARGS)
    return reg


GROW_CASES = _registry()                                               # {id: () -> case}; nothing is built at import
