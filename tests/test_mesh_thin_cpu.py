"""CPU: the oracle of the DTU protocol (tests/mesh_thin_oracle.py) against itself and against brute force -- the keys are distinct, the loop over
keys is the loop over the permuted array, its result is independent and maximal, the round scheme of the device gives the same set in the
predicted number of rounds, and the point filters decide hand-written rows as include/envgs_mesh.h and envgs_amd/mesh.py say."""
import functools

import numpy as np
import pytest

from tests import mesh_thin_cases as tc
from tests import mesh_thin_oracle as to

F32 = np.float32
ORDERS = [0, 1, None]


@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF])
def test_keys_are_distinct(seed):
    k = to.keys(2 ** 20, seed)
    assert k.min() >= 0 and k.max() < 2 ** 32 and np.unique(k).shape[0] == 2 ** 20
    assert np.array_equal(to.keys(5, None), np.arange(5))


@functools.lru_cache(maxsize=None)
def _prototype(name):
    points, radius = tc.PROTOTYPE[name]()
    return points, radius, to.neighbour_matrix(points, radius)


@pytest.mark.parametrize("name", list(tc.PROTOTYPE))
def test_loop_over_keys_is_the_loop_over_the_permuted_array(name):
    points, radius, _ = _prototype(name)
    for seed in (0, 1):
        key = to.keys(points.shape[0], seed)
        order = np.argsort(key, kind="stable")
        permuted = to.thin_loop(points[order], radius, np.arange(points.shape[0]))
        keep = to.thin_loop(points, radius, key)
        assert np.array_equal(keep[order], permuted)


@pytest.mark.parametrize("name", list(tc.PROTOTYPE))
def test_kept_sets_are_independent_and_maximal(name):
    points, radius, nb = _prototype(name)
    density = nb.sum() / points.shape[0]
    assert 1.5 < density < 60, density                            # the case has the neighbours its name claims, within a factor
    for seed in ORDERS:
        keep = to.thin(points, radius, seed)
        assert not nb[np.ix_(keep, keep)].any()                   # no two kept points are neighbours
        assert nb[:, keep][~keep].any(axis=1).all()               # every dropped point has a kept neighbour


@pytest.mark.parametrize("name", list(tc.PROTOTYPE))
def test_round_scheme_equals_the_loop(name):
    points, radius, nb = _prototype(name)
    for seed in ORDERS:
        key = to.keys(points.shape[0], seed)
        keep, rounds, history = to.thin_rounds(points, radius, key, nb)
        assert np.array_equal(keep, to.thin_loop(points, radius, key)), (name, seed)
        assert history[-1] == 0 and all(a > b for a, b in zip(history, history[1:]))
        if name == "collinear":
            assert rounds == (tc.COLLINEAR_N if seed is None else rounds) and keep.sum() == (300 if seed is None else keep.sum())
            assert seed is None or rounds <= 12
        elif seed is not None:
            assert rounds <= 16, (name, seed, history)            # about log N under a hash order


def test_radius_zero_and_non_finite_rows():
    points, which = tc.duplicates()
    for seed in ORDERS:
        key = to.keys(points.shape[0], seed)
        keep = to.thin(points, 0.0, seed)
        assert keep.sum() == 50 and not keep[which < 0].any()
        for pos in range(50):
            rows = np.flatnonzero(which == pos)
            assert keep[rows[np.argmin(key[rows])]]               # the survivor is the copy of smallest key
    assert to.thin(np.zeros((0, 3), F32), 1.0, 0).shape == (0,)


def test_filters_on_hand_written_rows():
    nan = np.nan
    p = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [-1e-7, 0.5, 0.5], [0.5, 1, 0.5], [nan, 0.5, 0.5], [0.5, np.inf, 0.5]], F32)
    assert to.in_box(p, (0, 0, 0), (1, 1, 1)).tolist() == [True, False, True, False, False, False, False]      # lo is inside, hi is not
    # voxel 2 from origin 1: g = rint((p - 1) / 2); ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0
    vol = np.zeros((3, 3, 3), bool)
    vol[0, 0, 0] = vol[2, 0, 0] = vol[2, 2, 2] = True
    q = np.array([[2, 1, 1], [4, 1, 1], [6, 1, 1], [0, 1, 1], [-0.01, 1, 1], [5.99, 5, 5], [6.01, 1, 1], [3, 1, 1], [1, nan, 1], [5, 5, 5.9]], F32)
    #             g 0.5 -> 0   1.5 -> 2   2.5 -> 2   -0.5 -> -0  -0.505 -> -1  2.495 -> 2,2,2  2.505 -> 3   1 (unset)   NaN        2,2,2.45 -> 2
    assert to.in_volume(q, vol, (1, 1, 1), 2.0).tolist() == [True, True, True, True, False, True, False, False, False, True]
    r = np.array([[0, 0, 1], [0, 0, 1.0000001], [0, 0, 0.9999999], [3, -1, 1], [nan, 0, 5], [0, 0, np.inf]], F32)
    assert to.above_plane(r, (1.0, 3.0, 2.0, -2.0)).tolist() == [False, True, False, False, False, False]        # on the plane is not above it


def test_cull_rule_on_hand_placed_vertices():
    K, R = [[10, 0, 4], [0, 10, 3], [0, 0, 1]], np.eye(3)
    mask = np.zeros((6, 8), np.uint8)
    mask[:, 4:] = 1                                               # the right half is the object
    v = np.array([[0, 0, -1],                                     # behind the camera: passes
                  [0, 0, 0],                                      # zc = 0: passes
                  [-1, 0, 1],                                     # u = -6: outside the image, passes
                  [0, 0.29, 1],                                   # v = 5.9: the last row, px 4: mask set
                  [0, 0.3, 1],                                    # v = 6 (or a rounding below it): decided by the fp32 rule either way
                  [-0.01, 0, 1],                                  # u = 3.9: px 3, outside the mask: fails
                  [0, 0, 1],                                      # u = 4 exactly: px 4, on the mask edge: passes
                  [np.nan, 0, 1], [0, np.inf, 1]], F32)           # not finite: fail
    keep = to.cull_vertices(v, [(K, R, [0, 0, 0])], [mask])
    assert keep.tolist()[:4] == [True, True, True, True] and keep.tolist()[5:] == [False, True, False, False]
    faces = np.array([[0, 1, 2], [0, 5, 1], [6, 3, 0], [0, 1, 9], [-1, 0, 1]], np.int32)
    fk = to.cull_faces(9, faces, keep)
    assert fk.tolist() == [True, False, True, False, False]
    m = to.select_faces(v, faces, None, fk)
    assert m.index.tolist() == [0, 1, 2, 3, 6] and m.faces.tolist() == [[0, 1, 2], [4, 3, 0]]
