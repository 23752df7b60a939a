"""CPU: the mesh evaluation without a GPU.  The counter hash of csrc/mesh_rng.h built for the host against the oracle's (tests/mesh_eval_oracle.py);
then, on the oracle alone, that the inputs chosen for the GPU tests are ones the oracle itself passes: sample totals near area x density,
samples uniform over a triangle, samples inside their faces.  Also the brute-force nearest on a case small enough to check by hand, and a
ground-truth cloud (a PLY without faces) through ckpt.load_mesh_ply."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_eval_cases as ec
from tests import mesh_eval_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- 1. the hash ----------------------------------------------------------------------------------------------------------------------------------------
def test_host_hash_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "mesh_rng_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "envgs_amd", "csrc", "mesh_rng_host.cpp")], check=True)
    rng = np.random.default_rng(5)
    edge = np.array([0, 0xFFFFFFFF, 1, 0x80000000], np.uint32)
    grid = np.stack(np.meshgrid(edge, edge, edge, indexing="ij"), axis=-1).reshape(-1, 3)      # 0 and 0xFFFFFFFF in each position, all combinations
    args = np.concatenate([grid, rng.integers(0, 2 ** 32, (2 ** 16 - grid.shape[0], 3), dtype=np.uint64).astype(np.uint32)])
    assert args.shape == (2 ** 16, 3)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.uint32(args.shape[0]).tobytes() + np.ascontiguousarray(args).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    out = np.fromfile(tmp_path / "out.bin", dtype=np.uint32)
    h, u = out[:2 ** 16], out[2 ** 16:].view(F32)
    want = eo.hash3(args[:, 0], args[:, 1], args[:, 2])
    assert np.array_equal(h, want)
    assert np.array_equal(u.view(np.uint32), eo.uniform(want).view(np.uint32)) and u.min() >= 0 and u.max() < 1
    assert len(np.unique(want)) > 2 ** 16 - 8                    # the hash does not collapse


# ---- 2. totals ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.SEEDED))
def test_sample_total_is_near_area_times_density(name):
    """Var floor(x + u) <= 1/4 per face, so 3 sqrt(F) is six sigma."""
    m = ec.SEEDED[name]()
    fc = eo.face_counts(m.vertices, m.faces, m.density, m.seed)
    expected = float((fc.area.astype(np.float64) * m.density).sum())
    S, F = int(fc.count.sum()), m.faces.shape[0]
    print("%s: F %d, S %d, expected %.1f, bound %.1f" % (name, F, S, expected, 3 * math.sqrt(F)))
    assert not fc.over and abs(S - expected) <= 3 * math.sqrt(F)
    assert (fc.count[~fc.valid] == 0).all()


def test_the_seeded_cases_are_what_the_gpu_tests_say_they_are():
    g = eo.face_counts(ec.giant().vertices, ec.giant().faces, ec.giant().density, ec.giant().seed).count
    assert 99000 < g[500] < 101000 and np.delete(g, 500).max() <= 1 and 0 < np.delete(g, 500).sum() < 999
    m = ec.many()
    assert (m.faces.shape[0] + 255) // 256 > 1024
    c = eo.face_counts(m.vertices, m.faces, m.density, m.seed).count
    assert set(np.unique(c)) == {0, 1, 2} and c[-300:].sum() > 0
    s = eo.face_counts(ec.soup().vertices, ec.soup().faces, ec.soup().density, ec.soup().seed)
    assert not s.valid[[5, 77, 100]].any() and (~s.valid).sum() > 3          # the planted faces, and those that name the NaN vertex


def test_written_counts_of_the_hand_made_meshes():
    for name, (m, counts) in ec.HAND.items():
        fc = eo.face_counts(m.vertices, m.faces, m.density, m.seed)
        assert fc.count.tolist() == counts and not fc.over, name
    tri = ec.HAND["one right triangle"][0]
    assert eo.face_counts(tri.vertices, tri.faces, 1e-9, 0).count.tolist() == [0]
    assert eo.face_counts(tri.vertices, tri.faces, 2.0 ** 23, 0).over                         # 2 x 2^23 = 2^24
    assert not eo.face_counts(tri.vertices, tri.faces, 2.0 ** 22, 0).over


# ---- 3. uniformity --------------------------------------------------------------------------------------------------------------------------------------------
def _chi2_sf(x, k):
    """P(chi2_k > x) = Q(k/2, x/2), the regularised upper incomplete gamma function; for the odd k = 15 by the finite series
    Q(n + 1/2, y) = erfc(sqrt y) + exp(-y) sum_{i=1..n} y^(i - 1/2) / Gamma(i + 1/2)."""
    assert k % 2 == 1
    y, n = x / 2.0, (k - 1) // 2
    return math.erfc(math.sqrt(y)) + math.exp(-y) * sum(y ** (i - 0.5) / math.gamma(i + 0.5) for i in range(1, n + 1))


def _chi2_quantile(p_upper, k):
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _chi2_sf(mid, k) > p_upper else (lo, mid)
    return hi


def test_samples_are_uniform_over_a_triangle():
    assert abs(_chi2_sf(24.996, 15) - 0.05) < 1e-4               # the textbook 95 % point of chi2_15
    bound = _chi2_quantile(1e-6, 15)
    assert 50 < bound < 70
    n = 2 ** 16
    for seed in (0, 1, 12345):
        u, v = eo.sample_uv(seed, np.zeros(n, np.int64), np.arange(n))
        u, v = u.astype(np.float64), v.astype(np.float64)
        # the 16 congruent sub-triangles of the 4 x 4 barycentric grid: 10 upright (i, j), 6 inverted
        a, b = np.minimum(np.floor(4 * u), 3), np.minimum(np.floor(4 * v), 3)
        inverted = (4 * u - a) + (4 * v - b) > 1
        cell = (a * 4 + b).astype(np.int64) * 2 + inverted
        counts = np.unique(cell, return_counts=True)[1]
        assert counts.shape[0] == 16 and counts.sum() == n
        chi2 = float(((counts - n / 16) ** 2 / (n / 16)).sum())
        print("seed %d: chi2 %.2f (bound %.2f)" % (seed, chi2, bound))
        assert chi2 < bound


# ---- 4. inside the face -----------------------------------------------------------------------------------------------------------------------------------------
def test_barycentric_coordinates_are_inside():
    for seed in (0, 7, 0xFFFFFFFF):
        rng = np.random.default_rng(seed)
        face, k = rng.integers(0, 2 ** 31, 200000), rng.integers(0, 2 ** 24, 200000)
        u, v = eo.sample_uv(seed, face, k)
        u, v = u.astype(np.float64), v.astype(np.float64)
        assert u.min() >= 0 and v.min() >= 0 and (u + v).max() <= 1
    for name in ec.SEEDED:
        m = ec.SEEDED[name]()
        s = eo.sample_surface(m.vertices, m.faces, m.colors, m.density, m.seed)
        assert s.u.min() >= 0 and s.v.min() >= 0 and (s.u.astype(np.float64) + s.v.astype(np.float64)).max() <= 1
        assert np.isfinite(s.points).all() and (np.diff(s.face) >= 0).all()


# ---- the brute force, by hand -------------------------------------------------------------------------------------------------------------------------------------
def test_brute_force_nearest_by_hand():
    p = np.array([[0, 0, 0], [2, 0, 0], [2, 0, 0], [np.nan, 0, 0], [10, 0, 0]], F32)
    q = np.array([[1, 0, 0], [2.1, 0, 0], [6, 0, 0], [np.inf, 0, 0], [7, 0, 0]], F32)
    d2, i = eo.nearest(q, p, 3.0)
    assert i.tolist() == [0, 1, -1, -1, 4] and d2[0] == 1 and np.isinf(d2[2]) and np.isinf(d2[3]) and d2[4] == 9      # the tie, the duplicate, the radius (inclusive)
    assert eo.nearest(q, p[:0], 3.0)[1].tolist() == [-1] * 5
    e = eo.evaluate(p[[0, 1, 4]], q[[0, 1, 2]], 3.0, 1.0)
    assert (e.found_pred, e.within_pred, e.found_ref, e.within_ref) == (2, 2, 2, 2) and abs(e.precision - 2 / 3) < 1e-15


# ---- a ground-truth cloud -------------------------------------------------------------------------------------------------------------------------------------------
def test_a_ply_without_faces_loads(tmp_path):
    from envgs_amd import ckpt
    pts = np.random.default_rng(1).random((10, 3), dtype=F32)
    for tail in ("", "element face 0\nproperty list uchar int vertex_indices\n"):
        path = str(tmp_path / "cloud.ply")
        with open(path, "wb") as fh:
            fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex 10\nproperty float x\nproperty float y\nproperty float z\n%send_header\n" % tail).encode())
            fh.write(pts.tobytes())
        v, f, c = ckpt.load_mesh_ply(path)
        assert np.array_equal(v, pts) and f.shape == (0, 3) and f.dtype == np.int32 and c is None
