"""CPU: the mesh clean-up oracle (tests/mesh_clean_oracle.py) on hand-made meshes whose answers are written out, the multi-object volume on the
oracle alone, the union-find of csrc/mesh_unionfind.h built for the host and run by several threads against the oracle, the argument checks of the
clean-up C-ABI that need no GPU, and the clean() rule.  (The HIP kernels are compared against the same oracle in tests/test_mesh_clean_gpu.py.)"""
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_clean_cases as cc
from tests import mesh_clean_oracle as co
from tests import mesh_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. hand-made meshes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.HAND))
def test_oracle_on_hand_made_meshes(name):
    V, faces, vlabel, flabel, nfaces, nverts = cc.HAND[name]
    c = co.components(V, faces)
    assert c.count == len(nfaces)
    assert c.vertex_label.tolist() == vlabel and c.face_label.tolist() == flabel
    assert c.faces.tolist() == nfaces and c.vertices.tolist() == nverts
    pv, pf = co.components_plain(V, faces)                      # the oracle's two formulations agree
    assert pv.tolist() == vlabel and pf.tolist() == flabel


def test_oracle_selection_on_hand_made_meshes():
    pos = lambda V: np.arange(3 * V, dtype=np.float32).reshape(V, 3)
    V, faces = cc.HAND["two disjoint triangles"][:2]
    s = co.select_faces(pos(V), faces, pos(V) + 100, [1, 1])    # all ones: exactly the unreferenced vertices 0 and 4 go
    assert s.vertex_index.tolist() == [1, 2, 3, 5, 6, 7] and s.faces.tolist() == [[3, 5, 4], [0, 1, 2]]
    assert np.array_equal(s.vertices, pos(V)[[1, 2, 3, 5, 6, 7]]) and np.array_equal(s.colors, s.vertices + 100)
    s = co.select_faces(pos(V), faces, None, [0, 7])            # any non-zero byte keeps
    assert s.vertex_index.tolist() == [1, 2, 3] and s.faces.tolist() == [[0, 1, 2]] and s.colors is None
    V, faces = cc.HAND["out of range"][:2]
    s = co.select_faces(pos(V), faces, None, [1, 1, 1])         # the two ignored faces are never selected
    assert s.vertex_index.tolist() == [1, 2, 3] and s.faces.tolist() == [[1, 2, 0]]
    s = co.select_faces(pos(V), faces, None, [1, 1, 0])
    assert s.vertices.shape == (0, 3) and s.faces.shape == (0, 3)
    V, faces = cc.HAND["no faces"][:2]
    s = co.select_faces(pos(V), faces, None, [])
    assert s.vertices.shape == (0, 3) and s.faces.shape == (0, 3) and s.vertex_index.shape == (0,)


# ---- 2. the multi-object volume ---------------------------------------------------------------------------------------------------------------------
def test_multi_object_volume_has_the_components_it_names():
    m = cc.multi_volume().mesh
    V, F = m.vertices.shape[0], m.faces.shape[0]
    assert (V, F) == (4928, 9836)
    c = co.components(V, m.faces)
    assert c.count == 6 and c.faces.tolist() == cc.MULTI_FACES and c.smallest.tolist() == cc.MULTI_SMALLEST
    assert int(c.faces.sum()) == F and int(c.vertices.sum()) == V and (c.vertex_label >= 0).all()
    for lab in range(6):
        part = co.select_faces(m.vertices, m.faces, None, c.face_label == lab)
        top = mo.mesh_topology(part.faces, part.vertices.shape[0])
        assert top.closed_oriented and top.all_referenced and top.euler == cc.MULTI_EULER[lab]
        assert part.vertices.shape[0] == c.vertices[lab]


@pytest.mark.parametrize("keep_largest", [1, 2, 3])
def test_multi_object_clean_equals_the_extraction_of_the_kept_objects(keep_largest):
    """The condition of tests/mesh_clean_cases.py: no cell crossed by one surface sees another object's distance.  Then removing a component from
    the mesh and removing its object from the volume are the same thing, array for array."""
    m = cc.multi_volume().mesh
    got = co.clean(m.vertices, m.faces, m.colors, keep_largest=keep_largest, min_faces=0)
    want = cc.multi_volume(cc.MULTI_KEPT[keep_largest]).mesh
    assert got.faces.shape[0] == sum(sorted(cc.MULTI_FACES)[-keep_largest:])
    assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.colors, want.colors) and np.array_equal(got.faces, want.faces)
    assert np.array_equal(m.vertices[got.vertex_index], got.vertices)


# ---- 3. the union-find header on the host -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_unionfind(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_unionfind")
    exe = str(d / "mesh_unionfind_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "envgs_amd", "csrc", "mesh_unionfind_host.cpp")], check=True)

    def run(V, faces, threads):
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([V, faces.shape[0]], np.uint32).tobytes() + np.ascontiguousarray(faces, np.int32).tobytes())
        subprocess.run([exe, src, dst, str(threads)], check=True)
        raw = np.fromfile(dst, np.int32)
        F = faces.shape[0]
        C = int(raw[V + F])
        assert raw.size == V + F + 1 + 2 * C
        return raw[:V], raw[V:V + F], C, raw[V + F + 1:V + F + 1 + C], raw[V + F + 1 + C:]
    return run


def _check_host(run, V, faces, threads):
    want = co.components(V, faces)
    vlabel, flabel, C, nfaces, nverts = run(V, faces, threads)
    assert C == want.count
    assert np.array_equal(vlabel, want.vertex_label) and np.array_equal(flabel, want.face_label)
    assert np.array_equal(nfaces, want.faces) and np.array_equal(nverts, want.vertices)
    return want


@pytest.mark.parametrize("threads", [4, 7])
def test_host_unionfind_equals_the_oracle_on_random_meshes(host_unionfind, threads):
    for seed, (V, F) in enumerate([(50, 20), (3000, 1500), (20000, 9000), (20000, 60000)]):
        faces = cc.random_mesh(V, F, seed)
        faces[::97, seed % 3] = V + seed                        # and some faces to ignore
        faces[5::89, (seed + 1) % 3] = -1
        want = _check_host(host_unionfind, V, faces, threads)
        assert (want.face_label == -1).sum() >= F // 97 and want.count >= 1
    for name in cc.HAND:
        V, faces = cc.HAND[name][:2]
        _check_host(host_unionfind, V, faces, threads)


@pytest.mark.parametrize("kind", ["reversed", "identity", "random"])
def test_host_unionfind_on_strips(host_unionfind, kind):
    for F in (1, 65, 20001):
        V, faces = cc.strip(F, kind)
        want = _check_host(host_unionfind, V, faces, 6)
        assert want.count == 1 and (want.vertex_label == 0).all() and want.faces.tolist() == [F] and want.vertices.tolist() == [V]
    V, faces = cc.crumbs(1001)
    want = _check_host(host_unionfind, V, faces, 5)
    assert want.count == 1001 and (want.vertex_label[2::4] == -1).all()


# ---- 4. the C-ABI ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from envgs_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_bad_arguments_are_rejected_before_any_gpu_work(lib):
    FAKE = 0x1000                                               # never dereferenced on the host; rejected calls launch nothing
    BIG = 1 << 31
    comp = lambda V=8, F=4, faces=FAKE, temp=FAKE, tb=1 << 30, vl=FAKE, fl=FAKE, cf=FAKE, cv=FAKE, cnt=FAKE: \
        lib.envgs_mesh_components(V, F, faces, temp, tb, vl, fl, cf, cv, cnt, None)
    for bad in (dict(V=BIG), dict(F=BIG), dict(faces=None), dict(temp=None), dict(temp=FAKE + 4), dict(vl=None), dict(fl=None), dict(cf=None),
                dict(cv=None), dict(cnt=None)):
        assert comp(**bad) == -1, bad
    need = lib.envgs_mesh_components_temp_bytes(1000, 4)
    assert 16 * 1000 <= need < 16 * 1000 + 4096                 # 16 B per vertex + the per-workgroup totals
    assert lib.envgs_mesh_components_temp_bytes(BIG, 4) == 0 and lib.envgs_mesh_components_temp_bytes(4, BIG) == 0
    assert comp(V=1000, tb=need - 1) == -2

    count = lambda V=8, F=4, faces=FAKE, keep=FAKE, temp=FAKE, tb=1 << 30, totals=FAKE: lib.envgs_mesh_select_count(V, F, faces, keep, temp, tb, totals, None)
    for bad in (dict(V=BIG), dict(F=BIG), dict(faces=None), dict(keep=None), dict(temp=None), dict(temp=FAKE + 8), dict(totals=None)):
        assert count(**bad) == -1, bad
    need = lib.envgs_mesh_select_temp_bytes(1000, 3000)
    assert 2 * 1000 <= need < 2 * 1000 + 4096                   # 2 B per vertex + the per-workgroup totals
    assert lib.envgs_mesh_select_temp_bytes(BIG, 4) == 0 and lib.envgs_mesh_select_temp_bytes(4, BIG) == 0
    assert count(V=1000, F=3000, tb=need - 1) == -2

    emit = lambda V=8, F=4, v=FAKE, c=None, faces=FAKE, keep=FAKE, temp=FAKE, tb=1 << 30, Vo=3, Fo=1, ov=FAKE, oc=None, of=FAKE, vi=None: \
        lib.envgs_mesh_select_emit(V, F, v, c, faces, keep, temp, tb, Vo, Fo, ov, oc, of, vi, None)
    for bad in (dict(V=BIG), dict(F=BIG), dict(v=None), dict(faces=None), dict(keep=None), dict(temp=None), dict(ov=None), dict(of=None),
                dict(Vo=9), dict(Fo=5), dict(Vo=BIG), dict(oc=FAKE)):          # more survivors than rows; colours asked for, none given
        assert emit(**bad) == -1, bad
    assert emit(V=1000, F=3000, tb=need - 1) == -2
    assert emit(Vo=0, Fo=0, ov=None, of=None) == 0              # nothing survives: nothing to launch


# ---- 5. CPU tensors ---------------------------------------------------------------------------------------------------------------------------------
def test_clean_up_on_cpu_tensors_raises():
    import torch
    from envgs_amd import mesh
    m = mesh.Mesh(vertices=torch.zeros(3, 3), faces=torch.zeros(1, 3, dtype=torch.int32), colors=None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.components(m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.select_faces(m, torch.ones(1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.clean(m)


# ---- 6. the clean() rule ----------------------------------------------------------------------------------------------------------------------------
def test_clean_rule_on_the_oracle():
    n = [5, 3, 3, 1, 7]
    kept = lambda **kw: sorted(np.asarray(n)[co.clean_keep(n, **kw)].tolist(), reverse=True)
    assert kept(keep_largest=2, min_faces=0) == [7, 5]
    assert kept(keep_largest=3, min_faces=0) == [7, 5, 3, 3]            # the tie at the threshold is kept
    assert kept(keep_largest=3, min_faces=4) == [7, 5]
    assert kept(keep_largest=9, min_faces=2) == [7, 5, 3, 3]            # more than there are: all with >= min_faces
    assert kept(keep_largest=5, min_faces=0) == [7, 5, 3, 3, 1]
    assert kept(keep_largest=None, min_faces=0) == [7, 5, 3, 3, 1]
    assert kept(keep_largest=0, min_faces=4) == [7, 5]
    assert kept() == []                                                  # the defaults: nothing here has 50 faces
