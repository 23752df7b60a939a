"""CPU: the mesh rasteriser's rule (include/envgs_mesh.h, "rasterisation").  csrc/mesh_raster.h is one text for the kernels and for the host: the
stand-alone program built from it here must give the key image of the independent oracle (tests/mesh_raster_oracle.py) bit for bit on every case of
tests/mesh_raster_cases.py, which checks the kernels' arithmetic without a GPU.  Then pins of the oracle itself, and the argument checks of
render_mesh / visible_faces that need no GPU.  PARITY UNPINNED: the semantics are this project's."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_raster_cases as rc
from tests import mesh_raster_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_MAX = 16                                                   # the starting value; the GPU tests read the real one from the ABI


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_raster") / "mesh_raster_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "envgs_amd", "csrc", "mesh_raster_host.cpp")], check=True)
    return exe


def _host_keys(exe, c, tmp_path):
    src, dst = str(tmp_path / (c.name + ".in")), str(tmp_path / (c.name + ".out"))
    with open(src, "wb") as f:
        f.write(np.array([c.H, c.W], np.int32).tobytes())
        f.write(np.array([len(c.cameras), len(c.vertices), len(c.faces)], np.uint32).tobytes())
        f.write(np.array([c.near], np.float32).tobytes())
        for cam in c.cameras:
            K = np.asarray(cam.K, np.float32)
            f.write(np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.asarray(cam.R, np.float32).ravel(), np.asarray(cam.T, np.float32).ravel()])
                    .astype(np.float32).tobytes())
        f.write(c.vertices.tobytes())
        f.write(c.faces.tobytes())
    subprocess.run([exe, src, dst], check=True)
    return np.fromfile(dst, np.uint64).reshape(len(c.cameras), c.H, c.W)


@pytest.mark.parametrize("c", rc.all_cases(SMALL_MAX), ids=lambda c: c.name)
def test_host_build_of_the_header_gives_the_oracles_keys(host_exe, tmp_path, c):
    got = _host_keys(host_exe, c, tmp_path)
    want = np.stack([ro.key_image(c.vertices, c.faces, cam, c.H, c.W, c.near) for cam in c.cameras])
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want), "%d of %d keys differ" % ((got != want).sum(), got.size)
    if c.name.startswith(("whole_image", "fan")):
        assert (want != ro.EMPTY).all()                          # these cover every pixel


def test_quad_pin():
    c = rc.quad()
    r = ro.render(c.vertices, c.faces, c.cameras, c.H, c.W, c.near)
    covered = r["face"][0] >= 0
    want = np.zeros((24, 32), bool)
    want[3:9, 4:12] = True                                      # left and top edges in, right and bottom edges out
    assert covered.sum() == 48 and np.array_equal(covered, want)
    ulp = np.abs(r["depth"][0][covered].view(np.int32).astype(np.int64) - int(np.float32(2.0).view(np.int32)))
    assert ulp.max() <= 1
    assert np.array_equal(r["seen"], [1, 1])


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("flat", [False, True])
def test_fan_pin(reverse, flat):
    """Consecutive spokes less than pi apart: every pixel belongs to exactly one face, also on the shared edges and at the apex."""
    for seed in range(10):
        c = rc.fan(12, 10, 100 + seed, reverse=reverse, flat=flat)
        cam = c.cameras[0]
        proj = ro.project(cam, c.vertices, c.near)
        single = np.stack([ro.face_keys(f, c.vertices, c.faces, cam, c.H, c.W, c.near, proj) for f in range(len(c.faces))])
        assert ((single != ro.EMPTY).sum(0) == 1).all()
        assert np.array_equal(single.min(0), ro.key_image(c.vertices, c.faces, cam, c.H, c.W, c.near))


def test_tie_pin():
    c = rc.duplicates()
    r = ro.render(c.vertices, c.faces, c.cameras, c.H, c.W, c.near)
    face = r["face"][0]
    assert (face >= 0).sum() > 50 and set(np.unique(face)) == {-1, 0}
    assert np.array_equal(r["seen"], [1, 0, 0, 0, 0])
    # each copy alone covers the same pixels at the same depth: both windings, every rotation of the corners
    alone = [ro.key_image(c.vertices, c.faces[f:f + 1], c.cameras[0], c.H, c.W, c.near) for f in range(len(c.faces))]
    assert all(np.array_equal(a, alone[0]) for a in alone)


def test_dropped_faces_pin():
    c = rc.dropped()
    r = ro.render(c.vertices, c.faces, c.cameras, c.H, c.W, c.near)
    assert not r["seen"][c.bad].any() and r["seen"][~c.bad][:-1].all()
    keep = np.flatnonzero(~c.bad)
    alone = ro.render(c.vertices, c.faces[keep], c.cameras, c.H, c.W, c.near)
    assert np.array_equal(np.where(alone["face"] >= 0, keep[alone["face"]], -1), r["face"]) and np.array_equal(alone["depth"], r["depth"])


def test_normal_faces_the_camera_under_both_windings():
    c = rc.interpenetrating()
    r = ro.render(c.vertices, c.faces, c.cameras, c.H, c.W, c.near)
    flipped = ro.render(c.vertices, c.faces[:, ::-1], c.cameras, c.H, c.W, c.near)
    hit = r["face"][0] >= 0
    assert set(np.unique(r["face"][0][hit])) == {0, 1}
    # the reversed face is another sequence of roundings (other corner 0, other order of the sums): the same coverage, values to a few ulp
    assert np.array_equal(r["face"], flipped["face"])
    assert np.allclose(r["normal"], flipped["normal"], rtol=0, atol=1e-6) and np.allclose(r["depth"], flipped["depth"], rtol=1e-6, atol=0)
    assert (r["normal"][0][hit][:, 2] < 0).all()                # R = I: towards the camera is -z
    assert np.allclose(np.linalg.norm(r["normal"][0][hit], axis=-1), 1.0, atol=1e-6)
    assert np.allclose(r["bary"][0][hit].sum(-1), 1.0, atol=1e-6)
    assert np.allclose(r["bary"][0], flipped["bary"][0][..., ::-1], rtol=0, atol=1e-6)


# ---- argument checks that need no GPU ---------------------------------------------------------------------------------------------------------------
def _cpu_mesh(**kw):
    m = dict(vertices=torch.zeros(3, 3), faces=torch.zeros(1, 3, dtype=torch.int32), colors=None)
    m.update(kw)
    return SimpleNamespace(**m)


def test_cpu_tensors_raise():
    from envgs_amd import mesh
    cams = [rc.camera(5, 3)]
    for fn in (mesh.render_mesh, mesh.visible_faces, mesh.cull_unseen):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(_cpu_mesh(), cams)


def test_bad_arguments_raise():
    from envgs_amd import mesh
    cams = [rc.camera(5, 3)]
    with pytest.raises(ValueError, match="share one size"):
        mesh.render_mesh(_cpu_mesh(), [rc.camera(5, 3), rc.camera(3, 5)])
    with pytest.raises(ValueError, match="share one size"):
        mesh.visible_faces(_cpu_mesh(), [])                      # no cameras and no size
    with pytest.raises(ValueError, match="image size"):
        mesh.render_mesh(_cpu_mesh(), cams, size=(0, 4))
    with pytest.raises(ValueError, match="unknown output"):
        mesh.render_mesh(_cpu_mesh(), cams, outputs=("depth", "albedo"))
    with pytest.raises(ValueError, match="NaN"):
        mesh.visible_faces(_cpu_mesh(), cams, near=float("nan"))
    for bad in (dict(vertices=torch.zeros(3, 3, dtype=torch.float64)), dict(faces=torch.zeros(1, 3, dtype=torch.int64)), dict(vertices=torch.zeros(3, 4)),
                dict(faces=torch.zeros(3, dtype=torch.int32)), dict(vertices=np.zeros((3, 3), np.float32))):
        for fn in (mesh.render_mesh, mesh.visible_faces):
            with pytest.raises(ValueError, match="tensor"):
                fn(_cpu_mesh(**bad), cams)
