"""CPU: the image output's oracle (tests/visualize_oracle.py) against the reference's own bytes (tests/golden/visualize_golden.npz), the PNG / PPM
encoders, the writer's file names, the argument checks of envgs_amd.visualize, and the stated deviations."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from envgs_amd import visualize as vis
from tests import visualize_cases as vc
from tests import visualize_oracle as orc

F = np.float32


@pytest.fixture(scope="module")
def gold():
    return vc.load()


# ---- oracle against the reference ---------------------------------------------------------------------------------------------------------------
def test_oracle_gives_the_reference_bytes_on_every_case(gold):
    """Every kind byte-exact; NORMAL and the table colour map may differ by one step on at most 1 % of their bytes (measured: 0 bytes, all cases)."""
    cases = vc.golden_cases(gold)
    assert len(cases) == 23 and {c[1]["kind"] for c in cases} == {"color", "gray", "depth", "normal", "gt", "error"}
    total = 0
    for name, plane, canvas, origin, key in cases:
        got, want = orc.plane_bytes(plane, canvas, origin), vc.reference_rgba(gold, key)
        assert got.shape == want.shape and got.dtype == np.uint8
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        n = int((d > 0).sum())
        print("%-24s %d of %d bytes differ, largest step %d" % (name, n, d.size, d.max()))
        total += n
        if name.split("/")[0] in vc.BANDED:
            assert d.max() <= 1 and n <= 0.01 * d.size, (name, n, int(d.max()))
        else:
            assert n == 0, (name, n, int(d.max()))
    print("differing bytes over all cases: %d" % total)


def test_golden_covers_what_the_issue_names(gold):
    dpt, acc, norm = gold["in/dpt"], gold["in/acc"], gold["in/norm"]
    assert dpt.shape == (1, 27, 22, 1) and (dpt == 0).sum() > 100 and (dpt > 0).sum() > 100            # depth with a zero background region
    assert (acc == 0).sum() > 100 and bool((norm[acc[..., 0] == 0] == 0).all())                        # a normal map with acc = 0 pixels
    assert gold["in/gt8"].dtype == np.uint8 and 0 < gold["in/msk"].mean() < 1                           # 8-bit ground truth, a mask, a background
    assert gold["render_crop/img"].shape == (31, 29, 4) and gold["depth_linear/img"].shape == (27, 22, 2)
    assert os.path.getsize(vc.GOLDEN) < 256 * 1024


# ---- the byte rule and the deviations -------------------------------------------------------------------------------------------------------------
def test_byte_rule_ties_to_even_clips_and_nan():
    v = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, -1.0, 2.0, np.nan, np.inf, -np.inf, 1.0, 0.0, 254.5 / 255], F)
    exact = (v * F(255.0))[:3]
    assert list(exact) == [0.5, 1.5, 2.5]                                                               # the products are exact: real ties
    assert list(orc.to_byte(v)) == [0, 2, 2, 0, 255, 0, 255, 0, 255, 0, int(np.round(F(254.5 / 255) * F(255.0)))]
    # a NaN anywhere in a plane ends as the byte 0, its alpha too
    img = np.full((1, 2, 2, 3), 0.5, F); img[0, 0, 0, 1] = np.nan
    acc = np.ones((1, 2, 2, 1), F); acc[0, 1, 1, 0] = np.nan
    b = orc.plane_bytes(dict(kind="color", img=img, acc=acc))
    assert list(b[0, 0, 0]) == [128, 0, 128, 255] and list(b[0, 1, 1]) == [128, 128, 128, 0]
    e = orc.plane_bytes(dict(kind="error", img=img, gt=np.zeros_like(img)))
    assert list(e[0, 0, 0]) == [0, 0, 0, 255] and list(e[0, 0, 1]) == [191, 191, 191, 255]              # 0.75 * 255 = 191.25


def test_depth_ranks_clamp_under_100_pixels():
    assert orc.depth_ranks(99) == (0, 98) and orc.depth_ranks(1) == (0, 0) and orc.depth_ranks(35) == (0, 34)        # int(N * 0.01) = 0: n = 1
    assert orc.depth_ranks(100) == (0, 99) and orc.depth_ranks(594) == (4, 589)
    for N in (1, 35, 99, 100, 594, 2900, 5700, 1200 * 1600):                                            # the reference's expression, a double product
        n = max(int(N * 0.01), 1)
        assert vis.depth_ranks(N) == orc.depth_ranks(N) == (n - 1, N - n)
    d = np.arange(35, dtype=F).reshape(1, 7, 5, 1) + F(1.0)
    near, far = orc.depth_range(d[0])
    assert (near, far) == (1.0, 35.0)                                                                 # the smallest and the largest
    b = orc.plane_bytes(dict(kind="depth", img=d))
    assert b[0, 0, 0, 0] == 255 and b[0, -1, -1, 0] == 0 and bool((b[..., 3] == 255).all())


def test_flat_depth_and_negative_zero():
    d = np.full((1, 4, 5, 1), 2.5, F)
    b = orc.plane_bytes(dict(kind="depth", img=d))                                                    # near == far: 1 where d <= near
    assert bool((b[..., :3] == 255).all())
    d[0, 1, 2, 0] = 3.0                                                                               # N = 20: n = 1, near 2.5, far 3.0
    d2 = np.full((1, 30, 30, 1), 2.5, F); d2[0, 0, 0, 0] = 9.0                                         # N = 900: n = 9, near = far = 2.5
    b2 = orc.plane_bytes(dict(kind="depth", img=d2))
    assert list(b2[0, 0, 0, :3]) == [0, 0, 0] and bool((b2[0, 1:, :, :3] == 255).all())
    z = np.zeros((1, 3, 4, 1), F); z[0, 0, 0, 0] = -0.0
    near, far = orc.depth_range(z[0])
    assert not np.signbit(near) and not np.signbit(far)


def test_table_counts_an_inner_knot_twice():
    table = np.array([[0.0, 0.1, 0.2], [0.4, 0.3, 0.2], [0.8, 0.9, 1.0]], F)
    c = orc.colormap_table(np.array([0.5, 0.25], F), table)
    assert np.array_equal(c[0], table[1] + table[1])                                                  # both segments count the knot
    assert np.array_equal(c[1], table[1] * F(0.5) + table[0] * F(0.5))


# ---- PNG and PPM ----------------------------------------------------------------------------------------------------------------------------------
def decode_png(data):
    """An 8-bit RGB / RGBA PNG whose rows all use filter 0 -> (H, W, C) uint8; checks every chunk's CRC."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (2, 6)
    C = 3 if ctype == 2 else 4
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(H, 1 + W * C)
    assert bool((rows[:, 0] == 0).all())
    return rows[:, 1:].reshape(H, W, C)


@pytest.mark.parametrize("shape", [(27, 22, 3), (27, 22, 4), (1, 1, 3), (1, 1, 4), (5, 7, 3), (3, 1, 3)])      # 7 * 3 = 21, 1 * 3 = 3: rows off a 4-byte multiple
@pytest.mark.parametrize("level", [0, 6, 9])
def test_png_round_trip(shape, level):
    a = np.random.default_rng(sum(shape) + level).integers(0, 256, shape, dtype=np.uint8)
    data = vis.encode_png(a, level)
    assert np.array_equal(decode_png(data), a)
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    assert im.mode == ("RGB" if shape[2] == 3 else "RGBA") and np.array_equal(np.asarray(im), a)


def test_ppm_and_encoder_checks():
    a = np.random.default_rng(3).integers(0, 256, (5, 7, 4), dtype=np.uint8)
    data = vis.encode_ppm(a)
    assert data.startswith(b"P6\n7 5\n255\n") and data[len(b"P6\n7 5\n255\n"):] == a[..., :3].tobytes()
    for bad in (a.astype(np.float32), a[..., :2], a[0], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="encode_png takes"):
            vis.encode_png(bad)


# ---- the writer: names and checks -------------------------------------------------------------------------------------------------------------------
def test_file_names_follow_the_pattern(tmp_path):
    w = vis.ImageWriter(str(tmp_path))
    assert w.path("RENDER", 3, 12) == os.path.join(str(tmp_path), "RENDER", "frame0012_camera0003.png")
    assert w.path("RENDER", 3, 12, "_gt").endswith("RENDER/frame0012_camera0003_gt.png")
    assert w.path("DEPTH", 0, 0, "_error").endswith("DEPTH/frame0000_camera0000_error.png")
    w2 = vis.ImageWriter(str(tmp_path), pattern="{camera:02d}/{type}_{frame:06d}", ext=".ppm")
    assert w2.path("ALPHA", 7, 5) == os.path.join(str(tmp_path), "07", "ALPHA_000005.ppm") and w2.store_alpha_channel is False
    assert w.close() == [] and w2.close() == []


def test_writer_argument_checks(tmp_path):
    for kw, msg in ((dict(ext=".jpg"), "ext must be"), (dict(workers=0), "workers must be"), (dict(compression=10), "compression must be"),
                    (dict(pattern="{type}/{view}"), "pattern must format"), (dict(max_pending=0), "max_pending must be")):
        with pytest.raises(ValueError, match=msg):
            vis.ImageWriter(str(tmp_path), **kw)
    w = vis.ImageWriter(str(tmp_path))
    with pytest.raises(ValueError, match="bytes must be"):
        w.add(torch.zeros(1, 1, 4, 5, 3, dtype=torch.uint8), ["RENDER"], 0, 0)
    with pytest.raises(ValueError, match="bytes must be"):
        w.add(torch.zeros(1, 1, 4, 5, 4), ["RENDER"], 0, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.add(torch.zeros(1, 1, 4, 5, 4, dtype=torch.uint8), ["RENDER"], 0, 0)
    w.close()
    with pytest.raises(RuntimeError, match="closed"):
        w.add(torch.zeros(1, 1, 4, 5, 4, dtype=torch.uint8), ["RENDER"], 0, 0)


# ---- image_planes: argument checks that need no GPU ---------------------------------------------------------------------------------------------------
def test_image_planes_argument_checks():
    img = torch.zeros(4, 5, 3)
    with pytest.raises(ValueError, match="1 to 16 planes"):
        vis.image_planes([], (4, 5))
    with pytest.raises(ValueError, match="1 to 16 planes"):
        vis.image_planes([vis.color(img)] * 17, (4, 5))
    with pytest.raises(TypeError, match="must be a Plane"):
        vis.image_planes([img], (4, 5))
    with pytest.raises(ValueError, match="empty images"):
        vis.image_planes([vis.color(img)], (0, 5))
    with pytest.raises(ValueError, match="leaves the 6 x 6 canvas"):
        vis.image_planes([vis.color(img)], (4, 5), canvas=(6, 6), origin=(2, 0))
    with pytest.raises(ValueError, match="img must be hwc images of 4 x 5 with at least 3 channels"):
        vis.image_planes([vis.color(torch.zeros(4, 5, 2))], (4, 5))
    with pytest.raises(ValueError, match="img must be chw images of 4 x 5"):
        vis.image_planes([vis.color(img, layout="chw")], (4, 5))
    with pytest.raises(ValueError, match="acc must be hwc images of 4 x 5 with 1 channels"):
        vis.image_planes([vis.color(img, acc=torch.zeros(4, 5, 3))], (4, 5))
    with pytest.raises(ValueError, match="one image .3-D. or a batch of images .4-D."):
        vis.image_planes([vis.color(torch.zeros(4, 5))], (4, 5))
    with pytest.raises(ValueError, match="img must be a float tensor, got torch.uint8"):
        vis.image_planes([vis.color(torch.zeros(4, 5, 3, dtype=torch.uint8))], (4, 5))
    with pytest.raises(ValueError, match="gt must be a float tensor or uint8"):
        vis.image_planes([vis.ground_truth(torch.zeros(4, 5, 3, dtype=torch.int32))], (4, 5))
    with pytest.raises(TypeError, match="img must be a tensor"):
        vis.image_planes([vis.color(np.zeros((4, 5, 3), F))], (4, 5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        vis.image_planes([vis.color(img)], (4, 5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        vis.to_bytes(img)
    with pytest.raises(ValueError, match="layout must be"):
        vis.color(img, layout="cwh")
    with pytest.raises(ValueError, match="weight and weight_mode go together"):
        vis.color(img, weight=torch.zeros(4, 5, 1))
    with pytest.raises(ValueError, match="weight_mode must be"):
        vis.color(img, weight=torch.zeros(4, 5, 1), weight_mode="half")
    with pytest.raises(ValueError, match="curve must be"):
        vis.depth(torch.zeros(4, 5, 1), curve="log")
    with pytest.raises(ValueError, match="needs curve='normalize'"):
        vis.depth(torch.zeros(4, 5, 1), curve="linear", table=torch.zeros(4, 3))


def test_c_abi_rejects_bad_arguments_without_a_launch():
    import ctypes
    from envgs_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    hdr = open(os.path.join(vc.ROOT, "include", "envgs_visualize.h")).read()
    assert "ENVGS_VIS_MAX_PLANES %d" % vis.MAX_PLANES in hdr and "ENVGS_VIS_MAX_TABLE %d" % vis.MAX_TABLE in hdr
    for k, name in enumerate(("COLOR", "GRAY", "DEPTH", "NORMAL", "GT", "ERROR")):
        assert "#define ENVGS_VIS_%s %d" % (name, k) in hdr and getattr(vis, name) == k
    assert ctypes.sizeof(_lib.VisMap) == 40 and ctypes.sizeof(_lib.VisPlane) == 40 + 5 * 40 + 24
    fake = ctypes.c_void_p(4096)                                   # never dereferenced: every call below is refused before a launch
    p = (_lib.VisPlane * 1)()
    p[0].kind, p[0].img.ptr = vis.COLOR, 4096
    ok = dict(n=1, B=1, H=4, W=5, Ho=4, Wo=5, x0=0, y0=0, out=fake)
    call = lambda **kw: (lambda a: lib.envgs_visualize_planes(a["n"], p, a["B"], a["H"], a["W"], a["Ho"], a["Wo"], a["x0"], a["y0"], a["out"], None))(dict(ok, **kw))
    for bad in (dict(n=17), dict(n=-1), dict(B=-1), dict(B=65536), dict(H=0), dict(W=0), dict(Ho=3), dict(x0=1), dict(y0=-1), dict(out=None),
                dict(out=ctypes.c_void_p(4098))):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0 and call(B=0) == 0
    for field, value in (("kind", 6), ("weight_mode", 3), ("curve", 2), ("gt_dtype", 2), ("flags", 4)):
        old = getattr(p[0], field); setattr(p[0], field, value)
        assert call() == -1, field
        setattr(p[0], field, old)
    p[0].img.ptr = None
    assert call() == -1                                            # COLOR without img
    p[0].img.ptr, p[0].weight_mode = 4096, 1
    assert call() == -1                                            # a weight mode without a weight
    p[0].weight_mode, p[0].kind = 0, vis.ERROR
    assert call() == -1                                            # ERROR without gt
    p[0].kind, p[0].curve = vis.DEPTH, 1
    assert call() == -1                                            # NORMALIZE without near_far
    p[0].near_far, p[0].table, p[0].table_k = 4096, 4096, 1
    assert call() == -1                                            # a table of one knot
    p[0].kind, p[0].curve = vis.COLOR, 0
    p[0].img.stride[3] = 1 << 31
    assert call() == -1                                            # a column stride beyond an int32
    s = (ctypes.c_int64 * 3)(20, 5, 1)
    rng = lambda **kw: (lambda a: lib.envgs_visualize_depth_range(a["B"], a["H"], a["W"], a["d"], s, a["r0"], a["r1"], a["nf"], a["t"], a["tb"], None))(
        dict(dict(B=1, H=4, W=5, d=fake, r0=0, r1=19, nf=fake, t=fake, tb=lib.envgs_visualize_depth_range_temp_bytes()), **kw))
    for bad in (dict(B=-1), dict(H=0), dict(r0=-1), dict(r1=20), dict(d=None), dict(nf=None), dict(t=None), dict(H=1 << 16, W=1 << 15)):
        assert rng(**bad) == -1, bad
    assert rng(tb=16) == -2 and rng(B=0) == 0
