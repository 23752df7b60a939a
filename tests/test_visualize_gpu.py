"""GPU: envgs_amd.visualize (csrc/visualize.hip) against the NumPy oracle (tests/visualize_oracle.py), byte for byte, and against the reference's
bytes (tests/golden/visualize_golden.npz); shapes around a wavefront and a workgroup, batches, layouts, crops, depth ties and colour tables; the
C-ABI on guard-banded buffers; the writer's files; and visualize_views over the EnvGS forward."""
import ctypes
import os

import numpy as np
import pytest
import torch

from envgs_amd import visualize as vis
from tests import visualize_cases as vc
from tests import visualize_oracle as orc
from tests.test_visualize import decode_png

pytestmark = pytest.mark.gpu
F = np.float32
MAPS = ("img", "weight", "acc", "gt", "msk")


@pytest.fixture(scope="module")
def gold():
    return vc.load()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def to_plane(p, dev, view=None):
    """An oracle plane (NumPy, hwc) as a vis.Plane of device tensors; view(name, tensor) may return another view of the same values (and its layout)."""
    kw = {}
    for name in MAPS:
        if p.get(name) is not None:
            t = torch.from_numpy(np.ascontiguousarray(p[name])).to(dev)
            kw[name] = view(name, t) if view else t
    for name in ("M", "table"):
        if p.get(name) is not None:
            kw[name] = torch.from_numpy(np.ascontiguousarray(p[name], F)).to(dev)
    opaque = bool(p.get("opaque"))
    kind = p["kind"]
    if kind == "color":
        return vis.color(kw["img"], acc=kw.get("acc"), weight=kw.get("weight"), weight_mode=p.get("weight_mode"), opaque=opaque)
    if kind == "gray":
        return vis.gray(kw["img"], acc=kw.get("acc"), opaque=opaque)
    if kind == "depth":
        return vis.depth(kw["img"], acc=kw.get("acc"), curve=p.get("curve", "normalize"), table=kw.get("table"), dpt_mult=p.get("dpt_mult", 1.0), opaque=opaque)
    if kind == "normal":
        return vis.normal(kw["img"], acc=kw.get("acc"), M=kw.get("M"), opaque=opaque)
    if kind == "gt":
        return vis.ground_truth(kw["gt"], msk=kw.get("msk"), bg=p.get("bg"), opaque=opaque)
    return vis.error(kw["img"], kw["gt"], msk=kw.get("msk"), bg=p.get("bg"), acc=kw.get("acc"), weight=kw.get("weight"), weight_mode=p.get("weight_mode"),
                     opaque=opaque)


def run(planes, size, dev, canvas=None, origin=(0, 0), view=None):
    return vis.image_planes([to_plane(p, dev, view) for p in planes], size, canvas, origin).cpu().numpy()


def same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    d = got != want
    if d.any():
        idx = tuple(int(v) for v in np.argwhere(d)[0])
        raise AssertionError("%s: %d of %d bytes differ; first at %s: kernel %d, oracle %d" % (what, int(d.sum()), d.size, idx, got[idx], want[idx]))


def sixteen(B, H, W, seed):
    """Sixteen planes over one set of random maps: every kind, every weight mode and curve, with and without each optional map."""
    g = np.random.default_rng(seed)
    r = lambda *s: g.random(s, dtype=F)
    rgb, env = r(B, H, W, 3) * F(1.2) - F(0.1), r(B, H, W, 3) * F(1.1)
    acc = np.where(r(B, H, W, 1) < 0.3, F(0.0), r(B, H, W, 1)).astype(F)
    spec, msk = r(B, H, W, 1), (r(B, H, W, 1) > 0.4).astype(F) * r(B, H, W, 1).round(1).astype(F)
    dpt = (F(2.0) + r(B, H, W, 1) * F(3.0)) * (acc > 0)
    nrm = g.standard_normal((B, H, W, 3)).astype(F) * acc
    q = np.linalg.qr(g.standard_normal((B, 3, 3)))[0].astype(F)
    gt, gt8 = (np.round(r(B, H, W, 3) * 255) / 255).astype(F), g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    bg, table = np.array([0.2, 0.5, 1.0], F), r(5, 3)
    return [dict(kind="color", img=rgb, acc=acc), dict(kind="color", img=rgb), dict(kind="color", img=rgb, acc=acc, opaque=True),
            dict(kind="color", img=rgb, weight=spec, weight_mode="one_minus", acc=acc), dict(kind="color", img=env, weight=spec, weight_mode="twice", acc=acc),
            dict(kind="gray", img=acc, acc=acc), dict(kind="gray", img=spec),
            dict(kind="depth", img=dpt, curve="linear", dpt_mult=0.25, acc=acc), dict(kind="depth", img=dpt, acc=acc),
            dict(kind="depth", img=dpt, table=table, dpt_mult=0.9),
            dict(kind="normal", img=nrm, M=q, acc=acc), dict(kind="normal", img=nrm),
            dict(kind="gt", gt=gt, msk=msk, bg=bg), dict(kind="gt", gt=gt8), dict(kind="gt", gt=msk, msk=msk, bg=bg),
            dict(kind="error", img=rgb, gt=gt8, msk=msk, bg=bg, acc=acc)]


# ---- the reference's cases ------------------------------------------------------------------------------------------------------------------------
def test_kernel_gives_the_oracle_and_the_reference_bytes_on_the_golden(gold, dev):
    for name, plane, canvas, origin, key in vc.golden_cases(gold):
        H, W = (plane.get("img") if plane.get("img") is not None else plane["gt"]).shape[1:3]
        got = run([plane], (H, W), dev, canvas, origin)[0]
        same_bytes(got, orc.plane_bytes(plane, canvas, origin), name)
        d = np.abs(got.astype(np.int32) - vc.reference_rgba(gold, key).astype(np.int32))
        if name.split("/")[0] in vc.BANDED:
            assert d.max() <= 1 and (d > 0).sum() <= 0.01 * d.size, name
        else:
            assert d.max() == 0, name


# ---- shapes around a wavefront and a workgroup; all sixteen planes in one call ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (27, 22), (3, 63), (3, 64), (3, 65), (2, 257)])
def test_sixteen_planes_in_one_call(H, W, dev):
    planes = sixteen(1, H, W, 100 * H + W)
    assert len(planes) == vis.MAX_PLANES
    got = run(planes, (H, W), dev)
    want = orc.image_planes(planes)
    for t, p in enumerate(planes):
        same_bytes(got[t], want[t], "%dx%d plane %d (%s)" % (H, W, t, p["kind"]))
    same_bytes(run(planes, (H, W), dev), got, "a second call")


def test_every_kind_alone_with_every_optional_map_missing(dev):
    H, W = 7, 5
    full = sixteen(1, H, W, 7)
    bare = [dict(kind="color", img=full[0]["img"]), dict(kind="gray", img=full[6]["img"]), dict(kind="depth", img=full[8]["img"], curve="linear"),
            dict(kind="depth", img=full[8]["img"]), dict(kind="normal", img=full[10]["img"]), dict(kind="gt", gt=full[12]["gt"]),
            dict(kind="gt", gt=full[12]["gt"], msk=full[12]["msk"]), dict(kind="gt", gt=full[12]["gt"], bg=full[12]["bg"]),
            dict(kind="error", img=full[0]["img"], gt=full[12]["gt"]), dict(kind="error", img=full[0]["img"], gt=full[12]["gt"], acc=full[0]["acc"]),
            dict(kind="error", img=full[0]["img"], gt=full[12]["gt"], msk=full[12]["msk"])]
    for p in bare + full:
        got = run([p], (H, W), dev)
        same_bytes(got[0], orc.plane_bytes(p), "%s alone" % p["kind"])
        if p.get("opaque") or (p["kind"] != "gt" and p.get("acc") is None):
            assert bool((got[..., 3] == 255).all())


def test_batch_images_equal_their_single_bytes(dev):
    B, H, W = 3, 9, 13
    planes = sixteen(B, H, W, 11)
    got = run(planes, (H, W), dev)
    want = orc.image_planes(planes)
    same_bytes(got, want, "B = 3")
    for b in range(B):
        one = [{k: (v[b:b + 1] if k in MAPS + ("M",) and v is not None else v) for k, v in p.items()} for p in planes]
        same_bytes(run(one, (H, W), dev)[:, 0], got[:, b], "image %d alone" % b)
    same_bytes(run(planes, (H, W), dev), got, "a second call")


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------------------
def test_layouts_are_read_in_place(dev):
    B, H, W = 2, 6, 10
    planes = sixteen(B, H, W, 13)
    base = run(planes, (H, W), dev)

    def as_chw(name, t):
        c = t.permute(0, 3, 1, 2).contiguous()
        return vis.chw(c)

    def permuted(name, t):                                   # channel-first storage seen as hwc
        v = t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
        assert not v.is_contiguous() or t.shape[-1] == 1
        return v

    def sliced(name, t):                                     # the first channels of a wider image, every second row and column of a larger one
        wide = torch.zeros(t.shape[0], 2 * H, 2 * W, t.shape[3] + 2, dtype=t.dtype, device=t.device)
        wide[:, ::2, ::2, :t.shape[3]] = t
        return wide[:, ::2, ::2, :t.shape[3]]

    def mixed(name, t):
        return as_chw(name, t) if name in ("acc", "weight") else t

    for how in (as_chw, permuted, sliced, mixed):
        same_bytes(run(planes, (H, W), dev, view=how), base, how.__name__)
    # a 4-channel uint8 photograph through its [..., :3] slice, allmap[1:2], and other float dtypes
    gt8 = torch.from_numpy(planes[13]["gt"]).to(dev)
    rgba = torch.cat([gt8, gt8[..., :1]], -1)
    got = vis.image_planes([vis.ground_truth(rgba[..., :3]), vis.ground_truth(rgba)], (H, W)).cpu().numpy()
    same_bytes(got[0], base[13], "[..., :3] of uint8 RGBA"); same_bytes(got[1], base[13], "uint8 RGBA")
    allmap = torch.rand(B, 7, H, W, device=dev)
    a = vis.image_planes([vis.gray(allmap[:, 1:2], layout="chw")], (H, W)).cpu().numpy()
    same_bytes(a[0], orc.plane_bytes(dict(kind="gray", img=allmap[:, 1:2].permute(0, 2, 3, 1).cpu().numpy())), "allmap[1:2]")
    rgb = torch.from_numpy(planes[0]["img"]).to(dev)
    same_bytes(vis.image_planes([vis.color(rgb.double())], (H, W)).cpu().numpy()[0], base[1], "float64 input")
    same_bytes(vis.to_bytes(rgb).cpu().numpy(), base[1], "to_bytes")
    same_bytes(vis.to_bytes(rgb[0], alpha=torch.from_numpy(planes[0]["acc"]).to(dev)[0]).cpu().numpy(), base[0][:1], "to_bytes with alpha")
    out = torch.full((2, B, H, W, 4), 7, dtype=torch.uint8, device=dev)
    assert vis.image_planes([vis.color(rgb), vis.color(rgb)], (H, W), out=out).data_ptr() == out.data_ptr()
    same_bytes(out.cpu().numpy()[1], base[1], "out=")
    with pytest.raises(ValueError, match="out must be"):
        vis.image_planes([vis.color(rgb)], (H, W), out=out)


def test_nan_gives_zero_and_uint8_is_its_float_twin(dev):
    H, W = 4, 16
    every = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, -1)                     # each of the 256 codes
    got = run([dict(kind="gt", gt=every)], (16, 16), dev)
    assert np.array_equal(got[0, 0, ..., 0], every[0, ..., 0])                                       # k / 255 * 255 rounds back to k
    same_bytes(got[0], orc.plane_bytes(dict(kind="gt", gt=every)), "uint8 codes")
    img = np.full((1, H, W, 3), 0.5, F); img[0, 1, 2, 1] = np.nan; img[0, 0, 0, 0] = np.inf; img[0, 0, 1, 0] = -np.inf
    acc = np.ones((1, H, W, 1), F); acc[0, 3, 3, 0] = np.nan
    d = np.linspace(1, 2, H * W, dtype=F).reshape(1, H, W, 1).copy(); d[0, 2, 2, 0] = np.nan
    planes = [dict(kind="color", img=img, acc=acc), dict(kind="error", img=img, gt=np.zeros_like(img), msk=acc, acc=acc), dict(kind="normal", img=img, acc=acc),
              dict(kind="depth", img=d, curve="linear"), dict(kind="depth", img=d, table=np.random.default_rng(1).random((4, 3), dtype=F))]
    got = run(planes, (H, W), dev)
    same_bytes(got, orc.image_planes(planes), "NaN planes")
    assert list(got[0, 0, 1, 2]) == [128, 0, 128, 255] and got[0, 0, 3, 3, 3] == 0 and got[0, 0, 0, 0, 0] == 255 and got[0, 0, 0, 1, 0] == 0
    assert list(got[3, 0, 2, 2, :3]) == [0, 0, 0]


# ---- depth: ties, a flat image, tables on their knots ---------------------------------------------------------------------------------------------------
def test_depth_ties_and_flat_images(dev):
    g = np.random.default_rng(5)
    H, W = 30, 41                                                                                  # N = 1230: n = 12
    ties = g.integers(0, 6, (1, H, W, 1)).astype(F) * F(0.5)                                       # six values, hundreds of ties at both ranks
    flat = np.full((1, H, W, 1), 2.5, F)
    almost = flat.copy(); almost[0, 0, :5, 0] = 9.0; almost[0, 1, :5, 0] = 0.25                     # fewer outliers than n: near == far == 2.5
    zeros = np.zeros((1, H, W, 1), F); zeros[0, ::2] = -0.0
    small = g.random((1, 7, 5, 1), dtype=F)                                                        # N = 35 < 100: n clamped to 1
    for name, d in (("ties", ties), ("flat", flat), ("almost flat", almost), ("signed zeros", zeros), ("under 100 pixels", small)):
        planes = [dict(kind="depth", img=d), dict(kind="depth", img=d, table=g.random((6, 3), dtype=F), dpt_mult=0.8)]
        got = run(planes, d.shape[1:3], dev)
        same_bytes(got, orc.image_planes(planes), name)
    got = run([dict(kind="depth", img=almost)], (H, W), dev)[0, 0]
    assert list(got[0, 0, :3]) == [0, 0, 0] and list(got[1, 0, :3]) == [255, 255, 255] and list(got[5, 5, :3]) == [255, 255, 255]
    # three images of one batch: each normalised on its own
    batch = np.concatenate([ties, flat, almost])
    same_bytes(run([dict(kind="depth", img=batch)], (H, W), dev), orc.image_planes([dict(kind="depth", img=batch)]), "batch of depths")


@pytest.mark.parametrize("K", [2, 9])
def test_table_values_on_the_knots(K, dev):
    # N = 45 < 100: near = min = 0, far = max = 1, so v = 1 - d exactly; d = 1 - k / 8 puts v on the knots of K = 9 (and on 0.5 for K = 2)
    d = np.concatenate([1 - np.arange(9) / 8, np.random.default_rng(K).random(36)]).astype(F).reshape(1, 5, 9, 1)
    assert d.min() == 0 and d.max() == 1
    table = np.random.default_rng(K + 1).random((K, 3), dtype=F)
    planes = [dict(kind="depth", img=d, table=table), dict(kind="depth", img=d, table=table[::-1].copy(), dpt_mult=0.5)]
    got = run(planes, (5, 9), dev)
    same_bytes(got, orc.image_planes(planes), "K = %d" % K)
    if K == 9:
        v = orc.normalize_depth(d[0, 0, 4, 0], F(0), F(1))
        assert v == F(0.5)
        c = orc.colormap_table(np.array([v]), table)[0]
        assert np.array_equal(c, table[4] + table[4])                                              # an inner knot: counted by both segments
        assert list(got[0, 0, 0, 4, :3]) == list(orc.to_byte(c))


# ---- crops ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [(0, 0), (6, 0), (0, 4), (6, 4), (2, 1)])
def test_crops_land_in_a_zero_canvas(origin, dev):
    H, W, canvas = 5, 7, (9, 13)
    planes = sixteen(2, H, W, 17)[:6]
    got = run(planes, (H, W), dev, canvas, origin)
    same_bytes(got, orc.image_planes(planes, canvas, origin), "origin %s" % (origin,))
    x0, y0 = origin
    outside = np.ones(canvas, bool); outside[y0:y0 + H, x0:x0 + W] = False
    assert bool((got[:, :, outside] == 0).all()) and bool((got[:, :, ~outside][..., 3] > 0).any())
    same_bytes(got[:, :, y0:y0 + H, x0:x0 + W], run(planes, (H, W), dev), "the crop itself")


# ---- the C-ABI on guard-banded buffers ------------------------------------------------------------------------------------------------------------------
GUARD, CANARY = 4096, 0xA5


@pytest.mark.parametrize("B,H,W,canvas,origin", [(2, 7, 5, (7, 5), (0, 0)), (1, 1, 1, (1, 1), (0, 0)), (3, 3, 65, (4, 67), (2, 1))])
def test_c_abi_on_guard_banded_buffers(B, H, W, canvas, origin, dev):
    from envgs_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    rgb, acc, dpt = (torch.rand(B, H, W, c, generator=g).to(dev) for c in (3, 1, 1))
    Ho, Wo = canvas
    n = 2 * B * Ho * Wo * 4
    raw = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
    nf_raw = torch.full((2 * B + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    nf = nf_raw[GUARD:GUARD + 2 * B]
    tb = lib.envgs_visualize_depth_range_temp_bytes()
    temp_raw = torch.full((tb + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
    st = _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    r0, r1 = vis.depth_ranks(H * W)
    assert lib.envgs_visualize_depth_range(B, H, W, _lib.ptr(dpt), (ctypes.c_int64 * 3)(H * W, W, 1), r0, r1, ctypes.c_void_p(nf.data_ptr()),
                                           ctypes.c_void_p(temp_raw.data_ptr() + GUARD), tb, st) == 0
    p = (_lib.VisPlane * 2)()
    hwc = lambda c: (ctypes.c_int64 * 4)(H * W * c, 1, W * c, c)
    p[0].kind = vis.COLOR
    p[0].img, p[0].acc = _lib.VisMap(rgb.data_ptr(), hwc(3)), _lib.VisMap(acc.data_ptr(), hwc(1))
    p[1].kind, p[1].curve, p[1].dpt_mult, p[1].near_far = vis.DEPTH, 1, 1.0, nf.data_ptr()
    p[1].img = _lib.VisMap(dpt.data_ptr(), hwc(1))
    assert lib.envgs_visualize_planes(2, p, B, H, W, Ho, Wo, origin[0], origin[1], ctypes.c_void_p(raw.data_ptr() + GUARD), st) == 0
    torch.cuda.synchronize()
    host = raw.cpu().numpy()
    assert bool((host[:GUARD] == CANARY).all()) and bool((host[GUARD + n:] == CANARY).all()), "written outside out"
    t = temp_raw.cpu().numpy()
    assert bool((t[:GUARD] == CANARY).all()) and bool((t[GUARD + tb:] == CANARY).all()), "written outside temp"
    f = nf_raw.cpu().numpy()
    assert bool(np.isnan(f[:GUARD]).all()) and bool(np.isnan(f[GUARD + 2 * B:]).all()) and not np.isnan(f[GUARD:GUARD + 2 * B]).any()
    planes = [dict(kind="color", img=rgb.cpu().numpy(), acc=acc.cpu().numpy()), dict(kind="depth", img=dpt.cpu().numpy())]
    same_bytes(host[GUARD:GUARD + n].reshape(2, B, Ho, Wo, 4), orc.image_planes(planes, canvas, origin), "C-ABI")
    want_nf = np.array([orc.depth_range(d) for d in dpt.cpu().numpy()], F)
    assert np.array_equal(f[GUARD:GUARD + 2 * B].reshape(B, 2), want_nf)


# ---- the writer ---------------------------------------------------------------------------------------------------------------------------------------
def test_writer_files_decode_to_the_bytes(tmp_path, dev):
    B, H, W = 2, 9, 7                                                                             # 7 * 3 = 21: a row off a 4-byte multiple
    planes = sixteen(B, H, W, 23)
    data = vis.image_planes([to_plane(p, dev) for p in (planes[0], planes[12], planes[15])], (H, W))
    want = data.cpu().numpy()
    with vis.ImageWriter(str(tmp_path / "a"), workers=2, max_pending=1) as w:
        paths = w.add(data, ["RENDER", ("RENDER", "_gt"), ("RENDER", "_error")], camera=[4, 5], frame=9)
        more = w.add(data[:1], ["ALPHA"], camera=[4, 5], frame=10)                                 # a second copy in flight: the first is drained
        assert len(paths) == 6 and len(more) == 2
    names = sorted(os.path.relpath(p, str(tmp_path / "a")) for p in w.written)
    assert names == sorted(["RENDER/frame0009_camera%04d%s.png" % (c, s) for c in (4, 5) for s in ("", "_gt", "_error")]
                           + ["ALPHA/frame0010_camera%04d.png" % c for c in (4, 5)])
    for t, s in enumerate(("", "_gt", "_error")):
        for b, c in enumerate((4, 5)):
            got = decode_png(open(str(tmp_path / "a" / "RENDER" / ("frame0009_camera%04d%s.png" % (c, s))), "rb").read())
            assert np.array_equal(got, want[t, b])
    with vis.ImageWriter(str(tmp_path / "b"), store_alpha_channel=False, compression=0) as w:
        w.add(data[:1, :1], ["RENDER"], 0, 0)
    assert np.array_equal(decode_png(open(w.written[0], "rb").read()), want[0, 0, ..., :3])
    with vis.ImageWriter(str(tmp_path / "c"), ext=".ppm") as w:
        w.add(data[:1, :1], ["RENDER"], 0, 0)
    raw = open(w.written[0], "rb").read()
    assert raw.startswith(b"P6\n7 9\n255\n") and raw[11:] == want[0, 0, ..., :3].tobytes()
    with pytest.raises(ValueError, match="2 types for 3 planes"):
        vis.ImageWriter(str(tmp_path / "d")).add(data, ["A", "B"], 0, 0)
    with pytest.raises(ValueError, match="camera has 3 labels for 2 images"):
        vis.ImageWriter(str(tmp_path / "d")).add(data, ["A", "B", "C"], [1, 2, 3], 0)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------------------
def test_visualize_views_writes_the_expected_files(tmp_path, dev):
    import diff_surfel_rasterization_wet_ch05 as pkg
    import diff_surfel_tracing as tpkg
    from envgs_amd import envgs_step, fused, synth
    H, W = 48, 64
    base = synth.base_gaussians(2000, seed=3)
    base["scales"] = base["scales"] * 5.0
    env = synth.env_gaussians(2000, seed=4, bound=12.0)
    base, env = ({k: v.to(dev) for k, v in d.items()} for d in (base, env))
    cams = [synth.orbit_camera(v, H=H, W=W, fx=1111.1 * W / 800.0, device=dev) for v in (1, 4)]
    bg, env_bg, deg = torch.zeros(3, device=dev), torch.tensor([0.1, 0.2, 0.3], device=dev), 3
    g = torch.Generator().manual_seed(5)
    photos = [torch.randint(0, 256, (H, W, 4), generator=g, dtype=torch.uint8).to(dev) for _ in cams]
    masks = [torch.rand(H, W, 1, generator=g).round().to(dev) for _ in cams]
    was = envgs_step.FUSED["on"]
    envgs_step.FUSED["on"] = True
    try:
        tracer = tpkg.SurfelTracer()
        with vis.ImageWriter(str(tmp_path)) as w:
            paths = vis.visualize_views(cams, base, env, deg, bg, env_bg, w, images=photos, masks=masks, labels=[(7, 0), (8, 2)], gt_bg=(0.0, 0.0, 0.0),
                                        tracer=tracer)
        with torch.no_grad():
            out = envgs_step.envgs_forward(pkg, tpkg, tracer, cams[1], synth.get_rays(cams[1]), base, env, bg, env_bg, deg)
            out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
            planes, names = vis.view_planes(out, cams[1], image=photos[1], mask=masks[1], gt_bg=(0.0, 0.0, 0.0))
            want = vis.image_planes(planes, (H, W)).cpu().numpy()
            surf_depth, _ = fused.surface_normal(out["base"]["allmap"], cams[1], 0.0)
    finally:
        envgs_step.FUSED["on"] = was
    rel = sorted(os.path.relpath(p, str(tmp_path)) for p in paths)
    expect = sorted("%s/frame%04d_camera%04d%s.png" % (t, f, c, s) for c, f in ((7, 0), (8, 2))
                    for t, s in [(t, "") for t in vis.TYPES] + [("RENDER", "_gt"), ("RENDER", "_error")])
    assert rel == expect and len(rel) == 20
    found = sorted(os.path.relpath(os.path.join(d, f), str(tmp_path)) for d, _, fs in os.walk(str(tmp_path)) for f in fs)
    assert found == expect
    assert names == [("RENDER", ""), ("RENDER", "_gt"), ("RENDER", "_error")] + [(t, "") for t in vis.TYPES[1:]]
    for (t, s), plane in zip(names, want):
        got = decode_png(open(str(tmp_path / t / ("frame0002_camera0008%s.png" % s)), "rb").read())
        assert got.shape == (H, W, 4) and np.array_equal(got, plane[0]), (t, s)
    # the pictures are the oracle's, from the forward's own tensors
    rgb, acc = out["rgb"].cpu().numpy()[None], out["base"]["allmap"][1:2].permute(1, 2, 0).cpu().numpy()[None]
    same_bytes(want[0], orc.plane_bytes(dict(kind="color", img=rgb, acc=acc)), "RENDER")
    same_bytes(want[1], orc.plane_bytes(dict(kind="gt", gt=photos[1][..., :3].cpu().numpy()[None], msk=masks[1].cpu().numpy()[None], bg=np.zeros(3, F))), "RENDER_gt")
    same_bytes(want[3], orc.plane_bytes(dict(kind="depth", img=surf_depth.permute(1, 2, 0).cpu().numpy()[None], acc=acc)), "DEPTH")
    same_bytes(want[4], orc.plane_bytes(dict(kind="gray", img=acc, acc=acc)), "ALPHA")
    assert want[0][..., :3].std() > 5 and want[3][..., :3].std() > 0                                     # pictures, not constants
