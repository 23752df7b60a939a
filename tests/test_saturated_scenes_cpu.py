"""CPU: the scenes of tests/saturated_scenes.py do reach what they are built for, in the REFERENCES ALONE (the float64 twins and the C oracles).

These are conditions on the committed seeds and sizes, not tolerances: they keep tests/test_saturated_gpu.py and the saturated cases of
tests/test_independent_f64_gpu.py meaningful.  If one fails after a change of a seed, a size or a builder, change the scene, never the floor or the cap.
The census of every committed scene is printed (pytest -s) and recorded in the error table."""
import numpy as np
import pytest
import torch

from oracle import raster as orc, trace as otr
from tests import saturated_scenes as S
from tests.util import cam_args, rel_err, record, record_fragile, FRAGILE_PX_MAX, CLAMP_RAYS_MAX

RASTER_BG = torch.tensor([0.2, 0.5, 0.9])          # test_raster_parity's
CAPPED_BLENDS_MIN = 20                              # raster: blends with opacity * G > 0.99 on non-audited pixels
CAPPED_RAYS_MIN = {"room600": 100, "room200": 50}   # tracer: rays with such a hit
STOPPED_SHARE_MIN = 0.10                            # scenes of P >= 600: pixels / rays that end on T (1 - alpha) < 1e-4


def oracle_raster(g, cam, sh, deg, bg=RASTER_BG):
    ca = cam_args(cam)
    col = dict(shs=g["shs"].numpy(), sh_degree=deg) if sh else dict(colors_precomp=g["colors_precomp"].numpy())
    return orc.raster_forward(g["means3D"].numpy(), g["opacities"].numpy(), ca["viewmatrix"].numpy(), ca["projmatrix"].numpy(), ca["campos"].numpy(), ca["W"], ca["H"],
                              bg=bg.numpy(), scales=g["scales"].numpy(), rotations=g["rotations"].numpy(), **col)


def audit_trace(g, ro, rd, sff, deg=None, **kw):
    return otr.trace_audit(ro.numpy(), rd.numpy(), g["means3D"].numpy(), g["scales"].numpy(), g["rotations"].numpy(), g["opacities"].numpy(), others=g["others"].numpy(),
                           start_from_first=sff, shs=(g["shs"].numpy() if deg is not None else None), sh_degree=(deg or 0), **kw)


def oracle_trace(g, ro, rd, sff, bg, deg=None):
    ckw = dict(shs=g["shs"].numpy(), sh_degree=deg) if deg is not None else dict(colors_precomp=g["colors_precomp"].numpy())
    return otr.trace_forward(ro.numpy(), rd.numpy(), g["means3D"].numpy(), g["scales"].numpy(), g["rotations"].numpy(), g["opacities"].numpy(), others=g["others"].numpy(),
                             bg=bg.numpy(), start_from_first=sff, **ckw)


@pytest.mark.parametrize("name", list(S.RASTER_CASES))
def test_raster_scene_census_and_audit(name):
    g, cam, c = S.raster_scene(name)
    ref = oracle_raster(g, cam, c["sh"], c["deg"])
    aud = orc.raster_audit(ref)
    cen = S.census_raster(g, cam, sh=c["sh"], sh_degree=c["deg"], exclude=aud["fragile"])
    print(S.census_line("raster " + name, cen))
    test = "saturated_cpu.raster." + name
    record_fragile(test, "fragile_px", aud["fragile"], FRAGILE_PX_MAX)
    record(test, "capped_blends", cen["capped"], "(float64 twin, non-audited pixels; floor %d; %d blends, %d on the low-pass branch)" % (CAPPED_BLENDS_MIN, cen["blends"], cen["lowpass"]))
    record(test, "stopped_px", cen["stopped_px"] / cen["pixels"], "(%d of %d pixels end early)" % (cen["stopped_px"], cen["pixels"]))
    assert cen["capped"] >= CAPPED_BLENDS_MIN, cen["capped"]
    if c["P"] >= 600:
        assert cen["stopped_px"] >= STOPPED_SHARE_MIN * cen["pixels"]
    assert cen["lowpass"] > 0 and cen["blends"] > cen["lowpass"]          # both branches of min(rho3d, rho2d)
    if name == "sphere1500":
        r = ref["ranges"].astype(np.int64)
        assert int((r[:, 1] - r[:, 0]).max()) > 256                        # more than one batch per tile
    if name == "sphere300_f64":
        assert not aud["fragile"].any()                                    # the float64 leg compares EVERY pixel


@pytest.mark.parametrize("name", list(S.TRACE_CASES))
def test_trace_scene_census_and_audit(name):
    g, ro, rd, c = S.trace_scene_of(name)
    a = audit_trace(g, ro, rd, c["camera"], deg=3, detail=True)
    cen = S.census_trace(g, ro, rd, c["camera"])
    print(S.census_line("tracer " + name, cen))
    test = "saturated_cpu.tracer." + name
    clamp = (a["kind"] & otr.KIND_CLAMP) != 0
    record_fragile(test, "fragile_rays.rgb_gradient_zeroed", clamp, CLAMP_RAYS_MAX, "(colour-clamp-fragile rays)")
    record(test, "fragile_rays", float(a["fragile"].mean()), "(%d of %d; recorded only: the doubly-capped stops, compared through their validated lists)" % (int(a["fragile"].sum()), cen["rays"]))
    record(test, "capped_rays", cen["capped_rays"], "(float64 twin; floor %d; %d blends, %d of them capped)" % (CAPPED_RAYS_MIN[name], cen["blends"], cen["capped"]))
    record(test, "stopped_rays", cen["stopped_rays"] / cen["rays"], "(%d of %d rays end early)" % (cen["stopped_rays"], cen["rays"]))
    assert not a["amb_overflow"].any()
    assert cen["capped_rays"] >= CAPPED_RAYS_MIN[name]
    if c["P"] >= 600:
        assert cen["stopped_rays"] >= STOPPED_SHARE_MIN * cen["rays"]
    if name == "room200":
        assert not a["fragile"].any()                                      # the float64 leg compares EVERY ray


def plates_tiles(ref, P):
    """The tiles of the plates scene whose list is longer than one 256-entry batch and in which the third plate (row P - 1) -- where every pixel stops -- sits
    at least one full batch before the list's last batch: [(tile, list length, position of the third plate)]."""
    r = ref["ranges"].astype(np.int64)
    out = []
    for t in range(r.shape[0]):
        n = int(r[t, 1] - r[t, 0])
        pos = np.nonzero(ref["point_list"][r[t, 0]:r[t, 1]] == P - 1)[0]
        if n > 256 and pos.size and pos[0] // 256 < (n - 1) // 256:
            out.append((t, n, int(pos[0])))
    return out


def test_plates_and_crowd_raster():
    g, cam = S.plates_and_crowd_raster()
    P = g["means3D"].shape[0]
    ref = oracle_raster(g, cam, True, 3)
    aud = orc.raster_audit(ref)
    cen = S.census_raster(g, cam, sh=True, sh_degree=3)
    print(S.census_line("raster plates_and_crowd", cen))
    H, W = ref["H"], ref["W"]
    assert not aud["fragile"].any()
    assert cen["stopped_px"] == H * W and int(ref["n_contrib"][0].max()) <= 3
    tiles = plates_tiles(ref, P)
    gx = (W + 15) // 16
    early = np.zeros((H, W), bool)
    for t, n, pos in tiles:
        ty, tx = t // gx, t % gx
        blk = ref["n_contrib"][0][ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
        assert int(blk.max()) <= pos                                       # the last blended entry of every pixel lies in front of the third plate
        early[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    record("saturated_cpu.raster.plates", "tiles_left_early", len(tiles), "(of %d; longest list %d entries)" % (gx * ((H + 15) // 16), max(n for _, n, _ in tiles)))
    assert len(tiles) >= 4
    w_in, _ = orc.raster_weight(ref, ~early)                               # the weights restricted to those tiles
    behind = np.zeros(P, bool)
    r = ref["ranges"].astype(np.int64)
    for t, n, pos in tiles:
        behind[ref["point_list"][r[t, 0] + pos + 1:r[t, 1]]] = True
    assert behind[:P - 3].sum() > 1000 and not behind[P - 3:].any()
    assert np.all(w_in[behind] == 0)


def test_plates_and_crowd_trace():
    g, ro, rd = S.plates_and_crowd_trace()
    a = audit_trace(g, ro, rd, False, deg=3, detail=True)
    cen = S.census_trace(g, ro, rd, False)
    print(S.census_line("tracer plates_and_crowd", cen))
    test = "saturated_cpu.tracer.plates"
    record_fragile(test, "fragile_rays.rgb_gradient_zeroed", (a["kind"] & otr.KIND_CLAMP) != 0, CLAMP_RAYS_MAX, "(colour-clamp-fragile rays)")
    record(test, "fragile_rays", float(a["fragile"].mean()), "(%d of %d; recorded only)" % (int(a["fragile"].sum()), cen["rays"]))
    record(test, "composited_over_accepted", cen["blends"] / cen["accepted"], "(%d of %d accepted hits are composited)" % (cen["blends"], cen["accepted"]))
    assert not a["amb_overflow"].any()
    assert cen["stopped_rays"] >= STOPPED_SHARE_MIN * cen["rays"]
    P = g["means3D"].shape[0]
    ref = oracle_trace(g, ro, rd, False, S.STACK_BG, deg=3)
    up = (rd[:, 2] > 0.5 * rd.norm(dim=-1)).numpy()                       # the rays that go up steeply meet the plates near their centres ...
    assert up.sum() > 100 and np.all(ref["nhits"][up & ~a["fragile"]] <= 40)
    assert ref["wet"][P - 3] > 100 and ref["wet"][P - 2] > 3               # ... and the first two plates carry their weight (the third stops them, unblended)
    assert cen["accepted"] > 3 * cen["blends"]                             # most accepted hits lie behind a stop


def _f32(x):
    return np.float32(x)


def stack_closed_form(colors=None):
    """The (1, 1, 1) stack in fp32: the first blend is capped, the second stops the ray (T (1 - 0.99f) = 9.99998e-5 < 1e-4f) and is NOT composited."""
    a, T = S.ALPHA_CAP32, S.T_AFTER_CAP32
    red = S.STACK_COLORS[0].numpy().astype(np.float32)
    bg = S.STACK_BG.numpy().astype(np.float32)
    return dict(alpha=a, final_T=T, rgb=(a * red + T * bg).astype(np.float32))


def test_the_doubly_capped_stop_is_decided_by_one_rounded_multiply():
    T = S.T_AFTER_CAP32
    assert _f32(T * T) < _f32(1e-4) and float(T) ** 2 < float(_f32(1e-4))
    assert (1e-4 - float(_f32(T * T))) / 1e-4 < 3e-6                       # a relative margin of ~2e-6: any other form of the product can flip it
    assert (1.0 - 0.99) ** 2 > 1e-4                                        # ... as the same expression in double does


@pytest.mark.parametrize("opac", S.STACKS, ids=lambda o: "-".join("%g" % x for x in o))
def test_stack_in_the_trace_oracle(opac):
    g, ro, rd = S.stack_trace(opac)
    ref = oracle_trace(g, ro, rd, False, S.STACK_BG)
    a = audit_trace(g, ro, rd, False)
    R = ro.shape[0]
    if opac == (1.0, 1.0, 1.0):
        cf = stack_closed_form()
        np.testing.assert_array_equal(ref["nhits"], np.full(R, 1))
        np.testing.assert_array_equal(ref["acc"].view(np.uint32), np.full(R, cf["alpha"]).view(np.uint32))
        np.testing.assert_array_equal(ref["final_T"].view(np.uint32), np.full(R, cf["final_T"]).view(np.uint32))
        np.testing.assert_array_equal(ref["rgb"].view(np.uint32), np.tile(cf["rgb"], (R, 1)).view(np.uint32))
        np.testing.assert_array_equal(ref["wet"], np.array([R * float(cf["alpha"]), 0.0, 0.0]))
        assert a["fragile"].all()              # the audit's margin does not know that the product of two caps is ONE rounded multiply: the stack tests assert these rays directly
    else:
        np.testing.assert_array_equal(ref["nhits"], np.full(R, 2))
        assert not a["fragile"].any()
        assert ref["wet"][2] == 0 and ref["wet"][1] > 0


@pytest.mark.parametrize("opac", S.STACKS, ids=lambda o: "-".join("%g" % x for x in o))
def test_stack_in_the_raster_oracle(opac):
    g, cam, central = S.stack_raster(opac)
    ref = oracle_raster(g, cam, False, 0, bg=S.STACK_BG)
    aud = orc.raster_audit(ref)
    cen = S.census_raster(g, cam, sh=False)
    m = central.numpy()
    assert m.sum() == 4
    assert np.all(cen["per_pixel"]["accepted"][m] == 3)
    if opac == (1.0, 1.0, 1.0):
        cf = stack_closed_form()
        assert np.all(ref["n_contrib"][0][m] == 1)
        np.testing.assert_array_equal(ref["final_T"][0][m].view(np.uint32), np.full(4, cf["final_T"]).view(np.uint32))
        np.testing.assert_array_equal(ref["allmap"][1][m].view(np.uint32), np.full(4, np.float32(1.0) - cf["final_T"]).view(np.uint32))
        np.testing.assert_array_equal(ref["out_color"][:, m].view(np.uint32), np.tile(cf["rgb"][:, None], (1, 4)).view(np.uint32))
        assert aud["fragile"][m].all()         # as in the tracer: asserted directly instead
    else:
        assert np.all(ref["n_contrib"][0][m] == 2)
        assert not aud["fragile"][m].any()


def test_float64_leg_scenes_c_oracle_distance():
    """The C oracle's own distance from float64 on the two scenes tests/test_independent_f64_gpu.py adds, in that file's metric and with its upstream
    gradients: at most HALF the leg's bounds (5e-5 values, 2e-4 gradients), so that a GPU failure there is a kernel finding and not the scene's fp32
    conditioning.  Measured: rasterizer 1.2e-5 / 4.0e-5, tracer 6.0e-7 / 2.7e-6."""
    from tests.test_independent_f64_gpu import saturated_raster_leg_inputs, saturated_tracer_leg_inputs, float64_raster, float64_tracer
    # rasterizer
    g, cam, c, bg, dcol, dall = saturated_raster_leg_inputs()
    L64, (c64, r64, a64, w64) = float64_raster(g, cam, True, 3, bg, dcol, dall)
    ref = oracle_raster(g, cam, True, 3, bg=bg)
    rb = orc.raster_backward(ref, dcol.numpy(), dall.numpy())
    np.testing.assert_array_equal(ref["radii"], r64.numpy())
    n = lambda t: t.detach().double().numpy()
    ev = max([rel_err(ref["out_color"], n(c64)), rel_err(ref["weight"], n(w64).reshape(-1))] + [rel_err(ref["allmap"][ch], n(a64[ch])) for ch in range(5)])
    q = g["rotations"].double()
    proj = lambda v: v - (v * q).sum(-1, keepdim=True) * q
    eg = max(rel_err(rb["dmeans3D"], n(L64["means3D"].grad)), rel_err(rb["dscales"], n(L64["scales"].grad)), rel_err(rb["dopacities"], n(L64["opacities"].grad).reshape(-1)),
             rel_err(rb["dshs"], n(L64["shs"].grad)), rel_err(proj(torch.from_numpy(rb["drots"]).double()).numpy(), proj(L64["rotations"].grad).numpy()))
    record("saturated_cpu.float64_leg.raster", "values", ev, "(C oracle against float64 eager, the GPU leg's metric; bound there 5e-5)")
    record("saturated_cpu.float64_leg.raster", "gradients", eg, "(C oracle against float64 autograd; bound there 2e-4)")
    assert ev < 2.5e-5 and eg < 1e-4, (ev, eg)
    # tracer
    g, ro, rd, c, bg, ups = saturated_tracer_leg_inputs()
    L64, o64, d64, outs = float64_tracer(g, ro, rd, True, c["camera"], 3, bg, ups)
    ref = oracle_trace(g, ro, rd, c["camera"], bg, deg=3)
    rb = otr.trace_backward(ref, ups[0].numpy(), ups[1][:, 0].numpy(), ups[2][:, 0].numpy(), ups[3].numpy(), ups[4].numpy())
    ev = max(rel_err(ref[k], n(x)) for k, x in zip(("rgb", "dpt", "acc", "norm", "aux", "wet"), outs))
    q = g["rotations"].double()
    eg = max(rel_err(rb["dmeans3D"], n(L64["means3D"].grad)), rel_err(rb["dscales"], n(L64["scales"].grad)), rel_err(rb["dopacities"], n(L64["opacities"].grad).reshape(-1)),
             rel_err(rb["dshs"], n(L64["shs"].grad)), rel_err(rb["dothers"], n(L64["others"].grad)), rel_err(proj(torch.from_numpy(rb["drots"])).numpy(), proj(L64["rotations"].grad).numpy()),
             rel_err(rb["dray_o"], n(o64.grad)), rel_err(rb["dray_d"], n(d64.grad)))
    record("saturated_cpu.float64_leg.tracer", "values", ev, "(C oracle against float64 eager; bound there 5e-5)")
    record("saturated_cpu.float64_leg.tracer", "gradients", eg, "(C oracle against float64 autograd; bound there 2e-4)")
    assert ev < 2.5e-5 and eg < 1e-4, (ev, eg)
