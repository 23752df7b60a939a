"""envgs_amd.model (include/envgs_model.h): raw surfel parameters -> the extensions' inputs, one launch each way.

CPU: the interface refuses what it cannot run (CPU tensors, inconsistent shapes, bad sizes at the C boundary).
GPU: the reference getters' own outputs (tests/golden/model_golden.pt), parity with the torch twin (ckpt.activate + the colour expression of
test_sh_colors_matches_torch + cat(sigmoid, sigmoid) + synth.get_disks) forward and backward, a float64 check of the rotation and sigmoid
gradients, the exact zeros FusedAdam's sparse update relies on, NULL upstreams, and one EnvGS step fed through the new keys of envgs_step."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from envgs_amd import ckpt, envgs_step, synth
from tests.util import TOL, check_close, small_scene

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_golden.pt")
RAW7 = ("_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_specular", "_roughness")
SIZES = (1, 3, 65, 257, 5000)              # a partial quad, a partial wave, a workgroup border (64 surfels per workgroup), several workgroups
LAYOUTS = ((0, 1), (0, 16), (1, 4), (1, 9), (2, 9), (2, 16), (3, 16))          # (D, M)


def raw_set(P, M=16, S=1, deg=3, seed=0, device="cpu"):
    """synth.base_gaussians pushed through the inverse activations: log scaling, a quaternion of length 0.5 .. 1.5, logit opacity / specular /
    roughness; the coefficients of tests/test_sh_degree_ladder.py:ladder_shs (large beyond the active degree, a sixth of the DCs clamp)."""
    from tests.test_sh_degree_ladder import ladder_shs
    g = synth.base_gaussians(P, seed=seed)
    gen = torch.Generator().manual_seed(1000 + seed)
    shs = ladder_shs(g["shs"], deg)[:, :M]
    raw = {"_xyz": g["means3D"], "_features_dc": shs[:, :1], "_features_rest": shs[:, 1:], "_scaling": torch.log(g["scales"]),
           "_rotation": g["rotations"] * (0.5 + torch.rand(P, 1, generator=gen)), "_opacity": torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4))}
    if S:
        raw["_specular"] = torch.logit(g["specular"]) + 0.5 * torch.randn(P, S, generator=gen)
        raw["_roughness"] = torch.randn(P, 1, generator=gen)
    return {k: v.to(device).contiguous() for k, v in raw.items()}


def leaves_of(raw, dtype=None, device=None):
    return {k: v.detach().to(device=device or v.device, dtype=dtype or v.dtype).clone().requires_grad_(True) for k, v in raw.items()}


def twin(raw, campos=None, deg=None):
    """The torch path of today on whatever device / dtype `raw` has: every output the three functions produce, by their public names."""
    a = ckpt.activate(raw)
    out = {k: a[k] for k in ("shs", "scales", "rotations", "opacities")}
    S = raw["_specular"].shape[1] if "_specular" in raw else 0
    if S:
        out["specular"], out["roughness"] = a["specular"], a["roughness"]
    if S == 1:
        out["others_precomp"] = torch.cat([a["specular"], a["roughness"]], dim=-1)
    if campos is not None:
        d = raw["_xyz"] - campos[None]; d = d / d.norm(dim=1, keepdim=True)
        rgb = torch.clamp_min(envgs_step.eval_sh(deg, a["shs"].transpose(1, 2), d) + 0.5, 0.0)
        out["colors_precomp"] = torch.cat([rgb, a["specular"], a["roughness"]], dim=-1) if S else rgb
    out["v"] = synth.get_disks(raw["_xyz"], a["scales"], a["rotations"])[0]
    return out


def fused_all(raw, campos, deg):
    """The three public functions on the same leaves: {function: its dict}."""
    from envgs_amd import model
    return dict(activate=model.activate(raw), raster=model.raster_inputs(raw, campos, torch.tensor([deg], device=campos.device)), tracer=model.tracer_inputs(raw))


DIFF = dict(activate=("shs", "scales", "rotations", "opacities", "specular", "roughness"), raster=("colors_precomp", "opacities", "scales", "rotations"),
            tracer=("shs", "opacities", "scales", "rotations", "others_precomp"))


def weighted_losses(f, t, seed, zero_rows=None):
    """sum over every differentiable output of every function of <w, output> with a random w per output (rows zero_rows zeroed), for the fused
    dicts f and the twin t -> (loss_fused, loss_twin)."""
    gen = torch.Generator().manual_seed(seed)
    lf = lt = 0.0
    for fn, keys in DIFF.items():
        for k in keys:
            if k not in f[fn]:
                continue
            w = torch.randn(t[k].shape, generator=gen).to(t[k].device)
            if zero_rows is not None:
                w[zero_rows] = 0
            lf = lf + (f[fn][k] * w).sum(); lt = lt + (t[k] * w).sum()
    return lf, lt


def grad_or_zero(t):
    return t.grad if t.grad is not None else torch.zeros_like(t)


# ---------------------------------------------------------------------------------------------------------------------------------------- CPU
def test_model_module_imports():
    from envgs_amd import model
    assert all(callable(getattr(model, n)) for n in ("activate", "raster_inputs", "tracer_inputs"))


def test_cpu_tensors_and_bad_shapes_are_refused():
    from envgs_amd import model
    raw = raw_set(8)
    cam = torch.zeros(3)
    calls = (lambda r: model.activate(r), lambda r: model.raster_inputs(r, cam, 3), lambda r: model.tracer_inputs(r))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(raw)
        bad = dict(raw, _opacity=raw["_opacity"][:5])                                   # inconsistent row counts
        with pytest.raises(ValueError):
            call(bad)
        bad = dict(raw, _features_rest=torch.zeros(8, 16, 3))                           # 17 coefficients
        with pytest.raises(ValueError):
            call(bad)
    with pytest.raises(ValueError):
        model.tracer_inputs(raw_set(8, S=3), others=True)
    with pytest.raises(ValueError):
        model.raster_inputs(raw_set(8, M=4, deg=1), cam, 2)                             # degree 2 needs 9 coefficients


def test_c_entry_points_validate_sizes_before_any_gpu_work():
    from envgs_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    ok = dict(P=10, sh_degree=1, sh_coeffs=4, spec_channels=1)
    for fn in (lib.envgs_surfel_inputs_forward, lib.envgs_surfel_inputs_backward):
        for bad in (dict(P=-1), dict(sh_degree=4), dict(sh_degree=-1), dict(sh_degree=2, sh_coeffs=8), dict(sh_coeffs=17), dict(spec_channels=2)):
            a = _lib.SurfelInputsArgs(**dict(ok, **bad))
            assert fn(a, None) == -1, bad
        assert fn(_lib.SurfelInputsArgs(**dict(ok, P=0)), None) == 0                     # nothing to do: no pointer is looked at, nothing is launched
    # the struct is what the header declares: four int32 and then pointers only, in the header's order
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "envgs_model.h")).read()
    body = hdr[hdr.index("typedef struct envgs_surfel_inputs_args"):hdr.index("} envgs_surfel_inputs_args")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for grp in re.findall(r"(?:int32_t|const float|float|uint8_t)\s+([\w\s,\*]+);", body) for n in grp.split(",")]
    assert names == [n for n, _ in _lib.SurfelInputsArgs._fields_]
    assert ctypes.sizeof(_lib.SurfelInputsArgs) == 16 + 8 * (len(names) - 4)


# ---------------------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_activate_reproduces_the_reference_getters():
    from envgs_amd import model
    dev = torch.device("cuda:0")
    blob = torch.load(GOLD, weights_only=True)
    sets, _ = ckpt.load_model_pt(GOLD, device=dev)
    for name, P in (("pcd", 24), ("env", 16)):
        raw = {k: v for k, v in sets[name].items() if k in ckpt.PT_PARAMS}
        assert raw["_xyz"].shape[0] == P
        a = model.activate(raw)
        assert set(a) == set(blob["activated"][name])
        for k, ref in blob["activated"][name].items():
            ref = ref.to(dev)
            if k in ("means3D", "shs"):
                assert torch.equal(a[k], ref), (name, k)
            else:
                torch.testing.assert_close(a[k], ref, rtol=1e-5, atol=1e-6, msg=lambda m: "%s %s: %s" % (name, k, m))
        assert a["means3D"] is raw["_xyz"]


@pytest.mark.gpu
@pytest.mark.parametrize("S", (0, 1, 3))
@pytest.mark.parametrize("D,M", LAYOUTS)
@pytest.mark.parametrize("P", SIZES)
def test_parity_with_the_torch_twin(P, D, M, S):
    from envgs_amd import fused
    dev = torch.device("cuda:0")
    raw0 = raw_set(P, M, S, D, seed=D + 4 * (M % 5), device=dev)
    campos = synth.orbit_camera(1, device=dev).camera_center
    lf_, lt_ = leaves_of(raw0), leaves_of(raw0)
    f, t = fused_all(lf_, campos, D), twin(lt_, campos, D)
    for fn, d in f.items():
        assert d["means3D"] is lf_["_xyz"]
        for k, v in d.items():
            if k in ("means3D", "f"):
                continue
            assert v.shape == t[k].shape, (fn, k)
            torch.testing.assert_close(v, t[k], rtol=1e-5, atol=1e-6, msg=lambda m: "%s %s: %s" % (fn, k, m))
    assert ("others_precomp" in f["tracer"]) == (S == 1) and f["raster"]["colors_precomp"].shape == (P, 3 + S + 1 if S else 3)
    assert torch.equal(f["tracer"]["f"].long(), synth.get_disks(raw0["_xyz"], t["scales"].detach(), t["rotations"].detach())[1].long())
    assert not f["tracer"]["v"].requires_grad
    v2, _ = fused.surfel_quads(raw0["_xyz"], torch.exp(raw0["_scaling"]), torch.nn.functional.normalize(raw0["_rotation"], dim=-1))
    torch.testing.assert_close(f["tracer"]["v"], v2, rtol=1e-5, atol=1e-6)
    if M == 16:
        sp = torch.sigmoid(raw0["_specular"]) if S else torch.zeros(P, 1, device=dev)
        ro = torch.sigmoid(raw0["_roughness"]) if S else torch.zeros(P, 1, device=dev)
        c2 = fused.sh_colors(raw0["_xyz"], torch.cat([raw0["_features_dc"], raw0["_features_rest"]], dim=1), campos, D, sp, ro)
        torch.testing.assert_close(f["raster"]["colors_precomp"][:, :3], c2[:, :3], rtol=1e-5, atol=1e-6)
    if P >= 6:
        rgb = f["raster"]["colors_precomp"][:, :3]
        assert (rgb[:P // 6] == 0).any() and (rgb[P // 6:] > 0).any()                   # the clamp (and its zero gradient) is exercised
    a, b = weighted_losses(f, t, seed=P + D)
    a.backward(); b.backward()
    for k in lf_:
        torch.testing.assert_close(lf_[k].grad, grad_or_zero(lt_[k]), rtol=1e-4, atol=1e-6, msg=lambda m: "d %s: %s" % (k, m))
    nb = (D + 1) ** 2
    if M > nb:
        # beyond the active degree only the shs upstreams arrive: the colour path contributes exactly nothing
        lf2 = leaves_of(raw0)
        fused_all(lf2, campos, D)["raster"]["colors_precomp"].sum().backward()
        assert float(lf2["_features_rest"].grad[:, nb - 1:].abs().max()) == 0.0
        if nb > 1:
            assert float(lf2["_features_rest"].grad[:, :nb - 1].abs().max()) > 0


def _rotation_floor(q, g):
    """sum |term| of d_rotation = (g - q^ (q^.g)) / |q|, elementwise: (|g| + |q^| |q^.g|) / |q|."""
    n = q.norm(dim=-1, keepdim=True); h = q / n
    return (g.abs() + h.abs() * (h * g).sum(-1, keepdim=True).abs()) / n


@pytest.mark.gpu
def test_rotation_and_sigmoid_gradients_against_float64():
    """check_close at TOL with floor_i = sum |term| of each gradient element: a and b are divided by floor_i and compared with floor 1, which is
    |a - b| / (|b| + floor_i).  A sigmoid gradient is the single term g s (1 - s), its own floor.  Where float32 saturates the sigmoid (raw +20,
    +-100: 1 + exp(-x) rounds to 1, or exp(-x) overflows) torch's float32 gradient is exactly 0 while the float64 one is not: those elements cannot
    meet a relative bound in any float32 implementation; they are asserted to be exactly 0, as torch's are, and kept out of the relative check.
    The float32 torch twin is held to the same bound first, on the CPU, so that the bound is known to be attainable on these inputs."""
    from envgs_amd import model
    dev = torch.device("cuda:0")
    P = 1000
    raw0 = raw_set(P, 16, 1, 3, seed=11)
    raw0["_opacity"][:4, 0] = torch.tensor([20.0, -20.0, 100.0, -100.0])
    raw0["_specular"][:4, 0] = torch.tensor([-100.0, 100.0, -20.0, 20.0])
    raw0["_roughness"][:4, 0] = torch.tensor([100.0, 20.0, -100.0, -20.0])
    raw0["_scaling"][4, 0], raw0["_scaling"][5, 1] = -87.0, 80.0
    gen = torch.Generator().manual_seed(5)
    names = {"_rotation": "rotations", "_opacity": "opacities", "_specular": "specular", "_roughness": "roughness"}
    w = {o: torch.randn(P, 4 if o == "rotations" else 1, generator=gen) for o in names.values()}
    w["scales"] = torch.randn(P, 2, generator=gen)

    def run(raw, act, dtype, device):
        out = act(raw)
        sum((out[o] * w[o].to(device=device, dtype=dtype)).sum() for o in w).backward()
        return out

    l64 = leaves_of(raw0, dtype=torch.float64); run(l64, ckpt.activate, torch.float64, "cpu")
    l32 = leaves_of(raw0); run(l32, ckpt.activate, torch.float32, "cpu")
    lg = leaves_of(raw0, device=dev); out = run(lg, model.activate, torch.float32, dev)
    tr = model.tracer_inputs(leaves_of(raw0, device=dev))
    for k, v in list(out.items()) + [("v", tr["v"]), ("others_precomp", tr["others_precomp"])]:
        assert bool(torch.isfinite(v).all()), k
    sc = out["scales"].detach()
    assert float(sc[5, 1]) == pytest.approx(math.exp(80.0), rel=1e-5) and float(sc[4, 0]) == pytest.approx(math.exp(-87.0), rel=1e-5)
    for k in lg:
        if k != "_xyz":
            assert bool(torch.isfinite(lg[k].grad).all()), k
    torch.testing.assert_close(lg["_scaling"].grad.cpu(), l32["_scaling"].grad, rtol=1e-4, atol=1e-6)
    floors = {"_rotation": _rotation_floor(l64["_rotation"].detach(), w["rotations"].double())}
    for k in ("_opacity", "_specular", "_roughness"):
        floors[k] = l64[k].grad.abs()
    for k, o in names.items():
        b = l64[k].grad
        sat = l32[k].grad == 0                                      # float32 saturation (sigmoids only; a rotation gradient is never exactly 0 here)
        assert int(sat.sum()) == (0 if k == "_rotation" else 3), (k, int(sat.sum()))
        fl = torch.where(sat, torch.ones_like(b), floors[k]).numpy()
        keep = ~sat.numpy()
        for who, a in (("float32 torch twin (CPU)", l32[k].grad), ("model.activate", lg[k].grad.cpu())):
            assert bool((a[sat] == 0).all()), (who, k)
            check_close("test_rotation_and_sigmoid_gradients_against_float64", "d %s, %s" % (k, who), a.double().numpy() / fl, b.numpy() / fl, tol=TOL,
                        keep=keep, floor=1.0)


@pytest.mark.gpu
def test_zero_upstream_rows_give_exactly_zero_raw_gradients():
    dev = torch.device("cuda:0")
    P = 1000
    raw0 = raw_set(P, 16, 1, 3, seed=2, device=dev)
    campos = synth.orbit_camera(1, device=dev).camera_center
    lv = leaves_of(raw0)
    f = fused_all(lv, campos, 3)
    rows = torch.arange(0, P, 3, device=dev)
    lf, _ = weighted_losses(f, twin(raw0, campos, 3), seed=1, zero_rows=rows)
    lf.backward()
    for k in RAW7 + ("_xyz",):
        g = lv[k].grad
        assert bool((g[rows] == 0).all()), k
        other = torch.ones(P, dtype=torch.bool, device=dev); other[rows] = False
        hit = (g[other].reshape(int(other.sum()), -1) != 0).any(dim=1)                      # (and the other rows did receive one; a surfel whose
        assert bool(hit.any() if k == "_xyz" else hit.all()), k                             #  three colours clamp has no view-direction term)


@pytest.mark.gpu
@pytest.mark.parametrize("fn,key", [("activate", k) for k in DIFF["activate"]] + [("raster", "colors_precomp"), ("tracer", "others_precomp")])
def test_one_output_alone_reaches_the_loss(fn, key):
    """Every other upstream of the function arrives as NULL; raw tensors the output does not depend on get zeros."""
    dev = torch.device("cuda:0")
    P = 257
    raw0 = raw_set(P, 16, 1, 2, seed=6, device=dev)
    campos = synth.orbit_camera(1, device=dev).camera_center
    lv, lt = leaves_of(raw0), leaves_of(raw0)
    f, t = fused_all(lv, campos, 2), twin(lt, campos, 2)
    w = torch.randn(t[key].shape, generator=torch.Generator().manual_seed(3)).to(dev)
    (f[fn][key] * w).sum().backward(); (t[key] * w).sum().backward()
    depends = {"shs": ("_features_dc", "_features_rest"), "scales": ("_scaling",), "rotations": ("_rotation",), "opacities": ("_opacity",),
               "specular": ("_specular",), "roughness": ("_roughness",), "others_precomp": ("_specular", "_roughness"),
               "colors_precomp": ("_xyz", "_features_dc", "_features_rest", "_specular", "_roughness")}[key]
    for k in RAW7 + (("_xyz",) if key == "colors_precomp" else ()):
        assert lv[k].grad is not None, k
        torch.testing.assert_close(lv[k].grad, grad_or_zero(lt[k]), rtol=1e-4, atol=1e-6, msg=lambda m: "d %s: %s" % (k, m))
        assert (float(lv[k].grad.abs().max()) > 0) == (k in depends), k
    if key != "colors_precomp":
        assert lv["_xyz"].grad is None


@pytest.mark.gpu
def test_step_through_the_new_keys_matches_the_activated_step():
    """One EnvGS forward + backward (-ch05, degree 3, 64 x 80, 400 base surfels) from the same raw leaves: fed through ckpt.activate as today, and
    through model.raster_inputs / model.tracer_inputs with colors_precomp and v taken by envgs_step's new keys."""
    import diff_surfel_rasterization_wet_ch05 as pkg
    import diff_surfel_tracing as tpkg
    from envgs_amd import model
    dev = torch.device("cuda:0")
    g, _ = small_scene(P=400, H=64, W=80, seed=0)
    cam = synth.orbit_camera(1, H=64, W=80, fx=1111.1 * 80 / 800.0, device=dev)
    e = synth.env_gaussians(800, seed=4, bound=12.0)
    inv = lambda d: {"_xyz": d["means3D"], "_features_dc": d["shs"][:, :1], "_features_rest": d["shs"][:, 1:], "_scaling": torch.log(d["scales"]),
                     "_rotation": d["rotations"] * 1.3, "_opacity": torch.logit(d["opacities"].clamp(1e-4, 1 - 1e-4))}
    raw_b = dict(inv(g), _specular=torch.logit(g["specular"]), _roughness=torch.logit(g["roughness"]))
    raw_e = inv(e)
    rays = synth.get_rays(cam)
    bg = torch.zeros(3, device=dev); env_bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    gen = torch.Generator().manual_seed(7)
    dcol = (torch.randn(64, 80, 3, generator=gen) / (64 * 80)).to(dev)
    dall = (torch.randn(7, 64, 80, generator=gen) / (64 * 80)).to(dev); dall[5:] = 0
    deg = torch.tensor([3], device=dev)
    was = envgs_step.FUSED["on"]
    res = {}
    try:
        envgs_step.FUSED["on"] = True
        for form in ("activated", "model"):
            lb = leaves_of({k: v.contiguous() for k, v in raw_b.items()}, device=dev)
            le = leaves_of({k: v.contiguous() for k, v in raw_e.items()}, device=dev)
            if form == "activated":
                base, env = ckpt.activate(lb), ckpt.activate(le)
            else:
                base, env = model.raster_inputs(lb, cam.camera_center, deg), model.tracer_inputs(le)
                assert "colors_precomp" in base and "shs" not in base and "v" in env and "others_precomp" not in env
            out = envgs_step.envgs_forward(pkg, tpkg, tpkg.SurfelTracer(), cam, rays, base, env, bg, env_bg, deg)
            ((out["rgb"] * dcol).sum() + (out["base"]["allmap"] * dall).sum()).backward()
            torch.cuda.synchronize()
            res[form] = (out["rgb"].detach().clone(), {"base." + k: v.grad.clone() for k, v in lb.items()} | {"env." + k: v.grad.clone() for k, v in le.items()})
    finally:
        envgs_step.FUSED["on"] = was
    err = float((res["model"][0] - res["activated"][0]).abs().max())
    print("rgb: max |model - activated| = %.3g" % err)
    assert err <= 1e-6
    for k, b in res["activated"][1].items():
        a = res["model"][1][k]
        d, m = float((a - b).abs().max()), float(b.abs().max())
        print("%-24s max |diff| %.3g  max |grad| %.3g" % (k, d, m))
        assert d <= 1e-4 * m and (m > 0 or k == "base._roughness"), k                    # (nothing in this loss reads the roughness channel)
