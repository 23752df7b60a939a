"""Seeded scenes in the regime EnvGS trains towards, and a census of what the compositing does on them (a plain module, CPU tensors only).

Every other parity scene of the suite (synth.base_gaussians, synth.env_gaussians, tests/test_oracle_trace.py:trace_scene) is a random-initialisation
cloud: uniform positions, random quaternions, opacities around 0.5 or far below.  On none of them does a blend reach the alpha cap (ALPHA_CAP = 0.99),
and pixels and rays end, if at all, after ~100 translucent hits.  A trained scene is the opposite: surfels lie ON surfaces with aligned normals, their
opacities saturate at 1, and a pixel or ray ends after two or three hits.  The builders here return the dict layout of tests/util.py:small_scene and
trace_scene:

  surface_object   rasterizer: a unit sphere of surfels (40 % of them at opacity exactly 1.0f), faint floaters in front of it
  room             tracer: the same construction at radius 4 with inward normals, rays from inside, some re-aimed at the cap zone of opaque wall surfels
  plates_and_crowd both: three large surfels of opacity 0.97 one behind the other in front of a crowd -- every covered pixel / ray stops at the third
                   plate, a factor 3.7 away from the termination threshold, with a long list behind it that must never be touched
  stack            both: three surfels on one axis, for the stop decision itself (two capped blends: T (1 - alpha) = 9.99998e-5 < 1e-4)

census_raster / census_trace count, on the float64 twins (oracle/eager.py, oracle/eager_trace.py: stats=), how often each scene reaches the cap, the
termination and the low-pass branch; tests/test_saturated_scenes_cpu.py asserts the floors that keep the GPU tests meaningful."""
import math

import numpy as np
import torch

from envgs_amd import synth

ALPHA_CAP32 = np.float32(0.99)
T_AFTER_CAP32 = np.float32(1.0) - ALPHA_CAP32            # 0.0099999905: the transmittance a capped first blend leaves


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def quat_from_normal(n, spin):
    """Unit quaternions (r, x, y, z) whose rotation takes +z to the unit vectors `n`, after a rotation by `spin` radians about z."""
    align = torch.stack([1.0 + n[:, 2], -n[:, 1], n[:, 0], torch.zeros_like(n[:, 0])], dim=-1)       # the shortest arc from z to n
    flip = align.norm(dim=-1) < 1e-6                                                                # n == -z: half a turn about x
    align[flip] = torch.tensor([0.0, 1.0, 0.0, 0.0])
    r1, x1, y1, z1 = _unit(align).unbind(-1)
    c, s = torch.cos(0.5 * spin), torch.sin(0.5 * spin)                                              # (c, 0, 0, s)
    return torch.stack([r1 * c - z1 * s, x1 * c + y1 * s, y1 * c - x1 * s, r1 * s + z1 * c], dim=-1)


def _log_uniform(gen, n, lo, hi):
    return torch.exp(math.log(lo) + torch.rand(n, generator=gen) * (math.log(hi) - math.log(lo)))


def _shell(P, gen, radius, inward, major, floater_radius, opaque_share=0.4):
    """Surfels on a sphere of `radius` (0.4 % radial noise), normals radial (+ 0.05 noise; pointing inwards if `inward`), a random spin; major scale
    log-uniform in `major`, minor = major / log-uniform(1, 8); raw opacity N(3, 1.5), `opaque_share` of the surface rows at raw 20 (1.0f after the
    sigmoid); the first eighth are floaters at `floater_radius` with opacity 0.01..0.06."""
    dirs = _unit(torch.randn(P, 3, generator=gen))
    r = radius * (1.0 + 0.004 * torch.randn(P, 1, generator=gen))
    nf = P // 8
    r[:nf] = floater_radius[0] + (floater_radius[1] - floater_radius[0]) * torch.rand(nf, 1, generator=gen)
    means = dirs * r
    nrm = _unit((-dirs if inward else dirs) + 0.05 * torch.randn(P, 3, generator=gen))
    rots = quat_from_normal(nrm, 2 * math.pi * torch.rand(P, generator=gen))
    big = _log_uniform(gen, P, *major)
    scales = torch.stack([big, big / _log_uniform(gen, P, 1.0, 8.0)], dim=-1)
    raw = 3.0 + 1.5 * torch.randn(P, generator=gen)
    raw[torch.rand(P, generator=gen) < opaque_share] = 20.0
    fo = 0.01 + 0.05 * torch.rand(nf, generator=gen)
    raw[:nf] = torch.log(fo / (1 - fo))
    opac = torch.sigmoid(raw)[:, None]
    shs = torch.cat([torch.rand(P, 1, 3, generator=gen) * 3.0 - 1.5, torch.randn(P, 15, 3, generator=gen) * 0.1], dim=1)
    return dict(means3D=means.contiguous(), scales=scales.contiguous(), rotations=rots.contiguous(), opacities=opac.contiguous(), shs=shs.contiguous()), nf


def _pixel_of(cam, means):
    """Pixel coordinates (pixel i's centre is at i) and camera depth of world points."""
    V = cam.world_view_transform
    pv = means @ V[:3, :3] + V[3, :3]
    fx, fy = float(cam.K[0, 0]), float(cam.K[1, 1])
    W, H = cam.image_width, cam.image_height
    return fx * pv[:, 0] / pv[:, 2] + (W - 1) / 2.0, fy * pv[:, 1] / pv[:, 2] + (H - 1) / 2.0, pv


def aim_at_pixels(g, cam, n, first=0):
    """Move up to `n` surfels of opacity 1.0f on the camera's side of the object (rows >= first) so that their centres project onto pixel centres, one
    pixel each: the pixel's ray meets such a surfel at rho = 0, inside its cap zone."""
    px, py, pv = _pixel_of(cam, g["means3D"])
    W, H = cam.image_width, cam.image_height
    V = cam.world_view_transform
    fx, fy = float(cam.K[0, 0]), float(cam.K[1, 1])
    front = (g["means3D"] * cam.camera_center).sum(-1) > 0.3 * cam.camera_center.norm()
    taken, done = set(), 0
    for i in torch.nonzero((g["opacities"][:, 0] == 1.0) & front)[:, 0].tolist():
        if i < first or done == n:
            continue
        ix, iy = int(round(float(px[i]))), int(round(float(py[i])))
        if not (0 <= ix < W and 0 <= iy < H) or (ix, iy) in taken:
            continue
        taken.add((ix, iy)); done += 1
        z = pv[i, 2]
        p = torch.stack([z * (ix - (W - 1) / 2.0) / fx, z * (iy - (H - 1) / 2.0) / fy, z])
        g["means3D"][i] = (p - V[3, :3]) @ V[:3, :3].t()
    return done


def surface_object(P, seed, C=3, scales=(0.05, 0.3)):
    """Rasterizer scene: see the module docstring.  Keeps `shs` and a C-channel `colors_precomp`; used with synth.orbit_camera."""
    gen = torch.Generator().manual_seed(seed)
    g, _ = _shell(P, gen, 1.0, False, scales, (1.05, 1.6))
    g["colors_precomp"] = torch.rand(P, C, generator=torch.Generator().manual_seed(seed + 7))
    return g


def raster_case(P, H, W, seed, C=3, view=1, fx=None, n_aimed=0):
    """surface_object with its orbit camera (fx defaults to small_scene's 1111.1 W / 800), n_aimed opaque surfels moved onto pixel centres."""
    g = surface_object(P, seed, C=C)
    cam = synth.orbit_camera(view, H=H, W=W, fx=(1111.1 * W / 800.0 if fx is None else fx))
    if n_aimed:
        aim_at_pixels(g, cam, n_aimed, first=P // 8)
    return g, cam


def _rays(R, gen, camera):
    """trace_scene's two ray kinds."""
    if camera:
        cam = synth.orbit_camera(2, H=20, W=20, fx=25.0, radius=1.0)
        ro, rd = synth.get_rays(cam)
        return ro.reshape(-1, 3)[:R].contiguous(), rd.reshape(-1, 3)[:R].contiguous()
    ro = torch.randn(R, 3, generator=gen) * 0.3
    rd = _unit(torch.randn(R, 3, generator=gen)) * (0.5 + torch.rand(R, 1, generator=gen))
    return ro.contiguous(), rd.contiguous()


def room(P, R, seed, n_aimed=0, camera=False):
    """Tracer scene: surfels on the inside of a sphere of radius 4, rays from inside it.  The first n_aimed rays are re-aimed (same origin, same length) at
    points within 0.1 sigma of the centres of wall surfels of opacity >= 0.995: the cap zone rho < 2 ln(o / 0.99) is a disc of ~0.14 sigma only."""
    gen = torch.Generator().manual_seed(seed)
    g, nf = _shell(P, gen, 4.0, True, (0.3, 1.5), (2.0, 3.5))
    g["others"] = torch.rand(P, 2, generator=gen)
    g["colors_precomp"] = torch.rand(P, 3, generator=gen)
    ro, rd = _rays(R, gen, camera)
    wall = torch.nonzero(g["opacities"][nf:, 0] >= 0.995)[:, 0] + nf
    n_aimed = min(n_aimed, ro.shape[0])
    if n_aimed and wall.numel():
        if camera:                                           # only the wall in front of the camera is inside its field of view
            fwd = _unit(rd.mean(0))
            inview = (_unit(g["means3D"][wall] - ro[0]) * fwd).sum(-1) > 0.9
            wall = wall[inview] if inview.any() else wall
        pick = wall[torch.randint(0, wall.numel(), (n_aimed,), generator=gen)]
        Rm = synth.build_rotation(g["rotations"][pick])
        rad = 0.1 * torch.sqrt(torch.rand(n_aimed, generator=gen)); ang = 2 * math.pi * torch.rand(n_aimed, generator=gen)
        tgt = g["means3D"][pick] + Rm[:, :, 0] * (g["scales"][pick, 0] * rad * torch.cos(ang))[:, None] \
            + Rm[:, :, 1] * (g["scales"][pick, 1] * rad * torch.sin(ang))[:, None]
        rd[:n_aimed] = _unit(tgt - ro[:n_aimed]) * rd[:n_aimed].norm(dim=-1, keepdim=True)
    return g, ro, rd.contiguous()


PLATE_OPACITY = 0.97        # three blends leave T = 2.7e-5: the third plate stops the pixel / ray, a factor 3.7 below T_EPS = 1e-4


def _append(g, extra):
    for k in g:
        g[k] = torch.cat([g[k], extra[k].to(g[k].dtype)], dim=0).contiguous()
    return g


def plates_and_crowd_raster(H=64, W=64, seed=4, C=3):
    """small_scene(P=3000, scale_mul=6) shrunk by 0.5 behind three plates that face the orbit camera at depths 2.2, 2.4, 2.6 (sigma = 20 world units:
    ~700 pixels, G > 0.99 over the whole image).  The plates are the LAST three rows.  Returns (g, cam)."""
    from tests.util import small_scene
    g, cam = small_scene(P=3000, H=H, W=W, seed=seed, C=C, sh=(C == 3), spread=0.5, scale_mul=6.0)
    g = {k: g[k] for k in ("means3D", "scales", "rotations", "opacities", "shs") + (("colors_precomp",) if C != 3 else ())}
    eye = cam.camera_center
    fwd = _unit(-eye)
    gen = torch.Generator().manual_seed(seed + 1)
    extra = dict(means3D=torch.stack([eye + fwd * d for d in (2.2, 2.4, 2.6)]), scales=torch.full((3, 2), 20.0),
                 rotations=quat_from_normal(-fwd[None].expand(3, 3).contiguous(), torch.tensor([0.3, 1.1, 2.0])),
                 opacities=torch.full((3, 1), PLATE_OPACITY), shs=torch.cat([torch.rand(3, 1, 3, generator=gen) * 3 - 1.5, torch.zeros(3, 15, 3)], dim=1))
    if C != 3:
        extra["colors_precomp"] = torch.rand(3, C, generator=gen)
    return _append(g, extra), cam


def plates_and_crowd_trace(P=2000, R=1024, seed=5):
    """The room with three plates (sigma = 8: twice the room's radius) across it at z = 1.5, 2.0, 2.5, facing the ray origins N(0, 0.3): the rays that
    go up meet all three.  The plates are the LAST three rows.  Returns (g, ro, rd)."""
    g, ro, rd = room(P, R, seed, n_aimed=0, camera=False)
    gen = torch.Generator().manual_seed(seed + 1)
    n = torch.tensor([[0.0, 0.0, -1.0]]).expand(3, 3).contiguous()
    extra = dict(means3D=torch.tensor([[0.0, 0.0, 1.5], [0.1, -0.1, 2.0], [-0.1, 0.1, 2.5]]), scales=torch.full((3, 2), 8.0),
                 rotations=quat_from_normal(n, torch.tensor([0.3, 1.1, 2.0])), opacities=torch.full((3, 1), PLATE_OPACITY),
                 shs=torch.cat([torch.rand(3, 1, 3, generator=gen) * 3 - 1.5, torch.zeros(3, 15, 3)], dim=1), others=torch.rand(3, 2, generator=gen),
                 colors_precomp=torch.rand(3, 3, generator=gen))
    return _append(g, extra), ro, rd


STACK_BG = torch.tensor([0.25, 0.5, 0.75])
STACK_COLORS = torch.eye(3)                                   # red, green, blue, front to back
STACKS = [(1.0, 1.0, 1.0), (1.0, 0.5, 1.0), (1.0, 0.98, 1.0)]


def stack_trace(opacities):
    """Three surfels of scale 0.5 at z = 2, 3, 4 facing the origin; four rays along +z through their centres, of lengths 1, 0.5, 1.5 and (from z = 0.5) 1.
    Every hit has u = v = 0 exactly, so G = 1, alpha = min(opacity, 0.99f) and the blend weights of the four rays are the same fp32 numbers: the
    per-surfel weight sums do not depend on the order of their atomic additions.  Returns (g, ro, rd)."""
    g = dict(means3D=torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 3.0], [0.0, 0.0, 4.0]]), scales=torch.full((3, 2), 0.5),
             rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(3, 1), opacities=torch.tensor(opacities, dtype=torch.float32)[:, None],
             colors_precomp=STACK_COLORS.clone(), others=torch.tensor([[0.2, 0.9], [0.5, 0.5], [0.8, 0.1]]),
             shs=torch.zeros(3, 16, 3))
    ro = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.5]])
    rd = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 0.5], [0.0, 0.0, 1.5], [0.0, 0.0, 1.0]])
    return g, ro, rd


def stack_raster(opacities, H=32, W=32, fx=200.0):
    """Three surfels of scale 0.3 on the orbit camera's axis at -0.4, 0, +0.4 (front to back), facing it; fx = 200 makes sigma ~15 pixels, so the four
    pixels around the principal point lie inside the cap disc (0.14 sigma) of all three.  Returns (g, cam, central (H,W) bool)."""
    cam = synth.orbit_camera(1, H=H, W=W, fx=fx)
    eye = cam.camera_center
    fwd = _unit(-eye)
    g = dict(means3D=torch.stack([fwd * d for d in (-0.4, 0.0, 0.4)]).contiguous(), scales=torch.full((3, 2), 0.3),
             rotations=quat_from_normal(-fwd[None].expand(3, 3).contiguous(), torch.zeros(3)), opacities=torch.tensor(opacities, dtype=torch.float32)[:, None],
             colors_precomp=STACK_COLORS.clone(), shs=torch.zeros(3, 16, 3))
    central = torch.zeros(H, W, dtype=torch.bool)
    central[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = True
    return g, cam, central


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# census on the float64 twins
def census_raster(g, cam, sh=True, sh_degree=3, scale_modifier=1.0, exclude=None):
    """What oracle/eager.py:rasterize (float64) does on the scene: dict(blends, capped, lowpass, accepted, stopped_px, pixels, per_pixel = the (H,W)
    arrays).  exclude: (H,W) bool of pixels to leave out of the totals (the oracle's audited pixels)."""
    from oracle import eager
    from tests.util import cam_args
    d = torch.float64
    ca = cam_args(cam)
    st = {}
    with torch.no_grad():
        eager.rasterize(g["means3D"].to(d), g["opacities"].to(d), ca["viewmatrix"].to(d), ca["projmatrix"].to(d), ca["campos"].to(d), ca["W"], ca["H"],
                        scales=g["scales"].to(d), rotations=g["rotations"].to(d), shs=(g["shs"].to(d) if sh else None),
                        colors_precomp=(None if sh else g["colors_precomp"].to(d)), sh_degree=sh_degree, scale_modifier=scale_modifier, pix_chunk=1024, stats=st)
    H, W = ca["H"], ca["W"]
    per = {k: v.reshape(H, W).numpy() for k, v in st.items()}
    m = np.ones((H, W), bool) if exclude is None else ~np.asarray(exclude, bool)
    return dict(blends=int(per["blends"][m].sum()), capped=int(per["capped"][m].sum()), lowpass=int(per["lowpass"][m].sum()), accepted=int(per["accepted"][m].sum()),
                stopped_px=int(per["stopped"][m].sum()), pixels=int(m.sum()), per_pixel=per)


def census_trace(g, ro, rd, start_from_first, scale_modifier=1.0):
    """What oracle/eager_trace.py:trace (float64) does on the scene: dict(blends, capped, capped_rays, accepted, stopped_rays, rays, per_ray)."""
    from oracle import eager_trace
    d = torch.float64
    st = {}
    with torch.no_grad():
        eager_trace.trace(ro.to(d), rd.to(d), g["means3D"].to(d), g["scales"].to(d), g["rotations"].to(d), g["opacities"].to(d), colors_precomp=g["colors_precomp"].to(d),
                          others=g["others"].to(d), start_from_first=start_from_first, scale_modifier=scale_modifier, stats=st)
    per = {k: v.numpy() for k, v in st.items()}
    return dict(blends=int(per["blends"].sum()), capped=int(per["capped"].sum()), capped_rays=int((per["capped"] > 0).sum()), accepted=int(per["accepted"].sum()),
                stopped_rays=int(per["stopped"].sum()), rays=int(ro.shape[0]), per_ray=per)


def census_line(name, c):
    unit = "px" if "stopped_px" in c else "rays"
    s = "%-44s blends %7d  capped %5d  stopped %5d of %5d %s  accepted %7d" % (name, c["blends"], c["capped"], c.get("stopped_px", c.get("stopped_rays")),
                                                                                c.get("pixels", c.get("rays")), unit, c["accepted"])
    if "lowpass" in c: s += "  low-pass %6d" % c["lowpass"]
    if "capped_rays" in c: s += "  rays with a capped hit %4d" % c["capped_rays"]
    return s


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The committed scenes: every scene tests/test_saturated_gpu.py and the float64 leg use, with the seeds at which the REFERENCE ALONE meets the census
# floors and audit caps of tests/test_saturated_scenes_cpu.py (re-run that file when a seed or a size changes).
RASTER_CASES = {
    "sphere600": dict(P=600, H=64, W=80, C=3, sh=True, deg=3, seed=2),
    "sphere1500": dict(P=1500, H=64, W=80, C=5, sh=False, deg=0, seed=1),                                  # tile lists longer than one 256-entry batch
    "sphere300_17x15": dict(P=300, H=17, W=15, C=7, sh=False, deg=0, seed=1, fx=1111.1 * 16 / 800.0, n_aimed=40),   # ~100 covered pixels: opaque surfels aimed at pixel centres
    # the float64 leg.  Of seeds 0..11 this one has no audited pixel AND the smallest fp32-to-float64 distance of the C oracle itself (1.2e-5 values, 4.0e-5
    # gradients; the others reach 7e-4 on dmeans3D / drotations: an edge-on surfel at the sphere's limb loses digits to px * Tw - Tu in ANY fp32 evaluation)
    "sphere300_f64": dict(P=300, H=48, W=64, C=3, sh=True, deg=3, seed=3),
}
TRACE_CASES = {
    "room600": dict(P=600, R=1024, seed=0, n_aimed=256, camera=False),
    "room200": dict(P=200, R=400, seed=1, n_aimed=128, camera=True),                                       # also the float64 leg (no audited ray at this seed)
}


def raster_scene(name):
    c = RASTER_CASES[name]
    g, cam = raster_case(c["P"], c["H"], c["W"], c["seed"], C=c["C"], fx=c.get("fx"), n_aimed=c.get("n_aimed", 0))
    return g, cam, c


def trace_scene_of(name):
    c = TRACE_CASES[name]
    return room(c["P"], c["R"], c["seed"], n_aimed=c["n_aimed"], camera=c["camera"]) + (c,)
