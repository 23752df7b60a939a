"""Round 8: ONE forward of the flagship's env trace (the configs[2] view's reflected rays over the 163 840-surfel env set, colour-only state and upstream
gradient), differentiated twice by each of two builds of the library in one process -- the record slots come from atomics in the forward, so only
backward passes over the SAME forward can be compared bit for bit.  The forward runs under <new.so>.
    python scratch/bsb_same_forward.py <new.so> <old.so>"""
import ctypes, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from envgs_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
from envgs_amd import synth, tracing, fused, envgs_step
import diff_surfel_tracing as tpkg
import diff_surfel_rasterization_wet_ch05 as pkg

tag = "same_forward"
dev = torch.device("cuda:0")
lib = _lib.load()
H = W = 800
g = synth.base_gaussians(300000, seed=0, device=dev)
ge = synth.env_gaussians(163840, seed=1, device=dev)
cam = synth.orbit_camera(0, n_views=8, H=H, W=W, fx=1111.1, device=dev)
rays = synth.get_rays(cam)
envgs_step.FUSED["on"] = True
base = {k: g[k] for k in ("means3D", "shs", "opacities", "scales", "rotations")}
base["specular"] = g["specular"]; base["roughness"] = g["roughness"]
tracer = tpkg.SurfelTracer()
with torch.no_grad():
    out = envgs_step.envgs_forward(pkg, tpkg, tracer, cam, rays, base, {k: ge[k] for k in base if k in ge}, torch.zeros(3, device=dev), torch.zeros(3, device=dev), torch.tensor([3], device=dev))
ro, rd = out["ref_o"].reshape(-1, 3).contiguous(), out["ref_d"].reshape(-1, 3).contiguous()

NAMES = []
while lib.envgs_prof_kernel_name(len(NAMES)):
    NAMES.append(lib.envgs_prof_kernel_name(len(NAMES)).decode())


def drain():
    r = {}
    for k, nm in enumerate(NAMES):
        t_, c_ = ctypes.c_double(0), ctypes.c_int(0)
        lib.envgs_prof_read(k, ctypes.byref(t_), ctypes.byref(c_))
        if c_.value:
            r[nm] = (t_.value / c_.value, c_.value)
    return r


def totals(counters):
    w = counters.cpu()
    v = w[_lib.CTR_TOTALS:_lib.CTR_TOTALS + 2 * _lib.TOT_COUNT].view(torch.int64)
    return [int(v[k]) for k in (_lib.TOT_ROUNDS, _lib.TOT_COOP_EXPAND, _lib.TOT_COOP_WALK, _lib.TOT_COOP_WAIT)]


ts = tpkg.SurfelTracingSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev), scale_modifier=1.0,
                                viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center,
                                prefiltered=False, debug=False, max_trace_depth=0, specular_threshold=0.0)
v, f = fused.surfel_quads(ge["means3D"], ge["scales"], ge["rotations"])
nodes, _ = tracing.build_bvh(v, ge["opacities"])
caps = tracing.CapState()
caps.colour_only = True
for it in range(4):                           # the capacity / row budget adapt over the first calls
    outs, saved = tracing.trace_forward(nodes, ro, rd, ge["means3D"], ge["shs"], None, None, ge["opacities"], ge["scales"], ge["rotations"], ts, False, caps=caps)
    torch.cuda.synchronize()
tc = tracing.last_trace_counts(); ent = sum(tracing.last_entry_counts())
R = ro.shape[0]
g_rgb = (torch.randn(R, 3, generator=torch.Generator().manual_seed(5)) / R).to(dev)
gr = (g_rgb, None, None, None, None)
print("sparse hits filed:", tc["sparse_hits"], "max_list", tc["max_list"], "cap", tc["cap"], "rays without rows", tc["rays_without_rows"], flush=True)
def run():
    out = tracing.trace_backward(saved, *gr)
    tracing.join_deferred_gradients(); torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items() if v is not None}
new1 = run(); new2 = run()
_lib._libs["product"] = _lib._open(os.path.abspath(sys.argv[2]))
old1 = run(); old2 = run()
for k in new1:
    m = float(old1[k].abs().max())
    print("%-14s change vs change %-9s parent vs parent %-9s change vs parent %-9s max|a-b|/max|b| %.3e" % (k, "bit-equal" if torch.equal(new1[k], new2[k]) else "differs",
          "bit-equal" if torch.equal(old1[k], old2[k]) else "differs", "bit-equal" if torch.equal(new1[k], old1[k]) else "differs", float((new1[k] - old1[k]).abs().max()) / max(m, 1e-30)), flush=True)
