"""Round 8: batch_surfel_bwd<true,false> on the flagship's env trace (the configs[2] view's reflected rays over the 163 840-surfel env set, colour-only
state and upstream gradient), under a library variant: time per launch from the library's HIP-event scope and -- when the variant was built with
-DENVGS_BSB_TIMING=1 -- where a wavefront's cycles go (the difference of the call's counter totals across ONE backward).
    python scratch/bsb_stage_split.py <library.so> [tag]"""
import ctypes, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from envgs_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
from envgs_amd import synth, tracing, fused, envgs_step
import diff_surfel_tracing as tpkg
import diff_surfel_rasterization_wet_ch05 as pkg

tag = sys.argv[2] if len(sys.argv) > 2 else os.path.basename(sys.argv[1])
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
for _ in range(3):
    tracing.trace_backward(saved, *gr)
torch.cuda.synchronize()
lib.envgs_prof_enable(1); drain()
for _ in range(10):
    tracing.trace_backward(saved, *gr)
torch.cuda.synchronize()
lib.envgs_prof_enable(0)
ms = drain().get("trace.batch_surfel_bwd", (float("nan"), 0))[0]
print("%s rays %d hits %.2f M entries %.3f M (%.1f hits/entry)  batch_surfel_bwd<true,false> %.4f ms per launch" % (tag, R, tc["hits"] / 1e6, ent / 1e6, tc["hits"] / max(ent, 1), ms), flush=True)
t0 = totals(saved.counters)
tracing.trace_backward(saved, *gr)
torch.cuda.synchronize()
d = [b - a for a, b in zip(t0, totals(saved.counters))]
if sum(d):
    s = float(sum(d))
    print("%s wavefront cycles of one launch: prologue/epilogue %d (%.1f %%)  stage() %d (%.1f %%)  entry bodies %d (%.1f %%)  group-top sync %d (%.1f %%)  | per entry: stage %.0f  body %.0f" % (
        tag, d[0], 100 * d[0] / s, d[1], 100 * d[1] / s, d[2], 100 * d[2] / s, d[3], 100 * d[3] / s, d[1] / max(ent, 1), d[2] / max(ent, 1)), flush=True)
