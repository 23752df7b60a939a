"""numpy/ctypes front-end of oracle/surfel_trace_oracle.c (test infrastructure only).
Mirrors SurfelTracer.__call__ (reference boundary: easyvolcap/utils/optix_utils.py:188-201)."""
import ctypes

import numpy as np

from .raster import lib, _p, _f32


class _TCfg(ctypes.Structure):
    _fields_ = [("P", ctypes.c_int), ("R", ctypes.c_int), ("D", ctypes.c_int), ("M", ctypes.c_int),
                ("max_trace_depth", ctypes.c_int), ("start_from_first", ctypes.c_int), ("has_others", ctypes.c_int),
                ("bg_len", ctypes.c_int), ("scale_modifier", ctypes.c_float), ("specular_threshold", ctypes.c_float)]


class _TDetail(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_void_p), ("amb_ids", ctypes.c_void_p), ("acap", ctypes.c_int32), ("namb", ctypes.c_void_p),
                ("pool_ids", ctypes.c_void_p), ("pool_tbits", ctypes.c_void_p), ("pool_alpha", ctypes.c_void_p), ("pool_flags", ctypes.c_void_p),
                ("pool_cap", ctypes.c_int64), ("cand_off", ctypes.c_void_p), ("ncand", ctypes.c_void_p), ("go", ctypes.c_void_p)]


# trc_audit's kind bits and candidate flags (oracle/surfel_trace_oracle.c: TRC_KIND_*, TRC_CAND_*)
KIND_DISAGREE, KIND_GEOM, KIND_TERM, KIND_CLAMP, KIND_BOUNCE = 1, 2, 4, 8, 16
CAND_HIT, CAND_AMB, CAND_BEHIND, CAND_STOPS = 1, 2, 4, 8
AMB_CAP = 8         # ambiguous candidates kept per ray; a ray with more is reported (namb > AMB_CAP) and left out by the tests


def _set_forced(L, forced, R):
    """forced = (ids (R, cap) int32, n (R,) int32, mask (R,) bool) or None: trc_set_forced_lists.  Returns what must stay alive over the call."""
    if forced is None:
        L.trc_set_forced_lists(None, None, None, ctypes.c_int(0))
        return None
    ids = np.ascontiguousarray(forced[0], np.int32); n = np.ascontiguousarray(forced[1], np.int32); mask = np.ascontiguousarray(forced[2]).astype(np.uint8)
    assert ids.ndim == 2 and ids.shape[0] == R and n.shape == (R,) and mask.shape == (R,), (ids.shape, n.shape, mask.shape, R)
    L.trc_set_forced_lists(_p(ids), _p(n), _p(mask), ctypes.c_int(ids.shape[1]))
    return ids, n, mask


def trace_forward(ray_o, ray_d, means3D, scales, rotations, opacities, *, shs=None, colors_precomp=None, others=None,
                  sh_degree=0, bg=None, max_trace_depth=0, specular_threshold=0.0, start_from_first=True, scale_modifier=1.0, forced=None):
    """forced = (ids (R, cap), n (R,), mask (R,)): the rays with mask set composite exactly those surfels in stage 0 (trc_set_forced_lists); the lists are
    remembered in the returned dict, so that trace_backward replays them."""
    L = lib()
    ray_o = _f32(ray_o).reshape(-1, 3); ray_d = _f32(ray_d).reshape(-1, 3)
    means3D = _f32(means3D); scales = _f32(scales); rotations = _f32(rotations); opacities = _f32(opacities).reshape(-1)
    shs = _f32(shs); colors_precomp = _f32(colors_precomp); others = _f32(others)
    P, R = means3D.shape[0], ray_o.shape[0]
    M = 0 if shs is None else shs.shape[1]
    bg = np.zeros(3, np.float32) if bg is None else _f32(bg).reshape(-1)
    cfg = _TCfg(P, R, int(sh_degree), M, int(max_trace_depth), (2 if start_from_first == 2 else int(bool(start_from_first))), int(others is not None),
                len(bg), float(scale_modifier), float(specular_threshold))
    ND = max_trace_depth + 1
    rgb = np.zeros((R, 3), np.float32); dpt = np.zeros(R, np.float32); acc = np.zeros(R, np.float32)
    norm = np.zeros((R, 3), np.float32); dist = np.zeros(R, np.float32); aux = np.zeros((R, 2), np.float32)
    mid = np.zeros((R, 16 * ND), np.float32); wet = np.zeros(P, np.float64)
    final_T = np.zeros(R, np.float32); nhits = np.zeros(R, np.int32)
    # the distortion shadow (trc_set_dist_shadow): stage 0's distortion in double from the float code's own alphas / distances, and the a-priori
    # fp32 rounding bound of its moment form -- what a HIP value is asserted against
    dist64 = np.zeros(R, np.float64); dist_bound = np.zeros(R, np.float64)
    L.trc_set_dist_shadow(_p(dist64), _p(dist_bound))
    forced = _set_forced(L, forced, R)
    L.trc_forward(ctypes.byref(cfg), _p(ray_o), _p(ray_d), _p(means3D), _p(scales), _p(rotations), _p(opacities), _p(shs),
                  _p(colors_precomp), _p(others), _p(bg), _p(rgb), _p(dpt), _p(acc), _p(norm), _p(dist), _p(aux), _p(mid),
                  _p(wet), _p(final_T), _p(nhits))
    return dict(cfg=cfg, rgb=rgb, dpt=dpt, acc=acc, norm=norm, dist=dist, aux=aux, mid=mid, wet=wet, final_T=final_T,
                nhits=nhits, bg=bg, dist64=dist64, dist_bound=dist_bound, forced=forced,
                inputs=dict(ray_o=ray_o, ray_d=ray_d, means3D=means3D, scales=scales, rotations=rotations,
                            opacities=opacities, shs=shs, colors_precomp=colors_precomp, others=others))


def trace_audit(ray_o, ray_d, means3D, scales, rotations, opacities, *, others=None, start_from_first=True, tmin=None,
                bounce_thr=None, scale_modifier=1.0, lcap=None, shs=None, sh_degree=0, detail=False, forced=None, pool_cap=1 << 22):
    """Fragility audit of one trace stage (trc_audit): dict(fragile (R,) bool, ids / tbits (R,lcap) front-to-back composited surfel ids and
    float bits of their hit distance, nhit (R,)).  tmin overrides the start_from_first rule (bounce stages: 1e-3); bounce_thr adds the bounce decisions.
    detail: also why and where -- kind (R,) KIND_* bits (kind != 0 <=> fragile), amb_ids (R, AMB_CAP) / namb (R,) the ambiguous surfels (namb > AMB_CAP:
    overflowed), go (R, lcap) per composited entry (1 = going on was decided, | 2 = its termination test is near the threshold), and `cand`: per FRAGILE or
    forced ray r a dict(ids, tbits, alpha, flags) of its candidates (float-accepted hits and ambiguous surfels) in (t, id) order, flags = CAND_* bits;
    None for the other rays (and for a ray the pool of pool_cap entries had no room for).
    forced = (ids, n, mask): the masked rays replay exactly those lists (trc_set_forced_lists); ids / nhit / go then describe the forced list in (t, id)
    order, and the candidates behind its last entry carry CAND_BEHIND and, where the walk may stop, CAND_STOPS."""
    L = lib()
    ray_o = _f32(ray_o).reshape(-1, 3); ray_d = _f32(ray_d).reshape(-1, 3)
    means3D = _f32(means3D); scales = _f32(scales); rotations = _f32(rotations); opacities = _f32(opacities).reshape(-1)
    others = _f32(others); shs = _f32(shs)          # shs (P,M,3) + sh_degree: audit the colour clamp as well (see trc_audit)
    P, R = means3D.shape[0], ray_o.shape[0]
    cfg = _TCfg(P, R, int(sh_degree) if shs is not None else 0, int(shs.shape[1]) if shs is not None else 0, 0, int(bool(start_from_first)),
                int(others is not None), 3, float(scale_modifier), 0.0)
    lcap = int(lcap or max(P, 1))
    fragile = np.zeros(max(R, 1), np.uint8); ids = np.full((max(R, 1), lcap), -1, np.int32); nhit = np.zeros(max(R, 1), np.int32)
    tbits = np.zeros((max(R, 1), lcap), np.uint32)
    if detail:
        Rm = max(R, 1)
        kind = np.zeros(Rm, np.uint8); amb_ids = np.full((Rm, AMB_CAP), -1, np.int32); namb = np.zeros(Rm, np.int32)
        pool_cap = int(max(pool_cap, P))
        pool_ids = np.zeros(pool_cap, np.int32); pool_tbits = np.zeros(pool_cap, np.uint32); pool_alpha = np.zeros(pool_cap, np.float32)
        pool_flags = np.zeros(pool_cap, np.uint8); cand_off = np.full(Rm, -1, np.int64); ncand = np.zeros(Rm, np.int32)
        go = np.zeros((Rm, lcap), np.uint8)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        det = _TDetail(vp(kind), vp(amb_ids), AMB_CAP, vp(namb), vp(pool_ids), vp(pool_tbits), vp(pool_alpha), vp(pool_flags), pool_cap, vp(cand_off), vp(ncand), vp(go))
        L.trc_set_audit_detail(ctypes.byref(det))
    else:
        L.trc_set_audit_detail(None)
    forced = _set_forced(L, forced, R)
    L.trc_audit(ctypes.byref(cfg), _p(ray_o), _p(ray_d), _p(means3D), _p(scales), _p(rotations), _p(opacities), _p(others), _p(shs),
                ctypes.c_float(-1.0 if tmin is None else float(tmin)), ctypes.c_float(-1.0 if bounce_thr is None else float(bounce_thr)),
                _p(fragile), _p(ids), _p(tbits), ctypes.c_int(lcap), _p(nhit))
    out = dict(fragile=fragile[:R].astype(bool), ids=ids[:R], tbits=tbits[:R], nhit=nhit[:R])
    if detail:
        cand = [None] * R
        for r in np.nonzero(cand_off[:R] >= 0)[0]:
            sl = slice(int(cand_off[r]), int(cand_off[r]) + int(ncand[r]))
            cand[r] = dict(ids=pool_ids[sl], tbits=pool_tbits[sl], alpha=pool_alpha[sl], flags=pool_flags[sl])
        out.update(kind=kind[:R], amb_ids=amb_ids[:R], namb=namb[:R], amb_overflow=namb[:R] > AMB_CAP, go=go[:R], cand=cand)
    return out


def trace_backward(fwd, dL_drgb, dL_ddpt, dL_dacc, dL_dnorm, dL_daux, want_cond=False):
    """want_cond: additionally `cond` = the noise scale of every gradient element (see trc_backward's comment), same keys."""
    L = lib()
    cfg = fwd["cfg"]; i = fwd["inputs"]
    P, R, M = cfg.P, cfg.R, cfg.M
    g = [_f32(x) for x in (dL_drgb, dL_ddpt, dL_dacc, dL_dnorm, dL_daux)]
    dmeans = np.zeros((P, 3)); dscales = np.zeros((P, 2)); drots = np.zeros((P, 4)); dopac = np.zeros(P)
    dshs = np.zeros((P, max(M, 1), 3)); dcolors = np.zeros((P, 3)); dothers = np.zeros((P, 2))
    dro = np.zeros((R, 3)); drd = np.zeros((R, 3))
    cnd = [np.zeros_like(x) for x in (dmeans, dscales, drots, dopac, (dshs if M > 0 else dcolors), dothers, dro, drd)]
    unc = [np.zeros_like(x) for x in cnd]
    _keep = _set_forced(L, fwd.get("forced"), R)            # the lists the forward composited (trace_forward(forced=...))
    L.trc_backward(ctypes.byref(cfg), _p(i["ray_o"]), _p(i["ray_d"]), _p(i["means3D"]), _p(i["scales"]), _p(i["rotations"]),
                   _p(i["opacities"]), _p(i["shs"]), _p(i["colors_precomp"]), _p(i["others"]), _p(fwd["bg"]), _p(g[0]), _p(g[1]),
                   _p(g[2]), _p(g[3]), _p(g[4]), _p(dmeans), _p(dscales), _p(drots), _p(dopac), _p(dshs), _p(dcolors), _p(dothers),
                   _p(dro), _p(drd), *[_p(x) for x in ((cnd + unc) if want_cond else [None] * 16)])
    out = dict(dmeans3D=dmeans, dscales=dscales, drots=drots, dopacities=dopac, dshs=dshs if M > 0 else None,
               dcolors=dcolors if M == 0 else None, dothers=dothers if i["others"] is not None else None,
               dray_o=dro, dray_d=drd)
    if want_cond:
        out["cond"] = dict(dmeans3D=cnd[0], dscales=cnd[1], drots=cnd[2], dopacities=cnd[3], dshs=cnd[4] if M > 0 else None,
                           dcolors=cnd[4] if M == 0 else None, dothers=cnd[5] if i["others"] is not None else None, dray_o=cnd[6], dray_d=cnd[7])
        out["unc"] = dict(dmeans3D=unc[0], dscales=unc[1], drots=unc[2], dopacities=unc[3], dshs=unc[4] if M > 0 else None,
                          dcolors=unc[4] if M == 0 else None, dothers=unc[5] if i["others"] is not None else None, dray_o=unc[6], dray_d=unc[7])
    return out
