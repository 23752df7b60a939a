"""ctypes loader for libenvgs_hip.so (the C-ABI of include/*.h).  Fails loudly: there is no CPU or
PyTorch fallback for the product path -- if the HIP library is missing or does not load, importing an
operator raises."""
import ctypes
import os

# torch FIRST: PyTorch-ROCm wheels carry their own libamdhip64, and whichever HIP runtime is loaded first serves every later library with
# the same SONAME.  If this library (linked against /opt/rocm) were opened before torch, torch would run on a runtime it was not built with
# and the stream handles it passes here would belong to a different runtime instance ("hipErrorNoDevice" at the first launch).
import torch  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libenvgs_hip.so")
_lib = None

c_void_p, c_int, c_uint32, c_size_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t


class RasterCfg(ctypes.Structure):
    """struct envgs_raster_cfg (include/envgs_raster.h)."""
    _fields_ = [("P", ctypes.c_int32), ("sh_degree", ctypes.c_int32), ("sh_coeffs", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("bg_len", ctypes.c_int32), ("debug", ctypes.c_int32), ("scale_modifier", ctypes.c_float),
                ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float), ("feature_f16", ctypes.c_int32)]


class AdamTensor(ctypes.Structure):
    """struct envgs_adam_tensor (include/envgs_optim.h)."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("numel", ctypes.c_int64), ("lr", ctypes.c_float), ("step", ctypes.c_float)]


class RowsTensor(ctypes.Structure):
    """struct envgs_rows_tensor (include/envgs_densify.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("row_bytes", ctypes.c_int64)]


class GrowTensor(ctypes.Structure):
    """struct envgs_grow_tensor (include/envgs_densify.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("row_bytes", ctypes.c_int64), ("kind", ctypes.c_int32), ("reserved0", ctypes.c_int32)]


class DensifyPlanArgs(ctypes.Structure):
    """struct envgs_densify_plan_args (include/envgs_densify.h)."""
    _fields_ = ([("P", ctypes.c_int64), ("N", ctypes.c_int32), ("flags", ctypes.c_uint32)]
                + [(n, ctypes.c_float) for n in ("grad_threshold", "size_limit", "split_screen_threshold", "min_opacity", "min_gradient", "r")]
                + [(n, ctypes.c_void_p) for n in ("ga", "dn", "mr", "wa", "scal", "opac", "cls", "scan", "counters", "temp")]
                + [("temp_bytes", ctypes.c_size_t)])


class DensifyRewriteArgs(ctypes.Structure):
    """struct envgs_densify_rewrite_args (include/envgs_densify.h)."""
    _fields_ = ([("P", ctypes.c_int64), ("out_rows", ctypes.c_int64), ("n_samples", ctypes.c_int64), ("N", ctypes.c_int32), ("count", ctypes.c_int32),
                 ("ratio_n", ctypes.c_double), ("r", ctypes.c_float), ("reserved0", ctypes.c_uint32)]
                + [(n, ctypes.c_void_p) for n in ("cls", "scan", "counters", "scal", "rotation", "samples")]
                + [("tensors", ctypes.POINTER(GrowTensor))])


class TraceLists(ctypes.Structure):
    """struct envgs_trace_lists (include/envgs_trace.h)."""
    _fields_ = [("hit_lists", ctypes.c_void_p), ("hit_cnt", ctypes.c_void_p), ("n_used", ctypes.c_void_p), ("cap", ctypes.c_int32),
                ("surf_acc", ctypes.c_void_p), ("surf_cnt", ctypes.c_void_p), ("surf_off", ctypes.c_void_p),
                ("scan_temp", ctypes.c_void_p), ("scan_temp_bytes", ctypes.c_size_t), ("ray_keys", ctypes.c_void_p),
                ("ray_order", ctypes.c_void_p), ("ray_sort_temp", ctypes.c_void_p), ("ray_sort_temp_bytes", ctypes.c_size_t),
                ("records", ctypes.c_void_p),
                ("num_records", ctypes.c_uint64), ("hit_state", ctypes.c_void_p), ("entries", ctypes.c_void_p), ("pairs", ctypes.c_void_p),
                ("n_entries", ctypes.c_void_p), ("compact_rows", ctypes.c_uint64), ("row_off", ctypes.c_void_p), ("batch_rows", ctypes.c_void_p),
                ("row_blk", ctypes.c_void_p), ("sh_perm", ctypes.c_void_p), ("state_planes", ctypes.c_int32),
                ("sparse_hits", ctypes.c_void_p), ("sparse_cap", ctypes.c_uint64),
                ("defer_reduce", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("bwd_order", ctypes.c_void_p)]


class TraceCfg(ctypes.Structure):
    """struct envgs_trace_cfg (include/envgs_trace.h)."""
    _fields_ = [("P", ctypes.c_int32), ("num_rays", ctypes.c_int32), ("sh_degree", ctypes.c_int32),
                ("sh_coeffs", ctypes.c_int32), ("max_trace_depth", ctypes.c_int32), ("start_from_first", ctypes.c_int32),
                ("has_others", ctypes.c_int32), ("bg_len", ctypes.c_int32), ("debug", ctypes.c_int32),
                ("ray_h", ctypes.c_int32), ("ray_w", ctypes.c_int32),
                ("scale_modifier", ctypes.c_float), ("specular_threshold", ctypes.c_float), ("feature_f16", ctypes.c_int32)]


# The counter block of a traced call (include/envgs_trace.h) and the ENVGS_DBG_TRACE bits (include/envgs_raster.h): the headers' names without
# their ENVGS_ prefix.  tests/test_abi.py compares every one of them with the header.
TRACE_COUNTER_WORDS, TRACE_COUNTER_MIRROR, TRACE_MAX_SEG = 96, 72, 4
CTR_RAY_FETCH, CTR_MAX_LIST, CTR_TOTALS = 0, 1, 2
(TOT_HITS, TOT_NODE_VISITS, TOT_ROUNDS, TOT_FOUND, TOT_PACKET_NODES, TOT_PACKET_LEAVES, TOT_COOP_EXPAND, TOT_COOP_WALK, TOT_COOP_WAIT,
 TOT_COUNT) = range(10)
CTR_STACK_OVERFLOWS, CTR_RAYS_WITHOUT_ROWS, CTR_ROW_CLAIM, CTR_LONG_QUEUE, CTR_SEG_FIRST_ROW = 20, 21, 22, 24, 28
CTR_BATCH_FETCH, CTR_BATCH_FETCH_STRIDE = 32, 8
CTR_SPARSE_FILED, CTR_BATCH_ENTRIES, CTR_SPARSE_SKIPPED = 64, 65, 66
DBG_TRACE, DBG_TRACE_NO_SORT, DBG_TRACE_SMALL_STACK, DBG_TRACE_PREPARE_INLINE = 0, 64, 1024, 16384
DBG_TRACE_RETIRED = 8 | 16 | 512 | 2048 | 4096 | 8192


class SupervisorArgs(ctypes.Structure):
    """struct envgs_supervisor_args (include/envgs_supervisor.h)."""
    _fields_ = ([("N", ctypes.c_int64), ("P", ctypes.c_int64), ("flags", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
                 ("weight", ctypes.c_float * 5), ("reserved1", ctypes.c_float)]
                + [(n, ctypes.c_void_p) for n in ("norm_map", "surf_norm_map", "acc_map", "dpt_map", "dist_map", "env_opacity", "prior", "msk", "R", "near_far")]
                + [(n, ctypes.c_int64) for n in ("norm_map_row", "norm_map_ch", "surf_norm_map_row", "surf_norm_map_ch", "acc_map_row", "dpt_map_row",
                                                 "dist_map_row", "env_opacity_row", "prior_row", "prior_ch", "msk_row")]
                + [(n, ctypes.c_void_p) for n in ("g_norm_map", "g_surf_norm_map", "g_acc_map", "g_dist_map", "g_env_opacity", "partial")])


class SurfelInputsArgs(ctypes.Structure):
    """struct envgs_surfel_inputs_args (include/envgs_model.h)."""
    _fields_ = ([(n, ctypes.c_int32) for n in ("P", "sh_degree", "sh_coeffs", "spec_channels")]
                + [(n, ctypes.c_void_p) for n in ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "specular", "roughness", "campos",
                                                  "scales", "rotations", "opacities", "specular_act", "roughness_act", "shs", "colors", "others", "vertices",
                                                  "clamped",
                                                  "g_scales", "g_rotations", "g_opacities", "g_specular_act", "g_roughness_act", "g_shs", "g_colors", "g_others",
                                                  "d_xyz", "d_features_dc", "d_features_rest", "d_scaling", "d_rotation", "d_opacity", "d_specular", "d_roughness")])


class TsdfVolume(ctypes.Structure):
    """struct envgs_tsdf_volume (include/envgs_mesh.h)."""
    _fields_ = ([(n, ctypes.c_int32) for n in ("nx", "ny", "nz")] + [(n, ctypes.c_float) for n in ("ox", "oy", "oz", "voxel")]
                + [(n, ctypes.c_void_p) for n in ("tsdf", "weight", "rgb")])


class TsdfView(ctypes.Structure):
    """struct envgs_tsdf_view (include/envgs_mesh.h)."""
    _fields_ = [("depth", ctypes.c_void_p), ("rgb", ctypes.c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("R", ctypes.c_float * 9), ("T", ctypes.c_float * 3), ("depth_max", ctypes.c_float), ("trunc", ctypes.c_float)]


class TsdfViews(ctypes.Structure):
    """struct envgs_tsdf_views (include/envgs_mesh.h)."""
    _fields_ = [("count", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("v", TsdfView * 8)]


class CullView(ctypes.Structure):
    """struct envgs_cull_view (include/envgs_mesh.h)."""
    _fields_ = [("mask", ctypes.c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("R", ctypes.c_float * 9), ("T", ctypes.c_float * 3)]


class CullViews(ctypes.Structure):
    """struct envgs_cull_views (include/envgs_mesh.h)."""
    _fields_ = [("count", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("v", CullView * 8)]


class MeshRasterView(ctypes.Structure):
    """struct envgs_mesh_raster_view (include/envgs_mesh.h)."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("R", ctypes.c_float * 9), ("T", ctypes.c_float * 3)]


class MeshRasterViews(ctypes.Structure):
    """struct envgs_mesh_raster_views (include/envgs_mesh.h)."""
    _fields_ = [("count", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("v", MeshRasterView * 8)]


class FuseSource(ctypes.Structure):
    """struct envgs_fuse_source (include/envgs_mesh.h)."""
    _fields_ = [("depth", ctypes.c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("fwd", ctypes.c_float * 12), ("back", ctypes.c_float * 12)]


class FuseSources(ctypes.Structure):
    """struct envgs_fuse_sources (include/envgs_mesh.h)."""
    _fields_ = [("count", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("v", FuseSource * 8)]


class VisMap(ctypes.Structure):
    """struct envgs_vis_map (include/envgs_visualize.h)."""
    _fields_ = [("ptr", ctypes.c_void_p), ("stride", ctypes.c_int64 * 4)]


class VisPlane(ctypes.Structure):
    """struct envgs_vis_plane (include/envgs_visualize.h)."""
    _fields_ = ([(n, ctypes.c_int32) for n in ("kind", "weight_mode", "curve", "gt_dtype")]
                + [("flags", ctypes.c_uint32), ("table_k", ctypes.c_int32), ("dpt_mult", ctypes.c_float), ("bg", ctypes.c_float * 3)]
                + [(n, VisMap) for n in ("img", "weight", "acc", "gt", "msk")]
                + [(n, ctypes.c_void_p) for n in ("M", "near_far", "table")])


# every symbol include/*.h declares: name -> (restype, argtypes)
_P = c_void_p
SYMBOLS = {
    "envgs_raster_scan_temp_bytes": (c_size_t, [ctypes.c_int32]),
    "envgs_raster_sort_temp_bytes": (c_size_t, [c_uint32, ctypes.c_int32, ctypes.c_int32]),
    "envgs_raster_project": (c_int, [ctypes.POINTER(RasterCfg)] + [_P] * 15 + [_P, c_size_t, ctypes.POINTER(c_uint32), _P]),
    "envgs_raster_bin_and_render": (c_int, [ctypes.POINTER(RasterCfg), c_uint32] + [_P] * 7 + [_P, c_size_t] + [_P] * 7 + [_P]),
    "envgs_raster_tile_queue_bytes": (c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "envgs_raster_bin_and_render_queued": (c_int, [ctypes.POINTER(RasterCfg), c_uint32] + [_P] * 7 + [_P, c_size_t] + [_P] * 8 + [_P]),
    "envgs_raster_backward_queued": (c_int, [ctypes.POINTER(RasterCfg), c_uint32] + [_P] * 30 + [_P]),
    "envgs_raster_render_audit": (c_int, [ctypes.POINTER(RasterCfg)] + [_P] * 11 + [ctypes.c_int32, _P, _P]),
    "envgs_raster_backward": (c_int, [ctypes.POINTER(RasterCfg), c_uint32] + [_P] * 29 + [_P]),
    "envgs_bvh_temp_bytes": (c_size_t, [ctypes.c_int32]),
    "envgs_bvh_node_floats": (c_size_t, [ctypes.c_int32]),
    "envgs_bvh_build": (c_int, [ctypes.c_int32, _P, _P, _P, _P, c_size_t, ctypes.c_int32, _P]),
    "envgs_bvh_refit": (c_int, [ctypes.c_int32, _P, _P, _P, _P, _P, c_size_t, ctypes.c_int32, _P]),
    "envgs_bvh_quality": (c_int, [ctypes.c_int32, _P, _P, _P]),
    "envgs_trace_ray_sort_temp_bytes": (c_size_t, [ctypes.c_int32]),
    "envgs_trace_ray_order": (c_int, [ctypes.c_int32, _P, _P, _P, ctypes.c_int32, _P, _P, _P, c_size_t, _P]),
    "envgs_trace_forward": (c_int, [ctypes.POINTER(TraceCfg)] + [_P] * 22 + [ctypes.POINTER(TraceLists), _P]),
    "envgs_trace_backward": (c_int, [ctypes.POINTER(TraceCfg)] + [_P] * 35 + [ctypes.POINTER(TraceLists), _P]),
    "envgs_trace_backward_join": (c_int, [_P]),
    "envgs_sh_colors_forward": (c_int, [ctypes.c_int32] * 4 + [_P] * 7 + [_P]),
    "envgs_sh_colors_backward": (c_int, [ctypes.c_int32] * 4 + [_P] * 9 + [_P]),
    "envgs_surfel_quads": (c_int, [ctypes.c_int32] + [_P] * 5 + [_P]),
    "envgs_blend_forward": (c_int, [ctypes.c_int32] * 3 + [_P] * 3 + [_P]),
    "envgs_blend_backward": (c_int, [ctypes.c_int32] * 3 + [_P] * 5 + [_P]),
    "envgs_bounce_rays_forward": (c_int, [ctypes.c_int32] + [_P] * 8 + [_P]),
    "envgs_bounce_rays_backward": (c_int, [ctypes.c_int32] + [_P] * 13 + [_P]),
    "envgs_bounce_blend_forward": (c_int, [ctypes.c_int32] + [_P] * 5 + [_P]),
    "envgs_bounce_blend_backward": (c_int, [ctypes.c_int32] + [_P] * 8 + [_P]),
    "envgs_bounce_pack_mid": (c_int, [ctypes.c_int32, _P, ctypes.c_int32, ctypes.c_int32] + [_P] * 8 + [_P]),
    "envgs_reflect_forward": (c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float] + [_P] * 8 + [_P]),
    "envgs_reflect_backward": (c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float] + [_P] * 11 + [_P]),
    "envgs_select_acc": (c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, _P, _P, _P]),
    "envgs_reflect_filtered_forward": (c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_int32] + [_P] * 10 + [_P]),
    "envgs_reflect_filtered_backward": (c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_int32] + [_P] * 13 + [_P]),
    "envgs_blend_filtered_forward": (c_int, [ctypes.c_int32] * 4 + [_P] * 6 + [_P]),
    "envgs_blend_filtered_backward": (c_int, [ctypes.c_int32] * 4 + [_P] * 7 + [_P]),
    "envgs_surface_normal_forward": (c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float] + [_P] * 4 + [_P]),
    "envgs_surface_normal_backward": (c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float] + [_P] * 5 + [_P]),
    "envgs_surfel_inputs_forward": (c_int, [ctypes.POINTER(SurfelInputsArgs), _P]),
    "envgs_surfel_inputs_backward": (c_int, [ctypes.POINTER(SurfelInputsArgs), _P]),
    "envgs_fused_adam": (c_int, [ctypes.c_int32, ctypes.POINTER(AdamTensor), ctypes.c_float, ctypes.c_float, ctypes.c_float, _P]),
    "envgs_compact_temp_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "envgs_compact_scan": (c_int, [ctypes.c_int64, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "envgs_compact_gather": (c_int, [ctypes.c_int32, ctypes.POINTER(RowsTensor), ctypes.c_int64, _P, _P, _P]),
    "envgs_compact_gather_rows": (c_int, [ctypes.c_int32, ctypes.POINTER(RowsTensor), ctypes.c_int64, ctypes.c_int64, _P, _P, _P]),
    "envgs_knn3_mean_dist2": (c_int, [ctypes.c_int32, _P, _P, _P]),
    "envgs_densify_stats": (c_int, [ctypes.c_int64, ctypes.c_int32] + [_P] * 8 + [_P]),
    "envgs_densify_plan_temp_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "envgs_densify_plan": (c_int, [ctypes.POINTER(DensifyPlanArgs), _P]),
    "envgs_densify_split_stds": (c_int, [ctypes.c_int64, ctypes.c_int32] + [_P] * 5 + [ctypes.c_int64, _P]),
    "envgs_densify_rewrite": (c_int, [ctypes.POINTER(DensifyRewriteArgs), _P]),
    "envgs_weight_select_temp_bytes": (ctypes.c_size_t, []),
    "envgs_weight_select": (c_int, [ctypes.c_int64, _P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, ctypes.c_size_t, _P]),
    "envgs_visibility_mask_temp_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "envgs_visibility_mask": (c_int, [ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "envgs_oversize_plan": (c_int, [ctypes.c_int64, c_uint32, ctypes.c_float, ctypes.c_float] + [_P] * 8 + [_P]),
    "envgs_tsdf_integrate": (c_int, [ctypes.POINTER(TsdfVolume), ctypes.POINTER(TsdfViews), ctypes.c_float, _P]),
    "envgs_mesh_temp_bytes": (c_size_t, [ctypes.c_int32] * 3),
    "envgs_mesh_count": (c_int, [ctypes.POINTER(TsdfVolume), ctypes.c_float, ctypes.c_float, _P, c_size_t, _P, _P]),
    "envgs_mesh_extract": (c_int, [ctypes.POINTER(TsdfVolume), ctypes.c_float, _P, c_size_t, c_uint32, c_uint32, _P, _P, _P, _P]),
    "envgs_mesh_components_temp_bytes": (c_size_t, [c_uint32, c_uint32]),
    "envgs_mesh_components": (c_int, [c_uint32, c_uint32, _P, _P, c_size_t] + [_P] * 5 + [_P]),
    "envgs_mesh_select_temp_bytes": (c_size_t, [c_uint32, c_uint32]),
    "envgs_mesh_select_count": (c_int, [c_uint32, c_uint32, _P, _P, _P, c_size_t, _P, _P]),
    "envgs_mesh_select_emit": (c_int, [c_uint32, c_uint32] + [_P] * 4 + [_P, c_size_t, c_uint32, c_uint32] + [_P] * 4 + [_P]),
    "envgs_mesh_simplify_temp_bytes": (c_size_t, [c_uint32, c_uint32] + [ctypes.c_int32] * 3),
    "envgs_mesh_simplify_cluster": (c_int, [c_uint32, c_uint32, _P, _P, _P] + [ctypes.c_float] * 4 + [ctypes.c_int32] * 3 + [_P, c_size_t] + [_P] * 6 + [_P]),
    "envgs_mesh_sample_temp_bytes": (c_size_t, [c_uint32, c_uint32]),
    "envgs_mesh_sample_count": (c_int, [c_uint32, c_uint32, _P, _P, ctypes.c_float, c_uint32, _P, c_size_t, _P, _P]),
    "envgs_mesh_sample_emit": (c_int, [c_uint32, c_uint32, _P, _P, _P, c_uint32, _P, c_size_t, c_uint32, _P, _P, _P, _P]),
    "envgs_points_grid_temp_bytes": (c_size_t, [c_uint32] + [ctypes.c_int32] * 3),
    "envgs_points_grid_build": (c_int, [c_uint32, _P] + [ctypes.c_float] * 4 + [ctypes.c_int32] * 3 + [_P, c_size_t, _P, _P, _P]),
    "envgs_points_nearest": (c_int, [c_uint32, _P] + [ctypes.c_float] * 5 + [ctypes.c_int32] * 3 + [_P] * 4 + [_P]),
    "envgs_points_thin_temp_bytes": (c_size_t, [c_uint32]),
    "envgs_points_thin_begin": (c_int, [c_uint32, _P, _P, c_size_t, _P, _P]),
    "envgs_points_thin_round": (c_int, [c_uint32, _P, ctypes.c_float, ctypes.c_int32, c_uint32] + [ctypes.c_float] * 4 + [ctypes.c_int32] * 4
                                + [_P, _P, _P, c_size_t] + [c_uint32] * 3 + [_P, _P]),
    "envgs_points_thin_keep": (c_int, [c_uint32, _P, c_size_t, _P, _P]),
    "envgs_mesh_cull_vertices": (c_int, [c_uint32, _P, ctypes.POINTER(CullViews), ctypes.c_int32, _P, _P]),
    "envgs_mesh_cull_faces": (c_int, [c_uint32, c_uint32, _P, _P, _P, _P]),
    "envgs_points_transform": (c_int, [c_uint32, _P, ctypes.POINTER(ctypes.c_float), _P, _P]),
    "envgs_points_register_temp_bytes": (c_size_t, [c_uint32]),
    "envgs_points_register_sums": (c_int, [c_uint32, _P, ctypes.POINTER(ctypes.c_float)] + [ctypes.c_float] * 5 + [ctypes.c_int32] * 3
                                   + [_P, _P, ctypes.POINTER(ctypes.c_double), _P, c_size_t] + [_P] * 4 + [_P]),
    "envgs_points_voxel_keys": (c_int, [c_uint32, _P] + [ctypes.c_float] * 4 + [ctypes.c_int32] * 3 + [_P, _P]),
    "envgs_points_voxel_temp_bytes": (c_size_t, [c_uint32]),
    "envgs_points_voxel_cluster": (c_int, [c_uint32, _P] + [ctypes.c_float] * 4 + [ctypes.c_int32] * 3 + [_P, _P, _P, c_size_t, _P, _P, _P]),
    "envgs_points_voxel_finish": (c_int, [c_uint32, _P] + [ctypes.c_float] * 4 + [ctypes.c_int32] * 3 + [_P, c_size_t, c_uint32, _P, _P]),
    "envgs_points_in_polygon": (c_int, [c_uint32, _P, ctypes.c_int32, ctypes.c_double, ctypes.c_double, c_uint32, _P, _P, _P]),
    "envgs_fuse_consistency": (c_int, [ctypes.c_int32, ctypes.c_int32, _P, ctypes.POINTER(FuseSources), ctypes.c_float, ctypes.c_float, ctypes.c_int32,
                                       _P, _P, _P]),
    "envgs_fuse_temp_bytes": (c_size_t, [ctypes.c_int32] * 3),
    "envgs_fuse_count": (c_int, [ctypes.c_int32] * 3 + [_P, _P, _P, c_uint32, ctypes.c_float, _P, _P, _P, c_size_t, _P, _P]),
    "envgs_fuse_emit": (c_int, [ctypes.c_int32] * 3 + [_P, _P, _P, c_size_t, _P, _P, _P, c_uint32] + [_P] * 4 + [_P]),
    "envgs_mesh_raster_small_max": (ctypes.c_int32, []),
    "envgs_mesh_raster_temp_bytes": (c_size_t, [ctypes.c_int32] * 3),
    "envgs_mesh_raster": (c_int, [c_uint32, c_uint32, _P, _P, _P, ctypes.POINTER(MeshRasterViews), ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                  ctypes.c_int32, _P, c_size_t] + [_P] * 7 + [_P]),
    "envgs_l1_ssim_partial_count": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "envgs_l1_ssim_forward": (c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P, _P]),
    "envgs_l1_ssim_backward": (c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P, ctypes.c_float, ctypes.c_float, _P, _P]),
    "envgs_image_metrics_partial_count": (ctypes.c_int64, [ctypes.c_int32] * 4),
    "envgs_image_metrics": (c_int, [ctypes.c_int32] * 4 + [_P, ctypes.POINTER(ctypes.c_int64), _P, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, _P, _P, _P]),
    "envgs_visualize_depth_range_temp_bytes": (c_size_t, []),
    "envgs_visualize_depth_range": (c_int, [ctypes.c_int32] * 3 + [_P, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_int64, _P, _P, c_size_t, _P]),
    "envgs_visualize_planes": (c_int, [ctypes.c_int32, ctypes.POINTER(VisPlane)] + [ctypes.c_int32] * 7 + [_P, _P]),
    "envgs_depth_percentiles_temp_bytes": (c_size_t, []),
    "envgs_depth_percentiles": (c_int, [ctypes.c_int64, _P, ctypes.c_int64, _P, _P, c_size_t, _P]),
    "envgs_supervisor_partial_count": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64]),
    "envgs_supervisor_forward": (c_int, [ctypes.POINTER(SupervisorArgs), _P]),
    "envgs_supervisor_finish": (c_int, [ctypes.POINTER(SupervisorArgs), _P, _P]),
    "envgs_supervisor_backward": (c_int, [ctypes.c_int64, _P, _P, _P, _P]),
    "envgs_debug_set": (None, [ctypes.c_int32, ctypes.c_int32]),
    "envgs_debug_get": (ctypes.c_int32, [ctypes.c_int32]),
    "envgs_prof_enable": (None, [c_int]),
    "envgs_prof_select": (None, [ctypes.c_uint64]),
    "envgs_prof_read": (c_int, [c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int)]),
    "envgs_prof_kernel_name": (ctypes.c_char_p, [c_int]),
}


LIB_DIAG_PATH = os.path.join(HERE, "libenvgs_hip_diag.so")
_libs = {}
_selected = {"kind": "product"}


def _open(path):
    if not os.path.exists(path):
        raise RuntimeError(
            "envgs_amd: %s is missing. Build it with `python -m envgs_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the render-and-trace path." % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """The library every entry point of the package calls into: the PRODUCT build, unless a test / `bench.py --diag` selected the diagnostic one."""
    global _lib
    kind = _selected["kind"]
    lib = _libs.get(kind)
    if lib is None:
        lib = _libs[kind] = _open(LIB_PATH if kind == "product" else LIB_DIAG_PATH)
    _lib = lib
    return lib


def select(kind):
    """"product" (default) or "diag": the diagnostic build adds the exact-math raster kernels (ENVGS_DBG_RASTER_EXACT) and the LDS alignment trap
    of the cooperative collection (csrc: ENVGS_DIAG).  Both export the same C-ABI; each keeps its own diagnostic switches and timers.  Returns the previous kind."""
    if kind not in ("product", "diag"):
        raise ValueError(kind)
    old = _selected["kind"]
    _selected["kind"] = kind
    load()
    return old


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def check(rc, what):
    if rc != 0:
        raise RuntimeError("envgs_amd: %s failed with code %d (%s)" % (
            what, rc, {-1: "bad argument", -2: "temp buffer too small"}.get(rc, "hipError_t")))
