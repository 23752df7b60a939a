/*
 * envgs_supervisor.h -- C-ABI of the fused geometry regularisers (the terms of easyvolcap/models/supervisors/envgs_supervisor.py:139-235
 * that EnvGS trains with next to the image loss of envgs_loss.h; configs/models/envgs.yaml:70-81), one view at a time:
 *
 *   norm_loss         a = unit(R unit(norm_map)), g = unit(2 prior - 1), unit(x) = x / (|x| + 1e-8);  mean of  s * (sum|a - g| + 1 - cos(a, g))
 *   gs_norm_loss      mean of  s * (1 - <norm_map, surf_norm_map>)
 *   msk_loss          mean (acc - m)^2,  m = [msk > 0.5 and |prior| > 0.25]
 *   gs_dist_loss      mean dist_map
 *   env_opacity_loss  'sparse': mean(log v + log(1 - v)), v = clamp(o, 1e-3, 1 - 1e-3);  'l1': mean |1 - o|
 *
 * s is 1, acc, the depth scale, or their product (per term, by flag); both are constants for the gradient.  The depth scale is
 * clip(1 - (d - near) / (far - near), 0, 1) with near / far the n-th smallest / largest depth, n = int(0.01 N) (depth_utils.py:65-71): exact
 * order statistics, found on the device by a radix select and read from a device buffer, so that nothing returns to the host.
 * When the two percentiles coincide (far == near: more than 99 % of the depths hold one value) the formula is 0 / 0 at every pixel with
 * d == near, and the reference's loss is NaN.  Here, deliberately, the scale is then 0 where d == near, 0 where d > near and 1 where d < near
 * (the clip is fminf(fmaxf(x, 0), 1), which returns its other operand for a NaN), and every output stays finite.
 *
 * Every tensor is addressed as base + row * row_stride (+ channel * channel_stride), strides in ELEMENTS, so channel-last maps and (3, H, W)
 * planes are both read in place.  Outputs are contiguous.
 */
#ifndef ENVGS_SUPERVISOR_H
#define ENVGS_SUPERVISOR_H

#include <stddef.h>
#include <stdint.h>

#include "envgs_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

/* columns of the partial-sum buffer and of envgs_supervisor_finish's output */
#define ENVGS_SUP_NORM 0
#define ENVGS_SUP_GS_NORM 1
#define ENVGS_SUP_MSK 2
#define ENVGS_SUP_DIST 3
#define ENVGS_SUP_ENV 4
#define ENVGS_SUP_TERMS 5

/* flags: which terms are evaluated, and how the two normal terms are scaled */
#define ENVGS_SUP_F_NORM (1u << 0)
#define ENVGS_SUP_F_GS_NORM (1u << 1)
#define ENVGS_SUP_F_MSK (1u << 2)
#define ENVGS_SUP_F_DIST (1u << 3)
#define ENVGS_SUP_F_ENV_SPARSE (1u << 4)
#define ENVGS_SUP_F_ENV_L1 (1u << 5)
#define ENVGS_SUP_F_NORM_ACC (1u << 6)
#define ENVGS_SUP_F_NORM_DPT (1u << 7)
#define ENVGS_SUP_F_GS_NORM_ACC (1u << 8)
#define ENVGS_SUP_F_GS_NORM_DPT (1u << 9)
#define ENVGS_SUP_F_ALL ((1u << 10) - 1u)

typedef struct envgs_supervisor_args {
    int64_t N, P;                       /* pixels (>= 100 when a depth scale is on, >= 1 otherwise); environment surfels (0 without that term) */
    uint32_t flags, reserved0;
    float weight[ENVGS_SUP_TERMS];      /* the loss weights: they scale the gradient maps */
    float reserved1;
    /* inputs; a pointer may be NULL when no selected term reads it */
    const float *norm_map, *surf_norm_map, *acc_map, *dpt_map, *dist_map, *env_opacity, *prior, *msk;
    const float *R;                     /* 9 floats, row-major world-to-camera rotation */
    const float *near_far;              /* 2 floats: envgs_depth_percentiles' output */
    int64_t norm_map_row, norm_map_ch, surf_norm_map_row, surf_norm_map_ch, acc_map_row, dpt_map_row, dist_map_row, env_opacity_row, prior_row,
        prior_ch, msk_row;
    /* d(sum_t weight_t * mean_t) / d input, contiguous (N,3), (N,3), (N), (N), (P); NULL = not wanted */
    float *g_norm_map, *g_surf_norm_map, *g_acc_map, *g_dist_map, *g_env_opacity;
    float *partial;                     /* (envgs_supervisor_partial_count, ENVGS_SUP_TERMS) floats out: per-workgroup sums of each term */
} envgs_supervisor_args;

/* Scratch of envgs_depth_percentiles (histograms and the select state). */
ENVGS_API size_t envgs_depth_percentiles_temp_bytes(void);

/* near_far[0] = the n-th smallest, near_far[1] = the n-th largest of the N floats depth[i * stride], n = N / 100; bit-exact elements of the
 * input (-0 counts as +0; NaNs are unspecified).  100 <= N < 2^31. */
ENVGS_API int envgs_depth_percentiles(int64_t N, const float *depth, int64_t stride, float *near_far, void *temp, size_t temp_bytes, void *stream);

/* Rows of the partial-sum buffer for N pixels and P environment surfels. */
ENVGS_API int64_t envgs_supervisor_partial_count(int64_t N, int64_t P);

/* One pass over the pixels (and the P opacities): per-workgroup sums of every selected term, and the gradient maps that are asked for. */
ENVGS_API int envgs_supervisor_forward(const envgs_supervisor_args *args, void *stream);

/* out[t] = mean of term t (t < ENVGS_SUP_TERMS; 0 for a term that is off), out[ENVGS_SUP_TERMS] = sum_t weight_t * out[t]: the partial sums
 * added in double by one workgroup.  out: 6 floats on the device. */
ENVGS_API int envgs_supervisor_finish(const envgs_supervisor_args *args, float *out, void *stream);

/* dst[i] = grad_out[0] * src[i], i < n: the chain rule over all gradient maps at once (they are one allocation).  grad_out: device scalar. */
ENVGS_API int envgs_supervisor_backward(int64_t n, const float *src, const float *grad_out, float *dst, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVGS_SUPERVISOR_H */
