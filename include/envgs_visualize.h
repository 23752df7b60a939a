/*
 * envgs_visualize.h -- C-ABI of the image output: the visualizer's maps as finished 8-bit RGBA on the device.
 *
 * Semantics: easyvolcap/runners/visualizers/volumetric_video_visualizer.py, generate_type (:84-268), with the lines it depends on, and the
 * quantisation of easyvolcap/utils/data_utils.py save_image (:1230), all in float32, one rounding per operation (the file is built with
 * -ffp-contract=off; / and sqrtf are the correctly rounded ones).
 *
 * Byte rule (save_image :1230, `(img * 255).clip(0, 255).round().astype(uint8)`):
 *   b = (uint8) rintf(min(max(v * 255.0f, 0.0f), 255.0f)), ties to even as np.round; a NaN gives 0 (the reference's cast of a NaN is undefined).
 *   Every other clip keeps a NaN a NaN, as torch.clip does, so a NaN anywhere ends as the byte 0.
 *
 * Plane kinds (r, g, b of a pixel; `a` is the alpha value, see below):
 *   COLOR   three channels of `img` (RENDER :193-197, SURFACE :151-153, SPECULAR with 3 channels :205-210), optionally weighted by the
 *           one-channel map `weight`:  ONE_MINUS  c * (1 - w)   DIFFUSE, envgs_sampler.py:413;   TWICE  (c * w) * 2   REFLECTION, envgs_sampler.py:476.
 *   GRAY    one channel of `img` on three (ALPHA :159-163, SPECULAR with 1 channel :208, ROUGHNESS :212-216).
 *   DEPTH   (:123-138) curve LINEAR: the depth itself; NORMALIZE (depth_utils.py normalize_depth :65-71, depth_curve_fn :74-77):
 *           v = 1 - (d - near) / (far - near), clipped to [0, 1], then the colour map's clip to [1e-6f, (float)(1 - 1e-6)] (color_utils.py:858-859).
 *           Both times `* dpt_mult` (:131) comes last.  near / far are read from `near_far` (per image: {near, far}), which
 *           envgs_visualize_depth_range fills on the device.  far <= near gives v = 1 where d <= near and 0 elsewhere (the reference divides by 0).
 *           Colour map: table == NULL is the reference's default 'linear' (color_utils.py:887-888), v on three channels.  Otherwise
 *           table is (table_k, 3) float32 with uniform knots and the rule of colormap_list (:907-917) holds, quirks included:
 *             for i in 0 .. K-2:  b0 = (float)(i / (K-1.0)), db = (float)((i+1) / (K-1.0) - i / (K-1.0))        (doubles, rounded once)
 *                                 t = (v - b0) / db;  if (0 <= t <= 1)  colour += c[i+1] * t + c[i] * (1 - t)
 *           -- a value exactly on an inner knot is counted by both segments.  The kernel evaluates the segment floor(v * (K-1)) and its two
 *           neighbours in the order of i; a segment further away cannot pass the test for K <= ENVGS_VIS_MAX_TABLE, and a failed test adds
 *           a zero (the table must be finite).
 *   NORMAL  (NORMAL :90-101, SURFACE_NORMAL :110-121, math_utils.py normalize :6-8)
 *           u = n / (sqrtf((nx*nx + ny*ny) + nz*nz) + 1e-8f);  m_j = (u0*M[j][0] + u1*M[j][1]) + u2*M[j][2]  (`norm @ R.mT`; M == NULL: m = u);
 *           m_y = -m_y, m_z = -m_z;  c = m * 0.5f + 0.5f;  c = c * acc (acc == NULL: left out).
 *   GT      `gt` (float32, or uint8 read as k / 255.0f), three channels, filled where ENVGS_VIS_BG is set and msk is given (:229-231):
 *           g = gt + bg * (1 - msk).
 *   ERROR   (:233-234) e = clip((d0*d0 + d1*d1) + d2*d2, 0, 1), d = c - g, on three channels; c by the COLOR rule, g by the GT rule.
 *
 * Alpha byte (:236-244): prediction planes `acc`; GT planes `msk`; ERROR planes clip(msk + acc, 0, 1); 255 where a map that rule reads is NULL or
 * ENVGS_VIS_OPAQUE is set (store_alpha_channel = False).
 *
 * Canvas (:252-266, uncrop_output_images): out is (n_planes, B, Ho, Wo, 4) uint8; the H x W maps land at column x0, row y0; every byte outside
 * the crop is 0.  One lane per output pixel and plane, one 32-bit store per lane.
 */
#ifndef ENVGS_VISUALIZE_H
#define ENVGS_VISUALIZE_H

#include <stddef.h>
#include <stdint.h>

#include "envgs_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ENVGS_VIS_MAX_PLANES 16
#define ENVGS_VIS_MAX_TABLE 65536

#define ENVGS_VIS_COLOR 0
#define ENVGS_VIS_GRAY 1
#define ENVGS_VIS_DEPTH 2
#define ENVGS_VIS_NORMAL 3
#define ENVGS_VIS_GT 4
#define ENVGS_VIS_ERROR 5

#define ENVGS_VIS_WEIGHT_NONE 0
#define ENVGS_VIS_WEIGHT_ONE_MINUS 1
#define ENVGS_VIS_WEIGHT_TWICE 2

#define ENVGS_VIS_CURVE_LINEAR 0
#define ENVGS_VIS_CURVE_NORMALIZE 1

#define ENVGS_VIS_GT_F32 0
#define ENVGS_VIS_GT_U8 1

#define ENVGS_VIS_OPAQUE 1u /* alpha byte 255 whatever maps are given */
#define ENVGS_VIS_BG 2u     /* bg holds a background colour */

/* A map read in place: ELEMENT strides {batch, channel, row, column}; ptr == NULL: no such map.  A one-channel map ignores the channel stride.
 * The channel and column strides must fit an int32. */
typedef struct envgs_vis_map {
    const void *ptr;
    int64_t stride[4];
} envgs_vis_map;

typedef struct envgs_vis_plane {
    int32_t kind, weight_mode, curve, gt_dtype;
    uint32_t flags;
    int32_t table_k;
    float dpt_mult;
    float bg[3];
    envgs_vis_map img, weight, acc, gt, msk; /* float32, but gt: gt_dtype */
    const float *M;                          /* NORMAL: (B, 3, 3) contiguous, or NULL */
    const float *near_far;                   /* DEPTH / NORMALIZE: (B, 2) */
    const float *table;                      /* DEPTH / NORMALIZE: (table_k, 3) contiguous, or NULL */
} envgs_vis_plane;

ENVGS_API size_t envgs_visualize_depth_range_temp_bytes(void);

/* near_far[b] = {the rank_near-th, the rank_far-th} smallest of the H * W depths of image b (0-based ranks, computed by the host: the reference's
 * n = int(N * p) gives rank_near = n - 1, rank_far = N - n), one exact radix select per image, -0 ranked with +0.  depth: float32,
 * strides {batch, row, column}.  No read-back: the plane kernel reads near_far on the device.
 * B == 0 returns 0 without a launch; B < 0, H or W < 1, H * W >= 2^31, a rank outside [0, H * W), a NULL pointer: ENVGS_ERR_BAD_ARG;
 * temp_bytes too small: ENVGS_ERR_TEMP_TOO_SMALL. */
ENVGS_API int envgs_visualize_depth_range(int32_t B, int32_t H, int32_t W, const float *depth, const int64_t *strides, int64_t rank_near,
                                          int64_t rank_far, float *near_far, void *temp, size_t temp_bytes, void *stream);

/* out: (n_planes, B, Ho, Wo, 4) uint8, contiguous, 4-byte aligned.  planes: a HOST array, copied into the kernel's arguments.
 * One launch, no allocation, no host synchronisation.  n_planes == 0 or B == 0 returns 0 without a launch.
 * ENVGS_ERR_BAD_ARG without a launch: n_planes outside [0, 16], B < 0, a size < 1, a crop that leaves the canvas, Ho * Wo >= 2^31, B > 65535,
 * a NULL or misaligned out, an unknown kind / mode / curve / dtype, a plane without the map its kind reads (img: COLOR, GRAY, DEPTH, NORMAL,
 * ERROR; gt: GT, ERROR; weight where weight_mode is set; near_far for NORMALIZE), table_k outside [2, ENVGS_VIS_MAX_TABLE] with a table,
 * a channel or column stride beyond an int32. */
ENVGS_API int envgs_visualize_planes(int32_t n_planes, const envgs_vis_plane *planes, int32_t B, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                     int32_t x0, int32_t y0, uint8_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVGS_VISUALIZE_H */
