/*
 * envgs_metrics.h -- C-ABI of the image evaluation: per-image MSE, PSNR and SSIM of a batch, finished on the device.
 *
 * Semantics: easyvolcap/utils/metric_utils.py (psnr :21-25, ssim :28-64) per image of the batch.
 *   mse  = mean((x - y)^2) over all channels and pixels                               (loss_utils.mse :311-312)
 *   psnr = 10 log10(1 / max(mse, 1e-10))                                               (identical images: 100 dB)
 *   ssim = mean over channels and pixels of the SSIM map of an 11-tap sigma-1.5 Gaussian window built in float32, ZERO padding of 5 on every
 *          side, each channel filtered on its own, C1 = 0.01^2, C2 = 0.03^2.  No lower size limit: a window wider than the image hangs over zeros.
 * The reference runs 6 grouped conv2d plus elementwise kernels and one .item() per metric and view; here one kernel writes one record per
 * 16x16 tile and channel and a second one, one workgroup per image, adds the records in a fixed order and finishes the row in float64.
 * No float atomics: two calls give identical bytes, and the row of image b does not depend on the other images of the batch.
 */
#ifndef ENVGS_METRICS_H
#define ENVGS_METRICS_H

#include <stddef.h>
#include <stdint.h>

#include "envgs_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dtype codes of the ground truth; a uint8 value k is read as the correctly rounded float32 quotient k / 255.0f (img.float() / 255) */
#define ENVGS_METRICS_GT_F32 0
#define ENVGS_METRICS_GT_U8 1

/* columns of a row of `out` */
#define ENVGS_METRICS_MSE 0
#define ENVGS_METRICS_PSNR 1
#define ENVGS_METRICS_SSIM 2
#define ENVGS_METRICS_COLS 3

/* Number of (ssim_sum, sq_err_sum) DOUBLE pairs envgs_image_metrics writes into `partial`: one per image, channel and 16x16 tile.
 * 0 for an empty batch or a non-positive size. */
ENVGS_API int64_t envgs_image_metrics_partial_count(int32_t B, int32_t C, int32_t H, int32_t W);

/* pred: float32; gt: float32 or uint8 (gt_dtype).  Both are read in place through ELEMENT strides {batch, channel, row, column} (host arrays
 * of four), so (B,H,W,C) images, (B,C,H,W) images and a [..., :3] slice of a 4-channel image need no copy.
 * partial: (count, 2) doubles, scratch.  out: (B, ENVGS_METRICS_COLS) doubles, contiguous.
 * B == 0 returns 0 without a launch.  H, W or C < 1, B < 0, a NULL pointer with B > 0, an unknown gt_dtype or more than 2^31 - 1 tiles
 * return ENVGS_ERR_BAD_ARG without a launch.  No host synchronisation, no allocation. */
ENVGS_API int envgs_image_metrics(int32_t B, int32_t C, int32_t H, int32_t W, const float *pred, const int64_t *pred_strides, const void *gt,
                                  const int64_t *gt_strides, int32_t gt_dtype, double *partial, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVGS_METRICS_H */
