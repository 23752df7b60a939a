/*
 * envgs_densify.h -- C-ABI of the densify / prune support kernels (third "next" row).
 *
 * The reference prunes with one boolean-mask gather per tensor -- parameter, exp_avg and exp_avg_sq of each of its 8 parameter groups
 * (`_prune_optimizer`, easyvolcap/utils/gaussian2d_utils.py:536-560; `prune_stats` :640-648): 24+ `tensor[mask]` calls, each its own
 * nonzero + gather + sync.  Here: ONE prefix scan of the keep mask (`envgs_compact_scan`, the caller reads the kept count once) and ONE
 * gather launch that compacts up to ENVGS_COMPACT_MAX_TENSORS row-major tensors of the per-Gaussian SoA (`envgs_compact_gather`).
 * Rows keep their relative order, exactly like `tensor[mask]`.
 *
 * `envgs_knn3_mean_dist2` is the initialisation helper the reference takes from `simple_knn.distCUDA2`
 * (gaussian2d_utils.py:432-440: scales = sqrt(mean squared distance to the 3 nearest neighbours)): exact brute force, LDS-tiled.
 */
#ifndef ENVGS_DENSIFY_H
#define ENVGS_DENSIFY_H

#include <stddef.h>
#include <stdint.h>

#include "envgs_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ENVGS_COMPACT_MAX_TENSORS 32

typedef struct envgs_rows_tensor {
    const void *src;         /* (P, row_bytes) contiguous */
    void *dst;               /* (>= kept, row_bytes) contiguous */
    int64_t row_bytes;       /* multiple of 4 */
} envgs_rows_tensor;

/* Scratch bytes of envgs_compact_scan for P rows. */
ENVGS_API size_t envgs_compact_temp_bytes(int64_t P);

/* positions[i] = number of kept rows before row i (P uint32, device); *n_kept (device uint32) = total kept.  keep: P bytes, non-zero = keep. */
ENVGS_API int envgs_compact_scan(int64_t P, const uint8_t *keep, uint32_t *positions, uint32_t *n_kept, void *temp, size_t temp_bytes,
                                 void *stream);

/* dst_t[positions[i]] = src_t[i] for every kept row i and every tensor t (host array of `count` descriptors, passed by value). */
ENVGS_API int envgs_compact_gather(int32_t count, const envgs_rows_tensor *tensors, int64_t P, const uint8_t *keep, const uint32_t *positions,
                                   void *stream);

/* The same gather for a caller that knows the kept count without reading *n_kept back: every dst has out_rows rows, and a kept row whose
 * position is at or beyond out_rows is dropped, never written. */
ENVGS_API int envgs_compact_gather_rows(int32_t count, const envgs_rows_tensor *tensors, int64_t P, int64_t out_rows, const uint8_t *keep,
                                        const uint32_t *positions, void *stream);

/* out[i] = mean of the squared distances from xyz[i] to its 3 nearest OTHER points (fewer if P < 4; 0 for P == 1).  xyz (P,3), out (P). */
ENVGS_API int envgs_knn3_mean_dist2(int32_t P, const float *xyz, float *out, void *stream);

/* ---- device-resident densification (SurfelSet(device_schedule=True)) ----------------------------------------------------------------------
 *
 * The per-step statistics of `add_densification_stats` (gaussian2d_utils.py:901-909 + the radius update of gaussian2d_sampler.py:330-332)
 * in ONE launch without a host round trip, and the first three stages of `densify_and_prune` (clone, split, prune by opacity / gradient,
 * :866-885) as ONE plan, ONE read-back and ONE rewrite of every parameter, both Adam moments and the four statistics.  A clone child
 * inherits the scale, opacity and statistics its parent is judged by, so what the later stages decide for the child is known from the
 * parent: the result of the three stages is a closed-form function of the set before the pass.
 */

/* For every surfel with filter != 0: denom += 1; xyz_gradient_accum += sqrt(gx^2 + gy^2 (+ gz^2)) (fp32, summed left to right, no FMA);
 * xyz_weight_accum += weight (if given); max_radii2D = max(max_radii2D, (float)radii) (if given).  grad (P, cols), cols 2 or 3. */
ENVGS_API int envgs_densify_stats(int64_t P, int32_t cols, const float *grad, const uint8_t *filter, const float *weight, const int32_t *radii,
                                  float *xyz_gradient_accum, float *denom, float *max_radii2D, float *xyz_weight_accum, void *stream);

#define ENVGS_GROW_MAX_CHILDREN 16            /* N, the children per split surfel */

/* envgs_densify_plan_args.flags: which optional thresholds are given */
#define ENVGS_PLAN_MIN_OPACITY 1u
#define ENVGS_PLAN_MIN_GRADIENT 2u
#define ENVGS_PLAN_SPLIT_SCREEN 4u

/* the bits of a surfel's byte in `cls`.  With avg(x) = x / denom in fp32, NaN -> 0:
 *   high = avg(ga) >= grad_threshold;  small = max(scal) <= size_limit;
 *   CLONE = small && high;  SPLIT = high && (!small || (SPLIT_SCREEN given && mr > split_screen_threshold));
 *   PRUNE_1 = (MIN_OPACITY given && opac < min_opacity) || (MIN_GRADIENT given && avg(ga) <= min_gradient && denom != 0): the surfel as it is;
 *   PRUNE_S = the same with avg(fl(ga * r)): its split children.  Only the one of the two that SPLIT selects is acted on.
 * The flag arrays: A = !SPLIT && !PRUNE_1;  B = CLONE && A;  D = SPLIT && !PRUNE_S;  E = CLONE && D;  S1 = SPLIT;  S2 = CLONE && SPLIT. */
#define ENVGS_GROW_CLS_CLONE 1u
#define ENVGS_GROW_CLS_SPLIT 2u
#define ENVGS_GROW_CLS_PRUNE_1 4u
#define ENVGS_GROW_CLS_PRUNE_S 8u

/* the words of `counters` (device; the host reads them back once) */
#define ENVGS_GROW_N_A 0                      /* originals kept as they are */
#define ENVGS_GROW_N_B 1                      /* clone children kept */
#define ENVGS_GROW_N_D 2                      /* kept split children of originals, per block */
#define ENVGS_GROW_N_E 3                      /* kept split children of clone children, per block */
#define ENVGS_GROW_N_S1 4                     /* originals selected for splitting */
#define ENVGS_GROW_N_S2 5                     /* clone children selected for splitting */
#define ENVGS_GROW_N_CLONE 6                  /* surfels cloned */
#define ENVGS_GROW_W_ALL 7                    /* max xyz_weight_accum, and max / min over the cloned surfels: order-preserving encodings, */
#define ENVGS_GROW_W_CLONE_MAX 8              /* internal to the rewrite */
#define ENVGS_GROW_W_CLONE_MIN 9
#define ENVGS_GROW_COUNTERS 16

typedef struct envgs_densify_plan_args {
    int64_t P;
    int32_t N;                                /* children per split surfel, 1 .. ENVGS_GROW_MAX_CHILDREN */
    uint32_t flags;
    float grad_threshold;
    float size_limit;                         /* size_threshold * spatial_scale */
    float split_screen_threshold;
    float min_opacity;
    float min_gradient;
    float r;                                  /* (float)(1 / (ratio N)): what a split child's gradient and radius statistics are scaled by */
    const float *ga, *dn, *mr, *wa;           /* xyz_gradient_accum, denom, max_radii2D, xyz_weight_accum: (P) each */
    const float *scal;                        /* (P,2) activated scales */
    const float *opac;                        /* (P) activated opacities; needed with ENVGS_PLAN_MIN_OPACITY */
    uint8_t *cls;                             /* out (P): class bits */
    uint32_t *scan;                           /* out (6 P): inclusive scan of the flag arrays [A|B|D|E|S1|S2] */
    uint32_t *counters;                       /* out (ENVGS_GROW_COUNTERS) */
    void *temp;
    size_t temp_bytes;                        /* >= envgs_densify_plan_temp_bytes(P) */
} envgs_densify_plan_args;

ENVGS_API size_t envgs_densify_plan_temp_bytes(int64_t P);

/* Decides every surfel and lays the result out: rows A, then B, then N blocks of (D then E), each in surfel order -- the order the three
 * staged stages leave.  Final rows = nA + nB + N (nD + nE).  6 P < 2^31. */
ENVGS_API int envgs_densify_plan(const envgs_densify_plan_args *args, void *stream);

/* stds (n_stds = N (nS1 + nS2), 3): (sx, sy, 0) of every split surfel, block after block, originals before clone children -- the argument of
 * the host's normal draw.  Rows at or beyond n_stds are not written. */
ENVGS_API int envgs_densify_split_stds(int64_t P, int32_t N, const uint8_t *cls, const uint32_t *scan, const uint32_t *counters, const float *scal,
                                       float *stds, int64_t n_stds, void *stream);

/* what a tensor of the rewrite is: decides the value of a row that is not a plain copy */
#define ENVGS_GROW_COPY 0                     /* a parameter: every child copies its parent */
#define ENVGS_GROW_MOMENT 1                   /* an Adam moment: children start at zero */
#define ENVGS_GROW_XYZ 2                      /* _xyz (P,3): split child = R(q / |q|) sample + xyz */
#define ENVGS_GROW_SCALING 3                  /* _scaling (P,2): split child = log(scal / (ratio N)) */
#define ENVGS_GROW_GRAD 4                     /* xyz_gradient_accum: split child * r */
#define ENVGS_GROW_DENOM 5                    /* denom: copied */
#define ENVGS_GROW_RADIUS 6                   /* max_radii2D: split child * r */
#define ENVGS_GROW_WEIGHT 7                   /* xyz_weight_accum: clone child * wmax0, split child * wmax1 */

typedef struct envgs_grow_tensor {
    const void *src;                          /* (P, row_bytes) contiguous */
    void *dst;                                /* (out_rows, row_bytes) contiguous */
    int64_t row_bytes;                        /* multiple of 4 */
    int32_t kind;
    int32_t reserved0;
} envgs_grow_tensor;

typedef struct envgs_densify_rewrite_args {
    int64_t P;
    int64_t out_rows;                         /* rows of every dst; no row at or beyond it is written */
    int64_t n_samples;                        /* rows of samples = N (nS1 + nS2) */
    int32_t N;
    int32_t count;                            /* tensors, <= ENVGS_COMPACT_MAX_TENSORS */
    double ratio_n;                           /* ratio N */
    float r;
    uint32_t reserved0;
    const uint8_t *cls;
    const uint32_t *scan;
    const uint32_t *counters;
    const float *scal;                        /* (P,2) activated scales */
    const float *rotation;                    /* (P,4) raw quaternions (r, x, y, z) */
    const float *samples;                     /* (n_samples, 3) */
    const envgs_grow_tensor *tensors;         /* host array, passed by value to the kernel */
} envgs_densify_rewrite_args;

ENVGS_API int envgs_densify_rewrite(const envgs_densify_rewrite_args *args, void *stream);

/* ---- the pruning tail on the device (SurfelSet(device_schedule="all")) ---------------------------------------------------------------------
 *
 * `prune_max_scene_and_screen` and `prune_visibility` (gaussian2d_utils.py:794-864) cut by order statistics of the per-surfel average weight
 * (`get_xyz_weight_avg`, :628-631).  The KEY of surfel i is xyz_weight_accum[i] / denom[i]: IEEE division, NaN -> 0, -0 counted as +0.
 */

/* Scratch bytes of envgs_weight_select (histograms of the three passes; does not depend on P). */
ENVGS_API size_t envgs_weight_select_temp_bytes(void);

/* Exact order statistics of the keys: a three-pass radix select (11 + 11 + 10 bits) over the order-preserving uint32 image of the key, for
 * n_ranks = 1 or 2 ranks in the same passes (rank1 is ignored when n_ranks == 1).  Per rank r (0-based, 0 <= r < P), on the device:
 * values[k] = the (r + 1)-th smallest key, bit for bit one of the keys; below[k] = the number of keys strictly below it.  Integer atomics only:
 * the result does not depend on the order of execution.  1 <= P < 2^31. */
ENVGS_API int envgs_weight_select(int64_t P, const float *xyz_weight_accum, const float *denom, int32_t n_ranks, int64_t rank0, int64_t rank1,
                                  float *values, uint32_t *below, void *temp, size_t temp_bytes, void *stream);

ENVGS_API size_t envgs_visibility_mask_temp_bytes(int64_t P);

/* keep (P bytes): 0 for the n_prune surfels of lowest key, 1 for the others.  cut / cut_below (device): envgs_weight_select's value and count
 * for rank n_prune - 1.  Every key below the cut goes; of the keys equal to the cut, the first n_prune - *cut_below in index order go (ranked
 * with a prefix scan, so the same rows whatever the launch order).  1 <= n_prune <= P < 2^31. */
ENVGS_API int envgs_visibility_mask(int64_t P, const float *xyz_weight_accum, const float *denom, int64_t n_prune, const float *cut,
                                    const uint32_t *cut_below, uint8_t *keep, void *temp, size_t temp_bytes, void *stream);

/* envgs_oversize_plan flags: which thresholds are given */
#define ENVGS_OVERSIZE_SCREEN 1u
#define ENVGS_OVERSIZE_SCENE 2u
#define ENVGS_OVERSIZE_WEIGHT 4u

/* The masks of `prune_max_scene_and_screen` in one launch:  big = max_radii2D > max_screen (SCREEN) | max(scal) > scene_limit (SCENE);
 * light = key < *quantile (WEIGHT; without it every surfel is light).  keep (P bytes) = !(big & light); split (P words) = big & !light;
 * counts (device, 2 words) = {rows pruned, rows to split}.  scal: (P,2) activated scales; scene_limit = spatial_scale * max_scene_threshold. */
ENVGS_API int envgs_oversize_plan(int64_t P, uint32_t flags, float max_screen, float scene_limit, const float *max_radii2D, const float *scal,
                                  const float *xyz_weight_accum, const float *denom, const float *quantile, uint8_t *keep, uint32_t *split,
                                  uint32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVGS_DENSIFY_H */
