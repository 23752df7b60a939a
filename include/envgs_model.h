/*
 * envgs_model.h -- C-ABI of the fused front end: from the RAW surfel parameters a training loop, the optimizer and the checkpoints hold
 * (_xyz, _features_dc, _features_rest, _scaling, _rotation, _opacity, _specular, _roughness) to the activated tensors the rasterizer and the
 * tracer take, one kernel each way.  The reference spends ~20 torch launches per set and direction on the same expressions:
 *   activations        easyvolcap/utils/gaussian2d_utils.py:329-390 (exp, F.normalize, sigmoid; get_features = cat(dc, rest))
 *   colour preparation gaussian2d_utils.py:1066-1084 (render() with pipe.convert_SHs_python: eval_sh + 0.5, clamp, cat with specular / roughness)
 *   tracer arguments   easyvolcap/utils/optix_utils.py:129-185 (others_precomp = cat(specular, roughness))
 *   quads              optix_utils.py:39-69 (get_disks)
 * Conventions as in envgs_glue.h (device pointers, hipStream_t as void*, 0 = ok, ENVGS_ERR_BAD_ARG on bad sizes / missing required pointers,
 * P == 0 returns 0 without a launch).  Most outputs are optional, so the arguments travel in a struct (as in envgs_supervisor.h).
 */
#ifndef ENVGS_MODEL_H
#define ENVGS_MODEL_H

#include <stddef.h>
#include <stdint.h>

#include "envgs_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct envgs_surfel_inputs_args {
    int32_t P;                  /* surfels */
    int32_t sh_degree;          /* D, 0..3: the ACTIVE degree of the colours */
    int32_t sh_coeffs;          /* M = 1 + rows of _features_rest, (D+1)^2 <= M <= 16 */
    int32_t spec_channels;      /* S in {0, 1, 3}; 0: the set has no _specular / _roughness */
    /* raw parameters: xyz (P,3), features_dc (P,1,3), features_rest (P,M-1,3) (NULL allowed when M = 1), scaling (P,2), rotation (P,4),
     * opacity (P,1), specular (P,S), roughness (P,1); campos (3), needed only for colours.  A pointer no requested output reads may be NULL. */
    const float *xyz, *features_dc, *features_rest, *scaling, *rotation, *opacity, *specular, *roughness, *campos;
    /* forward outputs, each written only if its pointer is not NULL:
     *   scales (P,2) = exp(scaling);  rotations (P,4) = q / max(|q|, 1e-12);  opacities (P,1), specular_act (P,S), roughness_act (P,1) = sigmoid
     *   shs (P,M,3) = cat(dc, rest), the get_features layout
     *   colors (P,C) = [clamp_min(eval_sh(D, features, normalize(xyz - campos)) + 0.5, 0) | sigmoid(specular) | sigmoid(roughness)],
     *       C = 3+S+1 (C = 3 when S = 0); dc and rest are read in place.  Comes with clamped (P,3) uint8 (both or neither).
     *   others (P,2) = [sigmoid(specular), sigmoid(roughness)], S = 1 only: the tracer's others_precomp
     *   vertices (4P,3): the get_disks corners from the raw scaling / rotation, corner order and arithmetic of envgs_surfel_quads */
    float *scales, *rotations, *opacities, *specular_act, *roughness_act, *shs, *colors, *others, *vertices;
    uint8_t *clamped;           /* forward: out, with colors; backward: in, required iff d_xyz is given */
    /* backward upstreams, one per differentiable output (vertices carry no gradient); NULL = that output did not reach the loss */
    const float *g_scales, *g_rotations, *g_opacities, *g_specular_act, *g_roughness_act, *g_shs, *g_colors, *g_others;
    /* backward outputs, fully written: d_features_dc (P,1,3), d_features_rest (P,M-1,3) (NULL allowed when M = 1), d_scaling, d_rotation,
     * d_opacity, and for S > 0 d_specular (P,S), d_roughness (P,1) (colors and others contributions summed).  d_xyz (P,3): give it iff colours
     * were produced in the forward; it holds the view-direction term only.  Coefficients beyond (D+1)^2 receive exactly g_shs (0 without it). */
    float *d_xyz, *d_features_dc, *d_features_rest, *d_scaling, *d_rotation, *d_opacity, *d_specular, *d_roughness;
} envgs_surfel_inputs_args;

/* Reads the sizes, the raw parameters and the forward outputs of *args. */
ENVGS_API int envgs_surfel_inputs_forward(const envgs_surfel_inputs_args *args, void *stream);

/* Reads the sizes, the raw parameters, clamped, the upstreams and the backward outputs of *args; the activations are recomputed from the raw
 * parameters (no activated tensor is kept for the backward).  d_rotation = (g - q^ (q^.g)) / |q|.  A surfel whose upstream rows are all zero
 * receives raw gradients that compare == 0. */
ENVGS_API int envgs_surfel_inputs_backward(const envgs_surfel_inputs_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVGS_MODEL_H */
