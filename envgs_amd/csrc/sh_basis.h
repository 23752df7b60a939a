// sh_basis.h -- the real SH basis of degree <= 3: its constants (the one set in the library; raster_project.hip, raster_project_bwd.hip and
// trace_common.h's kShForm use them too) and the two evaluations of the basis and its gradient, side by side:
//
//   basis16_exact / basis16_grad_exact             contraction OFF, statement by statement as the oracle: the per-SURFEL colour kernels
//                                                  (glue.hip: sh_colors_*, sh_record_bwd_q16; model.hip: surfel_inputs_*), whose dL/dSH is
//                                                  compared element by element against a second evaluation (see below)
//   basis16_contracted / basis16_grad_contracted   the compiler may contract (they follow their translation unit's setting, which build.py
//                                                  leaves on for the tracer): the per-HIT tracer kernels (trace_kbuffer.hip, trace_lists.hip,
//                                                  trace_surfel_bwd.hip, trace_common.h), on the timed path, compared through blended colours
//
// Caller's obligation: basis16_exact zeroes all 16 entries of b and fills those of degree <= D; basis16_contracted writes ONLY the (D + 1)^2
// entries of degree <= D and leaves the rest of b untouched, so its callers must read no entry beyond that.  Both gradients zero all 48 entries.
//
// The bodies are the same expressions and stay two: `#pragma clang fp contract` is lexical, so one body would have to be included twice or
// wrapped in a macro.  Moving a kernel from one pair to the other changes its rounding.
#pragma once
#include "common.h"

namespace envgs {

constexpr float kC0 = 0.28209479177387814f;
constexpr float kC1 = 0.4886025119029199f;
// the magnitudes of degree 2 and 3, named so that the tables below and kShForm are written from one set of literals
constexpr float kC2xy = 1.0925484305920792f, kC2zz = 0.31539156525252005f, kC2xx = 0.5462742152960396f;
constexpr float kC3a = 0.5900435899266435f, kC3b = 2.890611442640554f, kC3c = 0.4570457994644658f, kC3d = 0.3731763325901154f,
                kC3e = 1.445305721320277f;
static __device__ __constant__ float kC2[5] = {kC2xy, -kC2xy, kC2zz, -kC2xy, kC2xx};
static __device__ __constant__ float kC3[7] = {-kC3a, kC3b, -kC3c, kC3d, -kC3c, kC3e, -kC3a};

// The SH basis and its gradient are evaluated WITHOUT FMA contraction, statement by statement as oracle/surfel_raster_oracle.c does: a basis
// function near one of its zeros (2 zz - xx - yy -> 0) is a cancellation whose relative rounding error is unbounded, so two evaluations agree on
// dL/dSH = basis * dL/dcolour to 1e-4 RELATIVE only if they round the same way (round 4: the 16 of 14.4 M dshs elements beyond tolerance at
// full size were exactly these; the rasterizer's forward colours, raster_project.hip, have been bit-exact this way since round 1).
__device__ __forceinline__ void basis16_exact(int D, float x, float y, float z, float *b)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 16; k++) b[k] = 0.f;
    b[0] = kC0;
    if (D > 0) {
        b[1] = -kC1 * y; b[2] = kC1 * z; b[3] = -kC1 * x;
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = kC2[0] * xy; b[5] = kC2[1] * yz; b[6] = kC2[2] * (2.0f * zz - xx - yy); b[7] = kC2[3] * xz; b[8] = kC2[4] * (xx - yy);
            if (D > 2) {
                b[9] = kC3[0] * y * (3.0f * xx - yy); b[10] = kC3[1] * xy * z; b[11] = kC3[2] * y * (4.0f * zz - xx - yy);
                b[12] = kC3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy); b[13] = kC3[4] * x * (4.0f * zz - xx - yy);
                b[14] = kC3[5] * z * (xx - yy); b[15] = kC3[6] * x * (xx - 3.0f * yy);
            }
        }
    }
}

__device__ __forceinline__ void basis16_grad_exact(int D, float x, float y, float z, float *gx, float *gy, float *gz)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 16; k++) { gx[k] = 0.f; gy[k] = 0.f; gz[k] = 0.f; }
    if (D > 0) {
        gy[1] = -kC1; gz[2] = kC1; gx[3] = -kC1;
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            gx[4] = kC2[0] * y; gy[4] = kC2[0] * x;
            gy[5] = kC2[1] * z; gz[5] = kC2[1] * y;
            gx[6] = kC2[2] * -2.f * x; gy[6] = kC2[2] * -2.f * y; gz[6] = kC2[2] * 4.f * z;
            gx[7] = kC2[3] * z; gz[7] = kC2[3] * x;
            gx[8] = kC2[4] * 2.f * x; gy[8] = kC2[4] * -2.f * y;
            if (D > 2) {
                gx[9] = kC3[0] * 6.f * xy; gy[9] = kC3[0] * 3.f * (xx - yy);
                gx[10] = kC3[1] * yz; gy[10] = kC3[1] * xz; gz[10] = kC3[1] * xy;
                gx[11] = kC3[2] * -2.f * xy; gy[11] = kC3[2] * (4.f * zz - xx - 3.f * yy); gz[11] = kC3[2] * 8.f * yz;
                gx[12] = kC3[3] * -6.f * xz; gy[12] = kC3[3] * -6.f * yz; gz[12] = kC3[3] * 3.f * (2.f * zz - xx - yy);
                gx[13] = kC3[4] * (4.f * zz - 3.f * xx - yy); gy[13] = kC3[4] * -2.f * xy; gz[13] = kC3[4] * 8.f * xz;
                gx[14] = kC3[5] * 2.f * xz; gy[14] = kC3[5] * -2.f * yz; gz[14] = kC3[5] * (xx - yy);
                gx[15] = kC3[6] * 3.f * (xx - yy); gy[15] = kC3[6] * -6.f * xy;
            }
        }
    }
}

// The tracer's pair: the same expressions, no pragma (basis16_contracted fills only the entries of degree <= D).
__device__ __forceinline__ void basis16_contracted(int D, float x, float y, float z, float *b)
{
    b[0] = kC0;
    if (D > 0) {
        b[1] = -kC1 * y; b[2] = kC1 * z; b[3] = -kC1 * x;
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = kC2[0] * xy; b[5] = kC2[1] * yz; b[6] = kC2[2] * (2.0f * zz - xx - yy); b[7] = kC2[3] * xz; b[8] = kC2[4] * (xx - yy);
            if (D > 2) {
                b[9] = kC3[0] * y * (3.0f * xx - yy); b[10] = kC3[1] * xy * z; b[11] = kC3[2] * y * (4.0f * zz - xx - yy);
                b[12] = kC3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy); b[13] = kC3[4] * x * (4.0f * zz - xx - yy);
                b[14] = kC3[5] * z * (xx - yy); b[15] = kC3[6] * x * (xx - 3.0f * yy);
            }
        }
    }
}

__device__ __forceinline__ void basis16_grad_contracted(int D, float x, float y, float z, float *gx, float *gy, float *gz)
{
#pragma unroll
    for (int k = 0; k < 16; k++) { gx[k] = 0.f; gy[k] = 0.f; gz[k] = 0.f; }
    if (D > 0) {
        gy[1] = -kC1; gz[2] = kC1; gx[3] = -kC1;
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            gx[4] = kC2[0] * y; gy[4] = kC2[0] * x;
            gy[5] = kC2[1] * z; gz[5] = kC2[1] * y;
            gx[6] = kC2[2] * -2.f * x; gy[6] = kC2[2] * -2.f * y; gz[6] = kC2[2] * 4.f * z;
            gx[7] = kC2[3] * z; gz[7] = kC2[3] * x;
            gx[8] = kC2[4] * 2.f * x; gy[8] = kC2[4] * -2.f * y;
            if (D > 2) {
                gx[9] = kC3[0] * 6.f * xy; gy[9] = kC3[0] * 3.f * (xx - yy);
                gx[10] = kC3[1] * yz; gy[10] = kC3[1] * xz; gz[10] = kC3[1] * xy;
                gx[11] = kC3[2] * -2.f * xy; gy[11] = kC3[2] * (4.f * zz - xx - 3.f * yy); gz[11] = kC3[2] * 8.f * yz;
                gx[12] = kC3[3] * -6.f * xz; gy[12] = kC3[3] * -6.f * yz; gz[12] = kC3[3] * 3.f * (2.f * zz - xx - yy);
                gx[13] = kC3[4] * (4.f * zz - 3.f * xx - yy); gy[13] = kC3[4] * -2.f * xy; gz[13] = kC3[4] * 8.f * xz;
                gx[14] = kC3[5] * 2.f * xz; gy[14] = kC3[5] * -2.f * yz; gz[14] = kC3[5] * (xx - yy);
                gx[15] = kC3[6] * 3.f * (xx - yy); gy[15] = kC3[6] * -6.f * xy;
            }
        }
    }
}

}  // namespace envgs
