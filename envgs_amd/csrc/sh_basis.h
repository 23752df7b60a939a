// sh_basis.h -- the real SH basis of degree <= 3 and its gradient, as the per-surfel colour kernels evaluate them (glue.hip: sh_colors_*,
// sh_record_bwd_q16; model.hip: surfel_inputs_*), and the quad reduction of the four-lanes-per-surfel kernels.  ONE definition: two kernels
// agree on dL/dSH only if they round the basis the same way (see below).
#pragma once
#include "common.h"

namespace envgs {

constexpr float gC0 = 0.28209479177387814f;
constexpr float gC1 = 0.4886025119029199f;
static __device__ __constant__ float gC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                        -1.0925484305920792f, 0.5462742152960396f};
static __device__ __constant__ float gC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                        0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                        -0.5900435899266435f};

// The SH basis and its gradient are evaluated WITHOUT FMA contraction, statement by statement as oracle/surfel_raster_oracle.c does: a basis
// function near one of its zeros (2 zz - xx - yy -> 0) is a cancellation whose relative rounding error is unbounded, so two evaluations agree on
// dL/dSH = basis * dL/dcolour to 1e-4 RELATIVE only if they round the same way (round 4: the 16 of 14.4 M dshs elements beyond tolerance at
// full size were exactly these; the rasterizer's forward colours, raster_project.hip, have been bit-exact this way since round 1).
__device__ __forceinline__ void basis16(int D, float x, float y, float z, float *b)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 16; k++) b[k] = 0.f;
    b[0] = gC0;
    if (D > 0) {
        b[1] = -gC1 * y; b[2] = gC1 * z; b[3] = -gC1 * x;
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = gC2[0] * xy; b[5] = gC2[1] * yz; b[6] = gC2[2] * (2.0f * zz - xx - yy); b[7] = gC2[3] * xz; b[8] = gC2[4] * (xx - yy);
            if (D > 2) {
                b[9] = gC3[0] * y * (3.0f * xx - yy); b[10] = gC3[1] * xy * z; b[11] = gC3[2] * y * (4.0f * zz - xx - yy);
                b[12] = gC3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy); b[13] = gC3[4] * x * (4.0f * zz - xx - yy);
                b[14] = gC3[5] * z * (xx - yy); b[15] = gC3[6] * x * (xx - 3.0f * yy);
            }
        }
    }
}

__device__ __forceinline__ void basis16_grad(int D, float x, float y, float z, float *gx, float *gy, float *gz)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 16; k++) { gx[k] = 0.f; gy[k] = 0.f; gz[k] = 0.f; }
    if (D > 0) {
        gy[1] = -gC1; gz[2] = gC1; gx[3] = -gC1;
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            gx[4] = gC2[0] * y; gy[4] = gC2[0] * x;
            gy[5] = gC2[1] * z; gz[5] = gC2[1] * y;
            gx[6] = gC2[2] * -2.f * x; gy[6] = gC2[2] * -2.f * y; gz[6] = gC2[2] * 4.f * z;
            gx[7] = gC2[3] * z; gz[7] = gC2[3] * x;
            gx[8] = gC2[4] * 2.f * x; gy[8] = gC2[4] * -2.f * y;
            if (D > 2) {
                gx[9] = gC3[0] * 6.f * xy; gy[9] = gC3[0] * 3.f * (xx - yy);
                gx[10] = gC3[1] * yz; gy[10] = gC3[1] * xz; gz[10] = gC3[1] * xy;
                gx[11] = gC3[2] * -2.f * xy; gy[11] = gC3[2] * (4.f * zz - xx - 3.f * yy); gz[11] = gC3[2] * 8.f * yz;
                gx[12] = gC3[3] * -6.f * xz; gy[12] = gC3[3] * -6.f * yz; gz[12] = gC3[3] * 3.f * (2.f * zz - xx - yy);
                gx[13] = gC3[4] * (4.f * zz - 3.f * xx - yy); gy[13] = gC3[4] * -2.f * xy; gz[13] = gC3[4] * 8.f * xz;
                gx[14] = gC3[5] * 2.f * xz; gy[14] = gC3[5] * -2.f * yz; gz[14] = gC3[5] * (xx - yy);
                gx[15] = gC3[6] * 3.f * (xx - yy); gy[15] = gC3[6] * -6.f * xy;
            }
        }
    }
}

// lane ^ 1 and lane ^ 2 inside a quad (DPP quad_perm), and the sum over the quad in every one of its lanes
template <int CTRL> __device__ __forceinline__ float quad_xchg(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true)); }
__device__ __forceinline__ float quad_sum(float v) { v += quad_xchg<0xB1>(v); v += quad_xchg<0x4E>(v); return v; }

}  // namespace envgs
