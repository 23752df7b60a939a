// model.hip -- fused front end (include/envgs_model.h): raw surfel parameters -> the activated tensors, colours, tracer extras and quads the two
// extensions take, and the gradients back to the raw parameters; ONE HBM-streaming kernel each way.
//
// FOUR LANES PER SURFEL, as the sh_colors_*_q16 kernels of glue.hip: lane q of a quad owns coefficients 4q .. 4q+3 of the surfel's logical
// (M,3) coefficient row cat(dc, rest) = its dwords 12q .. 12q+11, so a wave covers 16 consecutive rows and every access instruction touches
// each 48 B chunk once.  _features_rest rows are 180 B, so consecutive rows are not 16 B aligned: the chunks are read and written as plain
// dwords (dc and rest IN PLACE, no concatenated copy) which the compiler merges into dword-aligned multi-dword accesses; per-surfel sums go
// through the DPP quad sum.  The small per-surfel tensors are spread over the quad's lanes (q = 0 colours, 1 scale, 2 sigmoids, 3 quads /
// rotation), so no lane walks the whole 192 B block.  No atomics, no LDS.
#include "common.h"
#include "sh_basis.h"
#include <cstdint>

#include "../../include/envgs_model.h"

namespace envgs {

typedef envgs_surfel_inputs_args ModelArgs;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }                 // torch's form: saturates to exactly 0 / 1

// Dwords 12q .. 12q+11 of row i of cat(dc (P,1,3), rest (P,M-1,3)).  FULL (M = 16): every dword exists; the first three come from dc in lane 0
// and from rest elsewhere, the other nine from rest in every lane.  Otherwise each dword is guarded by the row length 3M.
template <bool FULL>
__device__ __forceinline__ void load_chunk(const float *__restrict__ dc, const float *__restrict__ rest, size_t i, int q, int M, float (&x)[12])
{
    if constexpr (FULL) {
        const float *b = rest + i * 45 + 12 * q;                  // dword 12q+3 of the row (rest starts at dword 3)
        const float *a = q == 0 ? dc + 3 * i : b - 3;
#pragma unroll
        for (int f = 0; f < 3; f++) x[f] = a[f];
#pragma unroll
        for (int f = 3; f < 12; f++) x[f] = b[f - 3];
    } else {
        const int L = 3 * M;
#pragma unroll
        for (int f = 0; f < 12; f++) {
            const int e = 12 * q + f;
            x[f] = e < 3 ? dc[3 * i + e] : (e < L ? rest[i * (size_t)(L - 3) + (e - 3)] : 0.f);
        }
    }
}

template <bool FULL>
__device__ __forceinline__ void store_chunk(float *__restrict__ dc, float *__restrict__ rest, size_t i, int q, int M, const float (&x)[12])
{
    if constexpr (FULL) {
        float *b = rest + i * 45 + 12 * q;
        float *a = q == 0 ? dc + 3 * i : b - 3;
#pragma unroll
        for (int f = 0; f < 3; f++) a[f] = x[f];
#pragma unroll
        for (int f = 3; f < 12; f++) b[f - 3] = x[f];
    } else {
        const int L = 3 * M;
#pragma unroll
        for (int f = 0; f < 12; f++) {
            const int e = 12 * q + f;
            if (e < 3) dc[3 * i + e] = x[f];
            else if (e < L) rest[i * (size_t)(L - 3) + (e - 3)] = x[f];
        }
    }
}

// lane q's four entries of a 16-entry per-surfel table, zero beyond the active degree
__device__ __forceinline__ void quad_slice(const float *t, int q, int nb, float (&o)[4])
{
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const float v = q == 0 ? t[m] : q == 1 ? t[4 + m] : q == 2 ? t[8 + m] : t[12 + m];
        o[m] = (4 * q + m) < nb ? v : 0.f;
    }
}

template <bool FULL>
__global__ void __launch_bounds__(256)
surfel_inputs_fwd(const ModelArgs A)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(t & 3);
    const bool live = (t >> 2) < (size_t)A.P;
    const size_t i = live ? (t >> 2) : 0;                         // (lanes past the end compute surfel 0 and write nothing: the quad sum needs them)
    const int D = A.sh_degree, M = A.sh_coeffs, S = A.spec_channels, nb = (D + 1) * (D + 1);
    const int C = S ? 3 + S + 1 : 3;

    float x[12];
#pragma unroll
    for (int f = 0; f < 12; f++) x[f] = 0.f;
    if (A.shs || (A.colors && 4 * q < nb)) load_chunk<FULL>(A.features_dc, A.features_rest, i, q, M, x);
    if (A.shs && live) {
        float *o = A.shs + i * (size_t)(3 * M) + 12 * q;
        if constexpr (FULL) {
#pragma unroll
            for (int f = 0; f < 12; f++) o[f] = x[f];
        } else {
#pragma unroll
            for (int f = 0; f < 12; f++)
                if (12 * q + f < 3 * M) o[f] = x[f];
        }
    }
    if (A.colors) {                                                // (uniform: every lane of the quad reaches the DPP sum)
        const float dx = A.xyz[3 * i] - A.campos[0], dy = A.xyz[3 * i + 1] - A.campos[1], dz = A.xyz[3 * i + 2] - A.campos[2];
        const float il = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
        float b[16], bq[4];
        basis16_exact(D, dx * il, dy * il, dz * il, b);
        quad_slice(b, q, nb, bq);
        float r[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int f = 0; f < 12; f++) r[f % 3] += bq[f / 3] * x[f];
        const float r0 = quad_sum(r[0]) + 0.5f, r1 = quad_sum(r[1]) + 0.5f, r2 = quad_sum(r[2]) + 0.5f;
        if (live && q == 0) {
            A.clamped[3 * i] = r0 < 0.f; A.clamped[3 * i + 1] = r1 < 0.f; A.clamped[3 * i + 2] = r2 < 0.f;
            float *o = A.colors + i * C;
            o[0] = fmaxf(r0, 0.f); o[1] = fmaxf(r1, 0.f); o[2] = fmaxf(r2, 0.f);
        }
    }
    if (!live) return;
    if (q == 1) {
        if (A.scales) { A.scales[2 * i] = expf(A.scaling[2 * i]); A.scales[2 * i + 1] = expf(A.scaling[2 * i + 1]); }
        if (A.rotations) {
            const float r = A.rotation[4 * i], u = A.rotation[4 * i + 1], v = A.rotation[4 * i + 2], w = A.rotation[4 * i + 3];
            const float den = fmaxf(sqrtf(r * r + u * u + v * v + w * w), 1e-12f);                      // F.normalize: q / max(|q|, eps)
            A.rotations[4 * i] = r / den; A.rotations[4 * i + 1] = u / den; A.rotations[4 * i + 2] = v / den; A.rotations[4 * i + 3] = w / den;
        }
    } else if (q == 2) {
        if (A.opacities) A.opacities[i] = sigmoid_f(A.opacity[i]);
        if (S && (A.specular_act || A.roughness_act || A.colors || A.others)) {
            const float ro = sigmoid_f(A.roughness[i]);
            for (int s = 0; s < S; s++) {
                const float sp = sigmoid_f(A.specular[i * S + s]);
                if (A.specular_act) A.specular_act[i * S + s] = sp;
                if (A.colors) A.colors[i * C + 3 + s] = sp;
                if (A.others) A.others[2 * i] = sp;               // (S = 1 only: checked on the host)
            }
            if (A.roughness_act) A.roughness_act[i] = ro;
            if (A.colors) A.colors[i * C + 3 + S] = ro;
            if (A.others) A.others[2 * i + 1] = ro;
        }
    } else if (q == 3 && A.vertices) {
        // get_disks, the expressions of surfel_quads (glue.hip) on exp(scaling) and the raw quaternion; the two kernels contract differently (see
        // there) and agree to rounding, not to the bit
        float r = A.rotation[4 * i], x1 = A.rotation[4 * i + 1], y = A.rotation[4 * i + 2], z = A.rotation[4 * i + 3];
        const float inv = 1.0f / sqrtf(r * r + x1 * x1 + y * y + z * z);
        r *= inv; x1 *= inv; y *= inv; z *= inv;
        const float su = 3.0f * expf(A.scaling[2 * i]), sv = 3.0f * expf(A.scaling[2 * i + 1]);
        const float a[3] = {(1.f - 2.f * (y * y + z * z)) * su, (2.f * (x1 * y + r * z)) * su, (2.f * (x1 * z - r * y)) * su};       // rotation column 0
        const float b[3] = {(2.f * (x1 * y - r * z)) * sv, (1.f - 2.f * (x1 * x1 + z * z)) * sv, (2.f * (y * z + r * x1)) * sv};     // rotation column 1
        float *o = A.vertices + i * 12;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float m = A.xyz[3 * i + c];
            o[c] = m - a[c] + b[c]; o[3 + c] = m - a[c] - b[c]; o[6 + c] = m + a[c] + b[c]; o[9 + c] = m + a[c] - b[c];
        }
    }
}

template <bool FULL>
__global__ void __launch_bounds__(256)
surfel_inputs_bwd(const ModelArgs A)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(t & 3);
    const bool live = (t >> 2) < (size_t)A.P;
    const size_t i = live ? (t >> 2) : 0;
    const int D = A.sh_degree, M = A.sh_coeffs, S = A.spec_channels, nb = (D + 1) * (D + 1);
    const int C = S ? 3 + S + 1 : 3;

    float o[12];
#pragma unroll
    for (int f = 0; f < 12; f++) o[f] = 0.f;
    float ddx = 0.f, ddy = 0.f, ddz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, sum2 = 1.f, il = 1.f;
    if (A.g_colors) {                                              // (uniform)
        const float *g = A.g_colors + i * C;
        const float gc[3] = {A.clamped[3 * i] ? 0.f : g[0], A.clamped[3 * i + 1] ? 0.f : g[1], A.clamped[3 * i + 2] ? 0.f : g[2]};
        dx = A.xyz[3 * i] - A.campos[0]; dy = A.xyz[3 * i + 1] - A.campos[1]; dz = A.xyz[3 * i + 2] - A.campos[2];
        sum2 = dx * dx + dy * dy + dz * dz; il = 1.0f / sqrtf(sum2);
        const float x = dx * il, y = dy * il, z = dz * il;
        float b[16], gx[16], gy[16], gz[16], bq[4], gxq[4], gyq[4], gzq[4];
        basis16_exact(D, x, y, z, b);
        basis16_grad_exact(D, x, y, z, gx, gy, gz);
        quad_slice(b, q, nb, bq); quad_slice(gx, q, nb, gxq); quad_slice(gy, q, nb, gyq); quad_slice(gz, q, nb, gzq);
        float xs[12];
#pragma unroll
        for (int f = 0; f < 12; f++) xs[f] = 0.f;
        if (4 * q < nb) load_chunk<FULL>(A.features_dc, A.features_rest, i, q, M, xs);
        float sd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int f = 0; f < 12; f++) { o[f] = bq[f / 3] * gc[f % 3]; sd[f / 3] += xs[f] * gc[f % 3]; }
#pragma unroll
        for (int m = 0; m < 4; m++) { ddx += gxq[m] * sd[m]; ddy += gyq[m] * sd[m]; ddz += gzq[m] * sd[m]; }
        ddx = quad_sum(ddx); ddy = quad_sum(ddy); ddz = quad_sum(ddz);
    }
    if (A.g_shs) {
        const float *g = A.g_shs + i * (size_t)(3 * M) + 12 * q;
#pragma unroll
        for (int f = 0; f < 12; f++)
            if (FULL || 12 * q + f < 3 * M) o[f] += g[f];
    }
    if (!live) return;
    store_chunk<FULL>(A.d_features_dc, A.d_features_rest, i, q, M, o);
    if (q == 0) {
        if (A.d_xyz) {
            // d normalize(d) / d d applied to the basis-gradient sums; exact zeros without a colour gradient
            const float inv3 = il * il * il;
            A.d_xyz[3 * i] = A.g_colors ? ((sum2 - dx * dx) * ddx - dy * dx * ddy - dz * dx * ddz) * inv3 : 0.f;
            A.d_xyz[3 * i + 1] = A.g_colors ? (-dx * dy * ddx + (sum2 - dy * dy) * ddy - dz * dy * ddz) * inv3 : 0.f;
            A.d_xyz[3 * i + 2] = A.g_colors ? (-dx * dz * ddx - dy * dz * ddy + (sum2 - dz * dz) * ddz) * inv3 : 0.f;
        }
    } else if (q == 1) {
#pragma unroll
        for (int c = 0; c < 2; c++) A.d_scaling[2 * i + c] = A.g_scales ? A.g_scales[2 * i + c] * expf(A.scaling[2 * i + c]) : 0.f;
        float d = 0.f;
        if (A.g_opacities) { const float s = sigmoid_f(A.opacity[i]); d = A.g_opacities[i] * ((1.0f - s) * s); }
        A.d_opacity[i] = d;
    } else if (q == 2) {
        if (S) {
            const float *gcol = A.g_colors ? A.g_colors + i * C : nullptr;
            const bool any_s = A.g_specular_act || gcol || A.g_others, any_r = A.g_roughness_act || gcol || A.g_others;
            for (int s = 0; s < S; s++) {
                float d = 0.f;
                if (any_s) {
                    const float sp = sigmoid_f(A.specular[i * S + s]);
                    const float g = (A.g_specular_act ? A.g_specular_act[i * S + s] : 0.f) + (gcol ? gcol[3 + s] : 0.f) + (A.g_others ? A.g_others[2 * i] : 0.f);
                    d = g * ((1.0f - sp) * sp);
                }
                A.d_specular[i * S + s] = d;
            }
            float d = 0.f;
            if (any_r) {
                const float ro = sigmoid_f(A.roughness[i]);
                const float g = (A.g_roughness_act ? A.g_roughness_act[i] : 0.f) + (gcol ? gcol[3 + S] : 0.f) + (A.g_others ? A.g_others[2 * i + 1] : 0.f);
                d = g * ((1.0f - ro) * ro);
            }
            A.d_roughness[i] = d;
        }
    } else {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if (A.g_rotations) {
            // q^ = q / max(|q|, eps):  d = (g - q^ (q^.g)) / |q|;  below eps the clamp passes no gradient to the norm
            const float *g = A.g_rotations + 4 * i;
            const float r = A.rotation[4 * i], u = A.rotation[4 * i + 1], v = A.rotation[4 * i + 2], w = A.rotation[4 * i + 3];
            const float n = sqrtf(r * r + u * u + v * v + w * w), den = fmaxf(n, 1e-12f);
            const float h[4] = {r / den, u / den, v / den, w / den};
            const float dot = n > 1e-12f ? h[0] * g[0] + h[1] * g[1] + h[2] * g[2] + h[3] * g[3] : 0.f;
#pragma unroll
            for (int c = 0; c < 4; c++) d[c] = (g[c] - h[c] * dot) / den;
        }
#pragma unroll
        for (int c = 0; c < 4; c++) A.d_rotation[4 * i + c] = d[c];
    }
}

static bool sizes_ok(const ModelArgs *a)
{
    if (!a) return false;
    const int D = a->sh_degree, M = a->sh_coeffs, S = a->spec_channels;
    return a->P >= 0 && D >= 0 && D <= 3 && M >= (D + 1) * (D + 1) && M <= 16 && (S == 0 || S == 1 || S == 3);
}

}  // namespace envgs

using namespace envgs;

extern "C" {

int envgs_surfel_inputs_forward(const envgs_surfel_inputs_args *a, void *stream)
{
    if (!sizes_ok(a)) return ENVGS_ERR_BAD_ARG;
    if (a->P == 0) return 0;
    const int M = a->sh_coeffs, S = a->spec_channels;
    const bool feats = a->shs || a->colors, sig = S && (a->specular_act || a->roughness_act || a->colors || a->others);
    if (feats && (!a->features_dc || (M > 1 && !a->features_rest))) return ENVGS_ERR_BAD_ARG;
    if ((a->colors != nullptr) != (a->clamped != nullptr)) return ENVGS_ERR_BAD_ARG;
    if (a->colors && (!a->xyz || !a->campos)) return ENVGS_ERR_BAD_ARG;
    if ((a->scales || a->vertices) && !a->scaling) return ENVGS_ERR_BAD_ARG;
    if ((a->rotations || a->vertices) && !a->rotation) return ENVGS_ERR_BAD_ARG;
    if (a->vertices && !a->xyz) return ENVGS_ERR_BAD_ARG;
    if (a->opacities && !a->opacity) return ENVGS_ERR_BAD_ARG;
    if ((a->others && S != 1) || (!S && (a->specular_act || a->roughness_act))) return ENVGS_ERR_BAD_ARG;
    if (sig && (!a->specular || !a->roughness)) return ENVGS_ERR_BAD_ARG;
    const dim3 grid((unsigned)((4 * (size_t)a->P + 255) / 256));
    if (M == 16) hipLaunchKernelGGL(surfel_inputs_fwd<true>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL(surfel_inputs_fwd<false>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

int envgs_surfel_inputs_backward(const envgs_surfel_inputs_args *a, void *stream)
{
    if (!sizes_ok(a)) return ENVGS_ERR_BAD_ARG;
    if (a->P == 0) return 0;
    const int M = a->sh_coeffs, S = a->spec_channels;
    if (!a->d_features_dc || (M > 1 && !a->d_features_rest) || !a->d_scaling || !a->d_rotation || !a->d_opacity) return ENVGS_ERR_BAD_ARG;
    if (S && (!a->d_specular || !a->d_roughness)) return ENVGS_ERR_BAD_ARG;
    if (a->g_colors && (!a->d_xyz || !a->clamped || !a->xyz || !a->campos || !a->features_dc || (M > 1 && !a->features_rest))) return ENVGS_ERR_BAD_ARG;
    if (a->g_scales && !a->scaling) return ENVGS_ERR_BAD_ARG;
    if (a->g_rotations && !a->rotation) return ENVGS_ERR_BAD_ARG;
    if (a->g_opacities && !a->opacity) return ENVGS_ERR_BAD_ARG;
    if ((a->g_others && S != 1) || (!S && (a->g_specular_act || a->g_roughness_act))) return ENVGS_ERR_BAD_ARG;
    if (S && (a->g_specular_act || a->g_roughness_act || a->g_colors || a->g_others) && (!a->specular || !a->roughness)) return ENVGS_ERR_BAD_ARG;
    const dim3 grid((unsigned)((4 * (size_t)a->P + 255) / 256));
    if (M == 16) hipLaunchKernelGGL(surfel_inputs_bwd<true>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL(surfel_inputs_bwd<false>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

}  // extern "C"
