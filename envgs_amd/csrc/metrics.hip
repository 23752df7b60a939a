// metrics.hip -- image evaluation: per-image MSE, PSNR and SSIM of a batch, finished on the device (include/envgs_metrics.h).
#include "common.h"

#include "../../include/envgs_metrics.h"

// Compiled with -ffp-contract=off (envgs_amd/build.py): where the compiler may fuse a multiply into an add it fuses some and not others -- of the
// five filter sums it paired four into packed fused multiply-adds and left the fifth a multiply and an add -- so E[xy] rounded differently from
// E[x^2] on identical images and their SSIM came out 6e-8 below 1.  Every fused multiply-add here is written out (fmaf); everything else rounds
// once per operation.
namespace envgs {

constexpr int MT = 16;            // output tile
constexpr int MR = 5;             // window radius (11 taps)
constexpr int MH = MT + 2 * MR;   // tile + halo = 26

// metric_utils.gaussian(11, 1.5) in float32; pinned by tests/golden/image_metrics_golden.npz["win"].  NOT loss.hip's kWin: ssim_utils builds its
// window from a float32 exp, metric_utils rounds a Python float, and the outermost taps come out two ulp apart (...6c against ...70).  A constant image's
// variance E[x^2] - mu^2 is what the taps' sum leaves of it, so the window is matched to the bit, not to a tolerance.
__device__ __constant__ float kMetricWin[11] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
                                                0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

struct Strides4 { int64_t b, c, y, x; };

__device__ __forceinline__ float load_gt(const float *p, int64_t o) { return p[o]; }
__device__ __forceinline__ float load_gt(const uint8_t *p, int64_t o) { return __fdiv_rn((float)p[o], 255.0f); }      // img.float() / 255

// The sum over the 64 lanes in every lane, pairs added in the order of the butterfly lane ^ 1, 2, 4, 8, 16, 32: the same order on every call.
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

// One workgroup per (image, channel, 16x16 tile), a 1-D grid: block g writes record g = ((b * C + c) * tiles_y + ty) * tiles_x + tx.
template <typename GT>
__global__ void __launch_bounds__(256)
image_metrics_tiles(const int C, const int H, const int W, const int tiles_x, const int tiles_y, const float *__restrict__ pred, const Strides4 ps,
                    const GT *__restrict__ gt, const Strides4 gs, double *__restrict__ partial)
{
    __shared__ float sx[MH][MH + 1], sy[MH][MH + 1];
    __shared__ float hb[5][MH][MT + 1];
    __shared__ double red[2][4];
    const int tid = threadIdx.x;
    const unsigned g = blockIdx.x, tiles = (unsigned)tiles_x * (unsigned)tiles_y;
    const unsigned bc = g / tiles, tile = g - bc * tiles;
    const int b = (int)(bc / (unsigned)C), c = (int)(bc - (unsigned)b * (unsigned)C);
    const int ty0 = (int)(tile / (unsigned)tiles_x) * MT, tx0 = (int)(tile % (unsigned)tiles_x) * MT;
    const float *xc = pred + (int64_t)b * ps.b + (int64_t)c * ps.c;
    const GT *yc = gt + (int64_t)b * gs.b + (int64_t)c * gs.c;
    for (int i = tid; i < MH * MH; i += 256) {
        const int r = i / MH, q = i - r * MH;
        const int gy = ty0 + r - MR, gx = tx0 + q - MR;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;               // padding = 5: zeros outside the image
        sx[r][q] = in ? xc[(int64_t)gy * ps.y + (int64_t)gx * ps.x] : 0.f;
        sy[r][q] = in ? load_gt(yc, (int64_t)gy * gs.y + (int64_t)gx * gs.x) : 0.f;
    }
    __syncthreads();
    // the reference convolves with the 11x11 outer product of the window; it is separable: vertical pass into hb, horizontal pass per output pixel
    for (int i = tid; i < MT * MH; i += 256) {
        const int r = i / MH, q = i - r * MH;                                 // r: output row in the tile, q: column incl. halo
        float a = 0.f, bsum = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float u = sx[r + k][q], v = sy[r + k][q], w = kMetricWin[k];
            a = fmaf(w, u, a); bsum = fmaf(w, v, bsum); aa = fmaf(w, u * u, aa); bb = fmaf(w, v * v, bb); ab = fmaf(w, u * v, ab);
        }
        hb[0][q][r] = a; hb[1][q][r] = bsum; hb[2][q][r] = aa; hb[3][q][r] = bb; hb[4][q][r] = ab;
    }
    __syncthreads();
    const int ly = tid >> 4, lx = tid & 15;
    const int gy = ty0 + ly, gx = tx0 + lx;
    float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const float w = kMetricWin[k];
        mu1 = fmaf(w, hb[0][lx + k][ly], mu1); mu2 = fmaf(w, hb[1][lx + k][ly], mu2);
        e11 = fmaf(w, hb[2][lx + k][ly], e11); e22 = fmaf(w, hb[3][lx + k][ly], e22); e12 = fmaf(w, hb[4][lx + k][ly], e12);
    }
    double sval = 0.0, qval = 0.0;
    if (gy < H && gx < W) {
        // every product and sum of the map rounded on its own, as the reference's mu1_squ / mu2_squ / mu1_mu2 tensors are (see the top of the file):
        // with x == y numerator and denominator are the same bits and the map is exactly 1
        constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
        const float s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
        const float A1 = 2.f * m12 + C1, A2 = 2.f * s12 + C2, B1 = (m11 + m22) + C1, B2 = (s1 + s2) + C2;
        sval = (double)((A1 * A2) / (B1 * B2));
        const double d = (double)sx[ly + MR][lx + MR] - (double)sy[ly + MR][lx + MR];       // exact: both are float32
        qval = d * d;
    }
    // lanes inside a wavefront by the butterfly, the four wavefronts in index order: no atomics, one order
    const double ssum = wave_sum_f64(sval), qsum = wave_sum_f64(qval);
    if ((tid & 63) == 0) { red[0][tid >> 6] = ssum; red[1][tid >> 6] = qsum; }
    __syncthreads();
    if (tid == 0) {
        partial[2 * (size_t)g] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partial[2 * (size_t)g + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// One workgroup per image: thread t adds records t, t + 256, ... of its image in that order, then the 256 sums fold in halves (t += t + 128,
// + 64, ... + 1).  The order depends on C, H and W alone, so a row is the same bytes whatever else is in the batch.
__global__ void __launch_bounds__(256)
image_metrics_finish(const int C, const int H, const int W, const unsigned per_image, const double *__restrict__ partial, double *__restrict__ out)
{
    __shared__ double s[2][256];
    const int tid = threadIdx.x;
    const double *rec = partial + 2 * (size_t)blockIdx.x * per_image;
    double a = 0.0, q = 0.0;
    for (unsigned i = tid; i < per_image; i += 256) { a += rec[2 * (size_t)i]; q += rec[2 * (size_t)i + 1]; }
    s[0][tid] = a; s[1][tid] = q;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) { s[0][tid] += s[0][tid + h]; s[1][tid] += s[1][tid + h]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double n = (double)C * (double)H * (double)W;
        const double mse = s[1][0] / n;
        double *row = out + (size_t)blockIdx.x * ENVGS_METRICS_COLS;
        row[ENVGS_METRICS_MSE] = mse;
        row[ENVGS_METRICS_PSNR] = 10.0 * log10(1.0 / (mse < 1e-10 ? 1e-10 : mse));          // the reference's clip; a NaN stays a NaN
        row[ENVGS_METRICS_SSIM] = s[0][0] / n;
    }
}

}  // namespace envgs

using namespace envgs;

static int64_t metric_tiles(int32_t H, int32_t W) { return (int64_t)((H + MT - 1) / MT) * ((W + MT - 1) / MT); }

extern "C" {

int64_t envgs_image_metrics_partial_count(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)B * C * metric_tiles(H, W);
}

int envgs_image_metrics(int32_t B, int32_t C, int32_t H, int32_t W, const float *pred, const int64_t *pred_strides, const void *gt,
                        const int64_t *gt_strides, int32_t gt_dtype, double *partial, double *out, void *stream)
{
    if (B < 0 || C < 1 || H < 1 || W < 1 || (gt_dtype != ENVGS_METRICS_GT_F32 && gt_dtype != ENVGS_METRICS_GT_U8)) return ENVGS_ERR_BAD_ARG;
    if (B == 0) return 0;
    if (!pred || !pred_strides || !gt || !gt_strides || !partial || !out) return ENVGS_ERR_BAD_ARG;
    const int64_t per_image = (int64_t)C * metric_tiles(H, W);
    if (per_image > INT32_MAX / B) return ENVGS_ERR_BAD_ARG;                     // a 1-D grid of B * per_image workgroups
    const Strides4 ps{pred_strides[0], pred_strides[1], pred_strides[2], pred_strides[3]};
    const Strides4 gs{gt_strides[0], gt_strides[1], gt_strides[2], gt_strides[3]};
    const int tiles_x = (W + MT - 1) / MT, tiles_y = (H + MT - 1) / MT;
    const dim3 grid((unsigned)(B * per_image));
    if (gt_dtype == ENVGS_METRICS_GT_U8)
        hipLaunchKernelGGL(image_metrics_tiles<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, C, H, W, tiles_x, tiles_y, pred, ps,
                           (const uint8_t *)gt, gs, partial);
    else
        hipLaunchKernelGGL(image_metrics_tiles<float>, grid, dim3(256), 0, (hipStream_t)stream, C, H, W, tiles_x, tiles_y, pred, ps,
                           (const float *)gt, gs, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(image_metrics_finish, dim3(B), dim3(256), 0, (hipStream_t)stream, C, H, W, (unsigned)per_image, partial, out);
    return (int)hipGetLastError();
}

}  // extern "C"
