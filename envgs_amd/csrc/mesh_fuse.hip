// mesh_fuse.hip -- multi-view depth-map fusion (include/envgs_mesh.h, "depth fusion"): the consistency check of a reference depth map against
// its source views, and the order-preserving compaction of the surviving pixels into a point cloud.
//
//   fuse_consistency  a lane per reference pixel, a uniform loop over the (at most 8) sources of the launch.  The two affine maps of a pair
//                     travel by value in the kernel arguments and are read through the scalar path; the lane's only memory traffic is its own
//                     reference depth, at most four taps per source and one byte + one float out.
//   fuse_count        a lane per pixel of ALL views: the averaged depth, the final bit, the workgroup's number of kept pixels
//   launch_scan       over the per-workgroup totals (raster_bin.hip: the library's one device-wide scan)
//   fuse_total        the grand total as int64, from the last scanned counter
//   fuse_emit         a lane per pixel again: its place = the scanned total of the earlier workgroups + its rank inside the workgroup
// No atomic is issued anywhere: two runs give identical bytes.  Every store is an ordinary vector store.
#include "common.h"
#include "../../include/envgs_mesh.h"

namespace envgs {
namespace {

constexpr float FUSE_FLT_MAX = 3.402823466e+38f;
__device__ __forceinline__ bool fu_finite(float v) { return fabsf(v) <= FUSE_FLT_MAX; }                 // false on NaN and on +-inf

// grid_sample(mode='bilinear', padding_mode='border', align_corners=False) of one (H,W) map at the pixel coordinate (u, v): the taps inside the
// image are multiplied by their weights and added in the order (y0,x0) (y0,x1) (y1,x0) (y1,x1), a weight of 0 included (0 * NaN is NaN, as in
// torch); a tap outside the image -- x1 = W or y1 = H under the clip, where its weight is 0 -- is not read.
__device__ __forceinline__ float fu_sample(const float *__restrict__ map, const int H, const int W, const float u, const float v)
{
    const float ix = fminf(fmaxf(u - 0.5f, 0.f), (float)(W - 1)), iy = fminf(fmaxf(v - 0.5f, 0.f), (float)(H - 1));
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
    const bool xin = x0 + 1 < W, yin = y0 + 1 < H;
    const float *row0 = map + (size_t)y0 * (size_t)W + (size_t)x0;
    float s = row0[0] * (wx0 * wy0);
    if (xin) s += row0[1] * (wx1 * wy0);
    if (yin) {
        const float *row1 = row0 + W;
        s += row1[0] * (wx0 * wy1);
        if (xin) s += row1[1] * (wx1 * wy1);
    }
    return s;
}

__global__ void __launch_bounds__(256)
fuse_consistency(const uint32_t n, const int W, const float *__restrict__ dref, const envgs_fuse_sources S, const float abs_thresh,
                 const float rel_thresh, const int accumulate, uint8_t *__restrict__ count, float *__restrict__ sum)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float d = dref[i];
    const uint32_t y = i / (uint32_t)W, x = i - y * (uint32_t)W;
    const float xc = (float)x + 0.5f, yc = (float)y + 0.5f;
    uint32_t c = accumulate ? (uint32_t)count[i] : 0u;
    float acc = accumulate ? sum[i] : 0.f;
    if (d > 0.f && fu_finite(d)) {
        for (int k = 0; k < S.count; k++) {
            const envgs_fuse_source &P = S.v[k];
            const float *F = P.fwd, *B = P.back;
            // reference pixel -> source image
            const float px = d * (F[0] * xc + F[1] * yc + F[2]) + F[9];
            const float py = d * (F[3] * xc + F[4] * yc + F[5]) + F[10];
            const float pz = d * (F[6] * xc + F[7] * yc + F[8]) + F[11];
            const float u = px / pz, v = py / pz;
            if (!(fu_finite(u) && fu_finite(v))) continue;
            const float s = fu_sample(P.depth, P.H, P.W, u, v);
            if (!(s > 0.f && fu_finite(s))) continue;
            // source image, at the sampled depth -> reference camera
            const float qx = s * (B[0] * u + B[1] * v + B[2]) + B[9];
            const float qy = s * (B[3] * u + B[4] * v + B[5]) + B[10];
            const float z = s * (B[6] * u + B[7] * v + B[8]) + B[11];
            const float dx = qx / z - xc, dy = qy / z - yc;
            const float dist = sqrtf(dx * dx + dy * dy);
            const float rel = fabsf(z - d) / d;
            if (dist < abs_thresh && rel < rel_thresh) { c++; acc += z; }                   // every comparison is false on NaN
        }
    }
    count[i] = (uint8_t)(c < 255u ? c : 255u);
    sum[i] = acc;
}

__global__ void __launch_bounds__(256)
fuse_count(const uint32_t n, const float *__restrict__ depth, const uint8_t *__restrict__ count, const float *__restrict__ sum, const uint32_t min_count,
           const float pho_thresh, float *__restrict__ depth_avg, uint8_t *__restrict__ final_mask, uint32_t *__restrict__ tot)
{
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool on = false;
    if (i < n) {
        const float d = depth[i];
        const uint32_t c = count[i];
        depth_avg[i] = (sum[i] + d) / (float)(c + 1u);
        on = c >= min_count && d > pho_thresh;
        final_mask[i] = on ? 1 : 0;
    }
    uint32_t total;
    (void)block_exclusive_u32<4>(on ? 1u : 0u, s_w, total);
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

__global__ void fuse_total(const uint32_t *__restrict__ tot, const uint32_t nb, long long *__restrict__ total)
{
    if (threadIdx.x == 0) total[0] = (long long)tot[nb - 1];
}

// tot holds the INCLUSIVE scan over the workgroups here.  view_maps (V,12): A_v row major, then c_v.
__global__ void __launch_bounds__(256)
fuse_emit(const uint32_t n, const uint32_t HW, const uint32_t W, const float *__restrict__ depth_avg, const uint8_t *__restrict__ final_mask,
          const uint32_t *__restrict__ tot, const float *__restrict__ view_maps, const float *__restrict__ rgb, const float *__restrict__ normal,
          const uint32_t N, float *__restrict__ points, float *__restrict__ colors, float *__restrict__ normals, long long *__restrict__ index)
{
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool on = i < n && final_mask[i] != 0;
    uint32_t total;
    const uint32_t k = block_exclusive_u32<4>(on ? 1u : 0u, s_w, total) + (blockIdx.x ? tot[blockIdx.x - 1] : 0u);
    if (!on || k >= N) return;
    const uint32_t v = i / HW, r = i - v * HW, y = r / W, x = r - y * W;
    const float xc = (float)x + 0.5f, yc = (float)y + 0.5f, d = depth_avg[i];
    const float *M = view_maps + 12 * (size_t)v;
#pragma unroll
    for (int a = 0; a < 3; a++) points[3 * (size_t)k + a] = M[9 + a] + d * (M[3 * a] * xc + M[3 * a + 1] * yc + M[3 * a + 2]);
    const size_t plane = (size_t)v * 3 * HW + r;
    if (colors) {
#pragma unroll
        for (int a = 0; a < 3; a++) colors[3 * (size_t)k + a] = rgb[plane + (size_t)a * HW];
    }
    if (normals) {
#pragma unroll
        for (int a = 0; a < 3; a++) normals[3 * (size_t)k + a] = normal[plane + (size_t)a * HW];
    }
    if (index) index[k] = (long long)i;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }
constexpr uint64_t COUNT_LIMIT = 1ull << 31;

// the pixels of a call, 0 if the sizes are out of range
uint64_t fuse_pixels(int32_t V, int32_t H, int32_t W)
{
    if (V < 1 || H < 1 || W < 1) return 0;
    const uint64_t hw = (uint64_t)H * (uint64_t)W;
    if (hw >= COUNT_LIMIT) return 0;
    const uint64_t n = hw * (uint64_t)V;
    return n >= COUNT_LIMIT ? 0 : n;
}

// tot (nb) | scan scratch
struct FuseTemp { size_t tot, scan, scan_bytes, total; uint32_t nb; };
FuseTemp fuse_temp(uint32_t n)
{
    FuseTemp t;
    t.nb = blocks_of(n);
    t.tot = 0;
    t.scan = up256(4 * (size_t)t.nb);
    t.scan_bytes = scan_temp_bytes((int)t.nb);
    t.total = t.scan + up256(t.scan_bytes);
    return t;
}

}  // namespace
}  // namespace envgs

using namespace envgs;

extern "C" {

int envgs_fuse_consistency(int32_t H, int32_t W, const float *depth_ref, const envgs_fuse_sources *sources, float geo_abs_thresh, float geo_rel_thresh,
                           int32_t accumulate, uint8_t *count, float *sum, void *stream)
{
    const uint64_t n = fuse_pixels(1, H, W);
    if (!n || !depth_ref || !sources || sources->count < 0 || sources->count > ENVGS_TSDF_MAX_VIEWS || !count || !sum) return ENVGS_ERR_BAD_ARG;
    for (int k = 0; k < sources->count; k++)
        if (!sources->v[k].depth || sources->v[k].H != H || sources->v[k].W != W) return ENVGS_ERR_BAD_ARG;
    hipLaunchKernelGGL(fuse_consistency, dim3(blocks_of((uint32_t)n)), dim3(256), 0, (hipStream_t)stream, (uint32_t)n, (int)W, depth_ref, *sources,
                       geo_abs_thresh, geo_rel_thresh, (int)accumulate, count, sum);
    return (int)hipGetLastError();
}

size_t envgs_fuse_temp_bytes(int32_t V, int32_t H, int32_t W)
{
    const uint64_t n = fuse_pixels(V, H, W);
    return n ? fuse_temp((uint32_t)n).total : 0;
}

int envgs_fuse_count(int32_t V, int32_t H, int32_t W, const float *depth, const uint8_t *count, const float *sum, uint32_t min_count,
                     float pho_abs_thresh, float *depth_avg, uint8_t *final_mask, void *temp, size_t temp_bytes, int64_t *total, void *stream_)
{
    const uint64_t n = fuse_pixels(V, H, W);
    if (!n || !depth || !count || !sum || !depth_avg || !final_mask || !temp || !aligned16(temp) || !total) return ENVGS_ERR_BAD_ARG;
    const FuseTemp T = fuse_temp((uint32_t)n);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)temp;
    uint32_t *tot = (uint32_t *)(base + T.tot);
    hipLaunchKernelGGL(fuse_count, dim3(T.nb), dim3(256), 0, stream, (uint32_t)n, depth, count, sum, min_count, pho_abs_thresh, depth_avg, final_mask, tot);
    const int rc = launch_scan(tot, tot, (int)T.nb, base + T.scan, T.scan_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(fuse_total, dim3(1), dim3(64), 0, stream, (const uint32_t *)tot, T.nb, (long long *)total);
    return (int)hipGetLastError();
}

int envgs_fuse_emit(int32_t V, int32_t H, int32_t W, const float *depth_avg, const uint8_t *final_mask, const void *temp, size_t temp_bytes,
                    const float *view_maps, const float *rgb, const float *normal, uint32_t N, float *points, float *colors, float *normals,
                    int64_t *index, void *stream)
{
    const uint64_t n = fuse_pixels(V, H, W);
    if (!n || N > n || !depth_avg || !final_mask || !temp || !aligned16(temp) || !view_maps || (N && !points) || (colors && !rgb) || (normals && !normal))
        return ENVGS_ERR_BAD_ARG;
    const FuseTemp T = fuse_temp((uint32_t)n);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(fuse_emit, dim3(T.nb), dim3(256), 0, (hipStream_t)stream, (uint32_t)n, (uint32_t)((uint64_t)H * (uint64_t)W), (uint32_t)W, depth_avg,
                       final_mask, (const uint32_t *)((const char *)temp + T.tot), view_maps, rgb, normal, N, points, colors, normals, (long long *)index);
    return (int)hipGetLastError();
}

}  // extern "C"
