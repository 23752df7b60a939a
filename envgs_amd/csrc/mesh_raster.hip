// mesh_raster.hip -- a triangle z-buffer over up to 8 views per launch: exact depth, face, barycentric, normal and colour maps of an indexed mesh and
// the faces some camera sees (include/envgs_mesh.h, "rasterisation"; the rule itself is csrc/mesh_raster.h, one text for this file and the host).
//
//   mr_raster   a lane per (face, view): project, set up, and for every covered pixel of the clamped box one 64-bit atomicMin of
//               (bits(z) << 32) | face on the key image.  A box of at most MR_SMALL_MAX pixels is walked by its lane.  A larger one is filed in LDS and,
//               behind one barrier, walked by the whole workgroup: the four wavefronts take its 8 x 8 tiles in turn, a lane per pixel, and skip a
//               tile that lies wholly outside an edge (decided on wave-uniform values).  Nothing grows with F x views: the list holds at most
//               one entry per lane.  A plain load of the key skips a fragment that cannot win; keys only decrease, so a stale value only costs
//               an atomic.
//   mr_resolve  a lane per (pixel, view): decode the key, recompute the winner's edge functions, write the maps that were asked for, and store 1
//               to seen[face] (a plain same-value store).
// The launch boundary orders the two; the host adds nothing: no sync, no read-back.
#include "common.h"
#include "mesh_raster.h"

namespace envgs {
namespace {

constexpr int MR_SMALL_MAX = 16;
constexpr int MR_TILE = 8;                                       // 8 x 8 pixels = one wavefront

struct MrLarge {
    MrFace face;
    uint32_t f;
    int32_t x0, x1, y0, y1;
};

// corners of face f in view C; false: dropped.  An index outside [0, V) is never dereferenced.
__device__ __forceinline__ bool mr_load_face(const uint32_t V, const float *__restrict__ vertices, const int32_t *__restrict__ faces, const uint32_t f,
                                             const envgs_mesh_raster_view &C, const float near, MrFace &face, uint32_t (&idx)[3])
{
    MrVertex c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int32_t i = faces[3 * (size_t)f + k];
        if (i < 0 || (uint32_t)i >= V) return false;
        idx[k] = (uint32_t)i;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float *p = vertices + 3 * (size_t)idx[k];
        c[k] = mr_project(C, p[0], p[1], p[2], near);
    }
    return mr_setup(c[0], c[1], c[2], face);
}

// (px, py) is inside the image: the box is clamped to it
__device__ __forceinline__ void mr_fragment(const MrFace &face, const uint32_t f, const int32_t px, const int32_t py, const int32_t W,
                                            uint64_t *__restrict__ img, uint32_t &covered, uint32_t &issued)
{
    int64_t E[3];
    if (!mr_covers(face, px, py, E)) return;
    covered++;
    const uint64_t key = mr_key(mr_depth(face, E), f);
    uint64_t *dst = img + (size_t)py * (size_t)W + (size_t)px;
    if (key < __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        atomicMin(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)key);
        issued++;
    }
}

// true: no pixel centre of the tile [x0, x1] x [y0, y1] can be covered -- some edge function is negative at the centre where it is largest
__device__ __forceinline__ bool mr_tile_outside(const MrFace &f, const int32_t x0, const int32_t x1, const int32_t y0, const int32_t y1)
{
    const int64_t Px0 = (int64_t)MR_SUB * x0 + MR_HALF, Px1 = (int64_t)MR_SUB * x1 + MR_HALF;
    const int64_t Py0 = (int64_t)MR_SUB * y0 + MR_HALF, Py1 = (int64_t)MR_SUB * y1 + MR_HALF;
    bool out = false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const int64_t dx = (int64_t)f.X[j] - f.X[i], dy = (int64_t)f.Y[j] - f.Y[i];
        const int64_t Emax = dx * ((dx > 0 ? Py1 : Py0) - f.Y[i]) - dy * ((dy > 0 ? Px0 : Px1) - f.X[i]);
        out = out || Emax < 0;
    }
    return out;
}

__global__ void __launch_bounds__(256)
mr_raster(const uint32_t V, const uint32_t F, const float *__restrict__ vertices, const int32_t *__restrict__ faces, const envgs_mesh_raster_views views,
          const int32_t H, const int32_t W, const float near, uint64_t *__restrict__ keys, unsigned long long *__restrict__ stats)
{
    __shared__ MrLarge s_large[256];
    __shared__ uint32_t s_count;
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    const envgs_mesh_raster_view &C = views.v[blockIdx.y];
    uint64_t *img = keys + (size_t)blockIdx.y * (size_t)H * (size_t)W;
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();

    uint32_t covered = 0u, issued = 0u;
    MrFace face;
    uint32_t idx[3];
    if (f < F && mr_load_face(V, vertices, faces, f, C, near, face, idx)) {
        int32_t x0, x1, y0, y1;
        mr_box(face, H, W, x0, x1, y0, y1);
        if (x0 <= x1 && y0 <= y1) {
            if ((x1 - x0 + 1) * (y1 - y0 + 1) <= MR_SMALL_MAX) {                       // at most H W < 2^28
                for (int32_t py = y0; py <= y1; py++)
                    for (int32_t px = x0; px <= x1; px++) mr_fragment(face, f, px, py, W, img, covered, issued);
            } else {
                MrLarge &L = s_large[atomicAdd(&s_count, 1u)];                          // at most one per lane: 256 slots
                L.face = face; L.f = f; L.x0 = x0; L.x1 = x1; L.y0 = y0; L.y1 = y1;
            }
        }
    }
    __syncthreads();

    const uint32_t n_large = s_count;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t e = 0; e < n_large; e++) {
        const MrLarge &L = s_large[e];
        const int32_t tx = (L.x1 - L.x0 + MR_TILE) / MR_TILE, ty = (L.y1 - L.y0 + MR_TILE) / MR_TILE;
        const int32_t tiles = tx * ty;
        for (int32_t t = wave; t < tiles; t += 4) {
            const int32_t row = t / tx;
            const int32_t bx = L.x0 + MR_TILE * (t - row * tx), by = L.y0 + MR_TILE * row;
            const int32_t ex = min(bx + MR_TILE - 1, L.x1), ey = min(by + MR_TILE - 1, L.y1);
            if (mr_tile_outside(L.face, bx, ex, by, ey)) continue;
            const int32_t px = bx + (lane & 7), py = by + (lane >> 3);
            if (px <= ex && py <= ey) mr_fragment(L.face, L.f, px, py, W, img, covered, issued);
        }
    }

    if (stats) {                                                                        // kernel-uniform
#pragma nounroll
        for (int d = 1; d < 64; d <<= 1) { covered += (uint32_t)__shfl_xor((int)covered, d); issued += (uint32_t)__shfl_xor((int)issued, d); }
        if (lane == 0 && covered) { atomicAdd(&stats[0], (unsigned long long)covered); atomicAdd(&stats[1], (unsigned long long)issued); }
    }
}

struct MrMaps {
    float *depth;
    int32_t *face;
    float *bary, *normal, *color;
    uint8_t *seen;
};

__global__ void __launch_bounds__(256)
mr_resolve(const uint32_t V, const float *__restrict__ vertices, const float *__restrict__ colors, const int32_t *__restrict__ faces,
           const envgs_mesh_raster_views views, const int32_t H, const int32_t W, const float near, const uint64_t *__restrict__ keys, const MrMaps out)
{
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    const uint32_t pix = blockIdx.x * 256u + threadIdx.x;
    if (pix >= HW) return;
    const size_t o = (size_t)blockIdx.y * (size_t)HW + pix;
    const uint64_t key = keys[o];
    const bool hit = key != MR_EMPTY;
    const uint32_t f = (uint32_t)(key & 0xffffffffu);
    if (out.depth) out.depth[o] = hit ? mr_float((uint32_t)(key >> 32)) : 0.f;
    if (out.face) out.face[o] = hit ? (int32_t)f : -1;
    if (hit && out.seen) out.seen[f] = 1;
    if (!(out.bary || out.normal || out.color)) return;

    float b[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f};
    if (hit) {
        // the winner was drawn, so it sets up again, and the pixel is covered
        MrFace face;
        uint32_t idx[3];
        (void)mr_load_face(V, vertices, faces, f, views.v[blockIdx.y], near, face, idx);
        const int32_t py = (int32_t)(pix / (uint32_t)W), px = (int32_t)(pix - (uint32_t)py * (uint32_t)W);
        int64_t E[3];
        (void)mr_covers(face, px, py, E);
        double t[3];
        const double s = mr_terms(face, E, t);
        const float b0 = (float)(t[0] / s), b1 = (float)(t[1] / s), b2 = (float)(t[2] / s);
        b[0] = b0; b[1] = face.exchanged ? b2 : b1; b[2] = face.exchanged ? b1 : b2;   // back to the original corners
        if (out.normal) {
            float p[3][3];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int a = 0; a < 3; a++) p[k][a] = vertices[3 * (size_t)idx[k] + a];
            mr_normal(p[0], p[1], p[2], face.exchanged, n);
        }
        if (out.color) {
#pragma unroll
            for (int a = 0; a < 3; a++)
                c[a] = (b[0] * colors[3 * (size_t)idx[0] + a] + b[1] * colors[3 * (size_t)idx[1] + a]) + b[2] * colors[3 * (size_t)idx[2] + a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (out.bary) out.bary[3 * o + a] = b[a];
        if (out.normal) out.normal[3 * o + a] = n[a];
        if (out.color) out.color[3 * o + a] = c[a];
    }
}

size_t mr_temp_bytes(int32_t H, int32_t W, int32_t views)
{
    if (H < 1 || W < 1 || (int64_t)H * (int64_t)W >= (1ll << 28) || views < 0 || views > ENVGS_TSDF_MAX_VIEWS) return 0;
    return (size_t)views * (size_t)H * (size_t)W * sizeof(uint64_t);
}

}  // namespace
}  // namespace envgs

using namespace envgs;

extern "C" {

int32_t envgs_mesh_raster_small_max(void) { return MR_SMALL_MAX; }

size_t envgs_mesh_raster_temp_bytes(int32_t H, int32_t W, int32_t views) { return mr_temp_bytes(H, W, views); }

int envgs_mesh_raster(uint32_t V, uint32_t F, const float *vertices, const float *colors, const int32_t *faces, const envgs_mesh_raster_views *views,
                      int32_t H, int32_t W, float near, int32_t first, void *temp, size_t temp_bytes, float *depth, int32_t *face, float *bary,
                      float *normal, float *color, uint8_t *seen, uint64_t *stats, void *stream)
{
    if (!views || views->count < 0 || views->count > ENVGS_TSDF_MAX_VIEWS || V >= (1u << 31) || F >= (1u << 31)) return ENVGS_ERR_BAD_ARG;
    if (H < 1 || W < 1 || (int64_t)H * (int64_t)W >= (1ll << 28) || near != near) return ENVGS_ERR_BAD_ARG;
    if ((V && !vertices) || (F && !faces) || (color && V && !colors)) return ENVGS_ERR_BAD_ARG;
    const int n = views->count;
    const size_t need = mr_temp_bytes(H, W, n);
    if (n && (!temp || ((uintptr_t)temp & 15u))) return ENVGS_ERR_BAD_ARG;
    if (temp_bytes < need) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t s = (hipStream_t)stream;
    if (first && seen && F) {
        const hipError_t e = hipMemsetAsync(seen, 0, F, s);
        if (e != hipSuccess) return (int)e;
    }
    if (n == 0) return 0;
    const hipError_t e = hipMemsetAsync(temp, 0xff, need, s);
    if (e != hipSuccess) return (int)e;
    uint64_t *keys = reinterpret_cast<uint64_t *>(temp);
    if (F) {
        hipLaunchKernelGGL(mr_raster, dim3((F + 255u) / 256u, (unsigned)n), dim3(256), 0, s, V, F, vertices, faces, *views, H, W, near, keys,
                           reinterpret_cast<unsigned long long *>(stats));
    }
    const MrMaps maps{depth, face, bary, normal, color, seen};
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    hipLaunchKernelGGL(mr_resolve, dim3((HW + 255u) / 256u, (unsigned)n), dim3(256), 0, s, V, vertices, colors, faces, *views, H, W, near,
                       (const uint64_t *)keys, maps);
    return (int)hipGetLastError();
}

}  // extern "C"
