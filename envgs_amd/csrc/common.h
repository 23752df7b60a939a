// common.h -- shared device helpers for the gfx950 surfel kernels (wave64, CDNA4).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "../../include/envgs_raster.h"
#include "prof.h"

namespace envgs {

constexpr int TILE = ENVGS_TILE;              // 16x16 pixel tiles (binning granularity of the reference)
constexpr int GEOM = ENVGS_GEOM_STRIDE;       // floats per surfel record
constexpr int GREC = ENVGS_GRAD_STRIDE;       // floats per gradient record
constexpr float NEAR_N = 0.2f;
constexpr float FAR_N = 100.0f;
constexpr float FILTER_SIZE = 0.707106f;
constexpr float FILTER_INV_SQ = 2.0f;
constexpr float ALPHA_CAP = 0.99f;
constexpr float ALPHA_MIN = 1.0f / 255.0f;
constexpr float T_EPS = 0.0001f;

// Per-surfel FEATURE arrays (SH coefficients, precomputed colours) may be stored in fp32 or fp16 (cfg->feature_f16); they are converted on
// load and everything downstream is fp32.  `h` is wave-uniform.
struct Feat {
    const void *p;
    bool h;
    __device__ __forceinline__ float operator[](size_t i) const {
        return h ? __half2float(reinterpret_cast<const __half *>(p)[i]) : reinterpret_cast<const float *>(p)[i];
    }
    __device__ __forceinline__ Feat at(size_t i) const { return Feat{reinterpret_cast<const char *>(p) + i * (h ? 2 : 4), h}; }
};

#define ENVGS_CHECK_LAUNCH(cfg, stream)                                             \
    do {                                                                            \
        hipError_t e__ = hipGetLastError();                                         \
        if (e__ != hipSuccess) return (int)e__;                                     \
        if ((cfg)->debug) {                                                         \
            e__ = hipStreamSynchronize((hipStream_t)(stream));                      \
            if (e__ != hipSuccess) return (int)e__;                                 \
        }                                                                           \
    } while (0)

// ---- wave64 cross-lane helpers (DPP; no LDS traffic) -------------------------------------------
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf, bool BOUND = true>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, BANK_MASK, BOUND));
}
template <int CTRL> __device__ __forceinline__ int dpp_mov_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
// The sum over a quad in every one of its lanes: lane ^ 1, then lane ^ 2 (quad_perm).
__device__ __forceinline__ float quad_sum(float v) { v += dpp_mov<0xB1>(v); v += dpp_mov<0x4E>(v); return v; }

// Sum over the 64 lanes; the result is returned wave-uniform (in an SGPR via readlane 63).
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_mov<0xB1>(v);                 // quad_perm [1,0,3,2]  (xor 1)
    v += dpp_mov<0x4E>(v);                 // quad_perm [2,3,0,1]  (xor 2)
    v += dpp_mov<0x141>(v);                // row_half_mirror      (xor 4 once quads are uniform)
    v += dpp_mov<0x140>(v);                // row_mirror           (xor 8 once octets are uniform)
    v += dpp_mov<0x142, 0xa, 0xf, false>(v);   // row_bcast15 into rows 1,3
    v += dpp_mov<0x143, 0xc, 0xf, false>(v);   // row_bcast31 into rows 2,3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}


typedef unsigned envgs_u2 __attribute__((ext_vector_type(2)));

// Sum 64 per-lane values over the wavefront, value v ending in lane v (a full 64 x 64 transpose-reduce in ~140 instructions):
// v_permlane32_swap and v_permlane16_swap fold the four 16-lane rows together two values per instruction (row r then owns values
// 16r..16r+15), and inside a row a butterfly halves the value count per step -- each lane keeps the half its own lane-id bit selects and
// receives the partner's contribution to that half through DPP (row_mirror, row_half_mirror, quad reversals pair lanes across bit 3,2,1,0).
__device__ __forceinline__ float wave_reduce64(const float (&g)[64], const int lane)
{
    float z[32];
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const envgs_u2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(g[i]), __float_as_uint(g[i + 32]), false, false);
        z[i] = __uint_as_float(r.x) + __uint_as_float(r.y);
    }
    float w[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const envgs_u2 q = __builtin_amdgcn_permlane16_swap(__float_as_uint(z[k]), __float_as_uint(z[k + 16]), false, false);
        w[k] = __uint_as_float(q.x) + __uint_as_float(q.y);
    }
    const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; k++) a[k] = (b3 ? w[k + 8] : w[k]) + dpp_mov<0x140>(b3 ? w[k] : w[k + 8]);       // partner lane ^ 15
    float b[4];
#pragma unroll
    for (int k = 0; k < 4; k++) b[k] = (b2 ? a[k + 4] : a[k]) + dpp_mov<0x141>(b2 ? a[k] : a[k + 4]);       // partner lane ^ 7
    float c[2];
#pragma unroll
    for (int k = 0; k < 2; k++) c[k] = (b1 ? b[k + 2] : b[k]) + dpp_mov<0x1B>(b1 ? b[k] : b[k + 2]);        // partner lane ^ 3
    return (b0 ? c[1] : c[0]) + dpp_mov<0xB1>(b0 ? c[0] : c[1]);                                            // partner lane ^ 1
}

// Inclusive scans over the 64 lanes (DPP only: row_shr 1,2,4,8 inside each 16-lane row, then row_bcast15 / row_bcast31 carry the row
// totals forward).  `IDENT` fills lanes whose source falls outside the row / the selected rows.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_fill(float v, float ident) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ident), __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_scan_add(float v) {
    v += dpp_fill<0x111>(v, 0.f); v += dpp_fill<0x112>(v, 0.f); v += dpp_fill<0x114>(v, 0.f); v += dpp_fill<0x118>(v, 0.f);
    v += dpp_fill<0x142, 0xa>(v, 0.f);
    v += dpp_fill<0x143, 0xc>(v, 0.f);
    return v;
}
__device__ __forceinline__ float wave_scan_mul(float v) {
    v *= dpp_fill<0x111>(v, 1.f); v *= dpp_fill<0x112>(v, 1.f); v *= dpp_fill<0x114>(v, 1.f); v *= dpp_fill<0x118>(v, 1.f);
    v *= dpp_fill<0x142, 0xa>(v, 1.f);
    v *= dpp_fill<0x143, 0xc>(v, 1.f);
    return v;
}
__device__ __forceinline__ float wave_bcast(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

// The integer inclusive scan, same lane patterns as wave_scan_add (the binning / scan / sort kernels of raster_bin.hip, mesh.hip, mesh_clean.hip).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_fill_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_scan_add_u32(uint32_t v) {
    v += dpp_fill_u32<0x111>(v); v += dpp_fill_u32<0x112>(v); v += dpp_fill_u32<0x114>(v); v += dpp_fill_u32<0x118>(v);
    v += dpp_fill_u32<0x142, 0xa>(v);
    v += dpp_fill_u32<0x143, 0xc>(v);
    return v;
}

// Transpose-reduce of 4*N4 per-lane values over the wavefront in ~(2+1+1)*N4 + ... instructions instead of 7 per value:
//   v_permlane32_swap pairs value i with value i+2*N4 (one add leaves i's 32 partial sums in the low half, the other's in the high half),
//   v_permlane16_swap pairs again (each 16-lane row now owns ONE value), four DPP row rotations finish the row sums, and N4-1 selects
//   merge the registers.  Result: lane r*16+k (k < N4) returns the sum over all 64 lanes of value k + r*N4.
template <int N4>
__device__ __forceinline__ float wave_transpose_reduce(const float (&g)[4 * N4], const int lane)
{
    float z[2 * N4];
#pragma unroll
    for (int i = 0; i < 2 * N4; i++) {
        const envgs_u2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(g[i]), __float_as_uint(g[i + 2 * N4]), false, false);
        z[i] = __uint_as_float(r.x) + __uint_as_float(r.y);
    }
    float w[N4];
#pragma unroll
    for (int k = 0; k < N4; k++) {
        const envgs_u2 q = __builtin_amdgcn_permlane16_swap(__float_as_uint(z[k]), __float_as_uint(z[k + N4]), false, false);
        float v = __uint_as_float(q.x) + __uint_as_float(q.y);
        v += dpp_mov<0x128>(v);                // row_ror:8
        v += dpp_mov<0x124>(v);                // row_ror:4
        v += dpp_mov<0x122>(v);                // row_ror:2
        v += dpp_mov<0x121>(v);                // row_ror:1
        w[k] = v;
    }
    float out = w[0];
#pragma unroll
    for (int k = 1; k < N4; k++) out = ((lane & 15) == k) ? w[k] : out;
    return out;
}

__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// Exclusive prefix of `v` over the workgroup's NW wavefronts (thread order), and the workgroup total.  s_w: NW words of LDS.
template <int NW>
__device__ __forceinline__ uint32_t block_exclusive_u32(uint32_t v, uint32_t *s_w, uint32_t &total)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t inc = wave_scan_add_u32(v);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) { const uint32_t t = s_w[k]; all += t; before += (k < wave) ? t : 0u; }
    total = all;
    __syncthreads();
    return before + inc - v;
}

__device__ __forceinline__ void atomic_add_f32(float *p, float v) { unsafeAtomicAdd(p, v); }

// The XCD (0..7, each with a private L2) the calling wavefront really runs on.
__device__ __forceinline__ int xcc_id()
{
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return (int)(v & 7u);
}

// ---- tile queues of the persistent compositing grids (R6 / R7, raster_render.hip) ----------------
// A call's tile queue block (include/envgs_raster.h: tile_queue), in 32-bit words:
//   [0, 256)      R6's eight queue heads, one per 128 B line        [256, 512)  R7's
//   then order6[ntiles], order7[ntiles], tile_cost[ntiles]
// order[x * per .. ) with per = ceil(ntiles / 8) is queue x: the tiles of band x (the contiguous eighth xcd_tile() gives XCD x), heaviest
// cost class first, tile index ascending inside a class.
constexpr int TQ_CLASSES = 32;
constexpr int TQ_HEAD_STRIDE = 32;
constexpr int TQ_HEADS = 8 * TQ_HEAD_STRIDE;
struct TileQueue {
    uint32_t *heads6, *heads7, *order6, *order7, *tile_cost;
};
__host__ __device__ inline size_t tile_queue_words(int ntiles) { return 2 * (size_t)TQ_HEADS + 3 * (size_t)ntiles; }
inline TileQueue tile_queue_of(uint32_t *block, int ntiles)
{
    return TileQueue{block, block + TQ_HEADS, block + 2 * TQ_HEADS, block + 2 * TQ_HEADS + ntiles, block + 2 * TQ_HEADS + 2 * (size_t)ntiles};
}
constexpr uint32_t TQ_COST_MAX = (1u << 27) - 1u;         // costs saturate here: cost * TQ_CLASSES stays inside 32 bits
__host__ __device__ inline int tile_cost_class(uint32_t cost, uint32_t max_cost)
{
    return (int)((cost * (uint32_t)TQ_CLASSES) / (max_cost + 1u));                  // 0 .. TQ_CLASSES - 1
}

// Builds the queues from the tiles' costs and clears the eight heads: a counting sort into TQ_CLASSES classes, per band -- or, with one_queue,
// over all tiles into ONE queue (head 0; inside a class the bands follow each other, so tile index still ascends).  Called by every thread of ONE
// workgroup (a whole number of wavefronts).  cost(t) = hi[t * stride] - (lo ? lo[t * stride] : 0); hi == nullptr = every cost 0 (index order).
// The costs are read once, coalesced, and staged in LDS; an image of more than TQ_STAGE tiles (2 M pixels) gets index order.
// One workgroup runs this code once: what it costs is instruction fetch, so the loops stay rolled and there is one division, 32 bits wide.
constexpr int TQ_STAGE = 8192;
struct TileOrderLds {
    uint32_t hist[8 * TQ_CLASSES];     // tiles per (band, class)
    uint32_t base[8 * TQ_CLASSES];     // per (band, class): the next place in the order
    uint32_t max_cost;
    uint32_t cls[TQ_STAGE];            // per tile: its cost, then its class
};
__device__ __forceinline__ void build_tile_order(const uint32_t *hi, const uint32_t *lo, const int stride, const int ntiles, const bool one_queue,
                                                 uint32_t *__restrict__ order, uint32_t *__restrict__ heads, TileOrderLds &S)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nw = nthreads >> 6;
    if (tid < 8) heads[tid * TQ_HEAD_STRIDE] = 0u;
    if (ntiles > TQ_STAGE || !hi) {
        for (int t = tid; t < ntiles; t += nthreads) order[t] = (uint32_t)t;
        return;
    }
    for (int i = tid; i < 8 * TQ_CLASSES; i += nthreads) S.hist[i] = 0u;
    if (tid == 0) S.max_cost = 0u;
    __syncthreads();
    uint32_t m = 0u;
#pragma nounroll
    for (int t = tid; t < ntiles; t += nthreads) {
        uint32_t c = hi[(size_t)t * stride];
        if (lo) c -= lo[(size_t)t * stride];
        c = min(c, TQ_COST_MAX);
        S.cls[t] = c;
        m = max(m, c);
    }
#pragma nounroll
    for (int d = 1; d < 64; d <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    if (lane == 0) atomicMax(&S.max_cost, m);
    __syncthreads();
    const uint32_t max_cost = S.max_cost;
    const int per = (ntiles + 7) >> 3;
#pragma nounroll
    for (int t = tid; t < ntiles; t += nthreads) {
        const int k = tile_cost_class(S.cls[t], max_cost);
        S.cls[t] = (uint32_t)k;
        atomicAdd(&S.hist[(t / per) * TQ_CLASSES + k], 1u);
    }
    __syncthreads();
    // one wavefront per band takes its tiles to their places, 64 at a time: the lanes of one class (found with one ballot per class bit, no
    // loop over the classes) take consecutive places behind the class's running base, which the first of them moves on
    static_assert(TQ_CLASSES == 32, "five class bits");
    const unsigned long long lanes_before = (1ull << lane) - 1ull;
#pragma nounroll
    for (int row = wave; row < 8; row += nw) {
        const int first = row * per, cnt = max(0, min(per, ntiles - first));
        if (cnt == 0) continue;
        // lane k: where this band's tiles of class k start = the tiles of the heavier classes (of this band, or with one queue of every
        // band) + with one queue the earlier bands' tiles of class k
        uint32_t heavier = 0u, base = one_queue ? 0u : (uint32_t)first;
        if (lane < TQ_CLASSES) {
            if (one_queue) {
#pragma nounroll
                for (int x = 0; x < 8; x++) {
                    const uint32_t h = S.hist[x * TQ_CLASSES + lane];
                    heavier += h;
                    base += x < row ? h : 0u;
                }
            } else {
                heavier = S.hist[row * TQ_CLASSES + lane];
            }
        }
#pragma nounroll
        for (int k = 1; k < TQ_CLASSES; k++) {
            const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)heavier, k);
            base += k > lane ? h : 0u;
        }
        uint32_t *bases = S.base + row * TQ_CLASSES;         // this wavefront's alone
        if (lane < TQ_CLASSES) __hip_atomic_store(&bases[lane], base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma nounroll
        for (int start = 0; start < cnt; start += 64) {
            const int i = start + lane;
            const bool valid = i < cnt;
            const uint32_t c = valid ? S.cls[first + i] : 0u;
            unsigned long long same = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
            for (int bit = 0; bit < 5; bit++) {
                const bool on = (c >> bit) & 1u;
                const unsigned long long b = __builtin_amdgcn_ballot_w64(on);
                same &= on ? b : ~b;
            }
            if (valid) {
                const uint32_t rank = (uint32_t)__builtin_popcountll(same & lanes_before);
                const uint32_t b0 = __hip_atomic_load(&bases[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                order[b0 + rank] = (uint32_t)(first + i);
                if (rank == 0u) __hip_atomic_store(&bases[c], b0 + (uint32_t)__builtin_popcountll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
}

// ---- launchers implemented in the kernel translation units ---------------------------------------
int launch_project(const envgs_raster_cfg *cfg, const float *means3D, const float *scales, const float *rotations,
                   const float *opacities, const float *shs, const float *transmat_precomp, const float *viewmatrix,
                   const float *projmatrix, const float *campos, float *geom, float *rgb, uint8_t *clamped,
                   int32_t *radii, uint32_t *tiles_touched, hipStream_t stream);
int launch_scan(const uint32_t *in, uint32_t *out, int n, void *temp, size_t temp_bytes, hipStream_t stream);
size_t scan_temp_bytes(int n);
size_t sort_temp_bytes(uint32_t n, int width, int height);
int launch_bin(const envgs_raster_cfg *cfg, uint32_t N, const float *geom, const int32_t *radii, uint64_t *tile_pairs,
               uint64_t *keys_sorted, uint32_t *point_list, void *bin_temp, size_t bin_temp_bytes, uint32_t *ranges, hipStream_t stream,
               uint32_t *tile_queue = nullptr);
void launch_tile_order(int ntiles, const uint32_t *hi, const uint32_t *lo, int stride, uint32_t *order, uint32_t *heads, hipStream_t stream);
inline bool tile_one_queue() { return (debug_switch(ENVGS_DBG_BALANCE) & 4) == 0; }      // ENVGS_DBG_BALANCE value 4: one queue per band instead
size_t key_sort_temp_bytes(int n);
int launch_key_sort(int n, const uint64_t *keys_in, uint64_t *keys_out, int top_bit, void *temp, size_t temp_bytes, hipStream_t stream);
size_t ray_sort_temp_bytes(int R);
int launch_ray_sort(int R, const float *ray_o, const float *ray_d, const float4 *nodes, int P, uint64_t *pairs, uint32_t *order, void *temp,
                    size_t temp_bytes, hipStream_t stream);
int launch_render_fwd(const envgs_raster_cfg *cfg, const uint32_t *ranges, const uint32_t *point_list, const float *geom,
                      const float *colors, const float *bg, float *out_color, float *allmap, float *final_T,
                      int32_t *n_contrib, float *weight, hipStream_t stream, uint8_t *audit_contrib = nullptr, int audit_lmax = 0, int colors_f16 = 0,
                      uint8_t *contrib_mask = nullptr, const uint8_t *audit_skip = nullptr, uint32_t *tile_queue = nullptr);
int launch_render_bwd(const envgs_raster_cfg *cfg, const uint32_t *ranges, const uint32_t *point_list, const float *geom,
                      const float *colors, const float *bg, const float *final_T, const int32_t *n_contrib,
                      const float *dL_dcolor, const float *dL_dallmap, float *grad_rec, hipStream_t stream, int colors_f16 = 0,
                      const uint8_t *contrib_mask = nullptr, uint32_t *tile_queue = nullptr);
int launch_project_bwd(const envgs_raster_cfg *cfg, const float *geom, const float *means3D, const float *scales,
                       const float *rotations, const float *shs, const uint8_t *clamped, const float *transmat_precomp,
                       const int32_t *radii, const float *viewmatrix, const float *projmatrix, const float *campos,
                       const float *grad_rec, float *dmeans3D, float *dmeans2D, float *dscales, float *drots, float *dshs,
                       float *dcolors, float *dopacities, float *dtransmat_precomp, hipStream_t stream);

int launch_sh_record_bwd(int P, int D, const float *means3D, const float *shs, const float *campos, const uint8_t *clamped, const int32_t *radii,
                         const float *grad_rec, float *dmeans3D, float *dshs, hipStream_t stream);

__host__ __device__ inline int tile_bits(int width, int height) {
    int tiles = ((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE);
    int b = 0;
    while ((1 << b) < tiles) b++;
    return b < 1 ? 1 : b;
}

}  // namespace envgs
