// mesh_register.hip -- rigid registration and the Tanks-and-Temples protocol for gfx950 (include/envgs_mesh.h, "registration"): the fp32 rigid
// transformation, the 18 sums of one point-to-point ICP iteration over the exact grid search, the sparse voxel mean and the polygon crop volume.
// Built with -ffp-contract=off (build.py): the transformed rows, the cells, the squared distances and the fixed-point offsets follow the header's
// fp32 sequence operation for operation, and the double products of the sums and of the crossing test are never contracted either.
//
// Transformation
//   pt_apply       a lane per point: pt_transform of mesh_points.h
// Registration
//   rg_sums        a lane per source point: pt_transform, then pg_walk of mesh_points.h (the walk of envgs_points_nearest) on the moved point; a
//                  matched lane forms its 18 terms in double.  Lanes -> wavefront by a shuffle tree (lane l takes l + 32, then 16, 8, 4, 2, 1), the
//                  four wavefronts in order through LDS, one row of 18 doubles (144 B) per workgroup.  No atomic of any kind.
//   rg_final       ONE workgroup: thread t adds the rows t, t + 256, t + 512 .. in ascending order, then the same tree over the 256 threads
// Voxel mean (the keys are sorted in between by the caller)
//   vd_keys        a lane per point: the 63-bit key i | j << 21 | k << 42 of its cell (rule 1 of the simplification), or the largest int64
//   vd_heads       a lane per sorted slot: 1 where a new key begins;  launch_scan over the flags: the cluster of every slot
//   vd_accumulate  a lane per sorted slot: the fixed-point offsets of its point (sc_locate, rule 3) summed per cluster with integer atomics, the
//                  runs of one cluster inside a wavefront merged first (the pattern of sc_accumulate: the slots of a cluster are consecutive here)
//   vd_finish      a lane per cluster: a single member keeps its bits, else the rounded integer means
// Crop volume
//   pv_inside      a lane per point: the polygon's (u, v) columns staged in LDS (4 KB), the crossing number in double as the header writes it
#include "common.h"
#include "mesh_points.h"

#include "../../include/envgs_mesh.h"

namespace envgs {
namespace {

constexpr uint32_t COUNT_LIMIT = 1u << 31;
constexpr int RG_SUMS = ENVGS_REGISTER_SUMS;                      // n | sum d2 | sum a (3) | sum b (3) | sum a b^T (9, row major) | sum |a|^2

__global__ void __launch_bounds__(256)
pt_apply(const uint32_t N, const float *__restrict__ points, const Rigid M, float *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    float a[3];
    pt_transform(M, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], a);
#pragma unroll
    for (int e = 0; e < 3; e++) out[3 * (size_t)i + e] = a[e];
}

// ---- registration ---------------------------------------------------------------------------------------------------------------------------------------
// The 18 per-lane values -> thread 0 .. 17 of the workgroup holds the sum of value k: the order is fixed by the lane and wavefront numbers alone.
// Every lane of the workgroup must arrive here.
__device__ __forceinline__ double rg_block_sum(double (&t)[RG_SUMS], double (&s_part)[4][RG_SUMS])
{
#pragma unroll
    for (int k = 0; k < RG_SUMS; k++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t[k] += __shfl_down(t[k], d);          // lane 0 ends with the balanced tree over the 64 lanes
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < RG_SUMS; k++) s_part[threadIdx.x >> 6][k] = t[k];
    }
    __syncthreads();
    const uint32_t k = threadIdx.x < (uint32_t)RG_SUMS ? threadIdx.x : 0u;
    return ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
}

__global__ void __launch_bounds__(256)
rg_sums(const uint32_t Q, const float *__restrict__ source, const Rigid M, const float max_distance, const Grid g, const uint32_t *__restrict__ cell_end,
        const float4 *__restrict__ records, const double cx, const double cy, const double cz, double *__restrict__ rows, float *__restrict__ moved,
        float *__restrict__ dist2, int32_t *__restrict__ index)
{
    __shared__ double s_part[4][RG_SUMS];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    double t[RG_SUMS];
#pragma unroll
    for (int k = 0; k < RG_SUMS; k++) t[k] = 0.0;
    if (q < Q) {
        float a[3];
        pt_transform(M, source[3 * (size_t)q], source[3 * (size_t)q + 1], source[3 * (size_t)q + 2], a);
        const Best best = pg_walk(a[0], a[1], a[2], max_distance, g, cell_end, records);
        if (moved) {
#pragma unroll
            for (int e = 0; e < 3; e++) moved[3 * (size_t)q + e] = a[e];
        }
        if (dist2) dist2[q] = best.d2;
        if (index) index[q] = (int32_t)best.index;
        if (best.index != 0xffffffffu) {
            const float4 p = records[best.slot];                  // the grid does not keep the points: the matched coordinates are its record's
            const double ah[3] = {(double)a[0] - cx, (double)a[1] - cy, (double)a[2] - cz};
            const double bh[3] = {(double)p.x - cx, (double)p.y - cy, (double)p.z - cz};
            t[0] = 1.0;
            t[1] = (double)best.d2;
#pragma unroll
            for (int e = 0; e < 3; e++) { t[2 + e] = ah[e]; t[5 + e] = bh[e]; }
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) t[8 + 3 * r + c] = ah[r] * bh[c];
            }
            t[17] = ((ah[0] * ah[0]) + (ah[1] * ah[1])) + (ah[2] * ah[2]);
        }
    }
    const double s = rg_block_sum(t, s_part);
    if (threadIdx.x < (uint32_t)RG_SUMS) rows[(size_t)blockIdx.x * RG_SUMS + threadIdx.x] = s;
}

__global__ void __launch_bounds__(256)
rg_final(const uint32_t R, const double *__restrict__ rows, double *__restrict__ sums)
{
    __shared__ double s_part[4][RG_SUMS];
    double t[RG_SUMS];
#pragma unroll
    for (int k = 0; k < RG_SUMS; k++) t[k] = 0.0;
    for (uint32_t r = threadIdx.x; r < R; r += 256u) {
#pragma unroll
        for (int k = 0; k < RG_SUMS; k++) t[k] += rows[(size_t)r * RG_SUMS + k];
    }
    const double s = rg_block_sum(t, s_part);
    if (threadIdx.x < (uint32_t)RG_SUMS) sums[threadIdx.x] = s;
}

// ---- the sparse voxel mean ------------------------------------------------------------------------------------------------------------------------------
constexpr long long VD_NO_KEY = 0x7fffffffffffffffll;

__global__ void __launch_bounds__(256)
vd_keys(const uint32_t N, const float *__restrict__ points, const Grid g, long long *__restrict__ keys)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= N) return;
    const float x = points[3 * (size_t)v], y = points[3 * (size_t)v + 1], z = points[3 * (size_t)v + 2];
    long long key = VD_NO_KEY;
    if (ev_finite(x) && ev_finite(y) && ev_finite(z))
        key = (long long)pg_axis(x, g.o[0], g.cell, g.n[0]) | ((long long)pg_axis(y, g.o[1], g.cell, g.n[1]) << 21)
              | ((long long)pg_axis(z, g.o[2], g.cell, g.n[2]) << 42);
    keys[v] = key;
}

__global__ void __launch_bounds__(256)
vd_heads(const uint32_t N, const long long *__restrict__ keys, uint32_t *__restrict__ flags)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= N) return;
    const long long key = keys[s];
    flags[s] = (key != VD_NO_KEY && (s == 0 || keys[s - 1] != key)) ? 1u : 0u;
}

// per-cluster sums: pos (N,3) u64 | cnt (N) | idx (N) | key (N) i64
struct VoxelSums { unsigned long long *pos; uint32_t *cnt, *idx; long long *key; };

// scan holds the INCLUSIVE scan of the head flags: the cluster of slot s is scan[s] - 1
__global__ void __launch_bounds__(256)
vd_accumulate(const uint32_t N, const float *__restrict__ points, const Grid g, const long long *__restrict__ keys, const long long *__restrict__ order,
              const uint32_t *__restrict__ scan, const VoxelSums S, int32_t *__restrict__ cluster_of, uint32_t *__restrict__ count)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s == 0) *count = scan[N - 1];
    const int lane = lane_id();
    uint32_t cl = 0xffffffffu;
    long long key = VD_NO_KEY;
    uint32_t a[5] = {0, 0, 0, 0, 0};                              // q of x y z, members, point index
    if (s < N) {
        key = keys[s];
        const unsigned long long v = (unsigned long long)order[s];
        if (v < N) {                                              // an index outside the cloud is never dereferenced
            if (key != VD_NO_KEY) {
                cl = scan[s] - 1u;
                int32_t i;
#pragma unroll
                for (int e = 0; e < 3; e++) sc_locate(points[3 * (size_t)v + e], g.o[e], g.cell, g.n[e], i, a[e]);
                a[3] = 1; a[4] = (uint32_t)v;
            }
            if (cluster_of) cluster_of[v] = (int32_t)cl;          // no cluster is -1
        }
    }
    // runs of equal clusters over consecutive lanes: `start` = first lane of the own run, the last lane of a run adds its sum
    const uint32_t prev = (uint32_t)__shfl_up((int)cl, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != cl);
    const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const bool take = lane - d >= start;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const uint32_t o = (uint32_t)__shfl_up((int)a[k], d);
            a[k] += take ? o : 0u;
        }
    }
    if (!last || cl == 0xffffffffu) return;
#pragma unroll
    for (int c = 0; c < 3; c++) atomicAdd(S.pos + 3 * (size_t)cl + c, (unsigned long long)a[c]);
    atomicAdd(S.cnt + cl, a[3]);
    atomicAdd(S.idx + cl, a[4]);                                  // wraps when n > 1; read only when n == 1
    S.key[cl] = key;                                              // every member stores the same word
}

__global__ void __launch_bounds__(256)
vd_finish(const uint32_t N, const uint32_t C, const float *__restrict__ points, const Grid g, const VoxelSums S, float *__restrict__ out)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= C) return;
    const uint32_t n = S.cnt[c];
    if (n == 0) return;                                           // a C beyond the counted clusters: the row is left alone
    if (n == 1) {
        const uint32_t v = S.idx[c];
        if (v >= N) return;
#pragma unroll
        for (int e = 0; e < 3; e++) ((uint32_t *)out)[3 * (size_t)c + e] = ((const uint32_t *)points)[3 * (size_t)v + e];
        return;
    }
    const long long key = S.key[c];
    const uint32_t ijk[3] = {(uint32_t)(key & 0x1fffff), (uint32_t)((key >> 21) & 0x1fffff), (uint32_t)((key >> 42) & 0x1fffff)};
    const unsigned long long two_n = 2ull * n;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const uint32_t qm = (uint32_t)((2ull * S.pos[3 * (size_t)c + e] + n) / two_n);
        out[3 * (size_t)c + e] = g.o[e] + ((float)ijk[e] + (float)qm * POS_STEP) * g.cell;
    }
}

// ---- the crop volume --------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
pv_inside(const uint32_t N, const float *__restrict__ points, const int w, const int u, const int v, const double lo, const double hi, const uint32_t M,
          const double *__restrict__ polygon, uint8_t *__restrict__ inside)
{
    __shared__ double s_u[ENVGS_POLYGON_MAX], s_v[ENVGS_POLYGON_MAX];
    for (uint32_t j = threadIdx.x; j < M; j += 256u) { s_u[j] = polygon[3 * (size_t)j + u]; s_v[j] = polygon[3 * (size_t)j + v]; }
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const float p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
    const double pw = (double)p[w], pu = (double)p[u], pv = (double)p[v];
    bool in = ev_finite(p[0]) && ev_finite(p[1]) && ev_finite(p[2]) && lo <= pw && pw <= hi;
    if (in) {
        uint32_t crossings = 0;
        for (uint32_t j = 0; j < M; j++) {                        // every lane reads the same word: an LDS broadcast
            const uint32_t k = j + 1u == M ? 0u : j + 1u;
            const double uj = s_u[j], vj = s_v[j], uk = s_u[k], vk = s_v[k];
            if ((vj > pv) != (vk > pv) && pu < (uk - uj) * (pv - vj) / (vk - vj) + uj) crossings++;
        }
        in = (crossings & 1u) != 0;
    }
    inside[i] = in ? 1 : 0;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }

bool rigid_of(const float *M, Rigid &out)
{
    if (!M) return false;
    for (int i = 0; i < 12; i++) {
        if (!std::isfinite(M[i])) return false;
        out.m[i] = M[i];
    }
    return true;
}

// the grid of the nearest-point search (at most 1024 cells per axis, 2^27 in all), or 0
uint32_t search_cells(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1 || nx > ENVGS_POINTS_MAX_DIM || ny > ENVGS_POINTS_MAX_DIM || nz > ENVGS_POINTS_MAX_DIM) return 0;
    const uint64_t all = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    return all > ENVGS_POINTS_MAX_CELLS ? 0 : (uint32_t)all;
}

bool grid_ok(float ox, float oy, float oz, float cell)
{
    return cell > 0.0f && std::isfinite(cell) && std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz);
}

bool voxel_dims_ok(int32_t nx, int32_t ny, int32_t nz)
{
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= ENVGS_VOXEL_MAX_DIM && ny <= ENVGS_VOXEL_MAX_DIM && nz <= ENVGS_VOXEL_MAX_DIM;
}

// flags / scan (N) | scan scratch | pos (3N u64) | cnt (N) | idx (N) | key (N i64)
struct VoxelTemp { size_t scan, scratch, scratch_bytes, pos, cnt, idx, sums_end, key, total; };
VoxelTemp voxel_temp(uint32_t N)
{
    VoxelTemp t;
    t.scan = 0;
    t.scratch = up256(4 * (size_t)N);
    t.scratch_bytes = scan_temp_bytes((int)N);
    t.pos = t.scratch + up256(t.scratch_bytes);
    t.cnt = t.pos + up256(24 * (size_t)N);
    t.idx = t.cnt + up256(4 * (size_t)N);
    t.sums_end = t.idx + up256(4 * (size_t)N);                    // everything from pos to here starts at zero
    t.key = t.sums_end;
    t.total = t.key + up256(8 * (size_t)N);
    return t;
}

VoxelSums voxel_sums(char *base, const VoxelTemp &T)
{
    return {(unsigned long long *)(base + T.pos), (uint32_t *)(base + T.cnt), (uint32_t *)(base + T.idx), (long long *)(base + T.key)};
}

}  // namespace
}  // namespace envgs

using namespace envgs;

extern "C" {

int envgs_points_transform(uint32_t N, const float *points, const float *M, float *out, void *stream)
{
    Rigid R;
    if (N >= COUNT_LIMIT || !rigid_of(M, R) || (N && (!points || !out))) return ENVGS_ERR_BAD_ARG;
    if (N) hipLaunchKernelGGL(pt_apply, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, N, points, R, out);
    return (int)hipGetLastError();
}

size_t envgs_points_register_temp_bytes(uint32_t Q)
{
    if (Q >= COUNT_LIMIT) return 0;
    return up256(sizeof(double) * RG_SUMS * (size_t)(Q ? blocks_of(Q) : 1u));
}

int envgs_points_register_sums(uint32_t Q, const float *source, const float *M, float max_distance, float ox, float oy, float oz, float cell, int32_t nx,
                               int32_t ny, int32_t nz, const uint32_t *cell_end, const float *records, const double *center, void *temp, size_t temp_bytes,
                               double *sums, float *moved, float *dist2, int32_t *index, void *stream_)
{
    Rigid R;
    const uint32_t cells = search_cells(nx, ny, nz);
    if (Q >= COUNT_LIMIT || !rigid_of(M, R) || !cells || !grid_ok(ox, oy, oz, cell) || !cell_end || !aligned16(records)) return ENVGS_ERR_BAD_ARG;
    if (!(max_distance >= 0.0f) || !std::isfinite(max_distance) || !temp || !aligned16(temp) || !sums || (Q && !source)) return ENVGS_ERR_BAD_ARG;
    if (!center || !std::isfinite(center[0]) || !std::isfinite(center[1]) || !std::isfinite(center[2])) return ENVGS_ERR_BAD_ARG;
    if (temp_bytes < envgs_points_register_temp_bytes(Q)) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    if (Q == 0) return (int)hipMemsetAsync(sums, 0, sizeof(double) * RG_SUMS, stream);
    const Grid g = {{ox, oy, oz}, cell, {nx, ny, nz}};
    const uint32_t rows = blocks_of(Q);
    hipLaunchKernelGGL(rg_sums, dim3(rows), dim3(256), 0, stream, Q, source, R, max_distance, g, cell_end, (const float4 *)records, center[0], center[1], center[2], (double *)temp,
                       moved, dist2, index);
    hipLaunchKernelGGL(rg_final, dim3(1), dim3(256), 0, stream, rows, (const double *)temp, sums);
    return (int)hipGetLastError();
}

int envgs_points_voxel_keys(uint32_t N, const float *points, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny, int32_t nz, int64_t *keys,
                            void *stream)
{
    if (N >= COUNT_LIMIT || !voxel_dims_ok(nx, ny, nz) || !grid_ok(ox, oy, oz, cell) || (N && (!points || !keys))) return ENVGS_ERR_BAD_ARG;
    const Grid g = {{ox, oy, oz}, cell, {nx, ny, nz}};
    if (N) hipLaunchKernelGGL(vd_keys, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, N, points, g, (long long *)keys);
    return (int)hipGetLastError();
}

size_t envgs_points_voxel_temp_bytes(uint32_t N)
{
    return N >= COUNT_LIMIT ? 0 : voxel_temp(N).total;
}

int envgs_points_voxel_cluster(uint32_t N, const float *points, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny, int32_t nz,
                               const int64_t *sorted_keys, const int64_t *order, void *temp, size_t temp_bytes, int32_t *cluster, uint32_t *count,
                               void *stream_)
{
    if (N >= COUNT_LIMIT || !voxel_dims_ok(nx, ny, nz) || !grid_ok(ox, oy, oz, cell) || !temp || !aligned16(temp) || !count) return ENVGS_ERR_BAD_ARG;
    if (N && (!points || !sorted_keys || !order)) return ENVGS_ERR_BAD_ARG;
    const VoxelTemp T = voxel_temp(N);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)temp;
    hipError_t e;
    if (N == 0) return (int)hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    if ((e = hipMemsetAsync(base + T.pos, 0, T.sums_end - T.pos, stream)) != hipSuccess) return (int)e;
    const Grid g = {{ox, oy, oz}, cell, {nx, ny, nz}};
    uint32_t *scan = (uint32_t *)(base + T.scan);
    const dim3 wg(256), gp(blocks_of(N));
    hipLaunchKernelGGL(vd_heads, gp, wg, 0, stream, N, (const long long *)sorted_keys, scan);
    const int rc = launch_scan(scan, scan, (int)N, base + T.scratch, T.scratch_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(vd_accumulate, gp, wg, 0, stream, N, points, g, (const long long *)sorted_keys, (const long long *)order, (const uint32_t *)scan,
                       voxel_sums(base, T), cluster, count);
    return (int)hipGetLastError();
}

int envgs_points_voxel_finish(uint32_t N, const float *points, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny, int32_t nz, void *temp,
                              size_t temp_bytes, uint32_t C, float *out, void *stream)
{
    if (N >= COUNT_LIMIT || C > N || !voxel_dims_ok(nx, ny, nz) || !grid_ok(ox, oy, oz, cell) || !temp || !aligned16(temp)) return ENVGS_ERR_BAD_ARG;
    if (C && (!points || !out)) return ENVGS_ERR_BAD_ARG;
    const VoxelTemp T = voxel_temp(N);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    const Grid g = {{ox, oy, oz}, cell, {nx, ny, nz}};
    if (C) hipLaunchKernelGGL(vd_finish, dim3(blocks_of(C)), dim3(256), 0, (hipStream_t)stream, N, C, points, g, voxel_sums((char *)temp, T), out);
    return (int)hipGetLastError();
}

int envgs_points_in_polygon(uint32_t N, const float *points, int32_t axis, double axis_min, double axis_max, uint32_t M, const double *polygon,
                            uint8_t *inside, void *stream)
{
    if (N >= COUNT_LIMIT || axis < 0 || axis > 2 || M < 3 || M > ENVGS_POLYGON_MAX || !polygon || (N && (!points || !inside))) return ENVGS_ERR_BAD_ARG;
    if (std::isnan(axis_min) || std::isnan(axis_max)) return ENVGS_ERR_BAD_ARG;
    const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;
    if (N) hipLaunchKernelGGL(pv_inside, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, N, points, (int)axis, u, v, axis_min, axis_max, M, polygon,
                              inside);
    return (int)hipGetLastError();
}

}  // extern "C"
