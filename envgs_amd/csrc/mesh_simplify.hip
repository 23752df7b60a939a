// mesh_simplify.hip -- mesh simplification for gfx950 (include/envgs_mesh.h, "simplification of an indexed triangle mesh"): vertex clustering on
// a uniform grid.  Every sum is an integer sum and every slot is handed out by a scan, so the outputs do not depend on the schedule or on the
// numbering of the input vertices, and two runs give identical bytes.  Built with -ffp-contract=off (build.py): the cell and the fixed-point
// offset of a vertex follow the header's fp32 sequence operation for operation.
//
//   sc_assign      a lane per vertex: its cell (sc_locate), a plain store of 1 into the byte-per-cell table
//   sc_rank        a lane per cell: block scan of the marks; the block-local rank (<= 255) REPLACES the mark in the same byte -- only occupied
//                  cells are ever looked up again -- and one total per workgroup of 256 consecutive cells
//   launch_scan    over the per-workgroup totals (the pattern of mesh_count and sel_vscan): ascending cell = cluster number; C stays on the device
//   sc_accumulate  a lane per vertex: cluster = scanned base + rank byte -> vertex_cluster; the fixed-point offsets, the fixed-point colours, the
//                  member count and the vertex index are summed per cluster with integer atomics.  A mesh in cell order puts runs of consecutive
//                  vertices into one cell, a degenerate one all of them, and same-address atomics serialise (Guideline 12), so each wavefront
//                  first merges its runs of equal clusters with a segmented scan over the lanes (32-bit partial sums: 64 q < 2^32) and only
//                  the last lane of a run issues the adds (64-bit for the offsets, whose sums reach 2^51 / 2^55).
//   sc_finish      a lane per cluster: n = 1 copies the member (its index is the index sum), n > 1 takes the rounded integer means
//   sc_face_map    a lane per face: corners -> clusters (-1: out of range, never dereferenced, or no cell); keep = 1 iff all valid and distinct
//   sc_face_enter  a lane per kept face: fh_insert of mesh_facehash.h; the slot of its key goes to scratch
//   sc_face_keep   a lane per kept face: keep = (its slot ended up holding its own index), i.e. the lowest index of the triple up to rotation
// The compaction is envgs_mesh_select_count / _emit of mesh_clean.hip, called by the host on the clustered mesh.
#include "common.h"
#include "mesh_facehash.h"
#include "mesh_points.h"

#include "../../include/envgs_mesh.h"

namespace envgs {
namespace {

struct DeviceAtomics {
    typedef uint32_t cell;
    static __host__ __device__ __forceinline__ uint32_t load(const cell *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __host__ __device__ __forceinline__ uint32_t cas(cell *p, uint32_t expect, uint32_t desired)
    {
        __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;                                            // unchanged on success, the observed word on failure
    }
    static __host__ __device__ __forceinline__ void min(cell *p, uint32_t v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// Grid, POS_ONE / POS_STEP and sc_locate (rule 1 and the offset of rule 3): mesh_points.h, shared with the sparse voxel mean of mesh_register.hip
constexpr float COL_ONE = 65536.0f, COL_STEP = 1.0f / 65536.0f;          // 2^16
constexpr uint32_t NO_CLUSTER = 0xffffffffu;

__device__ __forceinline__ uint32_t sc_colour(float c)
{
    c = !(c > 0.0f) ? 0.0f : (c > 255.0f ? 255.0f : c);
    return (uint32_t)floorf(c * COL_ONE + 0.5f);
}

__device__ __forceinline__ bool sc_finite(const float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// the vertex's cell, or false
__device__ __forceinline__ bool sc_cell_of(const float *__restrict__ vertices, const uint32_t v, const Grid &g, uint32_t &cell, uint32_t (&q)[3])
{
    const float x = vertices[3 * (size_t)v], y = vertices[3 * (size_t)v + 1], z = vertices[3 * (size_t)v + 2];
    if (!(sc_finite(x) && sc_finite(y) && sc_finite(z))) return false;
    int32_t i, j, k;
    sc_locate(x, g.o[0], g.cell, g.n[0], i, q[0]);
    sc_locate(y, g.o[1], g.cell, g.n[1], j, q[1]);
    sc_locate(z, g.o[2], g.cell, g.n[2], k, q[2]);
    cell = (uint32_t)i + (uint32_t)g.n[0] * ((uint32_t)j + (uint32_t)g.n[1] * (uint32_t)k);
    return true;
}

__global__ void __launch_bounds__(256)
sc_assign(const uint32_t V, const float *__restrict__ vertices, const Grid g, uint8_t *__restrict__ mark)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    uint32_t cell, q[3];
    if (v < V && sc_cell_of(vertices, v, g, cell, q)) mark[cell] = 1;
}

__global__ void __launch_bounds__(256)
sc_rank(const uint32_t cells, uint8_t *mark, uint32_t *__restrict__ tot)
{
    __shared__ uint32_t s_w[4];
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    const uint32_t m = (c < cells && mark[c]) ? 1u : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_u32<4>(m, s_w, total);      // <= 255
    if (m) mark[c] = (uint8_t)ex;
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// per-cluster sums: pos (R,3) u64 | col (R,3) u64 | cnt (R) | idx (R) | cell (R)
struct Sums { unsigned long long *pos, *col; uint32_t *cnt, *idx, *cell; };

// tot holds the INCLUSIVE scan over the workgroups of sc_rank from here on
__global__ void __launch_bounds__(256)
sc_accumulate(const uint32_t V, const uint32_t cells, const float *__restrict__ vertices, const float *__restrict__ colors, const Grid g,
              const uint8_t *__restrict__ rank, const uint32_t *__restrict__ tot, const Sums S, int32_t *__restrict__ vertex_cluster,
              uint32_t *__restrict__ count)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v == 0) *count = tot[(cells + 255u) / 256u - 1u];
    const int lane = lane_id();
    uint32_t key = NO_CLUSTER, cell = 0;
    uint32_t a[8] = {0, 0, 0, 0, 0, 0, 0, 0};                     // q of x y z, q of r g b, members, vertex index
    if (v < V) {
        uint32_t q[3];
        if (sc_cell_of(vertices, v, g, cell, q)) {
            const uint32_t b = cell >> 8;
            key = (b ? tot[b - 1] : 0u) + rank[cell];
            a[0] = q[0]; a[1] = q[1]; a[2] = q[2]; a[6] = 1; a[7] = v;
            if (colors) {
#pragma unroll
                for (int c = 0; c < 3; c++) a[3 + c] = sc_colour(colors[3 * (size_t)v + c]);
            }
        }
        vertex_cluster[v] = (int32_t)key;                         // NO_CLUSTER is -1
    }
    // runs of equal clusters over consecutive lanes: `start` = first lane of the own run, the last lane of a run adds its sum
    const uint32_t prev = (uint32_t)__shfl_up((int)key, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != key);
    const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const bool take = lane - d >= start;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t o = (uint32_t)__shfl_up((int)a[k], d);
            a[k] += take ? o : 0u;
        }
    }
    if (!last || key == NO_CLUSTER) return;
#pragma unroll
    for (int c = 0; c < 3; c++) atomicAdd(S.pos + 3 * (size_t)key + c, (unsigned long long)a[c]);
    if (colors) {
#pragma unroll
        for (int c = 0; c < 3; c++) atomicAdd(S.col + 3 * (size_t)key + c, (unsigned long long)a[3 + c]);
    }
    atomicAdd(S.cnt + key, a[6]);
    atomicAdd(S.idx + key, a[7]);                                 // wraps when n > 1; read only when n == 1
    S.cell[key] = cell;                                           // every member stores the same word
}

__global__ void __launch_bounds__(256)
sc_finish(const uint32_t R, const uint32_t *__restrict__ count, const float *__restrict__ vertices, const float *__restrict__ colors, const Grid g,
          const Sums S, float *__restrict__ cl_vertices, float *__restrict__ cl_colors)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= R || c >= *count) return;
    const uint32_t n = S.cnt[c];
    if (n == 1) {
        const uint32_t v = S.idx[c];
#pragma unroll
        for (int e = 0; e < 3; e++) ((uint32_t *)cl_vertices)[3 * (size_t)c + e] = ((const uint32_t *)vertices)[3 * (size_t)v + e];
        if (cl_colors) {
#pragma unroll
            for (int e = 0; e < 3; e++) ((uint32_t *)cl_colors)[3 * (size_t)c + e] = ((const uint32_t *)colors)[3 * (size_t)v + e];
        }
        return;
    }
    const uint32_t cell = S.cell[c];
    const uint32_t nx = (uint32_t)g.n[0], ny = (uint32_t)g.n[1];
    const uint32_t ijk[3] = {cell % nx, (cell / nx) % ny, cell / nx / ny};
    const unsigned long long two_n = 2ull * n;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const uint32_t qm = (uint32_t)((2ull * S.pos[3 * (size_t)c + e] + n) / two_n);
        cl_vertices[3 * (size_t)c + e] = g.o[e] + ((float)ijk[e] + (float)qm * POS_STEP) * g.cell;
    }
    if (cl_colors) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const uint32_t qm = (uint32_t)((2ull * S.col[3 * (size_t)c + e] + n) / two_n);
            cl_colors[3 * (size_t)c + e] = (float)qm * COL_STEP;
        }
    }
}

__global__ void __launch_bounds__(256)
sc_face_map(const uint32_t V, const uint32_t F, const int32_t *__restrict__ faces, const int32_t *__restrict__ vertex_cluster,
            int32_t *__restrict__ cl_faces, uint8_t *__restrict__ keep)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F) return;
    uint32_t idx[3];
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 3; e++) { idx[e] = (uint32_t)faces[3 * (size_t)f + e]; ok = ok && idx[e] < V; }     // a negative index becomes >= 2^31 > V
    int32_t m[3];
#pragma unroll
    for (int e = 0; e < 3; e++) {
        m[e] = idx[e] < V ? vertex_cluster[idx[e]] : -1;
        ok = ok && m[e] >= 0;
        cl_faces[3 * (size_t)f + e] = m[e];
    }
    keep[f] = (ok && m[0] != m[1] && m[1] != m[2] && m[2] != m[0]) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
sc_face_enter(const uint32_t F, const int32_t *__restrict__ cl_faces, const uint8_t *__restrict__ keep, uint32_t *table, const unsigned long long slots,
              uint32_t *__restrict__ slot)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < F && keep[f]) slot[f] = fh_insert<DeviceAtomics>(table, slots, cl_faces, f);
}

__global__ void __launch_bounds__(256)
sc_face_keep(const uint32_t F, const uint32_t *__restrict__ table, const uint32_t *__restrict__ slot, uint8_t *__restrict__ keep)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < F && keep[f] && table[slot[f]] != f) keep[f] = 0;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }
constexpr uint32_t COUNT_LIMIT = 1u << 31;

// nx ny nz, or 0 if the grid is out of range
uint32_t grid_cells(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    const uint64_t xy = (uint64_t)nx * (uint64_t)ny;
    if (xy >= COUNT_LIMIT) return 0;
    const uint64_t all = xy * (uint64_t)nz;
    return all >= COUNT_LIMIT ? 0 : (uint32_t)all;
}

// mark (cells) | tot (nbc) | scan scratch | pos (3R u64) | col (3R u64) | cnt (R) | idx (R) | cell (R) | slot (F) | table (slots)
struct SimpTemp { size_t mark, tot, scan, scan_bytes, pos, col, cnt, idx, cell, sums_end, slot, table, total; uint32_t nbc, R; uint64_t slots; };
SimpTemp simp_temp(uint32_t V, uint32_t F, uint32_t cells)
{
    SimpTemp t;
    t.nbc = blocks_of(cells);
    t.R = V < cells ? V : cells;
    t.slots = fh_slots(F);
    t.mark = 0;
    t.tot = up256((size_t)cells);
    t.scan = t.tot + up256(4 * (size_t)t.nbc);
    t.scan_bytes = scan_temp_bytes((int)t.nbc);
    t.pos = t.scan + up256(t.scan_bytes);
    t.col = t.pos + up256(24 * (size_t)t.R);
    t.cnt = t.col + up256(24 * (size_t)t.R);
    t.idx = t.cnt + up256(4 * (size_t)t.R);
    t.sums_end = t.idx + up256(4 * (size_t)t.R);                  // everything from pos to here starts at zero
    t.cell = t.sums_end;
    t.slot = t.cell + up256(4 * (size_t)t.R);
    t.table = t.slot + up256(4 * (size_t)F);
    t.total = t.table + up256(4 * (size_t)t.slots);
    return t;
}

}  // namespace
}  // namespace envgs

using namespace envgs;

extern "C" {

size_t envgs_mesh_simplify_temp_bytes(uint32_t V, uint32_t F, int32_t nx, int32_t ny, int32_t nz)
{
    const uint32_t cells = grid_cells(nx, ny, nz);
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT || !cells) return 0;
    return simp_temp(V, F, cells).total;
}

int envgs_mesh_simplify_cluster(uint32_t V, uint32_t F, const float *vertices, const float *colors, const int32_t *faces, float ox, float oy, float oz,
                                float cell, int32_t nx, int32_t ny, int32_t nz, void *temp, size_t temp_bytes, float *cl_vertices, float *cl_colors,
                                int32_t *cl_faces, uint8_t *keep, int32_t *vertex_cluster, uint32_t *count, void *stream_)
{
    const uint32_t cells = grid_cells(nx, ny, nz);
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT || !cells || !temp || !aligned16(temp) || !count) return ENVGS_ERR_BAD_ARG;
    if (!(cell > 0.0f) || !std::isfinite(cell) || !std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz)) return ENVGS_ERR_BAD_ARG;
    if ((V && (!vertices || !vertex_cluster || !cl_vertices)) || (F && (!faces || !cl_faces || !keep)) || (cl_colors && !colors)) return ENVGS_ERR_BAD_ARG;
    const SimpTemp T = simp_temp(V, F, cells);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)temp;
    const dim3 wg(256), gv(blocks_of(V)), gf(blocks_of(F));
    hipError_t e;
    if (V == 0) {
        if ((e = hipMemsetAsync(count, 0, sizeof(uint32_t), stream)) != hipSuccess) return (int)e;
    } else {
        const Grid g = {{ox, oy, oz}, cell, {nx, ny, nz}};
        uint8_t *mark = (uint8_t *)(base + T.mark);
        uint32_t *tot = (uint32_t *)(base + T.tot);
        const Sums S = {(unsigned long long *)(base + T.pos), (unsigned long long *)(base + T.col), (uint32_t *)(base + T.cnt), (uint32_t *)(base + T.idx),
                        (uint32_t *)(base + T.cell)};
        if ((e = hipMemsetAsync(mark, 0, (size_t)cells, stream)) != hipSuccess) return (int)e;
        if ((e = hipMemsetAsync(base + T.pos, 0, T.sums_end - T.pos, stream)) != hipSuccess) return (int)e;
        hipLaunchKernelGGL(sc_assign, gv, wg, 0, stream, V, vertices, g, mark);
        hipLaunchKernelGGL(sc_rank, dim3(T.nbc), wg, 0, stream, cells, mark, tot);
        const int rc = launch_scan(tot, tot, (int)T.nbc, base + T.scan, T.scan_bytes, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(sc_accumulate, gv, wg, 0, stream, V, cells, vertices, cl_colors ? colors : nullptr, g, (const uint8_t *)mark, (const uint32_t *)tot, S,
                           vertex_cluster, count);
        hipLaunchKernelGGL(sc_finish, dim3(blocks_of(T.R)), wg, 0, stream, T.R, (const uint32_t *)count, vertices, colors, g, S, cl_vertices, cl_colors);
    }
    if (F) {
        uint32_t *table = (uint32_t *)(base + T.table), *slot = (uint32_t *)(base + T.slot);
        hipLaunchKernelGGL(sc_face_map, gf, wg, 0, stream, V, F, faces, (const int32_t *)vertex_cluster, cl_faces, keep);
        if (V) {
            if ((e = hipMemsetAsync(table, 0xff, 4 * (size_t)T.slots, stream)) != hipSuccess) return (int)e;
            hipLaunchKernelGGL(sc_face_enter, gf, wg, 0, stream, F, (const int32_t *)cl_faces, (const uint8_t *)keep, table, (unsigned long long)T.slots, slot);
            hipLaunchKernelGGL(sc_face_keep, gf, wg, 0, stream, F, (const uint32_t *)table, (const uint32_t *)slot, keep);
        }
    }
    return (int)hipGetLastError();
}

}  // extern "C"
