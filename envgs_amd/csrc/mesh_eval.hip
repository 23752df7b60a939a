// mesh_eval.hip -- mesh evaluation for gfx950 (include/envgs_mesh.h, "evaluation"): area-proportional surface samples with canonical bytes, and
// the exact nearest neighbour within a radius over a uniform grid.  Built with -ffp-contract=off (build.py): the face areas, the samples, the
// cells and the squared distances follow the header's fp32 sequence operation for operation.
//
// Sampling
//   ms_count       a lane per face: the count n_f of the face (0 for a face the header excludes), the workgroup-local exclusive scan of the counts,
//                  one total per workgroup of 256 consecutive faces; the 64-bit sum of all counts and the over-limit flag by integer atomics
//   launch_scan    over the per-workgroup totals only (the pattern of mesh_count)
//   ms_emit        a lane per OUTPUT sample: binary search for its workgroup in the scanned totals, then for its face in the 256 local offsets,
//                  so the stores are coalesced and one huge face is shared by as many lanes as it has samples
// Nearest neighbour
//   pg_count       a lane per point: its cell (rule 1 of the simplification) -> the per-point cell id; u32 histogram by atomics
//   pg_local       a lane per cell: workgroup-local exclusive scan of the histogram IN PLACE, one total per workgroup
//   launch_scan    over the per-workgroup totals
//   pg_base        a lane per cell: local offset + scanned base = first slot of the cell
//   pg_scatter     a lane per point: slot = atomic increment of its cell's word; the 16 B record (x, y, z, index bits) goes there.  Afterwards
//                  the word of a cell holds the END of the cell, and the end of cell c - 1 is the start of cell c: one array serves both.
//                  The slot order inside a cell depends on scheduling; the search result is a lexicographic minimum and does not.
//   pg_nearest     a lane per query: Chebyshev shells around the query's cell.  A run of x-adjacent cells is one contiguous run of records, so a
//                  shell is walked row by row: full rows on its four faces in j / k, the two end cells of the rows in between.
#include "common.h"
#include "mesh_rng.h"

#include "../../include/envgs_mesh.h"

namespace envgs {
namespace {

constexpr uint32_t COUNT_LIMIT = 1u << 31;
constexpr float FACE_LIMIT = 16777216.0f;                         // 2^24 samples of one face
constexpr uint32_t NO_CELL = 0xffffffffu;

struct Grid { float o[3]; float cell; int32_t n[3]; };

__device__ __forceinline__ bool ev_finite(const float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// ---- sampling ---------------------------------------------------------------------------------------------------------------------------------------
// the three corners of a face whose indices are in range; false otherwise (no index out of range is dereferenced)
__device__ __forceinline__ bool ms_indices(const int32_t *__restrict__ faces, const uint32_t f, const uint32_t V, uint32_t (&idx)[3])
{
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 3; e++) { idx[e] = (uint32_t)faces[3 * (size_t)f + e]; ok = ok && idx[e] < V; }      // a negative index becomes >= 2^31 > V
    return ok;
}

__device__ __forceinline__ void ms_load3(const float *__restrict__ p, const uint32_t v, float (&a)[3])
{
#pragma unroll
    for (int e = 0; e < 3; e++) a[e] = p[3 * (size_t)v + e];
}

// totals: [0] the 64-bit sum of the counts, [1] != 0 iff some face reached 2^24 samples
__global__ void __launch_bounds__(256)
ms_count(const uint32_t V, const uint32_t F, const float *__restrict__ vertices, const int32_t *__restrict__ faces, const float density, const uint32_t seed,
         uint32_t *__restrict__ local, uint32_t *__restrict__ tot, unsigned long long *__restrict__ totals)
{
    __shared__ uint32_t s_w[4];
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint32_t n = 0;
    bool over = false;
    uint32_t idx[3];
    if (f < F && ms_indices(faces, f, V, idx)) {
        float a[3], b[3], c[3];
        ms_load3(vertices, idx[0], a); ms_load3(vertices, idx[1], b); ms_load3(vertices, idx[2], c);
        bool fin = true;
#pragma unroll
        for (int e = 0; e < 3; e++) fin = fin && ev_finite(a[e]) && ev_finite(b[e]) && ev_finite(c[e]);
        const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const float area = 0.5f * sqrtf((nx * nx + ny * ny) + nz * nz);
        if (fin && ev_finite(area) && area != 0.0f) {
            const float t = area * density + rng_uniform(rng_hash(seed, f, RNG_COUNT_STREAM));
            if (t < FACE_LIMIT) n = (uint32_t)floorf(t);
            else over = true;
        }
    }
    uint32_t total;
    const uint32_t ex = block_exclusive_u32<4>(n, s_w, total);     // 256 counts below 2^24: the sum fits
    if (f < F) local[f] = ex;
    if (threadIdx.x == 0) {
        tot[blockIdx.x] = total;
        if (total) atomicAdd(totals, (unsigned long long)total);
    }
    if (__ballot(over) && lane_id() == 0) atomicOr(totals + 1, 1ull);
}

// tot holds the INCLUSIVE scan over the workgroups of ms_count
__global__ void __launch_bounds__(256)
ms_emit(const uint32_t F, const uint32_t nb, const uint32_t S, const float *__restrict__ vertices, const float *__restrict__ colors,
        const int32_t *__restrict__ faces, const uint32_t seed, const uint32_t *__restrict__ local, const uint32_t *__restrict__ tot,
        float *__restrict__ points, float *__restrict__ out_colors, int32_t *__restrict__ out_face)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= S || s >= tot[nb - 1]) return;                        // a sample beyond the counted total has no face: never searched for
    uint32_t lo = 0, hi = nb - 1;                                  // the first workgroup whose inclusive total exceeds s
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tot[mid] > s) hi = mid; else lo = mid + 1;
    }
    const uint32_t r = s - (lo ? tot[lo - 1] : 0u);
    const uint32_t f0 = lo * 256u;
    uint32_t a = 0, b = min(256u, F - f0) - 1u;                    // the last face of the workgroup whose local offset is <= r: faces of count 0
    while (a < b) {                                                // share the offset of their successor and lose to it
        const uint32_t mid = (a + b + 1u) >> 1;
        if (local[f0 + mid] <= r) a = mid; else b = mid - 1u;
    }
    const uint32_t f = f0 + a, k = r - local[f];
    const uint32_t ku = rng_bits24(rng_hash(seed, f, 2u * k)), kv = rng_bits24(rng_hash(seed, f, 2u * k + 1u));
    float u = (float)ku * 5.9604644775390625e-08f, v = (float)kv * 5.9604644775390625e-08f;
    if (ku + kv > (1u << 24)) { u = 1.0f - u; v = 1.0f - v; }      // u + v > 1, decided on the integers; 1 - u is exact
    const uint32_t ia = (uint32_t)faces[3 * (size_t)f], ib = (uint32_t)faces[3 * (size_t)f + 1], ic = (uint32_t)faces[3 * (size_t)f + 2];
    float pa[3], pb[3], pc[3];
    ms_load3(vertices, ia, pa); ms_load3(vertices, ib, pb); ms_load3(vertices, ic, pc);
#pragma unroll
    for (int e = 0; e < 3; e++) points[3 * (size_t)s + e] = (pa[e] + u * (pb[e] - pa[e])) + v * (pc[e] - pa[e]);
    if (out_colors) {
        ms_load3(colors, ia, pa); ms_load3(colors, ib, pb); ms_load3(colors, ic, pc);
#pragma unroll
        for (int e = 0; e < 3; e++) out_colors[3 * (size_t)s + e] = (pa[e] + u * (pb[e] - pa[e])) + v * (pc[e] - pa[e]);
    }
    if (out_face) out_face[s] = (int32_t)f;
}

// ---- the point grid -----------------------------------------------------------------------------------------------------------------------------------
// rule 1 of the simplification on one axis; the caller has checked that x is finite
__device__ __forceinline__ int32_t pg_axis(const float x, const float o, const float cell, const int32_t n)
{
    const float fl = floorf((x - o) / cell);
    return !(fl >= 1.0f) ? 0 : (fl >= 2147483648.0f ? n - 1 : min((int32_t)fl, n - 1));
}

__global__ void __launch_bounds__(256)
pg_count(const uint32_t N, const float *__restrict__ points, const Grid g, uint32_t *__restrict__ cell_of, uint32_t *__restrict__ hist)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
    uint32_t c = NO_CELL;
    if (ev_finite(x) && ev_finite(y) && ev_finite(z)) {
        c = (uint32_t)pg_axis(x, g.o[0], g.cell, g.n[0])
            + (uint32_t)g.n[0] * ((uint32_t)pg_axis(y, g.o[1], g.cell, g.n[1]) + (uint32_t)g.n[1] * (uint32_t)pg_axis(z, g.o[2], g.cell, g.n[2]));
        atomicAdd(hist + c, 1u);
    }
    cell_of[i] = c;
}

__global__ void __launch_bounds__(256)
pg_local(const uint32_t cells, uint32_t *hist, uint32_t *__restrict__ tot)
{
    __shared__ uint32_t s_w[4];
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    const uint32_t m = c < cells ? hist[c] : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_u32<4>(m, s_w, total);
    if (c < cells) hist[c] = ex;
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// tot holds the INCLUSIVE scan over the workgroups of pg_local
__global__ void __launch_bounds__(256)
pg_base(const uint32_t cells, uint32_t *__restrict__ start, const uint32_t *__restrict__ tot)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < cells && blockIdx.x) start[c] += tot[blockIdx.x - 1];
}

__global__ void __launch_bounds__(256)
pg_scatter(const uint32_t N, const float *__restrict__ points, const uint32_t *__restrict__ cell_of, uint32_t *__restrict__ cursor, float4 *__restrict__ records)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const uint32_t c = cell_of[i];
    if (c == NO_CELL) return;
    const uint32_t slot = atomicAdd(cursor + c, 1u);               // < the number of finite points <= N
    records[slot] = make_float4(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], __uint_as_float(i));
}

struct Best { float d2; uint32_t index; };

// the records of the cells c0 .. c1 of one row
__device__ __forceinline__ void pg_scan_cells(const uint32_t c0, const uint32_t c1, const uint32_t *__restrict__ cell_end, const float4 *__restrict__ records,
                                              const float qx, const float qy, const float qz, const float r2, Best &best)
{
    const uint32_t first = c0 ? cell_end[c0 - 1] : 0u, last = cell_end[c1];
    for (uint32_t s = first; s < last; s++) {
        const float4 p = records[s];
        const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
        const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
        const uint32_t i = __float_as_uint(p.w);
        if (d2 <= r2 && (d2 < best.d2 || (d2 == best.d2 && i < best.index))) { best.d2 = d2; best.index = i; }
    }
}

__global__ void __launch_bounds__(256)
pg_nearest(const uint32_t Q, const float *__restrict__ queries, const float max_distance, const Grid g, const uint32_t *__restrict__ cell_end,
           const float4 *__restrict__ records, float *__restrict__ dist2, int32_t *__restrict__ index)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= Q) return;
    const float qx = queries[3 * (size_t)q], qy = queries[3 * (size_t)q + 1], qz = queries[3 * (size_t)q + 2];
    Best best = {__uint_as_float(0x7f800000u), 0xffffffffu};
    if (ev_finite(qx) && ev_finite(qy) && ev_finite(qz)) {
        const int32_t nx = g.n[0], ny = g.n[1], nz = g.n[2];
        const int32_t ci = pg_axis(qx, g.o[0], g.cell, nx), cj = pg_axis(qy, g.o[1], g.cell, ny), ck = pg_axis(qz, g.o[2], g.cell, nz);
        const float r2 = max_distance * max_distance;
        // the last shell that holds a cell of the grid: an integer, so the loop ends whatever the floats are
        const int32_t rmax = max(max(max(ci, nx - 1 - ci), max(cj, ny - 1 - cj)), max(ck, nz - 1 - ck));
        for (int32_t r = 0; r <= rmax; r++) {
            const int32_t k0 = max(ck - r, 0), k1 = min(ck + r, nz - 1), j0 = max(cj - r, 0), j1 = min(cj + r, ny - 1);
            const int32_t i0 = max(ci - r, 0), i1 = min(ci + r, nx - 1);
            for (int32_t k = k0; k <= k1; k++) {
                const bool kface = k == ck - r || k == ck + r;
                for (int32_t j = j0; j <= j1; j++) {
                    const uint32_t row = (uint32_t)nx * ((uint32_t)j + (uint32_t)ny * (uint32_t)k);
                    if (kface || j == cj - r || j == cj + r) {
                        pg_scan_cells(row + (uint32_t)i0, row + (uint32_t)i1, cell_end, records, qx, qy, qz, r2, best);
                    } else {                                        // r >= 1 here: the two ends of the row, where they are inside the grid
                        if (ci - r >= 0) pg_scan_cells(row + (uint32_t)(ci - r), row + (uint32_t)(ci - r), cell_end, records, qx, qy, qz, r2, best);
                        if (ci + r < nx) pg_scan_cells(row + (uint32_t)(ci + r), row + (uint32_t)(ci + r), cell_end, records, qx, qy, qz, r2, best);
                    }
                }
            }
            const float b = ((float)r * g.cell) * 0.9990234375f;    // 1 - 2^-10: every point outside shell r is farther than b (header: the proof)
            if (best.d2 <= b * b || b > max_distance) break;
        }
    }
    dist2[q] = best.d2;
    index[q] = (int32_t)best.index;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }

// local (F) | tot (nb) | scan scratch
struct SampleTemp { size_t local, tot, scan, scan_bytes, total; uint32_t nb; };
SampleTemp sample_temp(uint32_t F)
{
    SampleTemp t;
    t.nb = blocks_of(F);
    t.local = 0;
    t.tot = up256(4 * (size_t)F);
    t.scan = t.tot + up256(4 * (size_t)t.nb);
    t.scan_bytes = scan_temp_bytes((int)t.nb);
    t.total = t.scan + up256(t.scan_bytes);
    return t;
}

// nx ny nz, or 0 if the grid is out of range
uint32_t grid_cells(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1 || nx > ENVGS_POINTS_MAX_DIM || ny > ENVGS_POINTS_MAX_DIM || nz > ENVGS_POINTS_MAX_DIM) return 0;
    const uint64_t all = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    return all > ENVGS_POINTS_MAX_CELLS ? 0 : (uint32_t)all;
}

bool grid_ok(float ox, float oy, float oz, float cell)
{
    return cell > 0.0f && std::isfinite(cell) && std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz);
}

// cell_of (N) | tot (nbc) | scan scratch
struct GridTemp { size_t cell_of, tot, scan, scan_bytes, total; uint32_t nbc; };
GridTemp grid_temp(uint32_t N, uint32_t cells)
{
    GridTemp t;
    t.nbc = blocks_of(cells);
    t.cell_of = 0;
    t.tot = up256(4 * (size_t)N);
    t.scan = t.tot + up256(4 * (size_t)t.nbc);
    t.scan_bytes = scan_temp_bytes((int)t.nbc);
    t.total = t.scan + up256(t.scan_bytes);
    return t;
}

}  // namespace
}  // namespace envgs

using namespace envgs;

extern "C" {

size_t envgs_mesh_sample_temp_bytes(uint32_t V, uint32_t F)
{
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT) return 0;
    return sample_temp(F).total;
}

int envgs_mesh_sample_count(uint32_t V, uint32_t F, const float *vertices, const int32_t *faces, float density, uint32_t seed, void *temp, size_t temp_bytes,
                            uint64_t *totals, void *stream_)
{
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT || !temp || !aligned16(temp) || !totals) return ENVGS_ERR_BAD_ARG;
    if (!(density > 0.0f) || !std::isfinite(density) || (V && !vertices) || (F && !faces)) return ENVGS_ERR_BAD_ARG;
    const SampleTemp T = sample_temp(F);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)temp;
    hipError_t e;
    if ((e = hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), stream)) != hipSuccess) return (int)e;
    if (F == 0) return 0;
    uint32_t *tot = (uint32_t *)(base + T.tot);
    hipLaunchKernelGGL(ms_count, dim3(T.nb), dim3(256), 0, stream, V, F, vertices, faces, density, seed, (uint32_t *)(base + T.local), tot,
                       (unsigned long long *)totals);
    const int rc = launch_scan(tot, tot, (int)T.nb, base + T.scan, T.scan_bytes, stream);
    if (rc) return rc;
    return (int)hipGetLastError();
}

int envgs_mesh_sample_emit(uint32_t V, uint32_t F, const float *vertices, const float *colors, const int32_t *faces, uint32_t seed, const void *temp,
                           size_t temp_bytes, uint32_t S, float *points, float *out_colors, int32_t *out_face, void *stream)
{
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT || S >= COUNT_LIMIT || !temp || !aligned16(temp)) return ENVGS_ERR_BAD_ARG;
    if ((S && (!points || !vertices || !faces || !F)) || (out_colors && !colors)) return ENVGS_ERR_BAD_ARG;
    const SampleTemp T = sample_temp(F);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    if (S == 0) return 0;
    const char *base = (const char *)temp;
    hipLaunchKernelGGL(ms_emit, dim3(blocks_of(S)), dim3(256), 0, (hipStream_t)stream, F, T.nb, S, vertices, out_colors ? colors : nullptr, faces, seed,
                       (const uint32_t *)(base + T.local), (const uint32_t *)(base + T.tot), points, out_colors, out_face);
    return (int)hipGetLastError();
}

size_t envgs_points_grid_temp_bytes(uint32_t N, int32_t nx, int32_t ny, int32_t nz)
{
    const uint32_t cells = grid_cells(nx, ny, nz);
    if (N >= COUNT_LIMIT || !cells) return 0;
    return grid_temp(N, cells).total;
}

int envgs_points_grid_build(uint32_t N, const float *points, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny, int32_t nz, void *temp,
                            size_t temp_bytes, uint32_t *cell_end, float *records, void *stream_)
{
    const uint32_t cells = grid_cells(nx, ny, nz);
    if (N >= COUNT_LIMIT || !cells || !grid_ok(ox, oy, oz, cell) || !temp || !aligned16(temp) || !cell_end) return ENVGS_ERR_BAD_ARG;
    if (N && (!points || !records || !aligned16(records))) return ENVGS_ERR_BAD_ARG;
    const GridTemp T = grid_temp(N, cells);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)temp;
    hipError_t e;
    if ((e = hipMemsetAsync(cell_end, 0, 4 * (size_t)cells, stream)) != hipSuccess) return (int)e;
    if (N == 0) return 0;
    const Grid g = {{ox, oy, oz}, cell, {nx, ny, nz}};
    uint32_t *cell_of = (uint32_t *)(base + T.cell_of), *tot = (uint32_t *)(base + T.tot);
    const dim3 wg(256), gp(blocks_of(N)), gc(T.nbc);
    hipLaunchKernelGGL(pg_count, gp, wg, 0, stream, N, points, g, cell_of, cell_end);
    hipLaunchKernelGGL(pg_local, gc, wg, 0, stream, cells, cell_end, tot);
    const int rc = launch_scan(tot, tot, (int)T.nbc, base + T.scan, T.scan_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(pg_base, gc, wg, 0, stream, cells, cell_end, (const uint32_t *)tot);
    hipLaunchKernelGGL(pg_scatter, gp, wg, 0, stream, N, points, (const uint32_t *)cell_of, cell_end, (float4 *)records);
    return (int)hipGetLastError();
}

int envgs_points_nearest(uint32_t Q, const float *queries, float max_distance, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny, int32_t nz,
                         const uint32_t *cell_end, const float *records, float *dist2, int32_t *index, void *stream)
{
    const uint32_t cells = grid_cells(nx, ny, nz);
    if (Q >= COUNT_LIMIT || !cells || !grid_ok(ox, oy, oz, cell) || !cell_end || !aligned16(records)) return ENVGS_ERR_BAD_ARG;
    if (!(max_distance >= 0.0f) || !std::isfinite(max_distance) || (Q && (!queries || !dist2 || !index))) return ENVGS_ERR_BAD_ARG;
    if (Q == 0) return 0;
    const Grid g = {{ox, oy, oz}, cell, {nx, ny, nz}};
    hipLaunchKernelGGL(pg_nearest, dim3(blocks_of(Q)), dim3(256), 0, (hipStream_t)stream, Q, queries, max_distance, g, cell_end, (const float4 *)records, dist2,
                       index);
    return (int)hipGetLastError();
}

}  // extern "C"
