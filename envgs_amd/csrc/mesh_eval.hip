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
//   pg_nearest     a lane per query: pg_walk of mesh_points.h, the Chebyshev shells around the query's cell (the registration calls the same walk)
// Thinning (header: "thinning"; over the same grid)
//   th_begin       a lane per point: its state (UNDECIDED, or DROPPED if not finite) and the first worklist of the undecided
//   th_round       a lane per undecided point: the cell rows of shells 0 .. R around it; a kept neighbour of lower key drops it, an undecided one
//                  blocks it, else it is kept; the blocked go to the other worklist, one atomic per wavefront.  No lane waits for another.
//   th_keep        a lane per point: the state as a byte
// Culling (header: "culling")
//   cull_vertices  a lane per vertex: up to 8 views by the pixel rule of tsdf_integrate;  cull_faces  a lane per face: all three corners kept
#include "common.h"
#include "mesh_points.h"
#include "mesh_rng.h"

#include "../../include/envgs_mesh.h"

namespace envgs {
namespace {

constexpr uint32_t COUNT_LIMIT = 1u << 31;
constexpr float FACE_LIMIT = 16777216.0f;                         // 2^24 samples of one face
constexpr uint32_t NO_CELL = 0xffffffffu;

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
// the cell of a point (pg_axis), the shell walk (pg_walk) and their types: mesh_points.h, shared with mesh_register.hip
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

__global__ void __launch_bounds__(256)
pg_nearest(const uint32_t Q, const float *__restrict__ queries, const float max_distance, const Grid g, const uint32_t *__restrict__ cell_end,
           const float4 *__restrict__ records, float *__restrict__ dist2, int32_t *__restrict__ index)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= Q) return;
    const float qx = queries[3 * (size_t)q], qy = queries[3 * (size_t)q + 1], qz = queries[3 * (size_t)q + 2];
    const Best best = pg_walk(qx, qy, qz, max_distance, g, cell_end, records);
    dist2[q] = best.d2;
    index[q] = (int32_t)best.index;
}

// ---- thinning (header: "thinning") ----------------------------------------------------------------------------------------------------------------
constexpr uint32_t TH_UNDECIDED = 0u, TH_KEPT = 1u, TH_DROPPED = 2u;
// the counters at the end of the scratch: three worklist lengths used in rotation (round t reads TH_LEN + t % 3, appends to TH_LEN + (t + 1) % 3 and
// clears TH_LEN + (t + 2) % 3 for round t + 1 to append to), and the number of rounds that found work
constexpr uint32_t TH_LEN = 0u, TH_ROUNDS = 3u, TH_COUNTERS = 4u;

// One atomic per wavefront: the lanes that want a slot are counted by a ballot, the first of them reserves the run, every one takes its rank in it.
// Every lane of the wavefront must arrive here.  A slot at or beyond cap is never written (there are at most cap appenders by construction).
__device__ __forceinline__ void th_append(const bool want, const uint32_t value, uint32_t *__restrict__ list, uint32_t *__restrict__ len, const uint32_t cap)
{
    const unsigned long long m = __ballot(want);
    if (!m) return;                                               // the same in every lane of the wavefront
    const int lane = lane_id(), leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(len, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    if (want) {
        const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (slot < cap) list[slot] = value;
    }
}

// a lane per point: the state, and the first worklist; counters[TH_LEN + 0] was cleared by the host call
__global__ void __launch_bounds__(256)
th_begin(const uint32_t N, const float *__restrict__ points, uint32_t *__restrict__ state, uint32_t *__restrict__ list, uint32_t *__restrict__ counters)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool fin = false;
    if (i < N) {
        fin = ev_finite(points[3 * (size_t)i]) && ev_finite(points[3 * (size_t)i + 1]) && ev_finite(points[3 * (size_t)i + 2]);
        state[i] = fin ? TH_UNDECIDED : TH_DROPPED;
    }
    th_append(fin, i, list, counters + TH_LEN, N);
}

// One round: a lane per undecided point.  It never waits for another lane: it reads whatever state its lower-keyed neighbours have at that moment,
// and a neighbour that is still undecided only postpones it to the next launch (header: why a stale state is harmless).
template <bool HASH>
__global__ void __launch_bounds__(256)
th_round(const uint32_t N, const float *__restrict__ points, const float r2, const uint32_t seed, const Grid g, const int32_t shells,
         const uint32_t *__restrict__ cell_end, const float4 *__restrict__ records, uint32_t *state, const uint32_t *__restrict__ list_in,
         uint32_t *__restrict__ list_out, uint32_t *__restrict__ counters, const uint32_t in, const uint32_t out, const uint32_t clear)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t m = min(counters[TH_LEN + in], N);
    if (t == 0) {
        counters[TH_LEN + clear] = 0u;
        if (m) counters[TH_ROUNDS] += 1u;                         // one lane of one launch, and the launches are in order
    }
    uint32_t i = 0;
    bool blocked = false;
    if (t < m && (i = list_in[t]) < N) {
        const float qx = points[3 * (size_t)i], qy = points[3 * (size_t)i + 1], qz = points[3 * (size_t)i + 2];
        const uint32_t key = HASH ? rng_hash(seed, i, RNG_THIN_STREAM) : i;
        const int32_t nx = g.n[0], ny = g.n[1], nz = g.n[2];
        const int32_t ci = pg_axis(qx, g.o[0], g.cell, nx), cj = pg_axis(qy, g.o[1], g.cell, ny), ck = pg_axis(qz, g.o[2], g.cell, nz);
        const int32_t k0 = max(ck - shells, 0), k1 = min(ck + shells, nz - 1), j0 = max(cj - shells, 0), j1 = min(cj + shells, ny - 1);
        const int32_t i0 = max(ci - shells, 0), i1 = min(ci + shells, nx - 1);
        bool dropped = false;
        for (int32_t k = k0; k <= k1 && !dropped; k++) {
            for (int32_t j = j0; j <= j1 && !dropped; j++) {
                const uint32_t row = (uint32_t)nx * ((uint32_t)j + (uint32_t)ny * (uint32_t)k);      // x-adjacent cells are one run of records
                const uint32_t c0 = row + (uint32_t)i0, first = c0 ? cell_end[c0 - 1] : 0u, last = min(cell_end[row + (uint32_t)i1], N);
                for (uint32_t s = first; s < last; s++) {
                    const float4 p = records[s];
                    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
                    const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                    const uint32_t o = __float_as_uint(p.w);
                    if (!(d2 <= r2) || o == i || o >= N) continue;
                    if ((HASH ? rng_hash(seed, o, RNG_THIN_STREAM) : o) > key) continue;
                    const uint32_t st = __hip_atomic_load(state + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (st == TH_KEPT) { dropped = true; break; }
                    blocked = blocked || st == TH_UNDECIDED;
                }
            }
        }
        if (dropped) blocked = false;
        if (!blocked) __hip_atomic_store(state + i, dropped ? TH_DROPPED : TH_KEPT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    th_append(blocked, i, list_out, counters + TH_LEN + out, N);
}

__global__ void __launch_bounds__(256)
th_keep(const uint32_t N, const uint32_t *__restrict__ state, uint8_t *__restrict__ keep)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < N) keep[i] = state[i] == TH_KEPT ? 1 : 0;
}

// ---- culling to masks (header: "culling") ----------------------------------------------------------------------------------------------------------
// a lane per vertex; the projection is that of tsdf_integrate (csrc/mesh.hip), operation for operation
__global__ void __launch_bounds__(256)
cull_vertices(const uint32_t V, const float *__restrict__ vertices, const envgs_cull_views views, const int accumulate, uint8_t *__restrict__ keep)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V) return;
    const float x = vertices[3 * (size_t)v], y = vertices[3 * (size_t)v + 1], z = vertices[3 * (size_t)v + 2];
    bool ok = ev_finite(x) && ev_finite(y) && ev_finite(z) && (!accumulate || keep[v] != 0);
    for (int vi = 0; vi < views.count && ok; vi++) {
        const envgs_cull_view &C = views.v[vi];
        const float zc = C.R[6] * x + C.R[7] * y + C.R[8] * z + C.T[2];
        if (!(zc > 0.f)) continue;
        const float xc = C.R[0] * x + C.R[1] * y + C.R[2] * z + C.T[0];
        const float yc = C.R[3] * x + C.R[4] * y + C.R[5] * z + C.T[1];
        const float fu = floorf(C.fx * (xc / zc) + C.cx), fv = floorf(C.fy * (yc / zc) + C.cy);
        if (!(fu >= 0.f && fu < (float)C.W && fv >= 0.f && fv < (float)C.H)) continue;
        ok = C.mask[(size_t)(int)fv * (size_t)C.W + (size_t)(int)fu] != 0;
    }
    keep[v] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(256)
cull_faces(const uint32_t V, const uint32_t F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ vertex_keep, uint8_t *__restrict__ face_keep)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F) return;
    uint32_t idx[3];
    face_keep[f] = ms_indices(faces, f, V, idx) && vertex_keep[idx[0]] && vertex_keep[idx[1]] && vertex_keep[idx[2]] ? 1 : 0;
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

// state (N) | worklist 0 (N) | worklist 1 (N) | counters
struct ThinTemp { size_t state, list[2], counters, total; };
ThinTemp thin_temp(uint32_t N)
{
    ThinTemp t;
    const size_t part = up256(4 * (size_t)N);
    t.state = 0;
    t.list[0] = part;
    t.list[1] = 2 * part;
    t.counters = 3 * part;
    t.total = t.counters + up256(4 * TH_COUNTERS);
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

size_t envgs_points_thin_temp_bytes(uint32_t N)
{
    return N >= COUNT_LIMIT ? 0 : thin_temp(N).total;
}

// count[0] = the length of worklist `slot`, count[1] = the rounds that found work
static int thin_report(const uint32_t *counters, uint32_t slot, uint32_t *count, hipStream_t stream)
{
    hipError_t e;
    if ((e = hipMemcpyAsync(count, counters + TH_LEN + slot, 4, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return (int)e;
    if ((e = hipMemcpyAsync(count + 1, counters + TH_ROUNDS, 4, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return (int)e;
    return (int)hipGetLastError();
}

int envgs_points_thin_begin(uint32_t N, const float *points, void *temp, size_t temp_bytes, uint32_t *count, void *stream_)
{
    if (N >= COUNT_LIMIT || !temp || !aligned16(temp) || !count || (N && !points)) return ENVGS_ERR_BAD_ARG;
    const ThinTemp T = thin_temp(N);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)temp;
    uint32_t *counters = (uint32_t *)(base + T.counters);
    hipError_t e;
    if ((e = hipMemsetAsync(counters, 0, 4 * TH_COUNTERS, stream)) != hipSuccess) return (int)e;
    if (N) hipLaunchKernelGGL(th_begin, dim3(blocks_of(N)), dim3(256), 0, stream, N, points, (uint32_t *)(base + T.state), (uint32_t *)(base + T.list[0]), counters);
    return thin_report(counters, 0, count, stream);
}

int envgs_points_thin_round(uint32_t N, const float *points, float radius, int32_t hashed, uint32_t seed, float ox, float oy, float oz, float cell, int32_t nx,
                            int32_t ny, int32_t nz, int32_t shells, const uint32_t *cell_end, const float *records, void *temp, size_t temp_bytes,
                            uint32_t first_round, uint32_t rounds, uint32_t undecided, uint32_t *count, void *stream_)
{
    const uint32_t cells = grid_cells(nx, ny, nz);
    if (N >= COUNT_LIMIT || !cells || !grid_ok(ox, oy, oz, cell) || !cell_end || !aligned16(records) || !temp || !aligned16(temp) || !count) return ENVGS_ERR_BAD_ARG;
    if (!(radius >= 0.0f) || !std::isfinite(radius) || shells < 0 || shells >= ENVGS_POINTS_MAX_DIM || (N && (!points || !records))) return ENVGS_ERR_BAD_ARG;
    const ThinTemp T = thin_temp(N);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)temp;
    uint32_t *counters = (uint32_t *)(base + T.counters), *state = (uint32_t *)(base + T.state);
    const Grid g = {{ox, oy, oz}, cell, {nx, ny, nz}};
    const float r2 = radius * radius;
    const uint32_t lanes = undecided < N ? undecided : N;
    uint32_t t = first_round;
    for (uint32_t r = 0; r < rounds && lanes; r++, t++) {
        uint32_t *in = (uint32_t *)(base + T.list[t & 1u]), *out = (uint32_t *)(base + T.list[(t + 1u) & 1u]);
        const uint32_t a = t % 3u, b = (t % 3u + 1u) % 3u, c = (t % 3u + 2u) % 3u;
        if (hashed)
            hipLaunchKernelGGL(th_round<true>, dim3(blocks_of(lanes)), dim3(256), 0, stream, N, points, r2, seed, g, shells, cell_end, (const float4 *)records,
                               state, (const uint32_t *)in, out, counters, a, b, c);
        else
            hipLaunchKernelGGL(th_round<false>, dim3(blocks_of(lanes)), dim3(256), 0, stream, N, points, r2, seed, g, shells, cell_end, (const float4 *)records,
                               state, (const uint32_t *)in, out, counters, a, b, c);
    }
    return thin_report(counters, t % 3u, count, stream);
}

int envgs_points_thin_keep(uint32_t N, const void *temp, size_t temp_bytes, uint8_t *keep, void *stream)
{
    if (N >= COUNT_LIMIT || !temp || !aligned16(temp) || (N && !keep)) return ENVGS_ERR_BAD_ARG;
    const ThinTemp T = thin_temp(N);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    if (N) hipLaunchKernelGGL(th_keep, dim3(blocks_of(N)), dim3(256), 0, (hipStream_t)stream, N, (const uint32_t *)((const char *)temp + T.state), keep);
    return (int)hipGetLastError();
}

int envgs_mesh_cull_vertices(uint32_t V, const float *vertices, const envgs_cull_views *views, int32_t accumulate, uint8_t *keep, void *stream)
{
    if (V >= COUNT_LIMIT || !views || views->count < 0 || views->count > ENVGS_TSDF_MAX_VIEWS || (V && (!vertices || !keep))) return ENVGS_ERR_BAD_ARG;
    for (int i = 0; i < views->count; i++)
        if (!views->v[i].mask || views->v[i].H < 1 || views->v[i].W < 1) return ENVGS_ERR_BAD_ARG;
    if (V) hipLaunchKernelGGL(cull_vertices, dim3(blocks_of(V)), dim3(256), 0, (hipStream_t)stream, V, vertices, *views, (int)accumulate, keep);
    return (int)hipGetLastError();
}

int envgs_mesh_cull_faces(uint32_t V, uint32_t F, const int32_t *faces, const uint8_t *vertex_keep, uint8_t *face_keep, void *stream)
{
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT || (F && (!faces || !face_keep)) || (F && V && !vertex_keep)) return ENVGS_ERR_BAD_ARG;
    if (F) hipLaunchKernelGGL(cull_faces, dim3(blocks_of(F)), dim3(256), 0, (hipStream_t)stream, V, F, faces, vertex_keep, face_keep);
    return (int)hipGetLastError();
}

}  // extern "C"
