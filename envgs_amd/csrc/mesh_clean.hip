// mesh_clean.hip -- mesh clean-up for gfx950 (include/envgs_mesh.h): connected components of an indexed triangle mesh, and order-preserving
// selection of faces with re-indexed vertices.  Integer work only: no float is computed and no float atomic is issued, vertices and colours are
// copied as 32-bit words, so every output is exact and two runs give identical bytes.
//
// Components (16 B of scratch per vertex):
//   cc_init          parent[v] = v, the two per-root counters = 0                                                   12 B written per vertex
//   cc_hook          a lane per face: the union-find of mesh_unionfind.h (find with path halving, atomicCAS hooks the LARGER root under the
//                    SMALLER, so every final root is the smallest vertex index of its component whatever the schedule).  Faces with an index
//                    outside [0, V) are skipped before anything is dereferenced.  No lane waits for another: the only retry is a failed CAS.
//   cc_flatten       parent[v] = root(v)
//   cc_face_count    faces per root.  A real mesh is one giant component plus crumbs, so a plain atomicAdd per face would put every adder on one
//                    row (the 14 x slow case of Guideline 12; the compiler's own coalescing covers only a uniform address).  CHOSEN FORM,
//                    block_add_by_key: the wavefront elects the first pending lane and ballots the lanes that hold the same root; the four
//                    wavefronts of the workgroup put that (root, population count) in LDS and the first one holding a root issues ONE atomicAdd of
//                    the workgroup's sum; further distinct roots get one add per wavefront each, and after AGG_ROUNDS (4) roots the lanes still
//                    pending add 1 each, to rows that are then necessarily spread.  Consecutive faces of the extractor are in cell order and
//                    nearly always agree, so a workgroup of the giant component issues one add of 256.
//   cc_vertex_count  vertices per root in the same form (only vertices whose root owns a face), and in the same pass the block scan that ranks the
//                    roots owning a face: block-local rank per root, one total per workgroup of 256 consecutive vertices
//   launch_scan      over the per-WORKGROUP totals (the pattern of mesh_count); ascending root = ascending smallest vertex = component number
//   cc_label_*       gathers vertex labels, the two count tables, C, and the face labels (label of the first index, -1 for an ignored face)
//
// Selection (2 B of scratch per vertex), in two phases around the one read-back of (V', F'):
//   sel_mark         a lane per face: survives = keep byte non-zero and indices in range; marks its three vertices with plain stores of 1; block
//                    total of survivors per workgroup of 256 consecutive faces
//   sel_vscan        block scan of the marks: block-local rank (1 B per vertex), total per workgroup
//   launch_scan x 2, sel_totals
//   sel_emit_v / sel_emit_f   survivors written at scanned base + block rank, faces re-indexed through the vertices' ranks.  No atomics hand out
//                    slots: relative order is part of the contract.
#include "common.h"
#include "mesh_unionfind.h"

#include "../../include/envgs_mesh.h"

namespace envgs {
namespace {

struct DeviceAtomics {
    typedef uint32_t cell;
    static __host__ __device__ __forceinline__ uint32_t load(const cell *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __host__ __device__ __forceinline__ void store(cell *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __host__ __device__ __forceinline__ uint32_t cas(cell *p, uint32_t expect, uint32_t desired)
    {
        __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;                                            // unchanged on success, the observed word on failure
    }
};

constexpr int AGG_ROUNDS = 4;

// table[key] += 1 for every thread with `on`, aggregated: lanes of a wavefront that hold the same key issue one add of their population count.
// Wave-uniform control flow (the ballots) and one workgroup barrier; no thread waits for memory written by another workgroup.
// The first key of each wavefront goes through LDS (s_key, s_cnt: 4 words each): the first wavefront of the workgroup that holds it adds the
// workgroup's sum.  To be called by every thread of the workgroup.
__device__ __forceinline__ void block_add_by_key(uint32_t *__restrict__ table, bool on, const uint32_t key, uint32_t *s_key, uint32_t *s_cnt)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    unsigned long long todo = __ballot(on);
    uint32_t k0 = 0, c0 = 0;
    if (todo) {
        k0 = (uint32_t)__shfl((int)key, __ffsll(todo) - 1);
        const unsigned long long same = __ballot(on && key == k0);
        c0 = (uint32_t)__popcll(same);
        on = on && key != k0;
        todo &= ~same;
    }
    if (lane == 0) { s_key[wave] = k0; s_cnt[wave] = c0; }
    __syncthreads();
    if (lane == 0 && c0) {
        bool first = true;
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const bool mine = s_cnt[w] && s_key[w] == k0;
            first = first && !(mine && w < wave);
            sum += mine ? s_cnt[w] : 0u;
        }
        if (first) atomicAdd(table + k0, sum);
    }
    for (int round = 1; round < AGG_ROUNDS && todo; round++) {
        const int leader = __ffsll(todo) - 1;
        const uint32_t k = (uint32_t)__shfl((int)key, leader);
        const unsigned long long same = __ballot(on && key == k);
        if (lane == leader) atomicAdd(table + k, (uint32_t)__popcll(same));
        on = on && key != k;
        todo &= ~same;
    }
    if (on) atomicAdd(table + key, 1u);
}

__device__ __forceinline__ bool face_in_range(const int32_t *__restrict__ faces, const uint32_t f, const uint32_t V, uint32_t (&idx)[3])
{
#pragma unroll
    for (int e = 0; e < 3; e++) idx[e] = (uint32_t)faces[3 * (size_t)f + e];                    // a negative index becomes >= 2^31 > V
    return idx[0] < V && idx[1] < V && idx[2] < V;
}

// ---- components -----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
cc_init(const uint32_t V, uint32_t *__restrict__ parent, uint32_t *__restrict__ nf, uint32_t *__restrict__ nv)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < V) { parent[v] = v; nf[v] = 0; nv[v] = 0; }
}

__global__ void __launch_bounds__(256)
cc_hook(const uint32_t V, const uint32_t F, const int32_t *__restrict__ faces, uint32_t *parent)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < F) (void)uf_hook_face<DeviceAtomics>(parent, V, faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]);
}

__global__ void __launch_bounds__(256)
cc_flatten(const uint32_t V, uint32_t *parent)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < V) (void)uf_flatten<DeviceAtomics>(parent, v);
}

__global__ void __launch_bounds__(256)
cc_face_count(const uint32_t V, const uint32_t F, const int32_t *__restrict__ faces, const uint32_t *__restrict__ parent, uint32_t *__restrict__ nf)
{
    __shared__ uint32_t s_key[4], s_cnt[4];
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint32_t idx[3];
    const bool on = f < F && face_in_range(faces, f, V, idx);
    block_add_by_key(nf, on, on ? parent[idx[0]] : 0u, s_key, s_cnt);
}

__global__ void __launch_bounds__(256)
cc_vertex_count(const uint32_t V, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ nf, uint32_t *__restrict__ nv,
                uint32_t *__restrict__ rloc, uint32_t *__restrict__ tot)
{
    __shared__ uint32_t s_w[4], s_key[4], s_cnt[4];
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const uint32_t r = v < V ? parent[v] : 0u;
    const bool ref = v < V && nf[r] > 0;
    block_add_by_key(nv, ref, r, s_key, s_cnt);
    const bool owns = ref && r == v;
    uint32_t total;
    const uint32_t ex = block_exclusive_u32<4>(owns ? 1u : 0u, s_w, total);
    if (owns) rloc[v] = ex;
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// tot holds the INCLUSIVE scan over the workgroups here; cap = min(V, F), the rows of the two tables
__global__ void __launch_bounds__(256)
cc_label_vertices(const uint32_t V, const uint32_t cap, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ nf, const uint32_t *__restrict__ nv,
                  const uint32_t *__restrict__ rloc, const uint32_t *__restrict__ tot, int32_t *__restrict__ vertex_label,
                  int32_t *__restrict__ comp_faces, int32_t *__restrict__ comp_vertices, uint32_t *__restrict__ count)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v == 0) *count = tot[(V + 255u) / 256u - 1u];
    if (v >= V) return;
    const uint32_t r = parent[v];
    int32_t label = -1;
    if (nf[r] > 0) {
        const uint32_t rb = r >> 8;
        const uint32_t l = (rb ? tot[rb - 1] : 0u) + rloc[r];
        label = (int32_t)l;
        if (r == v && l < cap) { comp_faces[l] = (int32_t)nf[v]; comp_vertices[l] = (int32_t)nv[v]; }
    }
    vertex_label[v] = label;
}

__global__ void __launch_bounds__(256)
cc_label_faces(const uint32_t V, const uint32_t F, const int32_t *__restrict__ faces, const int32_t *__restrict__ vertex_label,
               int32_t *__restrict__ face_label)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F) return;
    uint32_t idx[3];
    face_label[f] = face_in_range(faces, f, V, idx) ? vertex_label[idx[0]] : -1;
}

// ---- selection ------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
sel_mark(const uint32_t V, const uint32_t F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep, uint8_t *__restrict__ vused,
         uint32_t *__restrict__ cnt_f)
{
    __shared__ uint32_t s_w[4];
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint32_t idx[3];
    const bool on = f < F && keep[f] != 0 && face_in_range(faces, f, V, idx);
    if (on) { vused[idx[0]] = 1; vused[idx[1]] = 1; vused[idx[2]] = 1; }
    uint32_t total;
    (void)block_exclusive_u32<4>(on ? 1u : 0u, s_w, total);
    if (threadIdx.x == 0) cnt_f[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256)
sel_vscan(const uint32_t V, const uint8_t *__restrict__ vused, uint8_t *__restrict__ vloc, uint32_t *__restrict__ cnt_v)
{
    __shared__ uint32_t s_w[4];
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const uint32_t u = (v < V && vused[v]) ? 1u : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_u32<4>(u, s_w, total);      // <= 255
    if (v < V) vloc[v] = (uint8_t)ex;
    if (threadIdx.x == 0) cnt_v[blockIdx.x] = total;
}

__global__ void sel_totals(const uint32_t *__restrict__ cnt_v, const uint32_t nbv, const uint32_t *__restrict__ cnt_f, const uint32_t nbf,
                           uint32_t *__restrict__ totals)
{
    if (threadIdx.x == 0) totals[0] = cnt_v[nbv - 1];
    if (threadIdx.x == 1) totals[1] = cnt_f[nbf - 1];
}

// cnt_v / cnt_f hold INCLUSIVE scans over the workgroups from here on
__global__ void __launch_bounds__(256)
sel_emit_v(const uint32_t V, const uint8_t *__restrict__ vused, const uint8_t *__restrict__ vloc, const uint32_t *__restrict__ cnt_v,
           const uint32_t *__restrict__ vertices, const uint32_t *__restrict__ colors, const uint32_t Vout, uint32_t *__restrict__ out_vertices,
           uint32_t *__restrict__ out_colors, int32_t *__restrict__ vertex_index)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V || !vused[v]) return;
    const uint32_t n = (blockIdx.x ? cnt_v[blockIdx.x - 1] : 0u) + vloc[v];
    if (n >= Vout) return;
#pragma unroll
    for (int c = 0; c < 3; c++) out_vertices[3 * (size_t)n + c] = vertices[3 * (size_t)v + c];
    if (out_colors) {
#pragma unroll
        for (int c = 0; c < 3; c++) out_colors[3 * (size_t)n + c] = colors[3 * (size_t)v + c];
    }
    if (vertex_index) vertex_index[n] = (int32_t)v;
}

__global__ void __launch_bounds__(256)
sel_emit_f(const uint32_t V, const uint32_t F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep, const uint8_t *__restrict__ vloc,
           const uint32_t *__restrict__ cnt_v, const uint32_t *__restrict__ cnt_f, const uint32_t Fout, int32_t *__restrict__ out_faces)
{
    __shared__ uint32_t s_w[4];
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint32_t idx[3];
    const bool on = f < F && keep[f] != 0 && face_in_range(faces, f, V, idx);
    uint32_t total;
    const uint32_t n = block_exclusive_u32<4>(on ? 1u : 0u, s_w, total) + (blockIdx.x ? cnt_f[blockIdx.x - 1] : 0u);
    if (!on || n >= Fout) return;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const uint32_t b = idx[e] >> 8;
        out_faces[3 * (size_t)n + e] = (int32_t)((b ? cnt_v[b - 1] : 0u) + vloc[idx[e]]);
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }
constexpr uint32_t COUNT_LIMIT = 1u << 31;

// components: parent (V) | nf (V) | nv (V) | rloc (V) | tot (nb) | scan scratch
struct CompTemp { size_t parent, nf, nv, rloc, tot, scan, scan_bytes, total; uint32_t nb; };
CompTemp comp_temp(uint32_t V)
{
    CompTemp t;
    t.nb = blocks_of(V);
    const size_t plane = up256(4 * (size_t)V);
    t.parent = 0;
    t.nf = plane;
    t.nv = 2 * plane;
    t.rloc = 3 * plane;
    t.tot = 4 * plane;
    t.scan = t.tot + up256(4 * (size_t)t.nb);
    t.scan_bytes = scan_temp_bytes((int)t.nb);
    t.total = t.scan + up256(t.scan_bytes);
    return t;
}

// selection: vused (V) | vloc (V) | cnt_v (nbv) | cnt_f (nbf) | scan scratch
struct SelTemp { size_t vused, vloc, cnt_v, cnt_f, scan, scan_bytes, total; uint32_t nbv, nbf; };
SelTemp sel_temp(uint32_t V, uint32_t F)
{
    SelTemp t;
    t.nbv = blocks_of(V);
    t.nbf = blocks_of(F);
    t.vused = 0;
    t.vloc = up256((size_t)V);
    t.cnt_v = t.vloc + up256((size_t)V);
    t.cnt_f = t.cnt_v + up256(4 * (size_t)t.nbv);
    t.scan = t.cnt_f + up256(4 * (size_t)t.nbf);
    t.scan_bytes = scan_temp_bytes((int)(t.nbv > t.nbf ? t.nbv : t.nbf));
    t.total = t.scan + up256(t.scan_bytes);
    return t;
}

}  // namespace
}  // namespace envgs

using namespace envgs;

extern "C" {

size_t envgs_mesh_components_temp_bytes(uint32_t V, uint32_t F)
{
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT) return 0;
    return comp_temp(V).total;
}

int envgs_mesh_components(uint32_t V, uint32_t F, const int32_t *faces, void *temp, size_t temp_bytes, int32_t *vertex_label, int32_t *face_label,
                          int32_t *comp_faces, int32_t *comp_vertices, uint32_t *count, void *stream_)
{
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT || !temp || !aligned16(temp) || !count) return ENVGS_ERR_BAD_ARG;
    if ((F && (!faces || !face_label)) || (V && !vertex_label) || (V && F && (!comp_faces || !comp_vertices))) return ENVGS_ERR_BAD_ARG;
    const CompTemp T = comp_temp(V);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    if (V == 0 || F == 0) {                                       // nothing can be joined: every label -1, no component
        hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
        if (e == hipSuccess && V) e = hipMemsetAsync(vertex_label, 0xff, 4 * (size_t)V, stream);
        if (e == hipSuccess && F) e = hipMemsetAsync(face_label, 0xff, 4 * (size_t)F, stream);
        return (int)e;
    }
    char *base = (char *)temp;
    uint32_t *parent = (uint32_t *)(base + T.parent), *nf = (uint32_t *)(base + T.nf), *nv = (uint32_t *)(base + T.nv);
    uint32_t *rloc = (uint32_t *)(base + T.rloc), *tot = (uint32_t *)(base + T.tot);
    const dim3 gv(T.nb), gf(blocks_of(F)), wg(256);
    hipLaunchKernelGGL(cc_init, gv, wg, 0, stream, V, parent, nf, nv);
    hipLaunchKernelGGL(cc_hook, gf, wg, 0, stream, V, F, faces, parent);
    hipLaunchKernelGGL(cc_flatten, gv, wg, 0, stream, V, parent);
    hipLaunchKernelGGL(cc_face_count, gf, wg, 0, stream, V, F, faces, (const uint32_t *)parent, nf);
    hipLaunchKernelGGL(cc_vertex_count, gv, wg, 0, stream, V, (const uint32_t *)parent, (const uint32_t *)nf, nv, rloc, tot);
    const int rc = launch_scan(tot, tot, (int)T.nb, base + T.scan, T.scan_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(cc_label_vertices, gv, wg, 0, stream, V, V < F ? V : F, (const uint32_t *)parent, (const uint32_t *)nf, (const uint32_t *)nv,
                       (const uint32_t *)rloc, (const uint32_t *)tot, vertex_label, comp_faces, comp_vertices, count);
    hipLaunchKernelGGL(cc_label_faces, gf, wg, 0, stream, V, F, faces, (const int32_t *)vertex_label, face_label);
    return (int)hipGetLastError();
}

size_t envgs_mesh_select_temp_bytes(uint32_t V, uint32_t F)
{
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT) return 0;
    return sel_temp(V, F).total;
}

int envgs_mesh_select_count(uint32_t V, uint32_t F, const int32_t *faces, const uint8_t *keep, void *temp, size_t temp_bytes, uint32_t *totals,
                            void *stream_)
{
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT || !temp || !aligned16(temp) || !totals || (F && (!faces || !keep))) return ENVGS_ERR_BAD_ARG;
    const SelTemp T = sel_temp(V, F);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    if (V == 0 || F == 0) return (int)hipMemsetAsync(totals, 0, 2 * sizeof(uint32_t), stream);   // no face can survive, so no vertex does
    char *base = (char *)temp;
    uint8_t *vused = (uint8_t *)(base + T.vused), *vloc = (uint8_t *)(base + T.vloc);
    uint32_t *cnt_v = (uint32_t *)(base + T.cnt_v), *cnt_f = (uint32_t *)(base + T.cnt_f);
    const hipError_t e = hipMemsetAsync(vused, 0, (size_t)V, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sel_mark, dim3(T.nbf), dim3(256), 0, stream, V, F, faces, keep, vused, cnt_f);
    hipLaunchKernelGGL(sel_vscan, dim3(T.nbv), dim3(256), 0, stream, V, (const uint8_t *)vused, vloc, cnt_v);
    int rc = launch_scan(cnt_v, cnt_v, (int)T.nbv, base + T.scan, T.scan_bytes, stream);
    if (rc) return rc;
    rc = launch_scan(cnt_f, cnt_f, (int)T.nbf, base + T.scan, T.scan_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(sel_totals, dim3(1), dim3(64), 0, stream, (const uint32_t *)cnt_v, T.nbv, (const uint32_t *)cnt_f, T.nbf, totals);
    return (int)hipGetLastError();
}

int envgs_mesh_select_emit(uint32_t V, uint32_t F, const float *vertices, const float *colors, const int32_t *faces, const uint8_t *keep,
                           const void *temp, size_t temp_bytes, uint32_t Vout, uint32_t Fout, float *out_vertices, float *out_colors,
                           int32_t *out_faces, int32_t *vertex_index, void *stream_)
{
    if (V >= COUNT_LIMIT || F >= COUNT_LIMIT || Vout > V || Fout > F || !temp || !aligned16(temp)) return ENVGS_ERR_BAD_ARG;
    if ((V && !vertices) || (F && (!faces || !keep)) || (Vout && !out_vertices) || (Fout && !out_faces) || (out_colors && !colors))
        return ENVGS_ERR_BAD_ARG;
    const SelTemp T = sel_temp(V, F);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    if (Vout == 0 && Fout == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const char *base = (const char *)temp;
    const uint8_t *vused = (const uint8_t *)(base + T.vused), *vloc = (const uint8_t *)(base + T.vloc);
    const uint32_t *cnt_v = (const uint32_t *)(base + T.cnt_v), *cnt_f = (const uint32_t *)(base + T.cnt_f);
    if (Vout)
        hipLaunchKernelGGL(sel_emit_v, dim3(T.nbv), dim3(256), 0, stream, V, vused, vloc, cnt_v, (const uint32_t *)vertices, (const uint32_t *)colors, Vout,
                           (uint32_t *)out_vertices, (uint32_t *)out_colors, vertex_index);
    if (Fout) hipLaunchKernelGGL(sel_emit_f, dim3(T.nbf), dim3(256), 0, stream, V, F, faces, keep, vloc, cnt_v, cnt_f, Fout, out_faces);
    return (int)hipGetLastError();
}

}  // extern "C"
