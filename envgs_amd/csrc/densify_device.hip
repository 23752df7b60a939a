// densify_device.hip -- the device-resident densification mode of SurfelSet (include/envgs_densify.h, second half):
//
//   densify_stats     the per-step statistics of add_densification_stats in one launch, one lane per surfel, no host round trip
//   grow_plan         clone / split / prune-by-opacity-or-gradient decided per ORIGINAL surfel (a clone child inherits everything its parent is
//                     judged by, so the three staged stages are a closed-form function of the state before the pass): class bits + six flag
//                     arrays [A|B|D|E|S1|S2]; one launch_scan over them gives every output row and every sample index
//   grow_counters     segment totals next to the atomics of grow_plan: the ONE block of words the host reads back
//   grow_stds         the standard deviations of the split offsets, in the staged order, for the host's torch.normal call
//   grow_rewrite      every parameter, both Adam moments and the four statistics written once at their final size: a workgroup walks 256
//                     consecutive 4-byte words of one source tensor (compact_gather's shape) and stores each word to the 0 .. 2 + 2N rows it
//                     becomes; kept rows stay in order inside every segment, so the stores are contiguous runs as well
//
//   weight_select     the pruning tail (device_schedule="all"): exact order statistics of the average weight by the three-pass radix select of
//                     radix_select.h, the key computed from two arrays and the count below each selected value kept; visibility_mask turns a
//                     cut and a count into `prune_visibility`'s keep mask (ties by index order, ranked with a scan); oversize_plan is
//                     `prune_max_scene_and_screen`'s masks and counts in one launch
//
// Compiled with -ffp-contract=off (build.py): the decisions repeat torch's compare / divide bit for bit and the gradient norm is a fixed
// left-to-right sum, whatever the compiler would like to fuse.
#include "common.h"
#include "radix_select.h"

#include "../../include/envgs_densify.h"

namespace envgs {

constexpr uint8_t CLS_CLONE = ENVGS_GROW_CLS_CLONE, CLS_SPLIT = ENVGS_GROW_CLS_SPLIT, CLS_PRUNE_1 = ENVGS_GROW_CLS_PRUNE_1, CLS_PRUNE_S = ENVGS_GROW_CLS_PRUNE_S;

// ---- per-step statistics ----------------------------------------------------------------------------------------------------------------
template <int COLS>
__global__ void __launch_bounds__(256)
densify_stats(const long long P, const float *__restrict__ grad, const uint8_t *__restrict__ filter, const float *__restrict__ weight,
              const int32_t *__restrict__ radii, float *__restrict__ ga, float *__restrict__ dn, float *__restrict__ mr, float *__restrict__ wa)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P || !filter[i]) return;
    const float gx = grad[i * COLS], gy = grad[i * COLS + 1];
    float s = __fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy));
    if (COLS == 3) { const float gz = grad[i * COLS + 2]; s = __fadd_rn(s, __fmul_rn(gz, gz)); }
    dn[i] = __fadd_rn(dn[i], 1.0f);
    ga[i] = __fadd_rn(ga[i], __fsqrt_rn(s));
    if (weight) wa[i] = __fadd_rn(wa[i], weight[i]);
    if (radii) mr[i] = fmaxf(mr[i], (float)radii[i]);
}

// ---- plan -------------------------------------------------------------------------------------------------------------------------------
// the weight maxima travel as raw float_key words (float_key.h; 0 = "nothing yet": it decodes to a negative NaN, below every number)

__device__ __forceinline__ float stat_avg(float x, float d) { const float a = x / d; return a != a ? 0.0f : a; }        // IEEE division; NaN -> 0

__global__ void __launch_bounds__(256)
grow_plan(const envgs_densify_plan_args a)
{
    __shared__ uint32_t s_red[4][4];
    const long long P = a.P, i = (long long)blockIdx.x * 256 + threadIdx.x;
    uint32_t n_clone = 0, w_all = 0, w_clone_max = 0, w_clone_min = 0;
    if (i < P) {
        const float ga = a.ga[i], dn = a.dn[i], wa = a.wa[i];
        const float avg = stat_avg(ga, dn);
        const bool high = avg >= a.grad_threshold;
        const bool small = fmaxf(a.scal[2 * i], a.scal[2 * i + 1]) <= a.size_limit;
        const bool clone = small && high;
        const bool split = high && (!small || ((a.flags & ENVGS_PLAN_SPLIT_SCREEN) && a.mr[i] > a.split_screen_threshold));
        const bool occ = (a.flags & ENVGS_PLAN_MIN_OPACITY) && a.opac[i] < a.min_opacity;
        bool pr_1 = occ, pr_s = occ;
        if (a.flags & ENVGS_PLAN_MIN_GRADIENT) {
            pr_1 = pr_1 || (avg <= a.min_gradient && dn != 0.0f);
            pr_s = pr_s || (stat_avg(__fmul_rn(ga, a.r), dn) <= a.min_gradient && dn != 0.0f);
        }
        a.cls[i] = (clone ? CLS_CLONE : 0) | (split ? CLS_SPLIT : 0) | (pr_1 ? CLS_PRUNE_1 : 0) | (pr_s ? CLS_PRUNE_S : 0);
        a.scan[i] = (!split && !pr_1) ? 1u : 0u;                     // A: originals that stay
        a.scan[P + i] = (clone && !split && !pr_1) ? 1u : 0u;        // B: clone children that stay
        a.scan[2 * P + i] = (split && !pr_s) ? 1u : 0u;              // D: kept split children of originals (per block)
        a.scan[3 * P + i] = (clone && split && !pr_s) ? 1u : 0u;     // E: kept split children of clone children (per block)
        a.scan[4 * P + i] = split ? 1u : 0u;                         // S1, S2: the staged split selection, pruned or not (sample order)
        a.scan[5 * P + i] = (clone && split) ? 1u : 0u;
        n_clone = clone ? 1u : 0u;
        w_all = float_key(wa);
        if (clone) { w_clone_max = float_key(wa); w_clone_min = ~float_key(wa); }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n_clone += __shfl_xor(n_clone, d, 64);
        w_all = max(w_all, (uint32_t)__shfl_xor(w_all, d, 64));
        w_clone_max = max(w_clone_max, (uint32_t)__shfl_xor(w_clone_max, d, 64));
        w_clone_min = max(w_clone_min, (uint32_t)__shfl_xor(w_clone_min, d, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_red[wave][0] = n_clone; s_red[wave][1] = w_all; s_red[wave][2] = w_clone_max; s_red[wave][3] = w_clone_min; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t n = 0, m0 = 0, m1 = 0, m2 = 0;
        for (int k = 0; k < 4; k++) { n += s_red[k][0]; m0 = max(m0, s_red[k][1]); m1 = max(m1, s_red[k][2]); m2 = max(m2, s_red[k][3]); }
        if (n) atomicAdd(&a.counters[ENVGS_GROW_N_CLONE], n);
        atomicMax(&a.counters[ENVGS_GROW_W_ALL], m0);
        if (m1) atomicMax(&a.counters[ENVGS_GROW_W_CLONE_MAX], m1);
        if (m2) atomicMax(&a.counters[ENVGS_GROW_W_CLONE_MIN], m2);
    }
}

__global__ void grow_counters(const long long P, const uint32_t *__restrict__ scan, uint32_t *__restrict__ counters)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t prev = 0;
    for (int k = 0; k < 6; k++) { const uint32_t t = scan[(k + 1) * P - 1]; counters[k] = t - prev; prev = t; }
}

// wmax0 = max(wa) before the pass; wmax1 = the maximum once the clone children (wa * wmax0) are appended.  x -> fl(x * wmax0) is monotone,
// so the largest product belongs to the largest (wmax0 >= 0) or the smallest (wmax0 < 0) cloned weight.
__device__ __forceinline__ void grow_wmax(const uint32_t *__restrict__ counters, float &w0, float &w1)
{
    w0 = float_of_key(counters[ENVGS_GROW_W_ALL]);
    w1 = w0;
    if (counters[ENVGS_GROW_N_CLONE]) {
        const float sel = w0 < 0.0f ? float_of_key(~counters[ENVGS_GROW_W_CLONE_MIN]) : float_of_key(counters[ENVGS_GROW_W_CLONE_MAX]);
        w1 = fmaxf(w0, __fmul_rn(sel, w0));
    }
}

__global__ void __launch_bounds__(256)
grow_stds(const long long P, const int N, const uint8_t *__restrict__ cls, const uint32_t *__restrict__ scan, const uint32_t *__restrict__ counters,
          const float *__restrict__ scal, float *__restrict__ stds, const long long n_stds)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint8_t c = cls[i];
    if (!(c & CLS_SPLIT)) return;
    const long long nS = (long long)counters[ENVGS_GROW_N_S1] + counters[ENVGS_GROW_N_S2];
    const uint32_t base = scan[4 * P - 1];
    const float sx = scal[2 * i], sy = scal[2 * i + 1];
    for (int k = 0; k < 2; k++) {
        if (k == 1 && !(c & CLS_CLONE)) break;
        const long long sidx = (long long)(scan[(4 + k) * P + i] - 1u - base);
        for (int b = 0; b < N; b++) {
            const long long k3 = b * nS + sidx;
            if (k3 >= n_stds) continue;                               // (never, when the host sized stds from the counters)
            stds[k3 * 3] = sx; stds[k3 * 3 + 1] = sy; stds[k3 * 3 + 2] = 0.0f;
        }
    }
}

// ---- rewrite ----------------------------------------------------------------------------------------------------------------------------
struct GrowBatch {
    envgs_grow_tensor t[ENVGS_COMPACT_MAX_TENSORS];
    long long chunk_start[ENVGS_COMPACT_MAX_TENSORS + 1];     // prefix of 256-word chunks
    int count;
};

struct GrowCommon {
    long long P, out_rows, n_samples;
    int N;
    float r;
    double ratio_n;
    const uint8_t *cls;
    const uint32_t *scan, *counters;
    const float *scal, *rotation, *samples;
};

// row `col` of build_rotation(q) (envgs_amd/synth.py) applied to the sample (sx, sy, 0)
// (the rotation of glue.hip's surfel_quads, written out again on purpose: torch normalises with an IEEE division by the correctly rounded norm,
// and this must match it)
__device__ __forceinline__ float rotated_offset(const float *__restrict__ q4, const int col, const float sx, const float sy)
{
    const float n = __fsqrt_rn(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]);
    const float r = q4[0] / n, x = q4[1] / n, y = q4[2] / n, z = q4[3] / n;
    float r0, r1;
    if (col == 0) { r0 = 1.0f - 2.0f * (y * y + z * z); r1 = 2.0f * (x * y - r * z); }
    else if (col == 1) { r0 = 2.0f * (x * y + r * z); r1 = 1.0f - 2.0f * (x * x + z * z); }
    else { r0 = 2.0f * (x * z - r * y); r1 = 2.0f * (y * z + r * x); }
    return r0 * sx + r1 * sy;
}

__global__ void __launch_bounds__(256)
grow_rewrite(const GrowBatch B, const GrowCommon C)
{
    const long long chunk = blockIdx.x;
    int ti = 0;
    while (ti + 1 < B.count && chunk >= B.chunk_start[ti + 1]) ti++;
    const envgs_grow_tensor T = B.t[ti];
    const long long P = C.P, w = T.row_bytes >> 2;
    const long long e = (chunk - B.chunk_start[ti]) * 256 + threadIdx.x;
    if (e >= P * w) return;
    const long long row = e / w;
    const int col = (int)(e - row * w);
    const uint8_t c = C.cls[row];
    const bool clone = c & CLS_CLONE, split = c & CLS_SPLIT, pr_1 = c & CLS_PRUNE_1, pr_s = c & CLS_PRUNE_S;
    if (split ? pr_s : pr_1) return;                                 // nothing of this surfel survives
    const uint32_t v = reinterpret_cast<const uint32_t *>(T.src)[e];
    uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(T.dst);
    const int kind = T.kind;
    float w0 = 0.f, w1 = 0.f;
    if (kind == ENVGS_GROW_WEIGHT) grow_wmax(C.counters, w0, w1);
    if (!split) {
        const long long pa = (long long)(C.scan[row] - 1u), pb = clone ? (long long)(C.scan[P + row] - 1u) : 0;
        if (pa >= C.out_rows || pb >= C.out_rows) return;             // (never, when the host sized dst from the counters)
        dst[pa * w + col] = v;                                                                                          // A
        if (clone) {
            uint32_t b = v;
            if (kind == ENVGS_GROW_MOMENT) b = 0u;
            else if (kind == ENVGS_GROW_WEIGHT) b = __float_as_uint(__fmul_rn(__uint_as_float(v), w0));
            dst[pb * w + col] = b;                                                                                      // B
        }
        return;
    }
    const long long per_block = (long long)C.counters[ENVGS_GROW_N_D] + C.counters[ENVGS_GROW_N_E];
    const long long nS = (long long)C.counters[ENVGS_GROW_N_S1] + C.counters[ENVGS_GROW_N_S2];
    const uint32_t s_base = C.scan[4 * P - 1];
    const float f = __uint_as_float(v);
    for (int k = 0; k < 2; k++) {                                    // k = 0: children of the original (D); k = 1: of its clone child (E)
        if (k == 1 && !clone) break;
        const long long pos = (long long)(C.scan[(2 + k) * P + row] - 1u);
        const long long sidx = (long long)(C.scan[(4 + k) * P + row] - 1u - s_base);
        uint32_t fixed = v;
        switch (kind) {
        case ENVGS_GROW_MOMENT: fixed = 0u; break;
        case ENVGS_GROW_SCALING: fixed = __float_as_uint((float)log((double)C.scal[row * w + col] / C.ratio_n)); break;
        case ENVGS_GROW_GRAD: case ENVGS_GROW_RADIUS: fixed = __float_as_uint(__fmul_rn(f, C.r)); break;
        case ENVGS_GROW_WEIGHT: fixed = __float_as_uint(__fmul_rn(k ? __fmul_rn(f, w0) : f, w1)); break;
        default: break;
        }
        for (int b = 0; b < C.N; b++) {
            uint32_t o = fixed;
            const long long k3 = b * nS + sidx, po = pos + b * per_block;
            if (po >= C.out_rows || (kind == ENVGS_GROW_XYZ && k3 >= C.n_samples)) continue;
            if (kind == ENVGS_GROW_XYZ) o = __float_as_uint(rotated_offset(C.rotation + row * 4, col, C.samples[k3 * 3], C.samples[k3 * 3 + 1]) + f);
            dst[po * w + col] = o;
        }
    }
}

// ---- the pruning tail: order statistics of the average weight --------------------------------------------------------------------------
// radix_select.h over the key below.  The functor stays in this file: the key contains a division and this file is compiled with contraction
// off.
// get_xyz_weight_avg as an ordered word; -0 orders (and decodes) as +0
__device__ __forceinline__ uint32_t weight_key(const float wa, const float dn) { return float_key_canon(stat_avg(wa, dn)); }
__device__ __forceinline__ uint32_t cut_key(const float cut) { return weight_key(cut, 1.0f); }        // (x / 1 = x: the key of a selected value)

struct WeightKeys {
    const float *wa, *dn;
    __device__ __forceinline__ uint32_t operator()(long long i) const { return weight_key(wa[i], dn[i]); }
};

// ---- prune_visibility's mask ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
tie_flags(const long long P, const float *__restrict__ wa, const float *__restrict__ dn, const float *__restrict__ cut, uint32_t *__restrict__ flags)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < P) flags[i] = weight_key(wa[i], dn[i]) == cut_key(cut[0]) ? 1u : 0u;
}

// ties: the inclusive scan of tie_flags, i.e. the 1-based place of a tied key among the tied keys in index order
__global__ void __launch_bounds__(256)
visibility_mask(const long long P, const float *__restrict__ wa, const float *__restrict__ dn, const float *__restrict__ cut,
                const uint32_t *__restrict__ cut_below, const uint32_t n_prune, const uint32_t *__restrict__ ties, uint8_t *__restrict__ keep)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint32_t k = weight_key(wa[i], dn[i]), kc = cut_key(cut[0]), below = cut_below[0];
    const uint32_t tied_out = n_prune > below ? n_prune - below : 0u;
    keep[i] = (k < kc || (k == kc && ties[i] <= tied_out)) ? 0 : 1;
}

// ---- prune_max_scene_and_screen's masks -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
oversize_plan(const long long P, const uint32_t flags, const float max_screen, const float scene_limit, const float *__restrict__ mr,
              const float *__restrict__ scal, const float *__restrict__ wa, const float *__restrict__ dn, const float *__restrict__ quantile,
              uint8_t *__restrict__ keep, uint32_t *__restrict__ split, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t s_red[4][2];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    uint32_t n_prune = 0u, n_split = 0u;
    if (i < P) {
        const bool big = ((flags & ENVGS_OVERSIZE_SCREEN) && mr[i] > max_screen) ||
                         ((flags & ENVGS_OVERSIZE_SCENE) && fmaxf(scal[2 * i], scal[2 * i + 1]) > scene_limit);
        const bool light = !(flags & ENVGS_OVERSIZE_WEIGHT) || stat_avg(wa[i], dn[i]) < quantile[0];
        n_prune = (big && light) ? 1u : 0u;
        n_split = (big && !light) ? 1u : 0u;
        keep[i] = n_prune ? 0 : 1;
        split[i] = n_split;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { n_prune += __shfl_xor(n_prune, d, 64); n_split += __shfl_xor(n_split, d, 64); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_red[wave][0] = n_prune; s_red[wave][1] = n_split; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0u, b = 0u;
        for (int k = 0; k < 4; k++) { a += s_red[k][0]; b += s_red[k][1]; }
        if (a) atomicAdd(&counts[0], a);
        if (b) atomicAdd(&counts[1], b);
    }
}

}  // namespace envgs

using namespace envgs;

extern "C" {

int envgs_densify_stats(int64_t P, int32_t cols, const float *grad, const uint8_t *filter, const float *weight, const int32_t *radii,
                        float *xyz_gradient_accum, float *denom, float *max_radii2D, float *xyz_weight_accum, void *stream_)
{
    if (P < 0 || P >= (1ll << 31) || (cols != 2 && cols != 3)) return ENVGS_ERR_BAD_ARG;
    if (!grad || !filter || !xyz_gradient_accum || !denom || (weight && !xyz_weight_accum) || (radii && !max_radii2D)) return ENVGS_ERR_BAD_ARG;
    if (P == 0) return 0;
    const dim3 grid((unsigned)((P + 255) / 256));
    if (cols == 2)
        hipLaunchKernelGGL(densify_stats<2>, grid, dim3(256), 0, (hipStream_t)stream_, (long long)P, grad, filter, weight, radii,
                           xyz_gradient_accum, denom, max_radii2D, xyz_weight_accum);
    else
        hipLaunchKernelGGL(densify_stats<3>, grid, dim3(256), 0, (hipStream_t)stream_, (long long)P, grad, filter, weight, radii,
                           xyz_gradient_accum, denom, max_radii2D, xyz_weight_accum);
    return (int)hipGetLastError();
}

static bool grow_size_ok(int64_t P, int32_t N) { return P >= 0 && N >= 1 && N <= ENVGS_GROW_MAX_CHILDREN && P * 6 < (1ll << 31); }

size_t envgs_densify_plan_temp_bytes(int64_t P) { return scan_temp_bytes((int)(P > 0 && P * 6 < (1ll << 31) ? P * 6 : 1)); }

int envgs_densify_plan(const envgs_densify_plan_args *a, void *stream_)
{
    if (!a || !grow_size_ok(a->P, a->N) || !a->counters) return ENVGS_ERR_BAD_ARG;
    if (a->P > 0 && (!a->ga || !a->dn || !a->mr || !a->wa || !a->scal || !a->cls || !a->scan || !a->temp)) return ENVGS_ERR_BAD_ARG;
    if ((a->flags & ENVGS_PLAN_MIN_OPACITY) && a->P > 0 && !a->opac) return ENVGS_ERR_BAD_ARG;
    if (a->P > 0 && a->temp_bytes < envgs_densify_plan_temp_bytes(a->P)) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    hipError_t e = hipMemsetAsync(a->counters, 0, sizeof(uint32_t) * ENVGS_GROW_COUNTERS, stream);
    if (e != hipSuccess || a->P == 0) return (int)e;
    hipLaunchKernelGGL(grow_plan, dim3((unsigned)((a->P + 255) / 256)), dim3(256), 0, stream, *a);
    const int rc = launch_scan(a->scan, a->scan, (int)(a->P * 6), a->temp, a->temp_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(grow_counters, dim3(1), dim3(64), 0, stream, (long long)a->P, a->scan, a->counters);
    return (int)hipGetLastError();
}

int envgs_densify_split_stds(int64_t P, int32_t N, const uint8_t *cls, const uint32_t *scan, const uint32_t *counters, const float *scal,
                             float *stds, int64_t n_stds, void *stream_)
{
    if (!grow_size_ok(P, N) || n_stds < 0) return ENVGS_ERR_BAD_ARG;
    if (P == 0 || n_stds == 0) return 0;
    if (!cls || !scan || !counters || !scal || !stds) return ENVGS_ERR_BAD_ARG;
    hipLaunchKernelGGL(grow_stds, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, (long long)P, (int)N, cls, scan, counters,
                       scal, stds, (long long)n_stds);
    return (int)hipGetLastError();
}

int envgs_densify_rewrite(const envgs_densify_rewrite_args *a, void *stream_)
{
    if (!a || !grow_size_ok(a->P, a->N) || a->count < 0 || a->count > ENVGS_COMPACT_MAX_TENSORS || (a->count > 0 && !a->tensors)) return ENVGS_ERR_BAD_ARG;
    if (!(a->ratio_n > 0.0) || a->out_rows < 0 || a->n_samples < 0) return ENVGS_ERR_BAD_ARG;
    if (a->P == 0 || a->count == 0 || a->out_rows == 0) return 0;
    if (!a->cls || !a->scan || !a->counters) return ENVGS_ERR_BAD_ARG;
    GrowBatch B;
    B.count = 0;
    long long chunks = 0;
    for (int i = 0; i < a->count; i++) {
        const envgs_grow_tensor &t = a->tensors[i];
        if (t.row_bytes <= 0) continue;
        if ((t.row_bytes & 3) || !t.src || !t.dst || t.kind < ENVGS_GROW_COPY || t.kind > ENVGS_GROW_WEIGHT) return ENVGS_ERR_BAD_ARG;
        if (t.kind == ENVGS_GROW_XYZ && (t.row_bytes != 12 || !a->rotation || (a->n_samples > 0 && !a->samples))) return ENVGS_ERR_BAD_ARG;
        if (t.kind == ENVGS_GROW_SCALING && (t.row_bytes != 8 || !a->scal)) return ENVGS_ERR_BAD_ARG;
        if (t.kind >= ENVGS_GROW_GRAD && t.row_bytes != 4) return ENVGS_ERR_BAD_ARG;
        B.t[B.count] = t;
        B.chunk_start[B.count] = chunks;
        chunks += ((long long)a->P * (t.row_bytes >> 2) + 255) / 256;
        B.count++;
    }
    B.chunk_start[B.count] = chunks;
    if (chunks == 0) return 0;
    if (chunks >= (1ll << 31)) return ENVGS_ERR_BAD_ARG;
    GrowCommon C;
    C.P = a->P; C.out_rows = a->out_rows; C.n_samples = a->n_samples; C.N = a->N; C.r = a->r; C.ratio_n = a->ratio_n;
    C.cls = a->cls; C.scan = a->scan; C.counters = a->counters;
    C.scal = a->scal; C.rotation = a->rotation; C.samples = a->samples;
    hipLaunchKernelGGL(grow_rewrite, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream_, B, C);
    return (int)hipGetLastError();
}

size_t envgs_weight_select_temp_bytes(void) { return radix_select_temp_bytes(); }

int envgs_weight_select(int64_t P, const float *wa, const float *dn, int32_t n_ranks, int64_t rank0, int64_t rank1, float *values, uint32_t *below,
                        void *temp, size_t temp_bytes, void *stream_)
{
    if (P < 1 || P >= (1ll << 31) || (n_ranks != 1 && n_ranks != 2) || !wa || !dn || !values || !below || !temp) return ENVGS_ERR_BAD_ARG;
    if (n_ranks == 1) rank1 = rank0;
    if (rank0 < 0 || rank0 >= P || rank1 < 0 || rank1 >= P) return ENVGS_ERR_BAD_ARG;
    if (temp_bytes < envgs_weight_select_temp_bytes()) return ENVGS_ERR_TEMP_TOO_SMALL;
    return radix_select((long long)P, WeightKeys{wa, dn}, (uint32_t)rank0, (uint32_t)rank1, (int)n_ranks, values, below, temp, (hipStream_t)stream_);
}

static size_t tie_flag_bytes(int64_t P) { return ((size_t)(P > 0 ? P : 1) * sizeof(uint32_t) + 255) & ~(size_t)255; }

size_t envgs_visibility_mask_temp_bytes(int64_t P)
{
    const int64_t n = P > 0 && P < (1ll << 31) ? P : 1;
    return tie_flag_bytes(n) + scan_temp_bytes((int)n);
}

int envgs_visibility_mask(int64_t P, const float *wa, const float *dn, int64_t n_prune, const float *cut, const uint32_t *cut_below, uint8_t *keep,
                          void *temp, size_t temp_bytes, void *stream_)
{
    if (P < 1 || P >= (1ll << 31) || n_prune < 1 || n_prune > P || !wa || !dn || !cut || !cut_below || !keep || !temp) return ENVGS_ERR_BAD_ARG;
    if (temp_bytes < envgs_visibility_mask_temp_bytes(P)) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t s = (hipStream_t)stream_;
    uint32_t *flags = (uint32_t *)temp;
    const size_t fb = tie_flag_bytes(P);
    const dim3 grid((unsigned)((P + 255) / 256));
    hipLaunchKernelGGL(tie_flags, grid, dim3(256), 0, s, (long long)P, wa, dn, cut, flags);
    const int rc = launch_scan(flags, flags, (int)P, (char *)temp + fb, temp_bytes - fb, s);
    if (rc) return rc;
    hipLaunchKernelGGL(visibility_mask, grid, dim3(256), 0, s, (long long)P, wa, dn, cut, cut_below, (uint32_t)n_prune, flags, keep);
    return (int)hipGetLastError();
}

int envgs_oversize_plan(int64_t P, uint32_t flags, float max_screen, float scene_limit, const float *mr, const float *scal, const float *wa,
                        const float *dn, const float *quantile, uint8_t *keep, uint32_t *split, uint32_t *counts, void *stream_)
{
    if (P < 0 || P >= (1ll << 31) || (flags & ~7u) || !counts) return ENVGS_ERR_BAD_ARG;
    if (P > 0 && (!keep || !split)) return ENVGS_ERR_BAD_ARG;
    if (P > 0 && (((flags & ENVGS_OVERSIZE_SCREEN) && !mr) || ((flags & ENVGS_OVERSIZE_SCENE) && !scal))) return ENVGS_ERR_BAD_ARG;
    if (P > 0 && (flags & ENVGS_OVERSIZE_WEIGHT) && (!wa || !dn || !quantile)) return ENVGS_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream_;
    hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s);
    if (e != hipSuccess || P == 0) return (int)e;
    hipLaunchKernelGGL(oversize_plan, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (long long)P, flags, max_screen, scene_limit, mr, scal, wa, dn,
                       quantile, keep, split, counts);
    return (int)hipGetLastError();
}

}  // extern "C"
