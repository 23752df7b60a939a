// supervisor.hip -- fused geometry regularisers of the EnvGS supervisor and the exact depth percentiles they scale with (include/envgs_supervisor.h).
#include "common.h"
#include "radix_select.h"

#include "../../include/envgs_supervisor.h"

namespace envgs {

// ---- exact depth percentiles: radix_select.h over the canonical key of a strided depth read ------------------------------------------------
struct DepthKeys {
    const float *depth;
    long long stride;
    __device__ __forceinline__ uint32_t operator()(long long i) const { return float_key_canon(depth[i * stride]); }
};

// ---- the per-pixel terms ----------------------------------------------------------------------------------------------------------------
constexpr int SUP_THREADS = 256;
constexpr float SUP_EPS = 1e-8f;

struct V3 { float x, y, z; };
__device__ __forceinline__ float dot3(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ V3 load3(const float *p, long long row, long long rs, long long cs)
{
    const float *q = p + row * rs;
    return V3{q[0], q[cs], q[2 * cs]};
}
// The scale of a normal term: acc, the depth scale, both or neither.
__device__ __forceinline__ float sd_select(uint32_t F, uint32_t acc_flag, uint32_t dpt_flag, float acc, float sd)
{
    return ((F & acc_flag) ? acc : 1.f) * ((F & dpt_flag) ? sd : 1.f);
}
__device__ __forceinline__ float sign_of(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// Adjoint of y = x / (|x| + eps) at x with r = |x|, inv = 1 / (r + eps): gy * inv - x/|x| * <gy, x> * inv^2; |x| has gradient 0 at 0.
__device__ __forceinline__ V3 unit_adjoint(V3 x, float r, float inv, V3 gy)
{
    const float k = r > 0.f ? dot3(gy, x) * inv * inv / r : 0.f;
    return V3{gy.x * inv - x.x * k, gy.y * inv - x.y * k, gy.z * inv - x.z * k};
}

// d norm_loss / d norm_map on a pixel with norm_map == 0, in double.  There a = 0, so sign(a - g) = -sign(g) and d cos / d a = gn / eps, and both
// unit() adjoints at 0 are gy / eps: the row is (R^T (-sign(g) - gn / eps)) * k / eps^2, about 1e24 k.  Float operands carry their half ulp each
// into the three-term sum R^T gb, and where its terms cancel (a gradient nearly orthogonal to a world axis) the element keeps few digits; with the
// chain in double the result is the float64 statement rounded once.  k = scale * weight / N.
__device__ __forceinline__ V3 zero_normal_adjoint(V3 p, const float *R, double k)
{
    constexpr double eps = 1e-8, inv = 1e8;       // 1 / (0 + eps) and 1 / max(0, eps)
    const double t[3] = {2.0 * (double)p.x - 1.0, 2.0 * (double)p.y - 1.0, 2.0 * (double)p.z - 1.0};
    const double it = 1.0 / (sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) + eps);
    const double g[3] = {t[0] * it, t[1] * it, t[2] * it};
    const double ing = 1.0 / fmax(sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), eps);
    double gb[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double sg = g[c] > 0. ? 1. : (g[c] < 0. ? -1. : 0.);
        gb[c] = (-sg - g[c] * ing * inv) * k * inv;
    }
    return V3{(float)(((double)R[0] * gb[0] + (double)R[3] * gb[1] + (double)R[6] * gb[2]) * inv),
              (float)(((double)R[1] * gb[0] + (double)R[4] * gb[1] + (double)R[7] * gb[2]) * inv),
              (float)(((double)R[2] * gb[0] + (double)R[5] * gb[1] + (double)R[8] * gb[2]) * inv)};
}

__global__ void __launch_bounds__(SUP_THREADS)
supervisor_fwd(const envgs_supervisor_args A, const int pixel_blocks)
{
    __shared__ float red[ENVGS_SUP_TERMS][SUP_THREADS / 64];
    const int tid = threadIdx.x;
    const uint32_t F = A.flags;
    float v[ENVGS_SUP_TERMS] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if ((int)blockIdx.x < pixel_blocks) {
        const long long i = (long long)blockIdx.x * SUP_THREADS + tid;
        if (i < A.N) {
            const float inv_n = 1.0f / (float)A.N;
            float acc = 0.f, sd = 1.f;
            if (F & (ENVGS_SUP_F_NORM_ACC | ENVGS_SUP_F_GS_NORM_ACC | ENVGS_SUP_F_MSK)) acc = A.acc_map[i * A.acc_map_row];
            if (F & (ENVGS_SUP_F_NORM_DPT | ENVGS_SUP_F_GS_NORM_DPT)) {
                const float near = A.near_far[0], far = A.near_far[1];
                sd = fminf(fmaxf(1.0f - (A.dpt_map[i * A.dpt_map_row] - near) / (far - near), 0.f), 1.f);
            }
            V3 x{0.f, 0.f, 0.f}, p{0.f, 0.f, 0.f}, gx{0.f, 0.f, 0.f};
            if (F & (ENVGS_SUP_F_NORM | ENVGS_SUP_F_GS_NORM)) x = load3(A.norm_map, i, A.norm_map_row, A.norm_map_ch);
            if (F & (ENVGS_SUP_F_NORM | ENVGS_SUP_F_MSK)) p = load3(A.prior, i, A.prior_row, A.prior_ch);
            if (F & ENVGS_SUP_F_NORM) {
                const float *R = A.R;
                const float r0 = sqrtf(dot3(x, x)), i0 = 1.0f / (r0 + SUP_EPS);
                const V3 a0{x.x * i0, x.y * i0, x.z * i0};
                const V3 b{dot3(V3{R[0], R[1], R[2]}, a0), dot3(V3{R[3], R[4], R[5]}, a0), dot3(V3{R[6], R[7], R[8]}, a0)};   // to view space
                const float r1 = sqrtf(dot3(b, b)), i1 = 1.0f / (r1 + SUP_EPS);
                const V3 a{b.x * i1, b.y * i1, b.z * i1};
                const V3 t{2.f * p.x - 1.f, 2.f * p.y - 1.f, 2.f * p.z - 1.f};
                const float it = 1.0f / (sqrtf(dot3(t, t)) + SUP_EPS);
                const V3 g{t.x * it, t.y * it, t.z * it};
                const float ra = sqrtf(dot3(a, a)), ina = 1.0f / fmaxf(ra, SUP_EPS), ing = 1.0f / fmaxf(sqrtf(dot3(g, g)), SUP_EPS);
                const V3 gn{g.x * ing, g.y * ing, g.z * ing};
                const float agn = dot3(a, gn), c = agn * ina;
                const float s = sd_select(F, ENVGS_SUP_F_NORM_ACC, ENVGS_SUP_F_NORM_DPT, acc, sd);
                v[ENVGS_SUP_NORM] = s * (fabsf(a.x - g.x) + fabsf(a.y - g.y) + fabsf(a.z - g.z) + 1.0f - c);
                if (A.g_norm_map && r0 == 0.f) {
                    // background: the 1e24-fold amplified row, its scale included, in double
                    double sc = (F & ENVGS_SUP_F_NORM_ACC) ? (double)acc : 1.0;
                    if (F & ENVGS_SUP_F_NORM_DPT) {
                        const double near = (double)A.near_far[0], far = (double)A.near_far[1];
                        sc *= fmin(fmax(1.0 - ((double)A.dpt_map[i * A.dpt_map_row] - near) / (far - near), 0.0), 1.0);
                    }
                    gx = zero_normal_adjoint(p, R, sc * (double)A.weight[ENVGS_SUP_NORM] / (double)A.N);
                } else if (A.g_norm_map) {
                    // d cos / d a = gn / na - a/|a| * <a, gn> / na^2 (the clamp in na = max(|a|, eps) is a constant)
                    const float k = s * A.weight[ENVGS_SUP_NORM] * inv_n, q = ra > 0.f ? agn * ina * ina / ra : 0.f;
                    const V3 ga{(sign_of(a.x - g.x) - (gn.x * ina - a.x * q)) * k, (sign_of(a.y - g.y) - (gn.y * ina - a.y * q)) * k,
                                (sign_of(a.z - g.z) - (gn.z * ina - a.z * q)) * k};
                    const V3 gb = unit_adjoint(b, r1, i1, ga);
                    const V3 ga0{dot3(V3{R[0], R[3], R[6]}, gb), dot3(V3{R[1], R[4], R[7]}, gb), dot3(V3{R[2], R[5], R[8]}, gb)};
                    gx = unit_adjoint(x, r0, i0, ga0);
                }
            }
            if (F & ENVGS_SUP_F_GS_NORM) {
                const V3 sn = load3(A.surf_norm_map, i, A.surf_norm_map_row, A.surf_norm_map_ch);
                const float s = sd_select(F, ENVGS_SUP_F_GS_NORM_ACC, ENVGS_SUP_F_GS_NORM_DPT, acc, sd);
                v[ENVGS_SUP_GS_NORM] = s * (1.0f - dot3(x, sn));
                const float k = s * A.weight[ENVGS_SUP_GS_NORM] * inv_n;
                gx.x -= k * sn.x; gx.y -= k * sn.y; gx.z -= k * sn.z;
                if (A.g_surf_norm_map) {
                    float *o = A.g_surf_norm_map + 3 * i;
                    o[0] = -k * x.x; o[1] = -k * x.y; o[2] = -k * x.z;
                }
            }
            if (A.g_norm_map) {
                float *o = A.g_norm_map + 3 * i;
                o[0] = gx.x; o[1] = gx.y; o[2] = gx.z;
            }
            if (F & ENVGS_SUP_F_MSK) {
                const float m = (A.msk[i * A.msk_row] > 0.5f && sqrtf(dot3(p, p)) > 0.25f) ? 1.f : 0.f, e = acc - m;
                v[ENVGS_SUP_MSK] = e * e;
                if (A.g_acc_map) A.g_acc_map[i] = 2.0f * e * A.weight[ENVGS_SUP_MSK] * inv_n;
            }
            if (F & ENVGS_SUP_F_DIST) {
                v[ENVGS_SUP_DIST] = A.dist_map[i * A.dist_map_row];
                if (A.g_dist_map) A.g_dist_map[i] = A.weight[ENVGS_SUP_DIST] * inv_n;
            }
        }
    } else {
        const long long j = (long long)((int)blockIdx.x - pixel_blocks) * SUP_THREADS + tid;
        if (j < A.P) {
            const float o = A.env_opacity[j * A.env_opacity_row], k = A.weight[ENVGS_SUP_ENV] / (float)A.P;
            float g;
            if (F & ENVGS_SUP_F_ENV_SPARSE) {
                constexpr float lo = 1e-3f, hi = (float)(1.0 - 1e-3);
                const float c = fminf(fmaxf(o, lo), hi);
                v[ENVGS_SUP_ENV] = logf(c) + logf(1.0f - c);
                // the clamp passes the gradient on [1e-3, 1 - 1e-3]: the bounds as the reference's double scalars, not their float images
                // (float(0.999) lies above 0.999)
                const bool inside = (double)o >= 1e-3 && (double)o <= 1.0 - 1e-3;
                g = inside ? (1.0f / c - 1.0f / (1.0f - c)) * k : 0.f;
            } else {
                v[ENVGS_SUP_ENV] = fabsf(1.0f - o);
                g = -sign_of(1.0f - o) * k;
            }
            if (A.g_env_opacity) A.g_env_opacity[j] = g;
        }
    }
    // per-workgroup sums (DPP inside the wave, four waves through LDS); the caller adds the rows in double
#pragma unroll
    for (int t = 0; t < ENVGS_SUP_TERMS; t++) {
        const float w = wave_sum(v[t]);
        if ((tid & 63) == 0) red[t][tid >> 6] = w;
    }
    __syncthreads();
    if (tid < ENVGS_SUP_TERMS) A.partial[(size_t)blockIdx.x * ENVGS_SUP_TERMS + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

__global__ void __launch_bounds__(SUP_THREADS)
supervisor_finish(const envgs_supervisor_args A, const long long rows, float *__restrict__ out)
{
    __shared__ double red[ENVGS_SUP_TERMS][SUP_THREADS];
    const int tid = threadIdx.x;
    double s[ENVGS_SUP_TERMS] = {0., 0., 0., 0., 0.};
    for (long long r = tid; r < rows; r += SUP_THREADS)
#pragma unroll
        for (int t = 0; t < ENVGS_SUP_TERMS; t++) s[t] += (double)A.partial[r * ENVGS_SUP_TERMS + t];
#pragma unroll
    for (int t = 0; t < ENVGS_SUP_TERMS; t++) red[t][tid] = s[t];
    __syncthreads();
    for (int off = SUP_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off)
#pragma unroll
            for (int t = 0; t < ENVGS_SUP_TERMS; t++) red[t][tid] += red[t][tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        double loss = 0.;
        for (int t = 0; t < ENVGS_SUP_TERMS; t++) {
            const double cnt = (double)(t == ENVGS_SUP_ENV ? A.P : A.N);
            const double mean = cnt > 0. ? red[t][0] / cnt : 0.;
            out[t] = (float)mean;
            loss += (double)A.weight[t] * mean;
        }
        out[ENVGS_SUP_TERMS] = (float)loss;
    }
}

__global__ void __launch_bounds__(256)
scale_by_scalar(const long long n, const float *__restrict__ src, const float *__restrict__ grad_out, float *__restrict__ dst)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = grad_out[0] * src[i];
}

static int check_args(const envgs_supervisor_args *a)
{
    if (!a || !a->partial) return ENVGS_ERR_BAD_ARG;
    const uint32_t F = a->flags;
    if ((F & ~ENVGS_SUP_F_ALL) || !(F & (ENVGS_SUP_F_NORM | ENVGS_SUP_F_GS_NORM | ENVGS_SUP_F_MSK | ENVGS_SUP_F_DIST | ENVGS_SUP_F_ENV_SPARSE | ENVGS_SUP_F_ENV_L1)))
        return ENVGS_ERR_BAD_ARG;
    if (a->N < 1 || a->N >= (1ll << 31) || a->P < 0 || a->P >= (1ll << 31)) return ENVGS_ERR_BAD_ARG;
    if ((F & ENVGS_SUP_F_ENV_SPARSE) && (F & ENVGS_SUP_F_ENV_L1)) return ENVGS_ERR_BAD_ARG;
    const bool env = F & (ENVGS_SUP_F_ENV_SPARSE | ENVGS_SUP_F_ENV_L1);
    if (env ? (a->P < 1 || !a->env_opacity) : a->P != 0) return ENVGS_ERR_BAD_ARG;
    if ((F & ENVGS_SUP_F_NORM) && (!a->norm_map || !a->prior || !a->R)) return ENVGS_ERR_BAD_ARG;
    if ((F & ENVGS_SUP_F_GS_NORM) && (!a->norm_map || !a->surf_norm_map)) return ENVGS_ERR_BAD_ARG;
    if ((F & ENVGS_SUP_F_MSK) && (!a->acc_map || !a->msk || !a->prior)) return ENVGS_ERR_BAD_ARG;
    if ((F & ENVGS_SUP_F_DIST) && !a->dist_map) return ENVGS_ERR_BAD_ARG;
    if ((F & (ENVGS_SUP_F_NORM_ACC | ENVGS_SUP_F_GS_NORM_ACC)) && !a->acc_map) return ENVGS_ERR_BAD_ARG;
    if ((F & (ENVGS_SUP_F_NORM_DPT | ENVGS_SUP_F_GS_NORM_DPT)) && (!a->dpt_map || !a->near_far || a->N < 100)) return ENVGS_ERR_BAD_ARG;
    // a gradient map of an input no selected term reads would stay unwritten
    if (a->g_norm_map && !(F & (ENVGS_SUP_F_NORM | ENVGS_SUP_F_GS_NORM))) return ENVGS_ERR_BAD_ARG;
    if (a->g_surf_norm_map && !(F & ENVGS_SUP_F_GS_NORM)) return ENVGS_ERR_BAD_ARG;
    if (a->g_acc_map && !(F & ENVGS_SUP_F_MSK)) return ENVGS_ERR_BAD_ARG;
    if (a->g_dist_map && !(F & ENVGS_SUP_F_DIST)) return ENVGS_ERR_BAD_ARG;
    if (a->g_env_opacity && !env) return ENVGS_ERR_BAD_ARG;
    return 0;
}

static int pixel_block_count(int64_t N) { return (int)((N + SUP_THREADS - 1) / SUP_THREADS); }

}  // namespace envgs

using namespace envgs;

extern "C" {

size_t envgs_depth_percentiles_temp_bytes(void) { return radix_select_temp_bytes(); }

int envgs_depth_percentiles(int64_t N, const float *depth, int64_t stride, float *near_far, void *temp, size_t temp_bytes, void *stream)
{
    if (N < 100 || N >= (1ll << 31) || !depth || !near_far || !temp) return ENVGS_ERR_BAD_ARG;
    if (temp_bytes < envgs_depth_percentiles_temp_bytes()) return ENVGS_ERR_TEMP_TOO_SMALL;
    const uint32_t n = (uint32_t)(N / 100);           // the n-th smallest and the n-th largest depth
    return radix_select((long long)N, DepthKeys{depth, (long long)stride}, n - 1u, (uint32_t)N - n, 2, near_far, nullptr, temp, (hipStream_t)stream);
}

int64_t envgs_supervisor_partial_count(int64_t N, int64_t P)
{
    if (N < 1 || N >= (1ll << 31) || P < 0 || P >= (1ll << 31)) return 0;
    return (int64_t)pixel_block_count(N) + pixel_block_count(P);
}

int envgs_supervisor_forward(const envgs_supervisor_args *args, void *stream)
{
    const int rc = check_args(args);
    if (rc) return rc;
    const int pb = pixel_block_count(args->N), eb = pixel_block_count(args->P);
    hipLaunchKernelGGL(supervisor_fwd, dim3(pb + eb), dim3(SUP_THREADS), 0, (hipStream_t)stream, *args, pb);
    return (int)hipGetLastError();
}

int envgs_supervisor_finish(const envgs_supervisor_args *args, float *out, void *stream)
{
    const int rc = check_args(args);
    if (rc) return rc;
    if (!out) return ENVGS_ERR_BAD_ARG;
    const long long rows = (long long)pixel_block_count(args->N) + pixel_block_count(args->P);
    hipLaunchKernelGGL(supervisor_finish, dim3(1), dim3(SUP_THREADS), 0, (hipStream_t)stream, *args, rows, out);
    return (int)hipGetLastError();
}

int envgs_supervisor_backward(int64_t n, const float *src, const float *grad_out, float *dst, void *stream)
{
    if (n < 1 || n >= (1ll << 38) || !src || !grad_out || !dst) return ENVGS_ERR_BAD_ARG;
    hipLaunchKernelGGL(scale_by_scalar, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)n, src, grad_out, dst);
    return (int)hipGetLastError();
}

}  // extern "C"
