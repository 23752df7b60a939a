// visualize.hip -- image output: the visualizer's maps as finished 8-bit RGBA on the device (include/envgs_visualize.h).
#include "common.h"
#include "radix_select.h"

#include "../../include/envgs_visualize.h"

// Compiled with -ffp-contract=off (envgs_amd/build.py): every product, sum, quotient and square root below rounds once, in the order written,
// which is the order of the reference's float32 tensor expressions and of tests/visualize_oracle.py.  A byte is a rounding decision at k + 0.5:
// one fused multiply-add that the oracle does not make moves values across it.
namespace envgs {

// ---- depth range: radix_select.h over the canonical key of a strided depth read -------------------------------------------------------------
struct ImageDepthKeys {
    const float *depth;
    long long sy, sx;
    int W;
    __device__ __forceinline__ uint32_t operator()(long long i) const
    {
        const long long y = i / W, x = i - y * W;
        return float_key_canon(depth[y * sy + x * sx]);
    }
};

// ---- the planes ------------------------------------------------------------------------------------------------------------------------------
struct VisMap {                    // envgs_vis_map in 32 bytes: sixteen planes of five maps fit the kernel's argument block
    const void *p;
    int64_t sb, sy;
    int32_t sc, sx;
};

struct VisPlane {
    VisMap img, weight, acc, gt, msk;
    const float *M, *near_far, *table;
    float bg[3];
    float dpt_mult;
    int32_t table_k;
    uint8_t kind, weight_mode, curve, gt_u8, opaque, has_bg, pad0, pad1;
};

struct VisArgs { VisPlane pl[ENVGS_VIS_MAX_PLANES]; };
static_assert(sizeof(VisArgs) <= 3584, "the planes travel in the kernel's argument block (4 KiB)");

__device__ __forceinline__ int64_t vis_off(const VisMap &m, int b, int c, int y, int x)
{
    return (int64_t)b * m.sb + (int64_t)c * m.sc + (int64_t)y * m.sy + (int64_t)x * m.sx;
}
__device__ __forceinline__ float vis_ld(const VisMap &m, int b, int c, int y, int x) { return ((const float *)m.p)[vis_off(m, b, c, y, x)]; }

// torch.clip: a NaN stays a NaN (both compares are false)
__device__ __forceinline__ float clip_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// save_image: (img * 255).clip(0, 255).round().astype(uint8); NaN -> 0
__device__ __forceinline__ uint32_t to_byte(float v)
{
    const float s = clip_keep_nan(v * 255.0f, 0.0f, 255.0f);
    return s == s ? (uint32_t)rintf(s) : 0u;
}

__device__ __forceinline__ void load_color(const VisPlane &p, int b, int y, int x, float c[3])
{
    if (p.kind == ENVGS_VIS_GRAY) {
        c[0] = c[1] = c[2] = vis_ld(p.img, b, 0, y, x);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = vis_ld(p.img, b, k, y, x);
    if (p.weight_mode == ENVGS_VIS_WEIGHT_ONE_MINUS) {
        const float om = 1.0f - vis_ld(p.weight, b, 0, y, x);
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = c[k] * om;
    } else if (p.weight_mode == ENVGS_VIS_WEIGHT_TWICE) {
        const float w = vis_ld(p.weight, b, 0, y, x);
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = (c[k] * w) * 2.0f;
    }
}

__device__ __forceinline__ void load_gt(const VisPlane &p, int b, int y, int x, float g[3])
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int64_t o = vis_off(p.gt, b, k, y, x);
        g[k] = p.gt_u8 ? (float)((const uint8_t *)p.gt.p)[o] / 255.0f : ((const float *)p.gt.p)[o];
    }
    if (p.has_bg && p.msk.p) {
        const float om = 1.0f - vis_ld(p.msk, b, 0, y, x);
#pragma unroll
        for (int k = 0; k < 3; k++) g[k] = g[k] + p.bg[k] * om;
    }
}

// colormap_list over the candidate segments (see the header); v is not a NaN and lies in [1e-6, 1 - 1e-6]
__device__ __forceinline__ void table_color(const float *__restrict__ table, int K, float v, float c[3])
{
    c[0] = c[1] = c[2] = 0.0f;
    const double km1 = (double)(K - 1);
    int i0 = (int)floorf(v * (float)(K - 1));
    i0 = i0 < 0 ? 0 : (i0 > K - 2 ? K - 2 : i0);
    for (int i = i0 - 1; i <= i0 + 1; i++) {
        if (i < 0 || i > K - 2) continue;
        const double b0d = (double)i / km1, b1d = (double)(i + 1) / km1;
        const float b0 = (float)b0d, db = (float)(b1d - b0d);
        const float t = (v - b0) / db;
        if (t >= 0.0f && t <= 1.0f) {
            const float om = 1.0f - t;
#pragma unroll
            for (int k = 0; k < 3; k++) c[k] = c[k] + (table[3 * (i + 1) + k] * t + table[3 * i + k] * om);
        }
    }
}

// grid: x over the Ho * Wo pixels of the canvas, y the image, z the plane; block g of x covers pixels 256 g .. 256 g + 255
__global__ void __launch_bounds__(256)
visualize_planes(const VisArgs args, const int H, const int W, const int Ho, const int Wo, const int x0, const int y0, uint32_t *__restrict__ out)
{
    const unsigned pix = blockIdx.x * 256u + threadIdx.x, npix = (unsigned)Ho * (unsigned)Wo;
    if (pix >= npix) return;
    const int b = (int)blockIdx.y, t = (int)blockIdx.z, B = (int)gridDim.y;
    const VisPlane &p = args.pl[t];
    const int yo = (int)(pix / (unsigned)Wo), xo = (int)(pix - (unsigned)yo * (unsigned)Wo);
    const int y = yo - y0, x = xo - x0;
    uint32_t word = 0u;                                   // outside the crop: four zero bytes
    if (y >= 0 && y < H && x >= 0 && x < W) {
        float c[3];
        float a = 1.0f;
        bool has_a = false;
        switch (p.kind) {
        case ENVGS_VIS_COLOR:
        case ENVGS_VIS_GRAY:
            load_color(p, b, y, x, c);
            if (p.acc.p) { a = vis_ld(p.acc, b, 0, y, x); has_a = true; }
            break;
        case ENVGS_VIS_DEPTH: {
            const float d = vis_ld(p.img, b, 0, y, x);
            if (p.curve == ENVGS_VIS_CURVE_NORMALIZE) {
                const float near = p.near_far[2 * b], far = p.near_far[2 * b + 1];
                float v;
                if (far <= near) v = d <= near ? 1.0f : 0.0f;
                else v = clip_keep_nan(1.0f - (d - near) / (far - near), 0.0f, 1.0f);
                v = clip_keep_nan(v, 1e-6f, (float)(1.0 - 1e-6));
                if (p.table && v == v) table_color(p.table, p.table_k, v, c);
                else c[0] = c[1] = c[2] = v;
            } else {
                c[0] = c[1] = c[2] = d;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) c[k] = c[k] * p.dpt_mult;
            if (p.acc.p) { a = vis_ld(p.acc, b, 0, y, x); has_a = true; }
            break;
        }
        case ENVGS_VIS_NORMAL: {
            float n[3], m[3];
#pragma unroll
            for (int k = 0; k < 3; k++) n[k] = vis_ld(p.img, b, k, y, x);
            const float s = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) + 1e-8f;
#pragma unroll
            for (int k = 0; k < 3; k++) n[k] = n[k] / s;
            if (p.M) {
                const float *M = p.M + 9 * (size_t)b;
#pragma unroll
                for (int j = 0; j < 3; j++) m[j] = (n[0] * M[3 * j] + n[1] * M[3 * j + 1]) + n[2] * M[3 * j + 2];
            } else {
                m[0] = n[0]; m[1] = n[1]; m[2] = n[2];
            }
            m[1] = -m[1]; m[2] = -m[2];
#pragma unroll
            for (int k = 0; k < 3; k++) c[k] = m[k] * 0.5f + 0.5f;
            if (p.acc.p) {
                a = vis_ld(p.acc, b, 0, y, x); has_a = true;
#pragma unroll
                for (int k = 0; k < 3; k++) c[k] = c[k] * a;
            }
            break;
        }
        case ENVGS_VIS_GT:
            load_gt(p, b, y, x, c);
            if (p.msk.p) { a = vis_ld(p.msk, b, 0, y, x); has_a = true; }
            break;
        default: {                                        // ENVGS_VIS_ERROR
            float g[3];
            load_color(p, b, y, x, c);
            load_gt(p, b, y, x, g);
            const float d0 = c[0] - g[0], d1 = c[1] - g[1], d2 = c[2] - g[2];
            c[0] = c[1] = c[2] = clip_keep_nan((d0 * d0 + d1 * d1) + d2 * d2, 0.0f, 1.0f);
            if (p.msk.p && p.acc.p) { a = clip_keep_nan(vis_ld(p.msk, b, 0, y, x) + vis_ld(p.acc, b, 0, y, x), 0.0f, 1.0f); has_a = true; }
            break;
        }
        }
        const uint32_t ab = (has_a && !p.opaque) ? to_byte(a) : 255u;
        word = to_byte(c[0]) | (to_byte(c[1]) << 8) | (to_byte(c[2]) << 16) | (ab << 24);
    }
    out[((size_t)t * (size_t)B + (size_t)b) * (size_t)npix + pix] = word;
}

static bool pack_map(const envgs_vis_map &m, VisMap *o)
{
    o->p = m.ptr;
    if (!m.ptr) { o->sb = o->sy = 0; o->sc = o->sx = 0; return true; }
    if (m.stride[1] > INT32_MAX || m.stride[1] < INT32_MIN || m.stride[3] > INT32_MAX || m.stride[3] < INT32_MIN) return false;
    o->sb = m.stride[0]; o->sc = (int32_t)m.stride[1]; o->sy = m.stride[2]; o->sx = (int32_t)m.stride[3];
    return true;
}

static bool pack_plane(const envgs_vis_plane &h, VisPlane *k)
{
    if (h.kind < ENVGS_VIS_COLOR || h.kind > ENVGS_VIS_ERROR) return false;
    if (h.weight_mode < ENVGS_VIS_WEIGHT_NONE || h.weight_mode > ENVGS_VIS_WEIGHT_TWICE) return false;
    if (h.curve != ENVGS_VIS_CURVE_LINEAR && h.curve != ENVGS_VIS_CURVE_NORMALIZE) return false;
    if (h.gt_dtype != ENVGS_VIS_GT_F32 && h.gt_dtype != ENVGS_VIS_GT_U8) return false;
    if (h.flags & ~(ENVGS_VIS_OPAQUE | ENVGS_VIS_BG)) return false;
    const bool colour = h.kind == ENVGS_VIS_COLOR || h.kind == ENVGS_VIS_ERROR;
    if (h.kind != ENVGS_VIS_GT && !h.img.ptr) return false;
    if ((h.kind == ENVGS_VIS_GT || h.kind == ENVGS_VIS_ERROR) && !h.gt.ptr) return false;
    if (h.weight_mode != ENVGS_VIS_WEIGHT_NONE && (!colour || !h.weight.ptr)) return false;
    const bool norm = h.kind == ENVGS_VIS_DEPTH && h.curve == ENVGS_VIS_CURVE_NORMALIZE;
    if (norm && !h.near_far) return false;
    if (norm && h.table && (h.table_k < 2 || h.table_k > ENVGS_VIS_MAX_TABLE)) return false;
    if (!pack_map(h.img, &k->img) || !pack_map(h.weight, &k->weight) || !pack_map(h.acc, &k->acc) || !pack_map(h.gt, &k->gt) || !pack_map(h.msk, &k->msk))
        return false;
    k->M = h.kind == ENVGS_VIS_NORMAL ? h.M : nullptr;
    k->near_far = norm ? h.near_far : nullptr;
    k->table = norm ? h.table : nullptr;
    k->table_k = h.table_k;
    k->bg[0] = h.bg[0]; k->bg[1] = h.bg[1]; k->bg[2] = h.bg[2];
    k->dpt_mult = h.dpt_mult;
    k->kind = (uint8_t)h.kind; k->weight_mode = (uint8_t)h.weight_mode; k->curve = (uint8_t)h.curve; k->gt_u8 = h.gt_dtype == ENVGS_VIS_GT_U8;
    k->opaque = (h.flags & ENVGS_VIS_OPAQUE) != 0; k->has_bg = (h.flags & ENVGS_VIS_BG) != 0; k->pad0 = k->pad1 = 0;
    return true;
}

}  // namespace envgs

using namespace envgs;

extern "C" {

size_t envgs_visualize_depth_range_temp_bytes(void) { return radix_select_temp_bytes(); }

int envgs_visualize_depth_range(int32_t B, int32_t H, int32_t W, const float *depth, const int64_t *strides, int64_t rank_near, int64_t rank_far,
                                float *near_far, void *temp, size_t temp_bytes, void *stream)
{
    if (B < 0 || H < 1 || W < 1) return ENVGS_ERR_BAD_ARG;
    const int64_t N = (int64_t)H * W;
    if (N >= (1ll << 31) || rank_near < 0 || rank_near >= N || rank_far < 0 || rank_far >= N) return ENVGS_ERR_BAD_ARG;
    if (B == 0) return 0;
    if (!depth || !strides || !near_far || !temp) return ENVGS_ERR_BAD_ARG;
    if (temp_bytes < radix_select_temp_bytes()) return ENVGS_ERR_TEMP_TOO_SMALL;
    for (int b = 0; b < B; b++) {                         // one select per image, one after the other on the stream: they share `temp`
        const ImageDepthKeys keys{depth + (int64_t)b * strides[0], (long long)strides[1], (long long)strides[2], W};
        const int rc = radix_select((long long)N, keys, (uint32_t)rank_near, (uint32_t)rank_far, 2, near_far + 2 * (size_t)b, nullptr, temp,
                                    (hipStream_t)stream);
        if (rc != 0) return rc;
    }
    return 0;
}

int envgs_visualize_planes(int32_t n_planes, const envgs_vis_plane *planes, int32_t B, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t x0,
                           int32_t y0, uint8_t *out, void *stream)
{
    if (n_planes < 0 || n_planes > ENVGS_VIS_MAX_PLANES || B < 0 || B > 65535 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return ENVGS_ERR_BAD_ARG;
    if (x0 < 0 || y0 < 0 || (int64_t)x0 + W > Wo || (int64_t)y0 + H > Ho || (int64_t)Ho * Wo >= (1ll << 31)) return ENVGS_ERR_BAD_ARG;
    if (n_planes == 0 || B == 0) return 0;
    if (!planes || !out || ((uintptr_t)out & 3u)) return ENVGS_ERR_BAD_ARG;
    VisArgs args{};
    for (int t = 0; t < n_planes; t++)
        if (!pack_plane(planes[t], &args.pl[t])) return ENVGS_ERR_BAD_ARG;
    const unsigned npix = (unsigned)Ho * (unsigned)Wo;
    const dim3 grid((npix + 255u) / 256u, (unsigned)B, (unsigned)n_planes);
    hipLaunchKernelGGL(visualize_planes, grid, dim3(256), 0, (hipStream_t)stream, args, H, W, Ho, Wo, x0, y0, (uint32_t *)out);
    return (int)hipGetLastError();
}

}  // extern "C"
