// mesh_raster.h -- the rasterisation rule of include/envgs_mesh.h ("rasterisation") as functions for host and device: vertex projection and
// snapping, face set-up, the coverage test, the depth key and the attributes of a winner.  mesh_raster.hip rasterises with it, and a stand-alone
// host program (mesh_raster_host.cpp; built and run by tests/test_mesh_raster_cpu.py with -ffp-contract=off) runs it face by face on the CPU for
// the test against the NumPy oracle: one text, so the arithmetic of the kernels is checked without a GPU.
//
// Every float expression is written operation by operation; both users compile without contraction.  Edge arithmetic is int64: |X|, |Y| < 2^29 + 1
// and the pixel centres lie inside the same range wherever a conservative box leaves them, so a difference stays below 2^31, a product below 2^62
// and E_k, A below 2^63.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/envgs_mesh.h"

#if defined(__HIPCC__)
#define ENVGS_MR_FN __host__ __device__ __forceinline__
#else
#define ENVGS_MR_FN inline
#endif

namespace envgs {

constexpr int MR_SUB = 256;                                      // sub-pixel steps per pixel
constexpr int MR_HALF = 128;
constexpr float MR_LIMIT = 2097152.f;                            // 2^21 pixels
constexpr uint64_t MR_EMPTY = ~0ull;                             // the key of a pixel no face covers

struct MrVertex {
    int32_t X, Y;
    float zc;
    bool usable;
};

struct MrFace {                                                  // corners in the possibly exchanged order
    int32_t X[3], Y[3];
    float zc[3];
    int64_t A;                                                   // > 0
    bool exchanged;                                              // A < 0 before the exchange: corners 1 and 2 swapped
};

ENVGS_MR_FN uint32_t mr_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

ENVGS_MR_FN float mr_float(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

ENVGS_MR_FN bool mr_finite(float f) { return (mr_bits(f) & 0x7f800000u) != 0x7f800000u; }

ENVGS_MR_FN MrVertex mr_project(const envgs_mesh_raster_view &C, const float x, const float y, const float z, const float near)
{
    MrVertex r;
    const float xc = C.R[0] * x + C.R[1] * y + C.R[2] * z + C.T[0];
    const float yc = C.R[3] * x + C.R[4] * y + C.R[5] * z + C.T[1];
    const float zc = C.R[6] * x + C.R[7] * y + C.R[8] * z + C.T[2];
    const float u = C.fx * (xc / zc) + C.cx, v = C.fy * (yc / zc) + C.cy;
    r.zc = zc;
    r.usable = mr_finite(u) && mr_finite(v) && zc > near && fabsf(u) < MR_LIMIT && fabsf(v) < MR_LIMIT;
    r.X = r.usable ? (int32_t)rintf(u * (float)MR_SUB) : 0;     // |u * 256| < 2^29: the conversion is exact
    r.Y = r.usable ? (int32_t)rintf(v * (float)MR_SUB) : 0;
    return r;
}

// false: the face is dropped (a corner not usable, or zero area)
ENVGS_MR_FN bool mr_setup(const MrVertex &a, const MrVertex &b, const MrVertex &c, MrFace &f)
{
    if (!(a.usable && b.usable && c.usable)) return false;
    const int64_t A = ((int64_t)b.X - a.X) * ((int64_t)c.Y - a.Y) - ((int64_t)b.Y - a.Y) * ((int64_t)c.X - a.X);
    if (A == 0) return false;
    f.exchanged = A < 0;
    const MrVertex &p = f.exchanged ? c : b, &q = f.exchanged ? b : c;
    f.X[0] = a.X; f.Y[0] = a.Y; f.zc[0] = a.zc;
    f.X[1] = p.X; f.Y[1] = p.Y; f.zc[1] = p.zc;
    f.X[2] = q.X; f.Y[2] = q.Y; f.zc[2] = q.zc;
    f.A = f.exchanged ? -A : A;
    return true;
}

// the three edge functions at the centre of pixel (px, py) and the top-left rule
ENVGS_MR_FN bool mr_covers(const MrFace &f, const int32_t px, const int32_t py, int64_t (&E)[3])
{
    const int64_t Px = (int64_t)MR_SUB * px + MR_HALF, Py = (int64_t)MR_SUB * py + MR_HALF;
    bool in = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; k++) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const int64_t dx = (int64_t)f.X[j] - f.X[i], dy = (int64_t)f.Y[j] - f.Y[i];
        E[k] = dx * (Py - f.Y[i]) - dy * (Px - f.X[i]);
        in = in && (E[k] > 0 || (E[k] == 0 && (dy < 0 || (dy == 0 && dx > 0))));
    }
    return in;
}

// the three terms l_k iz_k and their sum s, in double
ENVGS_MR_FN double mr_terms(const MrFace &f, const int64_t (&E)[3], double (&t)[3])
{
    const double A = (double)f.A;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 3; k++) {
        const double l = (double)E[k] / A;
        const double iz = 1.0 / (double)f.zc[k];
        t[k] = l * iz;
    }
    return (t[0] + t[1]) + t[2];
}

ENVGS_MR_FN float mr_depth(const MrFace &f, const int64_t (&E)[3])
{
    double t[3];
    const double s = mr_terms(f, E, t);
    return (float)(1.0 / s);
}

ENVGS_MR_FN uint64_t mr_key(const float z, const uint32_t face) { return ((uint64_t)mr_bits(z) << 32) | face; }

// The pixels whose centre can lie inside [lo, hi] sub-pixel units along one axis of n pixels: first .. last, empty if first > last.
ENVGS_MR_FN void mr_span(const int32_t lo, const int32_t hi, const int32_t n, int32_t &first, int32_t &last)
{
    const int32_t a = (lo - MR_HALF + (MR_SUB - 1)) >> 8, b = (hi - MR_HALF) >> 8;      // ceil and floor: the shift of a negative number rounds down
    first = a < 0 ? 0 : a;
    last = b > n - 1 ? n - 1 : b;
}

ENVGS_MR_FN int32_t mr_min3(const int32_t a, const int32_t b, const int32_t c) { const int32_t m = a < b ? a : b; return m < c ? m : c; }
ENVGS_MR_FN int32_t mr_max3(const int32_t a, const int32_t b, const int32_t c) { const int32_t m = a > b ? a : b; return m > c ? m : c; }

// the clamped bounding box of a face in pixels
ENVGS_MR_FN void mr_box(const MrFace &f, const int32_t H, const int32_t W, int32_t &x0, int32_t &x1, int32_t &y0, int32_t &y1)
{
    mr_span(mr_min3(f.X[0], f.X[1], f.X[2]), mr_max3(f.X[0], f.X[1], f.X[2]), W, x0, x1);
    mr_span(mr_min3(f.Y[0], f.Y[1], f.Y[2]), mr_max3(f.Y[0], f.Y[1], f.Y[2]), H, y0, y1);
}

// the unit normal of the original corners, oriented towards the camera
ENVGS_MR_FN void mr_normal(const float (&p0)[3], const float (&p1)[3], const float (&p2)[3], const bool exchanged, float (&n)[3])
{
    const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
    if (len == 0.f) { n[0] = n[1] = n[2] = 0.f; return; }
    n[0] = cx / len; n[1] = cy / len; n[2] = cz / len;
    if (!exchanged) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }                      // A > 0 before the exchange: the product faces away
}

}  // namespace envgs
