// mesh_points.h -- the device functions that the point-cloud kernels of mesh_eval.hip and mesh_register.hip share (include/envgs_mesh.h,
// "evaluation" and "registration"): the cell of a point, the shell walk of the exact nearest-point search, and the fp32 rigid transformation.
// Both files are built with -ffp-contract=off (build.py), so one text gives one sequence of fp32 operations in every kernel that calls it: the
// nearest point the registration matches is the one envgs_points_nearest reports, and the row it transforms is the one envgs_points_transform
// writes.
#pragma once
#include "common.h"

namespace envgs {

struct Grid { float o[3]; float cell; int32_t n[3]; };

__device__ __forceinline__ bool ev_finite(const float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// rule 1 of the simplification on one axis; the caller has checked that x is finite
__device__ __forceinline__ int32_t pg_axis(const float x, const float o, const float cell, const int32_t n)
{
    const float fl = floorf((x - o) / cell);
    return !(fl >= 1.0f) ? 0 : (fl >= 2147483648.0f ? n - 1 : min((int32_t)fl, n - 1));
}

constexpr float POS_ONE = 1048576.0f, POS_STEP = 1.0f / 1048576.0f;      // 2^20: the fixed-point step of rule 3 of the simplification

// rule 1 and the offset of rule 3 of the simplification on one axis; the caller has checked that x is finite
__device__ __forceinline__ void sc_locate(const float x, const float o, const float cell, const int32_t n, int32_t &i, uint32_t &q)
{
    const float u = (x - o) / cell;
    const float fl = floorf(u);
    i = !(fl >= 1.0f) ? 0 : (fl >= 2147483648.0f ? n - 1 : min((int32_t)fl, n - 1));
    float f = u - (float)i;
    f = !(f > 0.0f) ? 0.0f : (f > 1.0f ? 1.0f : f);
    q = (uint32_t)floorf(f * POS_ONE + 0.5f);
}

// slot: the row of `records` that holds the best point (a caller that never reads it pays nothing for it)
struct Best { float d2; uint32_t index; uint32_t slot; };

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
        if (d2 <= r2 && (d2 < best.d2 || (d2 == best.d2 && i < best.index))) { best.d2 = d2; best.index = i; best.slot = s; }
    }
}

// The nearest point of the grid within max_distance of a query (header: "Nearest point within a radius"): Chebyshev shells around the query's
// cell.  A run of x-adjacent cells is one contiguous run of records, so a shell is walked row by row: full rows on its four faces in j / k, the
// two end cells of the rows in between.  -> d2 = +inf, index = 0xffffffff when there is no candidate or the query is not finite.
__device__ __forceinline__ Best pg_walk(const float qx, const float qy, const float qz, const float max_distance, const Grid &g,
                                        const uint32_t *__restrict__ cell_end, const float4 *__restrict__ records)
{
    Best best = {__uint_as_float(0x7f800000u), 0xffffffffu, 0u};
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
    return best;
}

// M: the upper 3 x 4 of a transformation, row major.  x' = ((M00 x + M01 y) + M02 z) + M03, likewise y' and z' (header: "registration", rule 1)
struct Rigid { float m[12]; };

__device__ __forceinline__ void pt_transform(const Rigid &M, const float x, const float y, const float z, float (&out)[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = ((M.m[4 * r] * x + M.m[4 * r + 1] * y) + M.m[4 * r + 2] * z) + M.m[4 * r + 3];
}

}  // namespace envgs
