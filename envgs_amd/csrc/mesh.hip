// mesh.hip -- mesh extraction for gfx950 (include/envgs_mesh.h): TSDF fusion of depth maps into a dense volume, marching tetrahedra over it.
//
//   tsdf_integrate   streaming: a lane owns 4 consecutive voxels of the x-fastest planes (16 B loads / stores), applies up to 8 views to them in
//                    registers in the order given and stores only the 16 B granules in which a voxel changed.  The volume crosses HBM once per
//                    launch; the depth / colour gathers (a wavefront's 256 voxels project onto a short pixel run) are served by the caches.
//                    No atomics, no LDS.  Compiled with -ffp-contract=off: every decision equals the NumPy oracle's fp32 sequence.
//   mesh_classify    per voxel one byte: bit 0 = inside (tsdf < level), bit 1 = observed (weight >= min_weight)           8 B read, 1 B written
//   mesh_count       a workgroup = 256 CONSECUTIVE voxels, so that workgroup order is voxel order.  Per voxel: the 7-bit mask of the crossed
//                    edges it owns that lie in an emitted cell (from the 27 neighbouring bytes), the triangle count of its own cell, a block
//                    scan; stores the mask (1 B), the block-local vertex base (2 B) and the workgroup's two totals
//   launch_scan      over the per-WORKGROUP totals (never over a per-voxel array), then mesh_totals leaves (V, F) for the one read-back
//   mesh_emit        per voxel: its vertices at base + rank; its cell's triangles at the scanned triangle base, each index =
//                    owner's base + popcount(owner's mask below the slot).  No atomics hand out slots: the order is part of the contract.
//
// The 6 x 16 case table of the Kuhn split is GENERATED at compile time from geometry (make_mt_table), orientation included: nothing is typed in.
#include "common.h"

#include "../../include/envgs_mesh.h"

namespace envgs {
namespace {

// ---- the Kuhn split ------------------------------------------------------------------------------------------------------------------------------
// Corner c of a cell has offset (c & 1, c >> 1 & 1, c >> 2 & 1).  Tetrahedron t runs 0 -> KC1[t] -> KC2[t] -> 7, adding one axis per step.
constexpr int KC1[6] = {1, 1, 2, 2, 4, 4};
constexpr int KC2[6] = {3, 5, 3, 6, 5, 6};
constexpr int SLOT_OF_DIR[8] = {-1, 0, 1, 3, 2, 4, 5, 6};       // direction bits (x = 1, y = 2, z = 4) -> slot
constexpr int DIR_OF_SLOT[7] = {1, 2, 4, 3, 5, 6, 7};

struct MtTable {
    uint8_t n[6][16];                          // triangles of (tetrahedron, sign case); bit q of the case = path corner q is inside
    uint8_t v[6][16][6];                       // their vertices: (lower corner of the crossed edge) << 3 | slot
};

struct MtInt3 { int x, y, z; };
constexpr MtInt3 mt_pos(int c) { return MtInt3{c & 1, (c >> 1) & 1, (c >> 2) & 1}; }

constexpr MtTable make_mt_table()
{
    MtTable T{};
    for (int t = 0; t < 6; t++) {
        const int c[4] = {0, KC1[t], KC2[t], 7};
        for (int m = 0; m < 16; m++) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int q = 0; q < 4; q++) { if ((m >> q) & 1) in[ni++] = q; else out[no++] = q; }
            int e[2][3][2] = {};               // triangles as edges (path corner, path corner)
            int nt = 0;
            if (ni == 1) { nt = 1; for (int k = 0; k < 3; k++) { e[0][k][0] = in[0]; e[0][k][1] = out[k]; } }
            else if (ni == 3) { nt = 1; for (int k = 0; k < 3; k++) { e[0][k][0] = out[0]; e[0][k][1] = in[k]; } }
            else if (ni == 2) {
                nt = 2;                        // quad AC AD BD BC, split along AC - BD
                const int A = in[0], B = in[1], C = out[0], D = out[1];
                e[0][0][0] = A; e[0][0][1] = C; e[0][1][0] = A; e[0][1][1] = D; e[0][2][0] = B; e[0][2][1] = D;
                e[1][0][0] = A; e[1][0][1] = C; e[1][1][0] = B; e[1][1][1] = D; e[1][2][0] = B; e[1][2][1] = C;
            }
            // inside -> outside, scaled by ni no > 0: sum(out) ni - sum(in) no
            int dx = 0, dy = 0, dz = 0;
            for (int k = 0; k < no; k++) { const MtInt3 p = mt_pos(c[out[k]]); dx += p.x * ni; dy += p.y * ni; dz += p.z * ni; }
            for (int k = 0; k < ni; k++) { const MtInt3 p = mt_pos(c[in[k]]); dx -= p.x * no; dy -= p.y * no; dz -= p.z * no; }
            for (int r = 0; r < nt; r++) {
                MtInt3 P[3] = {};              // twice the edge midpoints
                for (int k = 0; k < 3; k++) {
                    const MtInt3 a = mt_pos(c[e[r][k][0]]), b = mt_pos(c[e[r][k][1]]);
                    P[k] = MtInt3{a.x + b.x, a.y + b.y, a.z + b.z};
                }
                const int ux = P[1].x - P[0].x, uy = P[1].y - P[0].y, uz = P[1].z - P[0].z;
                const int wx = P[2].x - P[0].x, wy = P[2].y - P[0].y, wz = P[2].z - P[0].z;
                const int nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
                if (nx * dx + ny * dy + nz * dz < 0) {
                    const int s0 = e[r][1][0], s1 = e[r][1][1];
                    e[r][1][0] = e[r][2][0]; e[r][1][1] = e[r][2][1]; e[r][2][0] = s0; e[r][2][1] = s1;
                }
                for (int k = 0; k < 3; k++) {
                    const int q0 = e[r][k][0] < e[r][k][1] ? e[r][k][0] : e[r][k][1], q1 = e[r][k][0] < e[r][k][1] ? e[r][k][1] : e[r][k][0];
                    T.v[t][m][3 * r + k] = (uint8_t)((c[q0] << 3) | SLOT_OF_DIR[c[q0] ^ c[q1]]);
                }
            }
            T.n[t][m] = (uint8_t)nt;
        }
    }
    return T;
}

__constant__ const MtTable MT = make_mt_table();

// bit of voxel a + (dx,dy,dz), d in -1..1, in the 27-bit neighbourhood words
constexpr int nb_bit(int dx, int dy, int dz) { return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); }
// the 8 corners of the cell whose corner 0 is a + (ex,ey,ez), e in -1..0
constexpr uint32_t cell_bits(int ex, int ey, int ez)
{
    uint32_t m = 0;
    for (int c = 0; c < 8; c++) m |= 1u << nb_bit(ex + (c & 1), ey + ((c >> 1) & 1), ez + ((c >> 2) & 1));
    return m;
}

__device__ __forceinline__ int tet_case(uint32_t cube, int t)
{
    return (int)((cube & 1u) | (((cube >> KC1[t]) & 1u) << 1) | (((cube >> KC2[t]) & 1u) << 2) | (((cube >> 7) & 1u) << 3));
}
__device__ __forceinline__ uint32_t cube_triangles(uint32_t cube)
{
    uint32_t nt = 0;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const int pc = __popc((unsigned)tet_case(cube, t));
        nt += (pc == 2) ? 2u : ((pc == 1 || pc == 3) ? 1u : 0u);
    }
    return nt;
}

constexpr int FLAG_INSIDE = 1, FLAG_OBSERVED = 2;

// ---- kernels -------------------------------------------------------------------------------------------------------------------------------------
struct IntegArgs {
    envgs_tsdf_volume vol;
    envgs_tsdf_views views;
    float w_max;
};

__global__ void __launch_bounds__(256)
tsdf_integrate(const IntegArgs A, const uint32_t n, const int vec_planes, const int vec_rgb)
{
    const uint32_t lin0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (lin0 >= n) return;
    const int cnt = (n - lin0 < 4u) ? (int)(n - lin0) : 4;
    const bool full = cnt == 4;
    float *__restrict__ tsdf = A.vol.tsdf;
    float *__restrict__ weight = A.vol.weight;
    float *__restrict__ rgb = A.vol.rgb;
    float D[4], Wt[4], C[3][4];
    if (full && vec_planes) {
        const float4 d4 = *reinterpret_cast<const float4 *>(tsdf + lin0), w4 = *reinterpret_cast<const float4 *>(weight + lin0);
        D[0] = d4.x; D[1] = d4.y; D[2] = d4.z; D[3] = d4.w; Wt[0] = w4.x; Wt[1] = w4.y; Wt[2] = w4.z; Wt[3] = w4.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) { D[e] = e < cnt ? tsdf[lin0 + e] : 1.f; Wt[e] = e < cnt ? weight[lin0 + e] : 0.f; }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (rgb && full && vec_rgb) {
            const float4 c4 = *reinterpret_cast<const float4 *>(rgb + (size_t)c * n + lin0);
            C[c][0] = c4.x; C[c][1] = c4.y; C[c][2] = c4.z; C[c][3] = c4.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) C[c][e] = (rgb && e < cnt) ? rgb[(size_t)c * n + lin0 + e] : 0.f;
        }
    }
    // world position of the 4 voxels (they may wrap into the next row / slice)
    const uint32_t nx = (uint32_t)A.vol.nx, nxny = nx * (uint32_t)A.vol.ny;
    uint32_t k = lin0 / nxny, r = lin0 - k * nxny, j = r / nx, i = r - j * nx;
    float X[4], Y[4], Z[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        X[e] = A.vol.ox + (float)i * A.vol.voxel; Y[e] = A.vol.oy + (float)j * A.vol.voxel; Z[e] = A.vol.oz + (float)k * A.vol.voxel;
        if (++i == nx) { i = 0; if (++j == (uint32_t)A.vol.ny) { j = 0; k++; } }
    }
    unsigned changed = 0, cchanged = 0;
    for (int vi = 0; vi < A.views.count; vi++) {
        const envgs_tsdf_view &V = A.views.v[vi];
        const float *__restrict__ dmap = V.depth;
        const float *__restrict__ cmap = rgb ? V.rgb : nullptr;
        const float fW = (float)V.W, fH = (float)V.H;
        const size_t HW = (size_t)V.H * (size_t)V.W;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e >= cnt) continue;
            const float x = X[e], y = Y[e], z = Z[e];
            const float zc = V.R[6] * x + V.R[7] * y + V.R[8] * z + V.T[2];
            if (!(zc > 0.f)) continue;
            const float xc = V.R[0] * x + V.R[1] * y + V.R[2] * z + V.T[0];
            const float yc = V.R[3] * x + V.R[4] * y + V.R[5] * z + V.T[1];
            const float fu = floorf(V.fx * (xc / zc) + V.cx), fv = floorf(V.fy * (yc / zc) + V.cy);
            if (!(fu >= 0.f && fu < fW && fv >= 0.f && fv < fH)) continue;
            const size_t pix = (size_t)(int)fv * (size_t)V.W + (size_t)(int)fu;
            const float d = dmap[pix];
            if (!(d > 0.f && d <= V.depth_max)) continue;
            const float sdf = d - zc;
            if (sdf < -V.trunc) continue;
            const float val = fminf(1.0f, sdf / V.trunc);
            const float w = Wt[e], w1 = w + 1.0f;
            D[e] = (w * D[e] + val) / w1;
            if (cmap) {
#pragma unroll
                for (int c = 0; c < 3; c++) C[c][e] = (w * C[c][e] + cmap[(size_t)c * HW + pix]) / w1;
                cchanged |= 1u << e;
            }
            Wt[e] = fminf(w1, A.w_max);
            changed |= 1u << e;
        }
    }
    if (!changed) return;
    if (full && vec_planes) {
        *reinterpret_cast<float4 *>(tsdf + lin0) = make_float4(D[0], D[1], D[2], D[3]);
        *reinterpret_cast<float4 *>(weight + lin0) = make_float4(Wt[0], Wt[1], Wt[2], Wt[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) if ((changed >> e) & 1u) { tsdf[lin0 + e] = D[e]; weight[lin0 + e] = Wt[e]; }
    }
    if (!cchanged) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (full && vec_rgb) {
            *reinterpret_cast<float4 *>(rgb + (size_t)c * n + lin0) = make_float4(C[c][0], C[c][1], C[c][2], C[c][3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) if ((cchanged >> e) & 1u) rgb[(size_t)c * n + lin0 + e] = C[c][e];
        }
    }
}

// flags is padded to a multiple of 4 bytes
__global__ void __launch_bounds__(256)
mesh_classify(const float *__restrict__ tsdf, const float *__restrict__ weight, const uint32_t n, const int vec, const float level, const float min_weight,
              uint8_t *__restrict__ flags)
{
    const uint32_t lin0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (lin0 >= n) return;
    float d[4], w[4];
    if (vec && lin0 + 4u <= n) {
        const float4 d4 = *reinterpret_cast<const float4 *>(tsdf + lin0), w4 = *reinterpret_cast<const float4 *>(weight + lin0);
        d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w; w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) { const bool in = lin0 + e < n; d[e] = in ? tsdf[lin0 + e] : 1.f; w[e] = in ? weight[lin0 + e] : 0.f; }
    }
    uint32_t out = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const bool in = lin0 + e < n;
        const uint32_t f = (in && d[e] < level ? FLAG_INSIDE : 0) | (in && w[e] >= min_weight ? FLAG_OBSERVED : 0);
        out |= f << (8 * e);
    }
    *reinterpret_cast<uint32_t *>(flags + lin0) = out;
}

__global__ void __launch_bounds__(256)
mesh_count(const int nx, const int ny, const int nz, const uint8_t *__restrict__ flags, uint8_t *__restrict__ mask, uint16_t *__restrict__ vlocal,
           uint32_t *__restrict__ cnt_v, uint32_t *__restrict__ cnt_t)
{
    __shared__ uint32_t s_w[4];
    const uint32_t n = (uint32_t)nx * ny * nz, nxny = (uint32_t)nx * ny;
    const uint32_t lin = blockIdx.x * 256u + threadIdx.x;
    uint32_t m = 0, nt = 0;
    if (lin < n) {
        const int k = (int)(lin / nxny), r = (int)(lin - (uint32_t)k * nxny), j = r / nx, i = r - j * nx;
        uint32_t ok = 0, ins = 0;
#pragma unroll
        for (int dz = -1; dz <= 1; dz++)
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const bool in = (unsigned)(i + dx) < (unsigned)nx && (unsigned)(j + dy) < (unsigned)ny && (unsigned)(k + dz) < (unsigned)nz;
                    const uint32_t f = in ? flags[(long long)lin + dz * (long long)nxny + dy * nx + dx] : 0u;
                    ok |= ((f >> 1) & 1u) << nb_bit(dx, dy, dz);
                    ins |= (f & 1u) << nb_bit(dx, dy, dz);
                }
        // the 8 cells that have voxel a as a corner: valid iff all of their corners were observed (a voxel outside the grid never was)
        bool cv[2][2][2];
#pragma unroll
        for (int ez = -1; ez <= 0; ez++)
#pragma unroll
            for (int ey = -1; ey <= 0; ey++)
#pragma unroll
                for (int ex = -1; ex <= 0; ex++) cv[ez + 1][ey + 1][ex + 1] = (ok & cell_bits(ex, ey, ez)) == cell_bits(ex, ey, ez);
        const uint32_t in_a = (ins >> nb_bit(0, 0, 0)) & 1u;
#pragma unroll
        for (int s = 0; s < 7; s++) {
            const int d = DIR_OF_SLOT[s], dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
            const bool crossed = (((ins >> nb_bit(dx, dy, dz)) & 1u) ^ in_a) != 0;
            bool any = false;                  // the cells that contain the edge: offset 0 along the edge's axes, -1 or 0 along the others
#pragma unroll
            for (int ez = (dz ? 0 : -1); ez <= 0; ez++)
#pragma unroll
                for (int ey = (dy ? 0 : -1); ey <= 0; ey++)
#pragma unroll
                    for (int ex = (dx ? 0 : -1); ex <= 0; ex++) any = any || cv[ez + 1][ey + 1][ex + 1];
            m |= (crossed && any) ? (1u << s) : 0u;
        }
        if (cv[1][1][1]) {
            uint32_t cube = 0;
#pragma unroll
            for (int c = 0; c < 8; c++) cube |= ((ins >> nb_bit(c & 1, (c >> 1) & 1, (c >> 2) & 1)) & 1u) << c;
            nt = cube_triangles(cube);
        }
        mask[lin] = (uint8_t)m;
    }
    uint32_t total;
    const uint32_t ex = block_exclusive_u32<4>((uint32_t)__popc(m) | (nt << 16), s_w, total);      // <= 1792 vertices, <= 3072 triangles per workgroup
    if (lin < n) vlocal[lin] = (uint16_t)(ex & 0xffffu);
    if (threadIdx.x == 0) { cnt_v[blockIdx.x] = total & 0xffffu; cnt_t[blockIdx.x] = total >> 16; }
}

__global__ void mesh_totals(const uint32_t *__restrict__ cnt_v, const uint32_t *__restrict__ cnt_t, const uint32_t nb, uint32_t *__restrict__ totals)
{
    if (threadIdx.x == 0) totals[0] = cnt_v[nb - 1];
    if (threadIdx.x == 1) totals[1] = cnt_t[nb - 1];
}

// cnt_v / cnt_t hold INCLUSIVE scans over the workgroups here
__global__ void __launch_bounds__(256)
mesh_emit(const envgs_tsdf_volume vol, const float level, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ mask,
          const uint16_t *__restrict__ vlocal, const uint32_t *__restrict__ cnt_v, const uint32_t *__restrict__ cnt_t, const uint32_t V, const uint32_t F,
          float *__restrict__ vertices, float *__restrict__ colors, int32_t *__restrict__ faces)
{
    __shared__ uint32_t s_w[4];
    const int nx = vol.nx, ny = vol.ny, nz = vol.nz;
    const uint32_t n = (uint32_t)nx * ny * nz, nxny = (uint32_t)nx * ny;
    const uint32_t lin = blockIdx.x * 256u + threadIdx.x;
    uint32_t nt = 0, cube = 0;
    if (lin < n) {
        const int k = (int)(lin / nxny), r = (int)(lin - (uint32_t)k * nxny), j = r / nx, i = r - j * nx;
        const uint32_t m = mask[lin];
        if (m) {
            uint32_t vi = (blockIdx.x ? cnt_v[blockIdx.x - 1] : 0u) + vlocal[lin];
            const float da = vol.tsdf[lin];
            const float ax = vol.ox + (float)i * vol.voxel, ay = vol.oy + (float)j * vol.voxel, az = vol.oz + (float)k * vol.voxel;
#pragma unroll
            for (int s = 0; s < 7; s++) {
                if (!((m >> s) & 1u)) continue;
                const int d = DIR_OF_SLOT[s], dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
                const uint32_t lb = lin + (uint32_t)dx + (uint32_t)(dy * nx) + (uint32_t)dz * nxny;
                const float db = vol.tsdf[lb];
                const float t = (level - da) / (db - da);
                if (vi < V) {
                    const float bx = vol.ox + (float)(i + dx) * vol.voxel, by = vol.oy + (float)(j + dy) * vol.voxel, bz = vol.oz + (float)(k + dz) * vol.voxel;
                    vertices[3 * (size_t)vi] = ax + t * (bx - ax);
                    vertices[3 * (size_t)vi + 1] = ay + t * (by - ay);
                    vertices[3 * (size_t)vi + 2] = az + t * (bz - az);
                    if (colors) {
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            const float ca = vol.rgb[(size_t)c * n + lin], cb = vol.rgb[(size_t)c * n + lb];
                            colors[3 * (size_t)vi + c] = ca + t * (cb - ca);
                        }
                    }
                }
                vi++;
            }
        }
        if (i + 1 < nx && j + 1 < ny && k + 1 < nz) {
            bool valid = true;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const uint32_t f = flags[lin + (uint32_t)(c & 1) + (uint32_t)(((c >> 1) & 1) * nx) + (uint32_t)((c >> 2) & 1) * nxny];
                valid = valid && (f & FLAG_OBSERVED);
                cube |= (f & 1u) << c;
            }
            nt = valid ? cube_triangles(cube) : 0u;
        }
    }
    uint32_t total;
    uint32_t fi = block_exclusive_u32<4>(nt, s_w, total) + (blockIdx.x ? cnt_t[blockIdx.x - 1] : 0u);
    if (!nt) return;
    for (int t = 0; t < 6; t++) {
        const int cs = tet_case(cube, t);
        const int ntt = MT.n[t][cs];
        for (int q = 0; q < ntt; q++) {
            int32_t idx[3];
#pragma unroll
            for (int e = 0; e < 3; e++) {
                const uint32_t code = MT.v[t][cs][3 * q + e], p = code >> 3, slot = code & 7u;
                const uint32_t o = lin + (p & 1u) + ((p >> 1) & 1u) * (uint32_t)nx + ((p >> 2) & 1u) * nxny;
                const uint32_t ob = o >> 8;
                idx[e] = (int32_t)((ob ? cnt_v[ob - 1] : 0u) + vlocal[o] + (uint32_t)__popc((uint32_t)mask[o] & ((1u << slot) - 1u)));
            }
            if (fi < F) { faces[3 * (size_t)fi] = idx[0]; faces[3 * (size_t)fi + 1] = idx[1]; faces[3 * (size_t)fi + 2] = idx[2]; }
            fi++;
        }
    }
}

bool volume_ok(const envgs_tsdf_volume *v)
{
    if (!v || !v->tsdf || !v->weight) return false;
    if (v->nx < 2 || v->ny < 2 || v->nz < 2 || v->nx > ENVGS_MESH_MAX_DIM || v->ny > ENVGS_MESH_MAX_DIM || v->nz > ENVGS_MESH_MAX_DIM) return false;
    if ((long long)v->nx * v->ny * v->nz >= (1ll << 31)) return false;
    if (!(v->voxel > 0.f) || !(fabsf(v->voxel) <= 3.0e38f)) return false;
    return true;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// temp layout: flags (n, padded) | mask (n) | vlocal (n x 2 B) | cnt_v (nb) | cnt_t (nb) | scan scratch
struct MeshTemp { size_t flags, mask, vlocal, cnt_v, cnt_t, scan, scan_bytes, total; uint32_t nb; };
MeshTemp mesh_temp(long long n)
{
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    MeshTemp t;
    t.nb = (uint32_t)((n + 255) / 256);
    t.flags = 0;
    t.mask = up((size_t)n + 4);
    t.vlocal = t.mask + up((size_t)n);
    t.cnt_v = t.vlocal + up(2 * (size_t)n);
    t.cnt_t = t.cnt_v + up(4 * (size_t)t.nb);
    t.scan = t.cnt_t + up(4 * (size_t)t.nb);
    t.scan_bytes = scan_temp_bytes((int)t.nb);
    t.total = t.scan + up(t.scan_bytes);
    return t;
}

}  // namespace
}  // namespace envgs

using namespace envgs;

extern "C" {

int envgs_tsdf_integrate(const envgs_tsdf_volume *vol, const envgs_tsdf_views *views, float w_max, void *stream)
{
    if (!volume_ok(vol) || !views || views->count < 1 || views->count > ENVGS_TSDF_MAX_VIEWS || !(w_max >= 1.0f)) return ENVGS_ERR_BAD_ARG;
    for (int i = 0; i < views->count; i++) {
        const envgs_tsdf_view &v = views->v[i];
        if (!v.depth || v.H < 1 || v.W < 1 || v.H > 16384 || v.W > 16384 || !(v.trunc > 0.f) || !(v.depth_max > 0.f)) return ENVGS_ERR_BAD_ARG;
    }
    IntegArgs A;
    A.vol = *vol;
    A.views = *views;
    A.w_max = w_max;
    const uint32_t n = (uint32_t)((long long)vol->nx * vol->ny * vol->nz);
    const int vec_planes = aligned16(vol->tsdf) && aligned16(vol->weight);
    const int vec_rgb = aligned16(vol->rgb) && (n % 4u) == 0;
    const uint32_t blocks = (n + 1023u) / 1024u;
    hipLaunchKernelGGL(tsdf_integrate, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A, n, vec_planes, vec_rgb);
    return (int)hipGetLastError();
}

size_t envgs_mesh_temp_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 2 || ny < 2 || nz < 2 || nx > ENVGS_MESH_MAX_DIM || ny > ENVGS_MESH_MAX_DIM || nz > ENVGS_MESH_MAX_DIM) return 0;
    const long long n = (long long)nx * ny * nz;
    if (n >= (1ll << 31)) return 0;
    return mesh_temp(n).total;
}

int envgs_mesh_count(const envgs_tsdf_volume *vol, float level, float min_weight, void *temp, size_t temp_bytes, uint32_t *totals, void *stream_)
{
    if (!volume_ok(vol) || !temp || !totals || !aligned16(temp) || !(level == level) || !(min_weight == min_weight)) return ENVGS_ERR_BAD_ARG;
    const long long n = (long long)vol->nx * vol->ny * vol->nz;
    const MeshTemp T = mesh_temp(n);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)temp;
    uint8_t *flags = (uint8_t *)(base + T.flags), *mask = (uint8_t *)(base + T.mask);
    uint16_t *vlocal = (uint16_t *)(base + T.vlocal);
    uint32_t *cnt_v = (uint32_t *)(base + T.cnt_v), *cnt_t = (uint32_t *)(base + T.cnt_t);
    const int vec = aligned16(vol->tsdf) && aligned16(vol->weight);
    hipLaunchKernelGGL(mesh_classify, dim3(((uint32_t)n + 1023u) / 1024u), dim3(256), 0, stream, vol->tsdf, vol->weight, (uint32_t)n, vec, level, min_weight,
                       flags);
    hipLaunchKernelGGL(mesh_count, dim3(T.nb), dim3(256), 0, stream, vol->nx, vol->ny, vol->nz, flags, mask, vlocal, cnt_v, cnt_t);
    int rc = launch_scan(cnt_v, cnt_v, (int)T.nb, base + T.scan, T.scan_bytes, stream);
    if (rc) return rc;
    rc = launch_scan(cnt_t, cnt_t, (int)T.nb, base + T.scan, T.scan_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_totals, dim3(1), dim3(64), 0, stream, cnt_v, cnt_t, T.nb, totals);
    return (int)hipGetLastError();
}

int envgs_mesh_extract(const envgs_tsdf_volume *vol, float level, const void *temp, size_t temp_bytes, uint32_t V, uint32_t F, float *vertices,
                       float *colors, int32_t *faces, void *stream)
{
    if (!volume_ok(vol) || !temp || !aligned16(temp) || !(level == level) || V >= (1u << 31) || F >= (1u << 31)) return ENVGS_ERR_BAD_ARG;
    if ((V && !vertices) || (F && !faces) || (colors && !vol->rgb)) return ENVGS_ERR_BAD_ARG;
    const long long n = (long long)vol->nx * vol->ny * vol->nz;
    const MeshTemp T = mesh_temp(n);
    if (temp_bytes < T.total) return ENVGS_ERR_TEMP_TOO_SMALL;
    if (V == 0 && F == 0) return 0;
    const char *base = (const char *)temp;
    hipLaunchKernelGGL(mesh_emit, dim3(T.nb), dim3(256), 0, (hipStream_t)stream, *vol, level, (const uint8_t *)(base + T.flags),
                       (const uint8_t *)(base + T.mask), (const uint16_t *)(base + T.vlocal), (const uint32_t *)(base + T.cnt_v),
                       (const uint32_t *)(base + T.cnt_t), V, F, vertices, colors, faces);
    return (int)hipGetLastError();
}

}  // extern "C"
