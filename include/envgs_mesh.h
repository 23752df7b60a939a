/*
 * envgs_mesh.h -- C-ABI of mesh extraction: TSDF fusion of depth maps into a dense volume, marching tetrahedra over it, and the clean-up of
 * the extracted (or any other indexed) triangle mesh: connected components and order-preserving face selection.
 *
 * PARITY UNPINNED: the reference's fuser (easyvolcap/utils/tsdf_utils.py) cannot run as shipped and hands the marching step to libraries that
 * are not part of it, so nothing of it is recorded as a golden fixture.  The semantics below are this project's; tests/mesh_oracle.py and
 * tests/mesh_clean_oracle.py restate them independently in NumPy ("Mesh extraction").
 *
 * The library never allocates: the caller owns every buffer.  Bad arguments return ENVGS_ERR_BAD_ARG before any GPU work.
 */
#ifndef ENVGS_MESH_H
#define ENVGS_MESH_H

#include <stddef.h>
#include <stdint.h>

#include "envgs_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ENVGS_TSDF_MAX_VIEWS 8                /* views fused by one launch */
#define ENVGS_MESH_MAX_DIM 2048

/* A dense grid of nx ny nz voxels, x fastest; voxel (i,j,k) sits at (ox,oy,oz) + (i,j,k) voxel in world coordinates.
 * 2 <= n* <= ENVGS_MESH_MAX_DIM and nx ny nz < 2^31. */
typedef struct envgs_tsdf_volume {
    int32_t nx, ny, nz;
    float ox, oy, oz;
    float voxel;                              /* > 0 */
    float *tsdf;                              /* (nz,ny,nx), in units of the truncation distance; 1 = empty */
    float *weight;                            /* (nz,ny,nx); 0 = never observed */
    float *rgb;                               /* (3,nz,ny,nx) or NULL */
} envgs_tsdf_volume;

typedef struct envgs_tsdf_view {
    const float *depth;                       /* (H,W) z-depth; <= 0 = no measurement */
    const float *rgb;                         /* (3,H,W) or NULL */
    int32_t H, W;
    float fx, fy, cx, cy;                     /* the centre of pixel i is at i + 0.5 */
    float R[9];                               /* world -> camera, row major */
    float T[3];
    float depth_max;                          /* measurements beyond it are ignored (may be +inf) */
    float trunc;                              /* > 0, world units */
} envgs_tsdf_view;

typedef struct envgs_tsdf_views {
    int32_t count;                            /* 1 .. ENVGS_TSDF_MAX_VIEWS */
    int32_t reserved0;
    envgs_tsdf_view v[ENVGS_TSDF_MAX_VIEWS];
} envgs_tsdf_views;

/* Fuses `views->count` views into the volume in one pass over it; per voxel the views are applied in the order given, so the result is
 * bit for bit that of one launch per view.  Per voxel and view, in fp32, left to right, no FMA, IEEE division:
 *   x = ox + i voxel (y, z likewise);  xc = R00 x + R01 y + R02 z + T0 (yc, zc likewise);  skip unless zc > 0;
 *   u = fx (xc / zc) + cx,  v = fy (yc / zc) + cy;  px = floor(u), py = floor(v);  skip unless inside the image;
 *   d = depth[py][px];  skip unless 0 < d <= depth_max;  sdf = d - zc;  skip if sdf < -trunc;  val = min(1, sdf / trunc);
 *   D = (W D + val) / (W + 1)  (each rgb channel likewise, when the volume and the view both carry colour);  W = min(W + 1, w_max). */
ENVGS_API int envgs_tsdf_integrate(const envgs_tsdf_volume *vol, const envgs_tsdf_views *views, float w_max, void *stream);

/* Scratch bytes of envgs_mesh_count / envgs_mesh_extract for a volume of these dimensions (0 if they are out of range). */
ENVGS_API size_t envgs_mesh_temp_bytes(int32_t nx, int32_t ny, int32_t nz);

/* Marching tetrahedra over the Kuhn split of every cell (six tetrahedra from corner 0 to corner 7, one per permutation of the axes).
 * A cell is emitted iff all 8 corners have weight >= min_weight; a corner is inside iff tsdf < level.  Every crossed edge of an emitted
 * cell owns one vertex, kept by the edge's lower corner under slot 0..6 = direction (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1).
 *
 * envgs_mesh_count classifies the volume, counts vertices and triangles per workgroup of 256 consecutive voxels, scans the counts and leaves
 * totals[0] = V, totals[1] = F on the device; the caller reads them back (the one host sync) and sizes the outputs.  `temp` carries the
 * plan to envgs_mesh_extract and must not be touched in between. */
ENVGS_API int envgs_mesh_count(const envgs_tsdf_volume *vol, float level, float min_weight, void *temp, size_t temp_bytes, uint32_t *totals,
                               void *stream);

/* vertices (V,3) world coordinates, in ascending (owner voxel linear index, slot) order: a + t (b - a), t = (level - d_a) / (d_b - d_a), a the
 * lower corner; colors (V,3) interpolated the same way (NULL, or vol->rgb NULL: none); faces (F,3) int32, grouped by ascending cell index,
 * oriented so that the normal points from inside to outside.  A quad (two corners inside) is split along the diagonal from the edge between the
 * first inside and first outside corner to the edge between the last inside and last outside corner, in path order from corner 0 to corner 7.
 * No atomics: two runs give identical bytes.  Nothing at or beyond row V / F is written. */
ENVGS_API int envgs_mesh_extract(const envgs_tsdf_volume *vol, float level, const void *temp, size_t temp_bytes, uint32_t V, uint32_t F,
                                 float *vertices, float *colors, int32_t *faces, void *stream);

/* ---- clean-up of an indexed triangle mesh (csrc/mesh_clean.hip) ----------------------------------------------------------------------------
 * The mesh may come from anywhere (a loaded PLY, not only envgs_mesh_extract): V vertices, faces (F,3) int32, V and F below 2^31.
 * A face with any index outside [0, V) is IGNORED throughout: never dereferenced, joined to nothing, labelled -1, never selected.
 * V = 0 or F = 0 are valid.  Pointers to arrays of zero rows may be NULL; every other NULL, a count at or above 2^31 and a `temp` that is not
 * 16-byte aligned return ENVGS_ERR_BAD_ARG before any GPU work, a short `temp` ENVGS_ERR_TEMP_TOO_SMALL.  Integer work only (vertices and
 * colours are copied bit for bit): two runs give identical bytes. */

/* Scratch bytes of envgs_mesh_components: 16 B per vertex plus the per-workgroup totals (0 if a count is out of range). */
ENVGS_API size_t envgs_mesh_components_temp_bytes(uint32_t V, uint32_t F);

/* Connected components.  Two faces are connected iff they share a vertex INDEX: the components are those of the graph on the vertices whose
 * edges are the triangle sides.  That is a superset of adjacency across a shared edge; on the output of envgs_mesh_extract the two differ only
 * at pinch vertices (sheets that touch in one vertex without sharing an edge are one component here).  Vertices at equal positions under
 * different indices are different vertices.  A degenerate face (a,a,b) is an ordinary face that joins a and b; (a,a,a) is a component of one
 * vertex and one face.  A vertex no (valid) face names belongs to no component.
 * Components are numbered 0 .. C-1 by ascending smallest vertex index, so every output is independent of scheduling and of the order of the faces.
 *   vertex_label (V)  component of the vertex, -1 if unreferenced          face_label (F)  component of the face, -1 if ignored
 *   comp_faces, comp_vertices (min(V,F))  faces / vertices per component: rows 0 .. C-1 are written, C <= min(V, F)
 *   count             C, left on the device for the caller's one read-back */
ENVGS_API int envgs_mesh_components(uint32_t V, uint32_t F, const int32_t *faces, void *temp, size_t temp_bytes, int32_t *vertex_label,
                                    int32_t *face_label, int32_t *comp_faces, int32_t *comp_vertices, uint32_t *count, void *stream);

/* Scratch bytes of envgs_mesh_select_count / envgs_mesh_select_emit: 2 B per vertex plus the per-workgroup totals (0 if out of range). */
ENVGS_API size_t envgs_mesh_select_temp_bytes(uint32_t V, uint32_t F);

/* Order-preserving selection.  A face survives iff keep[f] != 0 and its three indices are in range; a vertex survives iff a surviving face names
 * it.  Survivors keep their relative order (on the output of envgs_mesh_extract: vertices ascending by (owner voxel, slot), faces grouped by
 * ascending cell), the faces are re-indexed.
 * envgs_mesh_select_count marks and scans, and leaves totals[0] = V', totals[1] = F' on the device; the caller reads them back (the one host
 * sync) and sizes the outputs.  `temp` carries the plan to envgs_mesh_select_emit and must not be touched in between; faces and keep must be
 * the same there. */
ENVGS_API int envgs_mesh_select_count(uint32_t V, uint32_t F, const int32_t *faces, const uint8_t *keep, void *temp, size_t temp_bytes,
                                      uint32_t *totals, void *stream);

/* out_vertices (V',3) and out_colors (V',3; NULL: none, else `colors` must be given) are the surviving rows of vertices / colors, bit for bit;
 * out_faces (F',3) the surviving faces in the new numbering; vertex_index (V') the old index of each new vertex (NULL: not wanted).
 * Vout <= V and Fout <= F are the totals read back; nothing at or beyond row Vout / Fout is written. */
ENVGS_API int envgs_mesh_select_emit(uint32_t V, uint32_t F, const float *vertices, const float *colors, const int32_t *faces, const uint8_t *keep,
                                     const void *temp, size_t temp_bytes, uint32_t Vout, uint32_t Fout, float *out_vertices, float *out_colors,
                                     int32_t *out_faces, int32_t *vertex_index, void *stream);

/* ---- simplification of an indexed triangle mesh: vertex clustering on a uniform grid (csrc/mesh_simplify.hip) ---------------------------------
 * The mesh is as for the clean-up (V and F below 2^31, any origin).  The grid has nx ny nz cells of edge `cell`, cell (i,j,k) covering
 * [o + (i,j,k) cell, o + (i+1,j+1,k+1) cell); its linear index is i + nx (j + ny k), x fastest.  1 <= n* and nx ny nz < 2^31; cell > 0; cell and
 * the origin are finite.  All float arithmetic is fp32, left to right, no FMA, IEEE division.
 *
 * 1. Cell of a vertex, per axis (x shown):  u = (x - ox) / cell;  fl = floor(u);
 *      i = 0 unless fl >= 1;  i = nx - 1 if fl >= 2^31;  i = min((int)fl, nx - 1) otherwise      (decided on the float, before any conversion)
 *    so positions outside the grid are clamped into its border cells.  A vertex with a coordinate that is not finite has NO cell (cluster -1).
 * 2. The clusters are the occupied cells, numbered 0 .. C-1 by ascending linear cell index: independent of scheduling and of the numbering
 *    of the input vertices.
 * 3. Representative of a cluster of n members.  n = 1: the member's position and colour, bit for bit.  n > 1, per axis and member:
 *      f = u - (float)i, then f = 0 unless f > 0, f = 1 if f > 1;   q = (uint32) floor(f * 1048576 + 0.5)                 (step 2^-20 of a cell)
 *      S = sum of q over the members, in 64-bit integers;   q_mean = (2 S + n) / (2 n), integer division                  (the rounded mean)
 *      coordinate = ox + ((float)i + (float)q_mean * 2^-20) * cell
 *    and per colour channel and member:
 *      c = 0 unless c > 0 (so NaN gives 0), c = 255 if c > 255;   q = (uint32) floor(c * 65536 + 0.5)                      (step 2^-16)
 *      S, q_mean as above;   channel = (float)q_mean * 2^-16
 *    Integer sums do not depend on the order of the adds: no float atomic is issued, two runs give identical bytes, and so do two numberings
 *    of the same vertices.
 * 4. Faces.  A face is mapped corner by corner to cluster numbers, in its corner order.  It is DROPPED if an index is outside [0, V) (such an
 *    index is never dereferenced), if a corner has no cell, if two corners share a cluster, or if a face of lower index that is not dropped by
 *    the preceding rules maps to the same oriented triple up to cyclic rotation: of equal faces the lowest index survives.  The reversed
 *    triple is a different face.
 * 5. The simplified mesh is envgs_mesh_select_count / _emit applied to the clustered mesh below: surviving faces in their old relative order,
 *    re-indexed; the clusters a surviving face names, in ascending cluster order.  On the output of envgs_mesh_extract with the volume's
 *    origin and cell = k voxel that is again a canonical order. */

/* Scratch bytes of envgs_mesh_simplify_cluster: 1 B per cell, 60 B per row of min(V, cells), 4 B per face, 4 B per slot of the face table (the
 * power of two >= 2 F), plus the per-workgroup totals.  0 if a count or the grid is out of range. */
ENVGS_API size_t envgs_mesh_simplify_temp_bytes(uint32_t V, uint32_t F, int32_t nx, int32_t ny, int32_t nz);

/* Steps 1-4.  No host sync: the outputs are sized by the bound R = min(V, nx ny nz) >= C.
 *   cl_vertices (R,3), cl_colors (R,3; NULL: none, else `colors` must be given)   rows 0 .. C-1 are written: the representatives
 *   cl_faces (F,3)     the mapped faces; a corner whose index is out of range or whose vertex has no cell is written as -1
 *   keep (F)           1 = the face survives rule 4, 0 = dropped
 *   vertex_cluster (V) cluster of each vertex, -1 = none
 *   count              C, left on the device
 * envgs_mesh_select_count / _emit on (R, F, cl_vertices, cl_colors, cl_faces, keep) then give the simplified mesh; rows C .. R-1 are never read.
 * V = 0 or F = 0 are valid (no face survives).  Pointers to arrays of zero rows may be NULL; every other NULL, a count at or above 2^31, a grid
 * out of range, a cell that is not positive and finite, an origin that is not finite and a `temp` that is not 16-byte aligned return
 * ENVGS_ERR_BAD_ARG before any GPU work, a short `temp` ENVGS_ERR_TEMP_TOO_SMALL. */
ENVGS_API int envgs_mesh_simplify_cluster(uint32_t V, uint32_t F, const float *vertices, const float *colors, const int32_t *faces, float ox, float oy,
                                          float oz, float cell, int32_t nx, int32_t ny, int32_t nz, void *temp, size_t temp_bytes,
                                          float *cl_vertices, float *cl_colors, int32_t *cl_faces, uint8_t *keep, int32_t *vertex_cluster,
                                          uint32_t *count, void *stream);

/* ---- evaluation: surface samples and exact nearest points (csrc/mesh_eval.hip, csrc/mesh_rng.h) ---------------------------------------------------
 * PARITY UNPINNED like the rest of this header: the reference has no mesh evaluation.  tests/mesh_eval_oracle.py restates what follows in NumPy.
 * All float arithmetic is fp32, left to right, no FMA, IEEE division and square root.
 *
 * Counter hash, on uint32:  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *                           h(seed, f, j) = mix(mix(mix(seed) ^ f) ^ j);   bits(h) = h >> 8;   uniform(h) = (float)bits(h) * 2^-24  (exact)
 *
 * Surface samples.  The mesh is as for the clean-up (V and F below 2^31, any origin); density > 0 is samples per unit area.
 * 1. Count of face f with corners a, b, c:  e1 = b - a, e2 = c - a, n = e1 x e2 with every component p*q - r*s as written;
 *      area = 0.5f * sqrtf((nx*nx + ny*ny) + nz*nz);   n_f = floor(area * density + uniform(h(seed, f, 0xFFFFFFFF)))
 *    n_f = 0 if an index is outside [0, V) (such an index is never dereferenced), if a corner coordinate or the area is not finite, or if the
 *    area is 0.  A face whose area * density + uniform is 2^24 or more sets the over-limit flag (and counts 0).
 * 2. The samples are ordered by ascending (f, k), k = 0 .. n_f - 1; S = sum of n_f.
 * 3. Sample k of face f:  hu = h(seed, f, 2k), hv = h(seed, f, 2k + 1);  u = uniform(hu), v = uniform(hv);
 *      if bits(hu) + bits(hv) > 2^24 (that is u + v > 1, decided on the integers) then u = 1 - u, v = 1 - v (both exact);
 *      point = (a + u * e1) + v * e2 per component; the colour is the same expression on the corner colours. */

/* Scratch bytes of envgs_mesh_sample_count / _emit: 4 B per face plus the per-workgroup totals (0 if a count is out of range). */
ENVGS_API size_t envgs_mesh_sample_temp_bytes(uint32_t V, uint32_t F);

/* Counts and scans, and leaves totals[0] = S as a 64-bit sum and totals[1] != 0 iff a face was over the limit, on the device; the caller reads
 * both back at once (the one host sync), refuses a flagged mesh or an S of 2^31 or more, and sizes the outputs.  `temp` carries the plan to
 * envgs_mesh_sample_emit and must not be touched in between; V, F, vertices, faces and seed must be the same there.  Pointers to arrays of zero
 * rows may be NULL; every other NULL, a count at or above 2^31, a density that is not positive and finite and a `temp` that is not 16-byte
 * aligned return ENVGS_ERR_BAD_ARG before any GPU work, a short `temp` ENVGS_ERR_TEMP_TOO_SMALL. */
ENVGS_API int envgs_mesh_sample_count(uint32_t V, uint32_t F, const float *vertices, const int32_t *faces, float density, uint32_t seed, void *temp,
                                      size_t temp_bytes, uint64_t *totals, void *stream);

/* points (S,3); out_colors (S,3; NULL: none, else `colors` must be given); out_face (S) the face of each sample (NULL: not wanted).  S is the
 * total read back; nothing at or beyond row S is written, and a row at or beyond the counted total is left alone.  No atomics: two runs give
 * identical bytes. */
ENVGS_API int envgs_mesh_sample_emit(uint32_t V, uint32_t F, const float *vertices, const float *colors, const int32_t *faces, uint32_t seed,
                                     const void *temp, size_t temp_bytes, uint32_t S, float *points, float *out_colors, int32_t *out_face, void *stream);

/* Nearest point within a radius.  For a query q and the points p_0 .. p_{N-1}:
 *      d2(q, p) = ((dx*dx) + (dy*dy)) + (dz*dz), d = q - p;   r2 = max_distance * max_distance
 *    the candidates are the points whose three coordinates are finite and whose d2 <= r2; the result is the candidate of least d2, of equal ones
 *    the one of lowest index; with no candidate, or a query that is not finite: dist2 = +inf, index = -1.
 * The result is a lexicographic minimum over a set, so it depends on no order inside the kernel: two runs, and two grids, give identical bytes.
 *
 * The grid is that of the simplification: nx ny nz cells of edge `cell` from the origin, x fastest, and the cell of a point is its rule 1, with
 * positions outside clamped into the border cells; here 1 <= n* <= ENVGS_POINTS_MAX_DIM and nx ny nz <= ENVGS_POINTS_MAX_CELLS.  A query starts
 * in its own cell by the same rule and visits the Chebyshev shells r = 0, 1, 2 .. around it, clipped to the grid.  After shell r, with
 *      b = ((float)r * cell) * (1 - 2^-10)
 * it stops if best_d2 <= b*b or b > max_distance; and it stops after the last shell that holds a cell of the grid, an integer known before the
 * loop, so no input makes a lane spin.
 *
 * Why the stop is exact.  The cell index of rule 1 is monotone in the coordinate, and the quotient (x - o) / cell it floors carries a relative
 * error of at most 2^-22 (one rounding of the difference, one of the division, and slack).  A point that is not in shells 0 .. r has a clamped index
 * that differs from the query's by at least r + 1 on some axis.  Between the two lie r whole cells, so with exact quotients the two coordinates
 * would differ by more than r cell; each computed quotient is off by at most 2^-22 of its magnitude, which is at most about n* <= 1024 cells inside
 * the grid (outside it clamping only moves the true position farther away), so the coordinates differ by more than cell (r - 2^-21 n*) >=
 * r cell (1 - 2^-11) for r >= 1 (for r = 0 the bound b = 0 claims nothing).  The computed d2 of such a point is at least the square of that
 * axis difference less 3 * 2^-24 relative rounding, and b = r cell (1 - 2^-10), rounded twice, stays below it.  So every point outside the
 * visited shells has d2 > b*b: it cannot beat, or tie, a best at or below b*b, and once b > max_distance it is no candidate. */
#define ENVGS_POINTS_MAX_DIM 1024
#define ENVGS_POINTS_MAX_CELLS (1u << 27)

/* Scratch bytes of envgs_points_grid_build: 4 B per point plus the per-workgroup totals of the cells (0 if a count or the grid is out of range). */
ENVGS_API size_t envgs_points_grid_temp_bytes(uint32_t N, int32_t nx, int32_t ny, int32_t nz);

/* Builds the grid over points (N,3): cell_end (nx ny nz) u32, the end of each cell in `records`, the end of cell c - 1 being the start of cell c;
 * records (N,4), 16-byte aligned: (x, y, z, index bits) of the finite points in cell order -- rows at or beyond their number are not written, and
 * the order inside a cell may depend on scheduling.  `temp` is free again when the call returns.  N = 0 is valid (records may be NULL).  Every
 * other NULL, a count at or above 2^31, a grid out of range, a cell that is not positive and finite, an origin that is not finite and a `temp`
 * or `records` that is not 16-byte aligned return ENVGS_ERR_BAD_ARG before any GPU work, a short `temp` ENVGS_ERR_TEMP_TOO_SMALL. */
ENVGS_API int envgs_points_grid_build(uint32_t N, const float *points, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny, int32_t nz,
                                      void *temp, size_t temp_bytes, uint32_t *cell_end, float *records, void *stream);

/* dist2 (Q) and index (Q) of queries (Q,3) against a grid built with the same origin, cell and dimensions; one query per lane in the given
 * order.  max_distance must be finite and >= 0.  Q = 0 is valid. */
ENVGS_API int envgs_points_nearest(uint32_t Q, const float *queries, float max_distance, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny,
                                   int32_t nz, const uint32_t *cell_end, const float *records, float *dist2, int32_t *index, void *stream);

/* ---- thinning: no two kept points within a radius, by the sequential rule of the DTU evaluation (csrc/mesh_eval.hip) -------------------------------
 * PARITY UNPINNED.  tests/mesh_thin_oracle.py restates what follows in NumPy.  fp32, left to right, no FMA.
 *
 * For the points p_0 .. p_{N-1} (N below 2^31) and a finite radius >= 0:
 *      d2(i, j) = ((dx*dx) + (dy*dy)) + (dz*dz), d = p_i - p_j;   r2 = radius * radius
 *    i and j are NEIGHBOURS iff the coordinates of both are finite, i != j and d2 <= r2.  The bound is inclusive; duplicates are neighbours, and
 *    radius = 0 removes exact duplicates only (a d2 of 0 between different positions can arise only where a product underflows, at differences
 *    below 2^-74; the shell bound below, like that of the nearest-point search, supposes no such underflow).
 *      hashed:      key(i) = h(seed, i, 0xFFFFFFFE)   (the counter hash above).  mix is a bijection of uint32 and so is xor with a constant, so for a
 *                   fixed seed i -> key(i) is a permutation: the keys are distinct and their order is strict without a tie-break
 *      not hashed:  key(i) = i, the given order
 *    The points are visited by ascending key.  A finite point is KEPT iff no kept neighbour has a smaller key; a point that is not finite is never
 *    kept and is nobody's neighbour.  That is the loop of the DTU script ("a point that is still alive is kept and kills everything within the
 *    radius") on the array permuted by key: the lexicographically first maximal independent set of the neighbour graph.  `keep` is a function of
 *    the points, the radius and the keys alone: it depends on no cell size, no scheduling and no number of rounds.
 *
 * Device form.  One uint32 state per point: UNDECIDED, KEPT or DROPPED; the points that are not finite start DROPPED.  A round gives a lane to
 * every undecided point i.  The lane walks the cells of shells 0 .. R around i's cell (the grid and the cell rule of the nearest-point search) and
 * considers every record j with d2 <= r2, j != i and key(j) < key(i), the key recomputed from the index in the record: a KEPT j makes i DROPPED
 * and ends the walk; an UNDECIDED j makes i blocked; a lane that is neither becomes KEPT.  The blocked points form the next round's worklist
 * (two buffers in turn, one integer atomic per wavefront; its order is free, since no result depends on it).
 *
 * Why a lane may read states that other lanes write in the same launch.  A state only ever moves from UNDECIDED to a final value, and a final
 * value is correct at the moment it is written: i is DROPPED only on seeing a lower-keyed neighbour KEPT, which stays so; i is KEPT only after seeing
 * every lower-keyed neighbour DROPPED, which stays so.  Whatever a lane reads is therefore either final and true, or UNDECIDED -- possibly stale --
 * which blocks it and costs a round, never a result.  Every round decides at least the undecided point of smallest key (all its lower-keyed
 * neighbours are final), so N rounds always suffice: the host loop is bounded by that integer and compares no float.  No lane waits inside a
 * kernel for another lane or workgroup; progress comes only from launching the next round.
 *
 * R, computed once by the caller in fp32, is the smallest integer with ((float)R * cell) * (1 - 2^-10) >= radius, clipped to the last shell that
 * can hold a cell of the grid (max(nx, ny, nz) - 1).  The expression is the b of the nearest-point search, whose proof gives: every point outside
 * shells 0 .. R has d2 > b*b >= r2, so it is no neighbour.  (radius = 0 gives R = 0: equal positions share a cell.)
 *
 * Scratch: state (N u32) | worklist (N u32) | worklist (N u32) | 4 counters, each part rounded up to 256 B.  `count` (2 u32, on the device):
 * count[0] = the undecided points left, count[1] = the rounds so far that found an undecided point. */

/* Scratch bytes of the three calls below (0 if N is 2^31 or more). */
ENVGS_API size_t envgs_points_thin_temp_bytes(uint32_t N);

/* Builds the states and the first worklist (the finite points) in `temp`, which carries them to the calls below, and reports into `count`. */
ENVGS_API int envgs_points_thin_begin(uint32_t N, const float *points, void *temp, size_t temp_bytes, uint32_t *count, void *stream);

/* Runs rounds first_round .. first_round + rounds - 1 (first_round counts every round launched since envgs_points_thin_begin, from 0) over a grid
 * built by envgs_points_grid_build on the same points, and reports into `count`.  `undecided` sizes the launches: the caller's latest read-back of
 * count[0] (or N before any); with 0 nothing is launched.  hashed != 0: the hash keys of `seed`; 0: index order.  `shells` is R above, 0 .. 1023.
 * Bad arguments as for envgs_points_nearest, plus a `temp` that is NULL or not 16-byte aligned. */
ENVGS_API int envgs_points_thin_round(uint32_t N, const float *points, float radius, int32_t hashed, uint32_t seed, float ox, float oy, float oz, float cell,
                                      int32_t nx, int32_t ny, int32_t nz, int32_t shells, const uint32_t *cell_end, const float *records, void *temp,
                                      size_t temp_bytes, uint32_t first_round, uint32_t rounds, uint32_t undecided, uint32_t *count, void *stream);

/* keep (N) uint8: 1 = kept.  To be called once count[0] is 0; a point still undecided is written as 0. */
ENVGS_API int envgs_points_thin_keep(uint32_t N, const void *temp, size_t temp_bytes, uint8_t *keep, void *stream);

/* ---- culling: the vertices some camera sees outside its mask (csrc/mesh_eval.hip) -------------------------------------------------------------------
 * A vertex is projected into a view BY THE PIXEL RULE OF envgs_tsdf_integrate (fp32, left to right, no FMA, IEEE division):
 *      xc = R00 x + R01 y + R02 z + T0 (yc, zc likewise);   u = fx (xc / zc) + cx,  v = fy (yc / zc) + cy;   px = floor(u),  py = floor(v)
 * It PASSES the view iff zc <= 0, or the pixel is outside the image, or mask[py][px] != 0.  A vertex is kept iff its three coordinates are finite
 * and it passes every view; a face is kept iff its three indices are in range and its three corners are kept.  So a mesh fused under masks and
 * culled under the same masks is treated by one rule. */
typedef struct envgs_cull_view {
    const uint8_t *mask;                      /* (H,W); 0 = outside the object */
    int32_t H, W;
    float fx, fy, cx, cy;
    float R[9];                               /* world -> camera, row major */
    float T[3];
} envgs_cull_view;

typedef struct envgs_cull_views {
    int32_t count;                            /* 0 .. ENVGS_TSDF_MAX_VIEWS */
    int32_t reserved0;
    envgs_cull_view v[ENVGS_TSDF_MAX_VIEWS];
} envgs_cull_views;

/* keep (V) uint8.  accumulate = 0: keep[v] = finite and passes every view given; != 0: the same AND the keep[v] already there, so that more than
 * ENVGS_TSDF_MAX_VIEWS views take several calls.  V at or above 2^31, a count outside 0 .. 8, a NULL mask or an empty image: ENVGS_ERR_BAD_ARG. */
ENVGS_API int envgs_mesh_cull_vertices(uint32_t V, const float *vertices, const envgs_cull_views *views, int32_t accumulate, uint8_t *keep, void *stream);

/* face_keep (F) uint8 from vertex_keep (V): the input of envgs_mesh_select_count / _emit.  An index outside [0, V) is never dereferenced. */
ENVGS_API int envgs_mesh_cull_faces(uint32_t V, uint32_t F, const int32_t *faces, const uint8_t *vertex_keep, uint8_t *face_keep, void *stream);

/* ---- registration and the Tanks-and-Temples protocol (csrc/mesh_register.hip, csrc/mesh_points.h) ---------------------------------------------------
 * PARITY UNPINNED: the reference has no registration.  The rules are this project's own, modelled on Open3D's point-to-point ICP, voxel
 * down-sampling and SelectionPolygonVolume and on the Tanks-and-Temples toolbox; tests/mesh_register_oracle.py restates them in NumPy.  All fp32
 * arithmetic is left to right, no FMA, IEEE division; the double arithmetic named below is never contracted either.
 *
 * 1. Transformation.  M (12 floats on the HOST, row major) is the upper 3 x 4 of a transformation, each entry already rounded to fp32:
 *      x' = ((M00 x + M01 y) + M02 z) + M03      y' = ((M10 x + M11 y) + M12 z) + M13      z' = ((M20 x + M21 y) + M22 z) + M23
 *    A row with a coordinate that is not finite gives a row of which no coordinate is finite.  envgs_points_transform and the registration call
 *    one device function (pt_transform), so the two cannot drift.
 *
 * 2. The sums of one ICP iteration.  For every source row p:  a = M p by rule 1;  b = the nearest target point within max_distance by the rule of
 *    envgs_points_nearest applied to a (the same candidates, the same tie-break by lowest index, the same result at every cell size; the walk is
 *    one device function, pg_walk, that both kernels call), its coordinates taken from the grid's record;  d2 = the fp32 d2 of that search.
 *    A row without a match (none within max_distance, or a or p not finite) adds nothing.  With c = `center`, three finite doubles on the HOST --
 *    the centre of the box of the finite target points, (lo + hi) / 2 per axis in double, which is a property of the points and not of the cell
 *    size -- and  ah = (double)a - c,  bh = (double)b - c  (exact for all practical inputs), a matched row adds, all in double:
 *      sums[0]      1                                   n, the number of matches (below 2^31, so exact)
 *      sums[1]      (double)d2
 *      sums[2..4]   ah          sums[5..7]   bh
 *      sums[8+3r+c] ah[r] * bh[c]                        row major: sum of ah bh^T
 *      sums[17]     ((ah0 ah0) + (ah1 ah1)) + (ah2 ah2)
 *    The order of the additions is a function of Q alone.  Source row q belongs to lane q mod 64 of wavefront (q / 64) mod 4 of workgroup
 *    q / 256; rows at or beyond Q and rows without a match contribute +0.
 *      lane -> wavefront:  lane l adds the value of lane l + 32, then of l + 16, 8, 4, 2, 1 (a lane whose partner is beyond 63 adds its own value
 *                          and feeds nobody); lane 0 ends with the balanced binary tree over the 64 lanes
 *      -> workgroup row:   ((w0 + w1) + w2) + w3 over its four wavefronts: one row of 18 doubles, 144 B, per workgroup
 *      -> the result:      ONE workgroup of 256 threads: thread t adds the rows t, t + 256, t + 512 .. in ascending order, starting from +0; the 256
 *                          thread sums are then added exactly as the 256 lane values of a row above
 *    No atomic is issued, float or integer: the 18 numbers are identical from run to run, and -- the match being a lexicographic minimum over a
 *    set -- at every cell size of the grid.
 *
 * 3. The solve is on the host in float64 (envgs_amd.mesh.rigid_from_sums):  am = sum ah / n, bm = sum bh / n;  H = sum ah bh^T - n am bm^T;
 *    U S V^T = svd(H);  D = diag(1, 1, det(V U^T));  R = V D U^T;  s = tr(S D) / (sum |ah|^2 - n |am|^2) with scale, else 1;
 *    t = bm - s R am, and the transformation in world coordinates is x -> s R x + (c + t - s R c).
 *
 * 4. Voxel mean: the sparse form of the simplification's clustering, for grids far beyond 2^31 cells.  The cell of a point is rule 1 of the
 *    simplification per axis, 1 <= n* <= ENVGS_VOXEL_MAX_DIM = 2^21; its key is i | j << 21 | k << 42, which orders the cells as the linear index
 *    of the simplification does (x fastest); a point that is not finite has the key 2^63 - 1 and no cluster (-1).  The clusters are the occupied
 *    keys in ascending order.  The representative is rule 3 of the simplification, word for word (one device function, sc_locate): a single
 *    member keeps its bits, otherwise 64-bit integer sums of the offsets in steps of 2^-20 of a cell and the rounded mean.  Integer sums depend on
 *    no order: two runs and two permutations of the input give identical bytes, and wherever the dense grid of envgs_mesh_simplify_cluster
 *    exists its rows 0 .. C-1 of cl_vertices are the same bytes.  The sort of the keys between envgs_points_voxel_keys and
 *    envgs_points_voxel_cluster is the caller's (any sort; only the grouping of equal keys and their ascending order are used).
 *
 * 5. Crop volume (Open3D's SelectionPolygonVolume).  axis 0 / 1 / 2 = X / Y / Z is the orthogonal axis w; (u, v) = (1, 2), (0, 2), (0, 1).  A
 *    point whose coordinates are finite is INSIDE iff axis_min <= p[w] <= axis_max and the number of edges (j, k = j + 1 mod M) with
 *      (v_j > p_v) != (v_k > p_v)   and   p_u < (u_k - u_j) * (p_v - v_j) / (v_k - v_j) + u_j
 *    is odd -- evaluated in double as written (product, quotient, sum), on the fp32 point converted to double and the double polygon. */
#define ENVGS_REGISTER_SUMS 18
#define ENVGS_VOXEL_MAX_DIM (1 << 21)
#define ENVGS_POLYGON_MAX 256

/* out (N,3) = rule 1 applied to points (N,3); the two must not overlap.  N = 0 is valid.  A NULL or non-finite M, a count at or above 2^31 and a NULL
 * array of rows return ENVGS_ERR_BAD_ARG before any GPU work. */
ENVGS_API int envgs_points_transform(uint32_t N, const float *points, const float *M, float *out, void *stream);

/* Scratch bytes of envgs_points_register_sums: 144 B per workgroup of 256 source rows (0 if Q is 2^31 or more). */
ENVGS_API size_t envgs_points_register_temp_bytes(uint32_t Q);

/* Rule 2 over source (Q,3) against a grid built by envgs_points_grid_build with the same origin, cell and dimensions: two launches (the rows, the
 * final workgroup), sums (18 doubles) left on the device.  Optional per-row outputs, NULL = not wanted: moved (Q,3) the transformed rows,
 * dist2 (Q) and index (Q) as envgs_points_nearest would give them for `moved`.  Q = 0 is valid: the sums are zero.  Bad arguments as for
 * envgs_points_nearest, plus a NULL or non-finite M or center, a NULL `sums` and a `temp` that is NULL or not 16-byte aligned: ENVGS_ERR_BAD_ARG before
 * any GPU work; a short `temp` ENVGS_ERR_TEMP_TOO_SMALL. */
ENVGS_API int envgs_points_register_sums(uint32_t Q, const float *source, const float *M, float max_distance, float ox, float oy, float oz, float cell,
                                         int32_t nx, int32_t ny, int32_t nz, const uint32_t *cell_end, const float *records, const double *center, void *temp,
                                         size_t temp_bytes, double *sums, float *moved, float *dist2, int32_t *index, void *stream);

/* keys (N) int64 of rule 4.  N = 0 is valid.  A dimension outside 1 .. 2^21, a cell that is not positive and finite, an origin that is not finite,
 * a count at or above 2^31: ENVGS_ERR_BAD_ARG before any GPU work. */
ENVGS_API int envgs_points_voxel_keys(uint32_t N, const float *points, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny, int32_t nz,
                                      int64_t *keys, void *stream);

/* Scratch bytes of envgs_points_voxel_cluster / _finish: 48 B per point plus the scan's scratch (0 if N is 2^31 or more). */
ENVGS_API size_t envgs_points_voxel_temp_bytes(uint32_t N);

/* sorted_keys (N): the keys in ascending order; order (N) int64: the point of each sorted slot (an entry outside [0, N) is never dereferenced).
 * Marks the first slot of every key, scans, and accumulates; leaves count = C on the device and, if wanted, cluster (N) int32 per POINT (-1 = none).
 * `temp` carries the sums to envgs_points_voxel_finish.  The caller reads C back (the one host sync) and sizes the output. */
ENVGS_API int envgs_points_voxel_cluster(uint32_t N, const float *points, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny, int32_t nz,
                                         const int64_t *sorted_keys, const int64_t *order, void *temp, size_t temp_bytes, int32_t *cluster,
                                         uint32_t *count, void *stream);

/* out (C,3): the representatives, C <= N the count read back; a row at or beyond the counted clusters is left alone. */
ENVGS_API int envgs_points_voxel_finish(uint32_t N, const float *points, float ox, float oy, float oz, float cell, int32_t nx, int32_t ny, int32_t nz,
                                        void *temp, size_t temp_bytes, uint32_t C, float *out, void *stream);

/* inside (N) uint8 by rule 5.  polygon: (M,3) doubles ON THE DEVICE, 3 <= M <= ENVGS_POLYGON_MAX.  N = 0 is valid.  An axis outside 0 .. 2, an M out
 * of range, a NULL polygon, a bound that is NaN: ENVGS_ERR_BAD_ARG before any GPU work. */
ENVGS_API int envgs_points_in_polygon(uint32_t N, const float *points, int32_t axis, double axis_min, double axis_max, uint32_t M, const double *polygon,
                                      uint8_t *inside, void *stream);

/* ---- depth fusion: consistency-filtered point clouds from depth maps (csrc/mesh_fuse.hip) -----------------------------------------------------------
 * PARITY PINNED by tests/golden/fuse_golden.npz: the rules are those of the reference's scripts/fusion/depth_fusion.py and
 * easyvolcap/utils/fusion_utils.py (depth_reprojection, depth_geometry_consistency, compute_consistency), whose recorded outputs the tests compare
 * with; tests/mesh_fuse_oracle.py restates them in NumPy float64.  The kernel applies transformations composed on the host in float64 instead of
 * the reference's chain of matrix products, so it agrees with the reference to rounding ("Depth fusion": the measured band), not to the bit.
 *
 * All views of a call share one size H x W; the centre of pixel (x, y) is (xc, yc) = (x + 0.5, y + 0.5).  With K, R, T of a camera (x_cam = R x + T):
 *
 * 1. A pair (reference r, source s) carries two affine maps of 12 floats, A (row major, 9) then b (3), composed in float64 and rounded once:
 *      fwd:   A = K_s R_s R_r^T K_r^-1,   b = K_s (T_s - R_s R_r^T T_r)          p_src = d_ref (A (xc, yc, 1)) + b
 *      back:  the same with r and s exchanged                                     p_ref = sampled (A (u, v, 1)) + b
 * 2. Per pair, in fp32:  (u, v) = p_src.xy / p_src.z;  sampled = the source depth at (u, v) as torch's grid_sample gives it with its defaults
 *    (bilinear, align_corners = False, padding_mode = 'border'):  ix = clip(u - 0.5, 0, W - 1), iy likewise; taps floor and floor + 1; the taps
 *    inside the image are multiplied by their weights, a weight of 0 included, and added in the order (y0,x0) (y0,x1) (y1,x0) (y1,x1); a tap outside
 *    the image can only carry the weight 0 and is not read.  z = p_ref.z, (x', y') = p_ref.xy / z.  The pair PASSES iff
 *      sqrt((x' - xc)^2 + (y' - yc)^2) < geo_abs_thresh   and   |z - d_ref| / d_ref < geo_rel_thresh   and   sampled > 0
 *    every comparison being false on NaN.  A reference pixel whose depth is not finite or not > 0 passes nothing (the reference lets a negative
 *    depth pass the relative test; its photometric mask drops the pixel afterwards), and a pair whose u, v or sampled depth is not finite fails.
 * 3. Per reference pixel: count = the passing sources (saturating at 255), sum = the sum of their z in source order.
 * 4. depth_avg = (sum + d_ref) / (count + 1);  final = count >= min_count and d_ref > pho_abs_thresh.
 * 5. The kept pixels in ascending (view, row, column) order give  point = c_v + depth_avg (A_v (xc, yc, 1)),  A_v = R_v^T K_v^-1 and c_v = -R_v^T T_v
 *    composed in float64 (12 floats per view ON THE DEVICE: A_v row major, then c_v). */
typedef struct envgs_fuse_source {
    const float *depth;                       /* (H,W) z-depth of the source view; <= 0 = no measurement */
    int32_t H, W;                             /* must equal the reference's */
    float fwd[12];                            /* reference pixel and depth -> source image: A (9), b (3) */
    float back[12];                           /* source pixel and sampled depth -> reference image */
} envgs_fuse_source;

typedef struct envgs_fuse_sources {
    int32_t count;                            /* 0 .. ENVGS_TSDF_MAX_VIEWS */
    int32_t reserved0;
    envgs_fuse_source v[ENVGS_TSDF_MAX_VIEWS];
} envgs_fuse_sources;

/* Rules 2 and 3 for one reference map depth_ref (H,W): count (H,W) uint8 and sum (H,W) float.  accumulate = 0: from zero; != 0: added to what is
 * there, so that more than ENVGS_TSDF_MAX_VIEWS sources take several calls and the sum stays in source order.  A count outside 0 .. 8, a NULL
 * pointer, an empty image, a source whose size differs from H x W and H W >= 2^31 return ENVGS_ERR_BAD_ARG and write nothing. */
ENVGS_API int envgs_fuse_consistency(int32_t H, int32_t W, const float *depth_ref, const envgs_fuse_sources *sources, float geo_abs_thresh,
                                     float geo_rel_thresh, int32_t accumulate, uint8_t *count, float *sum, void *stream);

/* Scratch bytes of envgs_fuse_count / envgs_fuse_emit: the per-workgroup totals and the scan's scratch (0 unless V, H, W >= 1 and V H W < 2^31). */
ENVGS_API size_t envgs_fuse_temp_bytes(int32_t V, int32_t H, int32_t W);

/* Rule 4 over all V H W pixels of depth, count, sum (V,H,W): writes depth_avg (V,H,W) float and final_mask (V,H,W) uint8, scans the kept pixels per
 * workgroup of 256 and leaves total[0] = N as a 64-bit integer on the device; the caller reads it back (the one host sync) and sizes the outputs.
 * `temp` (16-byte aligned) carries the plan to envgs_fuse_emit and must not be touched in between.  Bad arguments: ENVGS_ERR_BAD_ARG before any GPU
 * work; a short `temp`: ENVGS_ERR_TEMP_TOO_SMALL. */
ENVGS_API int envgs_fuse_count(int32_t V, int32_t H, int32_t W, const float *depth, const uint8_t *count, const float *sum, uint32_t min_count,
                               float pho_abs_thresh, float *depth_avg, uint8_t *final_mask, void *temp, size_t temp_bytes, int64_t *total, void *stream);

/* Rule 5: points (N,3); colors (N,3) gathered from rgb (V,3,H,W) and normals (N,3) from normal (V,3,H,W) (NULL: none, else the map must be given);
 * index (N) int64, the flat (view H + row) W + column of each point (NULL: not wanted).  N <= V H W is the total read back; nothing at or beyond row
 * N is written.  No atomics: two runs give identical bytes. */
ENVGS_API int envgs_fuse_emit(int32_t V, int32_t H, int32_t W, const float *depth_avg, const uint8_t *final_mask, const void *temp, size_t temp_bytes,
                              const float *view_maps, const float *rgb, const float *normal, uint32_t N, float *points, float *colors, float *normals,
                              int64_t *index, void *stream);

/* ---- rasterisation: exact depth, face and normal maps of a mesh, and the faces some camera sees (csrc/mesh_raster.hip, csrc/mesh_raster.h) ---------
 * PARITY UNPINNED: the reference renders meshes only through its OpenGL viewer, which is out of scope.  The rule is this
 * project's; tests/mesh_raster_oracle.py restates it in NumPy and Python integers.  csrc/mesh_raster.h is one text for the kernels and for the host.
 *
 * All views of a call share one size H x W.  The camera is the one cull_to_masks() and TSDFVolume.integrate() use: K, R world -> camera, T.  The
 * centre of pixel (px, py) is at (px + 0.5, py + 0.5).  Cameras travel by value, 8 views per launch (MAX_VIEWS).
 *
 * Vertex, per view.  float32, no contraction, the sequence of the culling rule:
 *   - xc = R00 x + R01 y + R02 z + T0, and yc, zc likewise.
 *   - u = fx (xc / zc) + cx,  v = fy (yc / zc) + cy.
 *   - The vertex is USABLE iff u and v are finite, zc > near, |u| < 2^21 and |v| < 2^21.  near is a float32 argument with default 0.
 *   - Its sub-pixel position is X = (int32) rint(u * 256), Y = (int32) rint(v * 256), with ties to even.
 *
 * Face.
 *   - A face is dropped whole iff one of these holds: an index is outside [0, V); a corner is not usable;
 *     A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) is 0.  A is int64, as are all edge arithmetic below.
 *   - There is NO CLIPPING: a face that crosses the camera plane is not drawn.  This is a stated deviation from what a graphics pipeline does.
 *   - If A < 0, corners 1 and 2 are exchanged and A is negated.  Both windings are drawn; there is no back-face culling.
 *
 * Coverage.
 *   - Let P = (256 px + 128, 256 py + 128).
 *   - For k = 0, 1, 2 let i = (k + 1) mod 3 and j = (k + 2) mod 3, in the possibly exchanged order.
 *   - Define dx = Xj - Xi, dy = Yj - Yi, and E_k = dx (P_y - Y_i) - dy (P_x - X_i).
 *   - The pixel is covered iff, for every k, E_k > 0 or (E_k == 0 and (dy < 0 or (dy == 0 and dx > 0))).  This is the top-left rule.
 *   - A pixel on an edge shared by two faces belongs to exactly one of them.
 *   - Any conservative bounding box may limit the pixels visited.  The result is defined by the rule over all H x W pixels.
 *
 * Depth.  In double:  l_k = (double) E_k / (double) A;  iz_k = 1.0 / (double) zc_k;  s = (l_0 iz_0 + l_1 iz_1) + l_2 iz_2;  z = (float) (1.0 / s).
 *
 * Winner.  The smallest 64-bit key (bits(z) << 32) | face index wins the pixel.  Equal depths go to the lowest face index.  The result does not
 * depend on the order in which faces arrive.
 *
 * Outputs per view.  Each is optional; what the caller does not request is not computed or written.
 *   depth  (n,H,W) float32     the winner's z; 0 where no face covers the pixel
 *   face   (n,H,W) int32       the winner's index; -1 where none
 *   bary   (n,H,W,3) float32   b_k = (float) ((l_k iz_k) / s), reported in the order of the face's ORIGINAL corners; 0 where none
 *   normal (n,H,W,3) float32   see below
 *   color  (n,H,W,3) float32   only for a mesh with colours: (b_0 c_0 + b_1 c_1) + b_2 c_2 per channel in float32, original corner order; 0 where none
 *   seen   (F) uint8           1 iff the face wins at least one pixel of at least one view; accumulated over the launches of a call
 *
 * The normal:
 *   - Take the world-space cross product (v1 - v0) x (v2 - v0) of the original corners in float32.  Each component is a b - c d with the two
 *     products rounded first.
 *   - Divide by its length: float32 sum of squares added left to right, IEEE sqrt, IEEE divide.
 *   - ORIENT IT TOWARDS THE CAMERA: negate it iff A > 0 before the exchange.  A cross product that points along +z of this y-down, z-forward camera
 *     faces away from it.
 *   - A length of 0 gives (0, 0, 0).
 *   - Where no face covers the pixel the normal is 0.
 *
 * Byte model.  The only scratch is the key image, 8 B per pixel and view of a launch (at most 8 views): it does not grow with F.  The raster pass
 * reads 12 B of indices and 36 B of corners per (face, view) and issues one 64-bit integer atomic-min per covered fragment that a plain load of
 * the key does not already rule out (keys only decrease, so a stale value costs an unnecessary atomic, never a result).  The resolve pass reads
 * 8 B per pixel and the winner's 48 B, and writes the requested maps. */
typedef struct envgs_mesh_raster_view {
    float fx, fy, cx, cy;
    float R[9];                               /* world -> camera, row major */
    float T[3];
} envgs_mesh_raster_view;

typedef struct envgs_mesh_raster_views {
    int32_t count;                            /* 0 .. ENVGS_TSDF_MAX_VIEWS */
    int32_t reserved0;
    envgs_mesh_raster_view v[ENVGS_TSDF_MAX_VIEWS];
} envgs_mesh_raster_views;

/* A face whose clamped bounding box holds at most this many pixels is walked by the lane that set it up; a larger one is handed to its whole
 * workgroup, which strides the box together in tiles of 8 x 8 pixels. */
ENVGS_API int32_t envgs_mesh_raster_small_max(void);

/* Scratch bytes of envgs_mesh_raster: the key image, 8 B per pixel and view (0 unless H, W >= 1, H W < 2^28 and 0 <= views <= 8). */
ENVGS_API size_t envgs_mesh_raster_temp_bytes(int32_t H, int32_t W, int32_t views);

/* One launch group: the key image is set to all-ones, the raster pass fills it, the resolve pass writes the maps of views->count views (row 0 of
 * every map pointer is the first view of THIS launch) and stores 1 to seen[f] of every winner.  first != 0: seen is cleared before; 0: it
 * accumulates.  NULL for an output that is not wanted (colors NULL: color must be NULL too).  stats: NULL, or 2 uint64 on the device that the
 * raster pass ADDS to: [0] fragments covered, [1] atomics issued (a measuring aid; it costs an atomic add per wavefront).  No host sync.
 * F = 0, V = 0 and count = 0 are valid: the maps of the views given are cleared.  V or F at or above 2^31, a size out of range, a count outside
 * 0 .. 8, a near that is NaN, a NULL array of rows and a `temp` that is NULL or not 16-byte aligned return ENVGS_ERR_BAD_ARG before any GPU work,
 * a short `temp` ENVGS_ERR_TEMP_TOO_SMALL. */
ENVGS_API int envgs_mesh_raster(uint32_t V, uint32_t F, const float *vertices, const float *colors, const int32_t *faces,
                                const envgs_mesh_raster_views *views, int32_t H, int32_t W, float near, int32_t first, void *temp, size_t temp_bytes,
                                float *depth, int32_t *face, float *bary, float *normal, float *color, uint8_t *seen, uint64_t *stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVGS_MESH_H */
