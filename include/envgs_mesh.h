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

#ifdef __cplusplus
}
#endif
#endif /* ENVGS_MESH_H */
