/*
 * envgs_mesh.h -- C-ABI of mesh extraction: TSDF fusion of depth maps into a dense volume, and marching tetrahedra over it.
 *
 * PARITY UNPINNED: the reference's fuser (easyvolcap/utils/tsdf_utils.py) cannot run as shipped and hands the marching step to libraries that
 * are not part of it, so nothing of it is recorded as a golden fixture.  The semantics below are this project's; tests/mesh_oracle.py restates
 * them independently in NumPy ("Mesh extraction").
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

#ifdef __cplusplus
}
#endif
#endif /* ENVGS_MESH_H */
