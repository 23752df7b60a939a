// mesh_raster_host.cpp -- the rasterisation rule of mesh_raster.h on the CPU, face by face, one view after the other.  Not part of libenvgs_hip.so
// (build.py compiles the .hip files only); tests/test_mesh_raster_cpu.py builds it with the host compiler (-ffp-contract=off, as build.py gives
// mesh_raster.hip) and compares its key image with the oracle's, bit for bit.  It is a program of its own, so it can also be built with
// -fsanitize=address,undefined and run by hand.
//
//   mesh_raster_host IN OUT
//   IN : int32 H, int32 W, uint32 views, uint32 V, uint32 F, float near, then views x 16 floats (fx fy cx cy, R row major, T),
//        V x 3 float vertices, F x 3 int32 indices
//   OUT: views x H x W uint64 keys, (bits(z) << 32) | face of the winner, all-ones where no face covers the pixel
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mesh_raster.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 3;
    int32_t size[2];
    uint32_t cnt[3];
    float near;
    if (fread(size, 4, 2, in) != 2 || fread(cnt, 4, 3, in) != 3 || fread(&near, 4, 1, in) != 1) return 3;
    const int32_t H = size[0], W = size[1];
    const uint32_t n = cnt[0], V = cnt[1], F = cnt[2];
    if (H < 1 || W < 1 || (int64_t)H * W >= (1 << 28) || n > 4096 || V >= (1u << 31) || F >= (1u << 31)) return 3;
    static_assert(sizeof(envgs_mesh_raster_view) == 64, "16 floats per view");
    std::vector<envgs_mesh_raster_view> views(n);
    std::vector<float> vertices(3 * (size_t)V);
    std::vector<int32_t> faces(3 * (size_t)F);
    if (n && fread(views.data(), 64, n, in) != n) return 3;
    if (V && fread(vertices.data(), 12, V, in) != V) return 3;
    if (F && fread(faces.data(), 12, F, in) != F) return 3;
    fclose(in);

    const size_t HW = (size_t)H * (size_t)W;
    std::vector<uint64_t> keys(n * HW, envgs::MR_EMPTY);
    for (uint32_t vi = 0; vi < n; vi++) {
        uint64_t *img = keys.data() + vi * HW;
        for (uint32_t f = 0; f < F; f++) {
            envgs::MrVertex c[3];
            bool ok = true;
            for (int k = 0; k < 3 && ok; k++) {
                const int32_t idx = faces[3 * (size_t)f + k];
                ok = idx >= 0 && (uint32_t)idx < V;
                if (ok) c[k] = envgs::mr_project(views[vi], vertices[3 * (size_t)idx], vertices[3 * (size_t)idx + 1], vertices[3 * (size_t)idx + 2], near);
            }
            envgs::MrFace face;
            if (!ok || !envgs::mr_setup(c[0], c[1], c[2], face)) continue;
            int32_t x0, x1, y0, y1;
            envgs::mr_box(face, H, W, x0, x1, y0, y1);
            for (int32_t py = y0; py <= y1; py++)
                for (int32_t px = x0; px <= x1; px++) {
                    int64_t E[3];
                    if (!envgs::mr_covers(face, px, py, E)) continue;
                    const uint64_t key = envgs::mr_key(envgs::mr_depth(face, E), f);
                    uint64_t &dst = img[(size_t)py * (size_t)W + (size_t)px];
                    if (key < dst) dst = key;
                }
        }
    }

    FILE *out = fopen(argv[2], "wb");
    if (!out) return 4;
    if (!keys.empty() && fwrite(keys.data(), 8, keys.size(), out) != keys.size()) return 4;
    return fclose(out) ? 4 : 0;
}
