// mesh_rng_host.cpp -- the counter hash of mesh_rng.h on the CPU.  Not part of libenvgs_hip.so (build.py compiles the .hip files only);
// tests/test_mesh_eval_cpu.py builds it with the host compiler and compares its output with the oracle's hash.  It is a program of its own, so
// it can also be built with -fsanitize=address,undefined and run by hand.
//
//   mesh_rng_host IN OUT
//   IN : uint32 n, then n x 3 uint32 (seed, f, j)
//   OUT: n uint32 h(seed, f, j), then n float32 uniform(h)
#include <cstdio>
#include <vector>

#include "mesh_rng.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t n;
    if (fread(&n, 4, 1, in) != 1 || n > (1u << 28)) return 3;
    std::vector<uint32_t> arg(3 * (size_t)n), h(n);
    std::vector<float> u(n);
    if (n && fread(arg.data(), 12, n, in) != n) return 3;
    fclose(in);
    for (uint32_t i = 0; i < n; i++) {
        h[i] = envgs::rng_hash(arg[3 * (size_t)i], arg[3 * (size_t)i + 1], arg[3 * (size_t)i + 2]);
        u[i] = envgs::rng_uniform(h[i]);
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 4;
    fwrite(h.data(), 4, n, out);
    fwrite(u.data(), 4, n, out);
    return fclose(out) ? 4 : 0;
}
