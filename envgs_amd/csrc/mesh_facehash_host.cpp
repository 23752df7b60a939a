// mesh_facehash_host.cpp -- the face table of mesh_facehash.h on the CPU: std::atomic slots, std::thread workers.  Not part of libenvgs_hip.so
// (build.py compiles the .hip files only); tests/test_mesh_simplify_cpu.py builds it with the host compiler and compares the survivors with the
// oracle's.  It is a program of its own, so it can also be built with -fsanitize=thread or -fsanitize=address,undefined and run by hand.
//
//   mesh_facehash_host IN OUT THREADS
//   IN : uint32 F, then F x 3 int32 mapped faces (cluster numbers), then F uint8 candidate flags (0 = dropped before the table)
//   OUT: F uint8: 1 = the face survives (a candidate, and the lowest index of its triple up to rotation)
//
// The workers take the faces in interleaved chunks of 16, so that neighbouring faces, which are the likely duplicates, are entered by
// different threads at the same time.  The two passes (enter, then compare the slot with the own index) are those of mesh_simplify.hip.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "mesh_facehash.h"

struct HostAtomics {
    typedef std::atomic<uint32_t> cell;
    static uint32_t load(const cell *p) { return p->load(std::memory_order_relaxed); }
    static uint32_t cas(cell *p, uint32_t expect, uint32_t desired)
    {
        p->compare_exchange_strong(expect, desired, std::memory_order_relaxed);
        return expect;                                            // unchanged on success, the observed word on failure
    }
    static void min(cell *p, uint32_t v)
    {
        uint32_t cur = p->load(std::memory_order_relaxed);
        while (v < cur && !p->compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
    }
};

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s IN OUT THREADS\n", argv[0]); return 2; }
    const int T = atoi(argv[3]);
    if (T < 1 || T > 256) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t F;
    if (fread(&F, 4, 1, in) != 1 || F >= (1u << 31)) return 3;
    std::vector<int32_t> tri(3 * (size_t)F);
    std::vector<uint8_t> keep(F);
    if (F && (fread(tri.data(), 12, F, in) != F || fread(keep.data(), 1, F, in) != F)) return 3;
    fclose(in);

    const uint64_t slots = envgs::fh_slots(F);
    std::vector<std::atomic<uint32_t>> table(slots);
    for (auto &s : table) s.store(envgs::FH_EMPTY, std::memory_order_relaxed);
    std::vector<uint32_t> slot(F);
    constexpr uint32_t CHUNK = 16;
    auto work = [&](int t, int pass) {
        for (uint32_t f0 = (uint32_t)t * CHUNK; f0 < F; f0 += (uint32_t)T * CHUNK)
            for (uint32_t f = f0; f < F && f < f0 + CHUNK; f++) {
                if (!keep[f]) continue;
                if (pass == 0) slot[f] = envgs::fh_insert<HostAtomics>(table.data(), slots, tri.data(), f);
                else keep[f] = HostAtomics::load(&table[slot[f]]) == f;
            }
    };
    for (int pass = 0; pass < 2; pass++) {
        std::vector<std::thread> pool;
        for (int t = 0; t < T; t++) pool.emplace_back([&, t] { work(t, pass); });
        for (auto &th : pool) th.join();
    }

    FILE *out = fopen(argv[2], "wb");
    if (!out) return 4;
    fwrite(keep.data(), 1, F, out);
    return fclose(out) ? 4 : 0;
}
