// mesh_unionfind_host.cpp -- the union-find of mesh_unionfind.h on the CPU: std::atomic parent cells, std::thread workers.  Not part of
// libenvgs_hip.so (build.py compiles the .hip files only); tests/test_mesh_clean_cpu.py builds it with the host compiler and compares its labels with
// the oracle's.  It is a program of its own, so it can also be built with -fsanitize=thread or -fsanitize=address,undefined and run by hand.
//
//   mesh_unionfind_host IN OUT THREADS
//   IN : uint32 V, uint32 F, then F x 3 int32 indices
//   OUT: V int32 vertex labels, F int32 face labels, uint32 C, C int32 faces per component, C int32 vertices per component
//
// The workers take the faces in interleaved chunks of 16, so that neighbouring faces are hooked by different threads at the same time.  The
// labelling after the hooking (flatten, rank the roots that own a face, gather) is the sequence of mesh_clean.hip, written serially.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "mesh_unionfind.h"

struct HostAtomics {
    typedef std::atomic<uint32_t> cell;
    static uint32_t load(const cell *p) { return p->load(std::memory_order_relaxed); }
    static void store(cell *p, uint32_t v) { p->store(v, std::memory_order_relaxed); }
    static uint32_t cas(cell *p, uint32_t expect, uint32_t desired)
    {
        p->compare_exchange_strong(expect, desired, std::memory_order_relaxed);
        return expect;                                            // unchanged on success, the observed word on failure
    }
};

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s IN OUT THREADS\n", argv[0]); return 2; }
    const int T = atoi(argv[3]);
    if (T < 1 || T > 256) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t hdr[2];
    if (fread(hdr, 4, 2, in) != 2) return 3;
    const uint32_t V = hdr[0], F = hdr[1];
    if (V >= (1u << 31) || F >= (1u << 31)) return 3;
    std::vector<int32_t> faces(3 * (size_t)F);
    if (F && fread(faces.data(), 12, F, in) != F) return 3;
    fclose(in);

    std::vector<std::atomic<uint32_t>> parent(V);
    for (uint32_t v = 0; v < V; v++) HostAtomics::store(&parent[v], v);
    std::vector<uint8_t> valid(F);
    constexpr uint32_t CHUNK = 16;
    auto hook = [&](int t) {
        for (uint32_t f0 = (uint32_t)t * CHUNK; f0 < F; f0 += (uint32_t)T * CHUNK)
            for (uint32_t f = f0; f < F && f < f0 + CHUNK; f++)
                valid[f] = envgs::uf_hook_face<HostAtomics>(parent.data(), V, faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]);
    };
    auto flatten = [&](int t) {
        for (uint32_t v0 = (uint32_t)t * CHUNK; v0 < V; v0 += (uint32_t)T * CHUNK)
            for (uint32_t v = v0; v < V && v < v0 + CHUNK; v++) (void)envgs::uf_flatten<HostAtomics>(parent.data(), v);
    };
    for (int pass = 0; pass < 2; pass++) {
        std::vector<std::thread> pool;
        for (int t = 0; t < T; t++) pool.emplace_back([&, t] { if (pass == 0) hook(t); else flatten(t); });
        for (auto &th : pool) th.join();
    }

    std::vector<uint32_t> nf(V, 0), nv(V, 0);
    for (uint32_t f = 0; f < F; f++) if (valid[f]) nf[HostAtomics::load(&parent[(uint32_t)faces[3 * (size_t)f]])]++;
    std::vector<int32_t> rank(V, -1), vlabel(V, -1), flabel(F, -1), cf, cv;
    uint32_t C = 0;
    for (uint32_t v = 0; v < V; v++) if (HostAtomics::load(&parent[v]) == v && nf[v]) rank[v] = (int32_t)C++;
    for (uint32_t v = 0; v < V; v++) {
        const uint32_t r = HostAtomics::load(&parent[v]);
        if (nf[r]) { vlabel[v] = rank[r]; nv[r]++; }
    }
    for (uint32_t v = 0; v < V; v++) if (rank[v] >= 0) { cf.push_back((int32_t)nf[v]); cv.push_back((int32_t)nv[v]); }
    for (uint32_t f = 0; f < F; f++) if (valid[f]) flabel[f] = vlabel[(uint32_t)faces[3 * (size_t)f]];

    FILE *out = fopen(argv[2], "wb");
    if (!out) return 4;
    fwrite(vlabel.data(), 4, V, out);
    fwrite(flabel.data(), 4, F, out);
    fwrite(&C, 4, 1, out);
    fwrite(cf.data(), 4, C, out);
    fwrite(cv.data(), 4, C, out);
    return fclose(out) ? 4 : 0;
}
