// mesh_unionfind.h -- lock-free union-find over vertex indices, written against an atomics policy so that the HIP kernels of mesh_clean.hip
// and a stand-alone host program (mesh_unionfind_host.cpp: std::atomic cells, std::thread workers; built and run by tests/test_mesh_clean_cpu.py)
// execute exactly this code.
//
// A policy `A` gives
//     typename A::cell                                  one 32-bit parent word
//     uint32_t A::load(const cell *p)                   relaxed atomic load
//     void     A::store(cell *p, uint32_t v)            relaxed atomic store
//     uint32_t A::cas(cell *p, uint32_t expect, uint32_t desired)      compare-and-swap, returns the word that was there
//
// Invariant: parent[x] <= x at every moment (x is a root iff parent[x] == x).  The caller initialises parent[x] = x; uf_unite only ever replaces
// a root's own index by a SMALLER index; the path halving of uf_find stores, into a vertex that is no root any more, an index that was an ancestor
// of it when it was read (a plain relaxed store: a late one may put an older, farther ancestor back, which costs steps and nothing else; a
// compare-and-swap on a non-root always fails, so no hook is overwritten).  So every chain descends strictly, the forest never has a cycle, and
// once everything is united the root of a component is its SMALLEST vertex index whatever the schedule was: that is what makes the labelling
// deterministic.
//
// No loop here waits for another thread.  uf_find walks a strictly descending chain.  uf_unite retries only after a failed compare-and-swap,
// and resumes from the word that compare-and-swap returned, which is below the index it tried to hook: at most `hi` retries, each one caused
// by another thread's successful hook, none depending on what a later load observes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ENVGS_UF_FN __host__ __device__ __forceinline__
#else
#define ENVGS_UF_FN inline
#endif

namespace envgs {

// root of x, halving the path on the way
template <class A>
ENVGS_UF_FN uint32_t uf_find(typename A::cell *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = A::load(parent + x);
        if (p == x) return x;
        const uint32_t gp = A::load(parent + p);
        if (gp == p) return p;
        A::store(parent + x, gp);                                 // x is not a root and never becomes one again, so no hook is lost
        x = gp;
    }
}

// root of x without writing anything
template <class A>
ENVGS_UF_FN uint32_t uf_root(const typename A::cell *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = A::load(parent + x);
        if (p == x) return x;
        x = p;
    }
}

// joins the sets of a and b: the larger root is hooked under the smaller
template <class A>
ENVGS_UF_FN void uf_unite(typename A::cell *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = uf_find<A>(parent, a);
        b = uf_find<A>(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }       // a = the larger root
        const uint32_t was = A::cas(parent + a, a, b);
        if (was == a) return;
        a = was;                                                  // somebody hooked a first: go on from where they put it (was < a)
    }
}

// one face: its indices are joined iff all three lie in [0, V); returns whether they do
template <class A>
ENVGS_UF_FN bool uf_hook_face(typename A::cell *parent, uint32_t V, int32_t i0, int32_t i1, int32_t i2)
{
    const uint32_t a = (uint32_t)i0, b = (uint32_t)i1, c = (uint32_t)i2;  // a negative index becomes >= 2^31 > V
    if (a >= V || b >= V || c >= V) return false;
    if (a != b) uf_unite<A>(parent, a, b);
    if (b != c) uf_unite<A>(parent, b, c);
    return true;
}

// after every face is hooked: parent[x] = root of x.  Concurrent flattening is safe: whatever a walker reads is an ancestor.
template <class A>
ENVGS_UF_FN uint32_t uf_flatten(typename A::cell *parent, uint32_t x)
{
    const uint32_t r = uf_root<A>(parent, x);
    if (r != x) A::store(parent + x, r);
    return r;
}

}  // namespace envgs
