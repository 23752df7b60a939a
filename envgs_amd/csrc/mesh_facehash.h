// mesh_facehash.h -- lock-free table that finds, among faces given as oriented triples of cluster numbers, the lowest face index of every
// triple up to cyclic rotation.  Written against an atomics policy so that the HIP kernels of mesh_simplify.hip and a stand-alone host program
// (mesh_facehash_host.cpp: std::atomic slots, std::thread workers; built and run by tests/test_mesh_simplify_cpu.py) execute exactly this code.
//
// A policy `A` gives
//     typename A::cell                                  one 32-bit slot
//     uint32_t A::load(const cell *p)                   relaxed atomic load
//     uint32_t A::cas(cell *p, uint32_t expect, uint32_t desired)      compare-and-swap, returns the word that was there
//     void     A::min(cell *p, uint32_t v)              atomic unsigned minimum
//
// The table has a power of two of slots, at least 2 F, all FH_EMPTY at the start.  A slot holds a FACE INDEX; the key of the slot is the
// canonical triple of that face, read from `tri` (the mapped faces, complete before the first insert: written by an earlier kernel / before the
// threads start, never during).  Linear probing, no deletion:
//   * a slot leaves FH_EMPTY exactly once, by the compare-and-swap of the face that claims it, and from then on only ever holds faces of that
//     one key (A::min replaces a face by an equal face of lower index), so its key never changes;
//   * a face walks from its hash until it claims an empty slot or meets a slot of its own key; every slot it passed holds another key for good,
//     so all faces of one key end in the same slot, whatever the schedule.  WHICH slot may depend on the schedule; its final content, the
//     lowest face index of the key, does not.
// No loop waits for another thread: a failed compare-and-swap returns the face that won the slot, and the walker compares keys with it at
// once.  The walk ends within the table because it is at most half full.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ENVGS_FH_FN __host__ __device__ __forceinline__
#else
#define ENVGS_FH_FN inline
#endif

namespace envgs {

constexpr uint32_t FH_EMPTY = 0xffffffffu;

// slots for F faces: the power of two >= max(2 F, 2)
ENVGS_FH_FN uint64_t fh_slots(uint32_t F)
{
    uint64_t n = 2;
    while (n < 2 * (uint64_t)F) n <<= 1;
    return n;
}

struct FhKey { uint32_t a, b, c; };

// rotates the triple so that its smallest member comes first (the members of a face that reaches the table are distinct)
ENVGS_FH_FN FhKey fh_canonical(uint32_t a, uint32_t b, uint32_t c)
{
    FhKey k;
    if (a < b && a < c) { k.a = a; k.b = b; k.c = c; }
    else if (b < c) { k.a = b; k.b = c; k.c = a; }
    else { k.a = c; k.b = a; k.c = b; }
    return k;
}

ENVGS_FH_FN FhKey fh_key_of(const int32_t *tri, uint32_t f)
{
    return fh_canonical((uint32_t)tri[3 * (size_t)f], (uint32_t)tri[3 * (size_t)f + 1], (uint32_t)tri[3 * (size_t)f + 2]);
}

ENVGS_FH_FN uint64_t fh_hash(const FhKey k)
{
    uint64_t h = ((uint64_t)k.a << 32 | k.b) * 0x9e3779b97f4a7c15ull;
    h ^= h >> 29;
    h += k.c;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 32;
    return h;
}

// enters face f; returns the slot of its key
template <class A>
ENVGS_FH_FN uint32_t fh_insert(typename A::cell *table, uint64_t slots, const int32_t *tri, uint32_t f)
{
    const FhKey k = fh_key_of(tri, f);
    uint64_t s = fh_hash(k) & (slots - 1);
    for (;;) {
        uint32_t g = A::load(table + s);
        if (g == FH_EMPTY) {
            g = A::cas(table + s, FH_EMPTY, f);
            if (g == FH_EMPTY) return (uint32_t)s;                // claimed
        }
        const FhKey o = fh_key_of(tri, g);                        // g < F: only face indices are ever stored
        if (o.a == k.a && o.b == k.b && o.c == k.c) {
            if (f < g) A::min(table + s, f);
            return (uint32_t)s;
        }
        s = (s + 1) & (slots - 1);
    }
}

}  // namespace envgs
