// mesh_rng.h -- the counter hash of the surface sampler (include/envgs_mesh.h, "evaluation"): a stateless uint32 hash of (seed, face, counter), so
// that sample k of face f is the same number whichever lane computes it.  Usable on host and device: mesh_eval.hip samples with it, and a
// stand-alone host program (mesh_rng_host.cpp; built and run by tests/test_mesh_eval_cpu.py) prints it for the test against the NumPy oracle.
//
//   mix(x):        x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16          (all on uint32)
//   h(seed, f, j) = mix(mix(mix(seed) ^ f) ^ j)
//   uniform(h)    = (float)(h >> 8) * 2^-24: a multiple of 2^-24 in [0, 1), exact in fp32
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ENVGS_RNG_FN __host__ __device__ __forceinline__
#else
#define ENVGS_RNG_FN inline
#endif

namespace envgs {

constexpr uint32_t RNG_COUNT_STREAM = 0xffffffffu;               // the counter of a face's rounding draw; samples use 2k and 2k + 1
// The counter of a point's thinning key, key(i) = rng_hash(seed, i, RNG_THIN_STREAM).  rng_mix is a bijection of uint32 (xor-shifts and odd
// multipliers are invertible) and so is xor with a constant, so for a fixed seed i -> key(i) is a permutation of uint32: the keys of distinct
// points are distinct and the order by key is strict without a tie-break.
constexpr uint32_t RNG_THIN_STREAM = 0xfffffffeu;

ENVGS_RNG_FN uint32_t rng_mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

ENVGS_RNG_FN uint32_t rng_hash(uint32_t seed, uint32_t f, uint32_t j) { return rng_mix(rng_mix(rng_mix(seed) ^ f) ^ j); }

// the 24 bits a uniform is made of, and the uniform
ENVGS_RNG_FN uint32_t rng_bits24(uint32_t h) { return h >> 8; }
ENVGS_RNG_FN float rng_uniform(uint32_t h) { return (float)(h >> 8) * 5.9604644775390625e-08f; }

}  // namespace envgs
