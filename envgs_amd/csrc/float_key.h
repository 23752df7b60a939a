// float_key.h -- floats as uint32 words of the same order, host + device (tests/test_float_key.py runs these functions on the CPU).
//
// The mapping flips every bit of a negative float and the sign bit of a non-negative one, so unsigned compare of the keys is the float
// order: -inf < ... < -0 < +0 < ... < +inf (NaNs land beyond the infinities on their sign's side).  No float has key 0 short of a negative
// NaN, so a zeroed word can stand for "nothing yet" under an unsigned max.
//
// Two encoders, deliberately different in one key:
//  * float_key        raw and injective: -0 and +0 keep different keys and float_of_key returns exactly the bits that went in.  For
//                     reductions that must hand back one of their inputs -- densify_device.hip's grow_plan / grow_wmax (atomicMax over the
//                     accumulated weights).
//  * float_key_canon  -0 gets the key of +0 (and decodes as +0).  For everything that ranks, counts or tests equality the way a float
//                     compare does, where -0 == +0: the radix selects (supervisor.hip's depth percentiles, densify_device.hip's weight
//                     statistics) and the tie / below-the-cut tests on their results (tie_flags, visibility_mask).  With the raw encoder a -0
//                     would be counted below a +0 cut that torch calls a tie.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ENVGS_FK_FN __host__ __device__ __forceinline__
#else
#define ENVGS_FK_FN inline
#endif

namespace envgs {

ENVGS_FK_FN uint32_t float_key(float f)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

ENVGS_FK_FN uint32_t float_key_canon(float f)
{
    uint32_t b = __builtin_bit_cast(uint32_t, f);
    if (b == 0x80000000u) b = 0u;                    // -0 orders with +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

ENVGS_FK_FN float float_of_key(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

}  // namespace envgs
