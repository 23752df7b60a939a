// radix_select.h -- exact order statistics of up to two ranks by a three-pass radix select over uint32 keys (float_key.h gives the keys of
// floats).  Users: supervisor.hip (depth percentiles; the key is a strided depth read) and densify_device.hip (the average weight; the key is
// computed from two arrays).  What differs between them is only the key functor, where the ranks come from (both pass them from the host) and
// whether the count below each selected value is wanted (`below`, nullable).
//
// digits: bits 31..21 (2048 bins), 20..10 (2048 bins), 9..0 (1024 bins).  Both ranks are selected in the same passes: after pass 0 each has its
// own 11-bit prefix, and passes 1 / 2 histogram only the keys under either prefix.  Integer atomics only (LDS per workgroup, then one global
// add per non-empty bin), so the result does not depend on the order of execution.
#pragma once
#include "common.h"
#include "float_key.h"

namespace envgs {

constexpr int SEL_BINS0 = 2048, SEL_BINS1 = 2048, SEL_BINS2 = 1024;
constexpr int SEL_H0 = 0, SEL_H1 = SEL_H0 + SEL_BINS0, SEL_H2 = SEL_H1 + 2 * SEL_BINS1, SEL_STATE = SEL_H2 + 2 * SEL_BINS2;   // uint32 offsets
constexpr int SEL_WORDS = SEL_STATE + 4;            // state: prefix of either statistic, rank of either inside its prefix
constexpr int SEL_THREADS = 256;

// Keys: a functor passed by value, uint32_t operator()(long long i) const -- the key of element i.
template <int PASS, class Keys>
__global__ void __launch_bounds__(SEL_THREADS)
radix_select_hist(const long long N, uint32_t *__restrict__ temp, const Keys keys)
{
    constexpr int BINS = PASS == 2 ? SEL_BINS2 : SEL_BINS0, SETS = PASS == 0 ? 1 : 2;
    __shared__ uint32_t h[SETS * BINS];
    const int tid = threadIdx.x;
    for (int b = tid; b < SETS * BINS; b += SEL_THREADS) h[b] = 0u;
    uint32_t p0 = 0u, p1 = 0u;
    if (PASS > 0) { p0 = temp[SEL_STATE]; p1 = temp[SEL_STATE + 1]; }
    __syncthreads();
    for (long long i = (long long)blockIdx.x * SEL_THREADS + tid; i < N; i += (long long)gridDim.x * SEL_THREADS) {
        const uint32_t k = keys(i);
        if (PASS == 0) {
            atomicAdd(&h[k >> 21], 1u);
        } else {
            const uint32_t top = PASS == 1 ? (k >> 21) : (k >> 10), dig = PASS == 1 ? ((k >> 10) & 2047u) : (k & 1023u);
            if (top == p0) atomicAdd(&h[dig], 1u);
            if (top == p1) atomicAdd(&h[BINS + dig], 1u);
        }
    }
    __syncthreads();
    uint32_t *g = temp + (PASS == 0 ? SEL_H0 : PASS == 1 ? SEL_H1 : SEL_H2);
    for (int b = tid; b < SETS * BINS; b += SEL_THREADS) {
        const uint32_t v = h[b];
        if (v) atomicAdd(&g[b], v);
    }
}

// One workgroup: the bin that holds rank r of a histogram (the first bin whose inclusive prefix sum exceeds r), for either statistic.  The rank
// left inside the last bin is the number of equal keys before the statistic, so what is below the selected value is the rank minus that.
template <int PASS>
__global__ void __launch_bounds__(SEL_THREADS)
radix_select_pick(const uint32_t rank0, const uint32_t rank1, const int n_ranks, uint32_t *__restrict__ temp, float *__restrict__ values,
                  uint32_t *__restrict__ below)
{
    constexpr int BINS = PASS == 2 ? SEL_BINS2 : SEL_BINS0, PER = BINS / SEL_THREADS;
    __shared__ uint32_t sums[SEL_THREADS];
    const int tid = threadIdx.x;
    uint32_t rank[2], prefix[2];
    if (PASS == 0) { rank[0] = rank0; rank[1] = rank1; prefix[0] = prefix[1] = 0u; }
    else { rank[0] = temp[SEL_STATE + 2]; rank[1] = temp[SEL_STATE + 3]; prefix[0] = temp[SEL_STATE]; prefix[1] = temp[SEL_STATE + 1]; }
    __syncthreads();                                  // every lane holds the state before any lane replaces it
    for (int which = 0; which < 2; which++) {
        const uint32_t *hist = temp + (PASS == 0 ? SEL_H0 : (PASS == 1 ? SEL_H1 : SEL_H2) + which * BINS);
        uint32_t c[PER], s = 0u;
#pragma unroll
        for (int q = 0; q < PER; q++) { c[q] = hist[tid * PER + q]; s += c[q]; }
        sums[tid] = s;
        __syncthreads();
        for (int off = 1; off < SEL_THREADS; off <<= 1) {
            const uint32_t v = tid >= off ? sums[tid - off] : 0u;
            __syncthreads();
            sums[tid] += v;
            __syncthreads();
        }
        const uint32_t incl = sums[tid];
        uint32_t run = incl - s;
        const uint32_t r = rank[which];
        if (r >= run && r < incl) {                   // true in exactly one lane (the total is the number of keys under the prefix, > r)
            int bin = PER - 1;
            bool found = false;
#pragma unroll
            for (int q = 0; q < PER; q++) {           // the first bin whose running total passes r; `run` ends as the count in the bins before it
                if (!found) {
                    if (r < run + c[q]) { bin = q; found = true; }
                    else run += c[q];
                }
            }
            const uint32_t digit = (uint32_t)(tid * PER + bin);
            if (PASS == 0) { temp[SEL_STATE + which] = digit; temp[SEL_STATE + 2 + which] = r - run; }
            if (PASS == 1) { temp[SEL_STATE + which] = (prefix[which] << 11) | digit; temp[SEL_STATE + 2 + which] = r - run; }
            if (PASS == 2 && which < n_ranks) {
                values[which] = float_of_key((prefix[which] << 10) | digit);
                if (below) below[which] = (which ? rank1 : rank0) - (r - run);
            }
        }
        __syncthreads();
    }
}

inline size_t radix_select_temp_bytes() { return (size_t)SEL_WORDS * sizeof(uint32_t); }

// values[0 .. n_ranks) = the rank0-th and rank1-th smallest of the N keys (0-based), decoded as floats; below (if given) the number of keys
// under each.  With n_ranks == 1 pass rank1 = rank0.  temp: radix_select_temp_bytes().  Arguments are the caller's to check.
template <class Keys>
inline int radix_select(const long long N, const Keys keys, const uint32_t rank0, const uint32_t rank1, const int n_ranks, float *values,
                        uint32_t *below, void *temp, hipStream_t s)
{
    uint32_t *t = (uint32_t *)temp;
    hipError_t e = hipMemsetAsync(t, 0, radix_select_temp_bytes(), s);
    if (e != hipSuccess) return (int)e;
    const int blocks = (int)min((long long)512, (long long)((N + SEL_THREADS * 8 - 1) / (SEL_THREADS * 8)));
    hipLaunchKernelGGL((radix_select_hist<0, Keys>), dim3(blocks), dim3(SEL_THREADS), 0, s, N, t, keys);
    hipLaunchKernelGGL(radix_select_pick<0>, dim3(1), dim3(SEL_THREADS), 0, s, rank0, rank1, n_ranks, t, values, below);
    hipLaunchKernelGGL((radix_select_hist<1, Keys>), dim3(blocks), dim3(SEL_THREADS), 0, s, N, t, keys);
    hipLaunchKernelGGL(radix_select_pick<1>, dim3(1), dim3(SEL_THREADS), 0, s, rank0, rank1, n_ranks, t, values, below);
    hipLaunchKernelGGL((radix_select_hist<2, Keys>), dim3(blocks), dim3(SEL_THREADS), 0, s, N, t, keys);
    hipLaunchKernelGGL(radix_select_pick<2>, dim3(1), dim3(SEL_THREADS), 0, s, rank0, rank1, n_ranks, t, values, below);
    return (int)hipGetLastError();
}

}  // namespace envgs
