// What the searches over a postings segment share (kernels_postings_search.hip: the OR search; kernels_postings_phrase.hip: the phrase search;
// kernels_postings_boolean.hip: the boolean search): the bounded bisection, the bits of a binary32 and the score of one posting.  One copy, so
// every search gives a posting the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vpt {

// the first p in [lo, hi] with a[p] >= v, or hi when there is none in [lo, hi): a sorted (non-decreasing) array; at most 64 steps
template <typename T>
__device__ __forceinline__ uint64_t first_at_least(const T* a, uint64_t lo, uint64_t hi, uint64_t v) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (uint64_t(a[mid]) >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ uint32_t bits_of(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
__device__ __forceinline__ float float_of(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// The score of one posting under one weight, in binary32, one rounding per operation, in the order of the definition (include/vaporetto_hip.h).
__device__ __forceinline__ float bm25_term(float w, uint32_t tf, uint32_t dl, float k1, float b, float avgdl) {
#pragma clang fp contract(off)
    const float r = float(dl) / avgdl;
    const float br = b * r;
    const float nb = 1.0f - b;
    const float norm = nb + br;
    const float K = k1 * norm;
    const float f = float(tf);
    const float k11 = k1 + 1.0f;
    const float num = f * k11;
    const float den = f + K;
    const float q = num / den;
    return w * q;
}

}  // namespace vpt
