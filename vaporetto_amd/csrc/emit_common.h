// What the flat kernels over runs of sentences share (kernels_emit.hip: the writer; kernels_tokens.hip: the token spans): the workgroup's
// shape, its prefix sums, the label masks, and the chain of the runs' positions (ONE decoupled look-back per workgroup).
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"

namespace vpt {

constexpr int kEmitThreads = 256;
constexpr int kEmitWaves = kEmitThreads / 64;

__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {   // total over the 64 lanes, in every lane
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(x)), d)), hi = uint32_t(__shfl_xor(int(uint32_t(x >> 32)), d));
        x += uint64_t(lo) | (uint64_t(hi) << 32);
    }
    return x;
}

__device__ __forceinline__ uint32_t one_flags(uint32_t y) { return zero_bytes(y ^ 0x01010101u); }   // bytes equal to 1
__device__ __forceinline__ uint32_t one16(const uint4& y) { return flag_bytes_to_mask16(one_flags(y.x), one_flags(y.y), one_flags(y.z), one_flags(y.w)); }
__device__ __forceinline__ uint32_t unk_flags(uint32_t y) { return ~zero_bytes(y & 0xFEFEFEFEu) & 0x80808080u; }   // bytes above 1
__device__ __forceinline__ uint32_t unk16(const uint4& y) { return flag_bytes_to_mask16(unk_flags(y.x), unk_flags(y.y), unk_flags(y.z), unk_flags(y.w)); }
// which of the 16 bytes at offset `off` lie in [lo, hi) (offsets from the same base)
__device__ __forceinline__ uint32_t in_range16_rel(uint32_t off, uint32_t lo, uint32_t hi) {
    const uint32_t a = lo > off ? (lo - off < 16u ? lo - off : 16u) : 0u;
    const uint32_t b = hi > off ? (hi - off < 16u ? hi - off : 16u) : 0u;
    return ((1u << b) - 1u) & ~((1u << a) - 1u);   // (b < a: nothing)
}

// exclusive prefix sum of x over the workgroup's threads (two packed 16-bit counts or one 32-bit one); *total = the sum.  kAgain: the same wtot
// serves the next sum at once (a loop of sums) -- a second barrier; the sums of a piece that come once have words of their own and take one
template <bool kAgain = true>
__device__ __forceinline__ uint32_t flat_block_scan(uint32_t x, uint32_t* wtot, uint32_t lane, uint32_t wave, uint32_t* total) {
    const uint32_t incl = wave_inclusive_scan(x);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < uint32_t(kEmitWaves); ++k) {
        const uint32_t u = wtot[k];
        if (k < wave) woff += u;
        tot += u;
    }
    if (kAgain) __syncthreads();   // wtot is written again by the next sum
    *total = tot;
    return woff + incl - x;
}

// The chain of the runs' positions (one word per run: flag << 62 | value; 1: the run's size, 2: the position behind it).  A run's size is
// published as soon as it is known; the WAVE that calls place_run walks back over the earlier runs' words, 64 per trip, until one holds a
// position, publishes the run's own and returns where the run starts.
__device__ __forceinline__ void publish_run_size(const EmitFuse& F, uint64_t blk, uint64_t size) {
    __hip_atomic_store(F.state + blk, (uint64_t(1) << 62) | size, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t place_run(const EmitFuse& F, uint64_t blk, uint64_t size, uint32_t lane) {
    constexpr uint64_t kVal = (uint64_t(1) << 62) - 1;
    const uint64_t start = (F.chain_in ? *F.chain_in : 0ull) & kVal;   // where the call's text starts (a call chained behind another: EmitFuse)
    uint64_t base = 0;
    bool anchored = false;   // the sum has reached a run whose position is known (or the front's sentinel): it holds `start`
    for (uint64_t p = blk; p > 0;) {
        const bool have = uint64_t(lane) < p;
        uint64_t w = (uint64_t(2) << 62) | start;   // in front of run 0
        if (have) w = __hip_atomic_load(F.state + (p - 1 - uint64_t(lane)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t pending = __ballot((w >> 62) == 0), prefixed = __ballot((w >> 62) == 2);
        const int first = prefixed ? __ffsll((long long)prefixed) - 1 : 64;   // the nearest run whose position is known
        const uint64_t need = first < 63 ? (uint64_t(2) << first) - 1 : ~uint64_t(0);
        if (pending & need) { __builtin_amdgcn_s_sleep(2); continue; }         // not all published yet: look again
        base += wave_sum64(int(lane) <= first ? (w & kVal) : 0);
        if (first < 64) { anchored = true; break; }
        p -= 64;
    }
    // run 0, or a walk that ran off the front exactly at a multiple of 64 runs with none of them placed yet (then no lane held the sentinel:
    // found on MI355X by the chained chunks of vpt_tokenize_batch with one-sentence runs -- a misplaced run's text landed in an earlier chunk's)
    if (!anchored) base += start;
    if (lane == 0) {
#ifndef VPT_EMIT_NO_PREFIX   // (test builds, tests/test_kernel_emu.py: the runs publish their sizes only, so every look-back walks to the launch's front)
        __hip_atomic_store(F.state + blk, (uint64_t(2) << 62) | ((base + size) & kVal), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    }
    return base;
}

}  // namespace vpt
