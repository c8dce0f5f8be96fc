// The vocabulary counter (vocab_count.hpp; VocabCounterView, kernels.hpp): token surface -> 64-bit count, accumulated on the device over the
// FINISHED span CSRs of a corpus (the id pass's conventions and its definition of a surface, vocab_resolve.h), so that corpus -> vocabulary ->
// ids runs without a token string leaving the device.  A count call is THREE launches over the batch's tokens, a lane per token in tiles of
// kVocabTile; the launch boundaries are the only ordering relied on.
//   keys      token -> document, start, end (vocab_resolve.h); at most max_chars chars decoded (strict UTF-8) and hashed with the vocabulary's
//             hash; one record per token into the batch's scratch.  Not counted, and one more in ctrl[kVcSkipped] (summed per wave before the
//             atomic): an empty token, one that is not strict UTF-8 inside its span, one of more than max_chars chars; one of more than
//             4 * max_chars bytes is not even read.  A token the arrays do not describe is kErrBadTokenCsr and neither.
//   insert    a lane probes from its home slot.  Empty: compare-and-swap (token index + 1) in; the winner notes the slot in its own record.  A
//             representative of this call: hash and chars from the records, then the two surfaces char by char as they are looked up -- both
//             live in the immutable text, nothing has to be published.  A committed key: chars and fingerprint, then the arena's code points.
//             A match is one atomic add on the slot's count; a mismatch moves on to the next slot.
//   commit    every representative takes a key index and arena space by atomic add, decodes its surface once more into the arena, writes its
//             key record and stores the committed word into its slot.
// NO LANE EVER WAITS for another: every probe loop is bounded by n_slots, there is no lock, no spin and no retry-until.  Where a lane cannot go
// on -- more than max_keys keys, more than arena_chars code points, a probe that has seen every slot -- it sets the sticky `full` word and the
// batch's kErrVocabCounterFull and goes on; a counter that is full is left alone by every later launch until it is reset.
// Counts are integer atomics: the result does not depend on the order of the lanes.  No kernel keeps an array of chars: no scratch.
// Every index is bounded before it indexes anything: a representative's token index below the batch's tokens, a key index below max_keys, a
// key's code points inside the arena, a slot below n_slots.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"
#include "pattern_tagger.hpp"
#include "vocab_resolve.h"

namespace vpt {
namespace {

__device__ __forceinline__ uint32_t* vc_full_word(const VocabCounterView& C) { return reinterpret_cast<uint32_t*>(C.ctrl + kVcFull); }
__device__ __forceinline__ bool vc_is_full(const VocabCounterView& C) { return *reinterpret_cast<const volatile uint32_t*>(C.ctrl + kVcFull) != 0; }
__device__ __forceinline__ void vc_set_full(const VocabCountParams& P) {
    atomicOr(vc_full_word(P.C), 1u);
    atomicOr(P.status, kErrVocabCounterFull);
}
__device__ __forceinline__ void vc_add(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
__device__ __forceinline__ uint64_t vc_fetch_add(uint64_t* p, uint64_t v) {
    return uint64_t(atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v));
}
// the lanes of a wave that hold `mine`, added to *p by one of them (every lane of the wave comes here)
__device__ __forceinline__ void vc_wave_add(uint64_t* p, bool mine) {
    const uint64_t m = __ballot(mine);
    if ((threadIdx.x & 63u) == 0 && m) vc_add(p, uint64_t(__popcll(m)));
}

__global__ __launch_bounds__(kVocabTile) void vocab_count_keys_kernel(const VocabCountParams P) {
    __shared__ uint64_t soff[kVocabLdsOffsets];   // token_offsets[d_lo ..]: the tile's documents and the end of the last
    __shared__ uint64_t edge[2];                  // d_lo, d_hi
    const uint32_t tid = threadIdx.x;
    uint32_t err = vocab_check_offsets(P);
    if (blockIdx.x == 0 && tid == 0 && vc_is_full(P.C)) err |= kErrVocabCounterFull;   // full since an earlier call: said again at this sync
    const uint64_t n_tok = vocab_token_count(P);
    const uint64_t t0 = uint64_t(blockIdx.x) * kVocabTile;
    if (t0 >= n_tok) {   // (the whole workgroup: nothing below is reached by a part of it)
        if (err) atomicOr(P.status, err);
        return;
    }
    uint64_t d_lo;
    const uint32_t n_own = vocab_tile_slice(P, n_tok, t0, soff, edge, &d_lo);
    const uint64_t tok = t0 + tid;
    bool skipped = false;
    if (tok < n_tok) {
        uint64_t db, h = 0;
        uint32_t start, end, chars = 0;
        const bool ok = vocab_token_span(P, tok, n_own, d_lo, soff, &db, &start, &end);
        if (!ok) err |= kErrBadTokenCsr;
        const uint32_t nbytes = ok ? end - start : 0u;
        const uint64_t b_at = ok ? db + start : 0ull;
        if (nbytes != 0 && uint64_t(nbytes) <= 4ull * P.C.max_chars) {
            const uint64_t b_end = b_at + nbytes;
            uint64_t at = b_at;
            uint32_t len = 0;
            bool key = true;
            h = kRuleHashSeed;
            while (at < b_end) {
                uint32_t cp;
                if (len == P.C.max_chars || !vocab_next_char(P.text, &at, b_end, P.cinfo, &cp)) { key = false; break; }
                h = rule_hash_step(h, cp);
                ++len;
            }
            if (key) { h = rule_hash_finish(h, len); chars = len; }
        }
        skipped = ok && chars == 0;
        P.rec[2 * tok] = make_uint4(uint32_t(h), uint32_t(h >> 32), uint32_t(b_at), uint32_t(b_at >> 32));
        P.rec[2 * tok + 1] = make_uint4(nbytes, chars, kVcNoSlot, 0u);
    }
    vc_wave_add(P.C.ctrl + kVcSkipped, skipped);
    if (err) atomicOr(P.status, err);
}

__global__ __launch_bounds__(kVocabTile) void vocab_count_insert_kernel(const VocabCountParams P) {
    const uint64_t tok = uint64_t(blockIdx.x) * kVocabTile + threadIdx.x;
    const uint64_t n_tok = vocab_token_count(P);
    const bool was_full = vc_is_full(P.C);
    bool counted = false;
    if (tok < n_tok && !was_full) {
        const uint4 r0 = P.rec[2 * tok], r1 = P.rec[2 * tok + 1];
        const uint32_t chars = r1.y;
        if (chars != 0) {
            const uint64_t h = uint64_t(r0.x) | (uint64_t(r0.y) << 32), b_at = uint64_t(r0.z) | (uint64_t(r0.w) << 32), b_end = b_at + r1.x;
            const uint32_t fp = r0.y, mask = P.C.n_slots - 1u;
            uint32_t slot = uint32_t(h) & mask, found = kVcNoSlot;
            for (uint32_t tries = 0; tries <= mask; ++tries, slot = (slot + 1) & mask) {   // every slot once at most
                uint64_t e = P.C.slots[slot];
                if (e == 0) {
                    e = atomic_cas_u64(P.C.slots + slot, 0, tok + 1);
                    if (e == 0) {   // this token represents its surface in this call
                        P.rec[2 * tok + 1].z = slot;
                        found = slot;
                        break;
                    }
                }
                bool same;
                if (e & kVcCommitted) {
                    const uint64_t k = e & ~kVcCommitted;
                    same = k < P.C.max_keys;
                    uint4 key = make_uint4(0, 0, 0, 0);
                    if (same) key = P.C.keys[k];
                    same = same && key.y == chars && key.z == fp && uint64_t(key.x) + chars <= P.C.arena_chars;
                    uint64_t v = b_at;
                    for (uint32_t j = 0; j < chars && same; ++j) {
                        uint32_t cp = 0;
                        same = vocab_next_char(P.text, &v, b_end, P.cinfo, &cp) && P.C.arena[key.x + j] == cp;
                    }
                } else {
                    const uint64_t o = e - 1;
                    if (o >= n_tok) break;   // no token of this call (a counter that was not reset after a call failed): full
                    const uint4 q0 = P.rec[2 * o], q1 = P.rec[2 * o + 1];
                    same = q0.x == r0.x && q0.y == r0.y && q1.y == chars;
                    uint64_t v = b_at, w = uint64_t(q0.z) | (uint64_t(q0.w) << 32);
                    const uint64_t w_end = w + q1.x;
                    for (uint32_t j = 0; j < chars && same; ++j) {
                        uint32_t ca = 0, cb = 1;
                        same = vocab_next_char(P.text, &v, b_end, P.cinfo, &ca) && vocab_next_char(P.text, &w, w_end, P.cinfo, &cb) && ca == cb;
                    }
                }
                if (same) { found = slot; break; }
            }
            if (found != kVcNoSlot) {
                vc_add(P.C.counts + found, 1);
                counted = true;
            } else {
                vc_set_full(P);
            }
        }
    }
    vc_wave_add(P.C.ctrl + kVcCounted, counted);
}

__global__ __launch_bounds__(kVocabTile) void vocab_count_commit_kernel(const VocabCountParams P) {
    const uint64_t tok = uint64_t(blockIdx.x) * kVocabTile + threadIdx.x;
    const uint64_t n_tok = vocab_token_count(P);
    if (tok >= n_tok || vc_is_full(P.C)) return;
    const uint4 r0 = P.rec[2 * tok], r1 = P.rec[2 * tok + 1];
    const uint32_t chars = r1.y, slot = r1.z;
    if (chars == 0 || slot >= P.C.n_slots || P.C.slots[slot] != tok + 1) return;   // no representative
    const uint64_t k = vc_fetch_add(P.C.ctrl + kVcKeys, 1);
    if (k >= P.C.max_keys) { vc_set_full(P); return; }
    const uint64_t first = vc_fetch_add(P.C.ctrl + kVcArena, chars);
    if (first > P.C.arena_chars || chars > P.C.arena_chars - first) { vc_set_full(P); return; }
    uint64_t v = uint64_t(r0.z) | (uint64_t(r0.w) << 32);
    const uint64_t v_end = v + r1.x;
    for (uint32_t j = 0; j < chars; ++j) {
        uint32_t cp = 0;
        if (!vocab_next_char(P.text, &v, v_end, P.cinfo, &cp)) break;   // (the key pass decoded these very bytes)
        P.C.arena[first + j] = cp;
    }
    P.C.keys[k] = make_uint4(uint32_t(first), chars, r0.y, 0u);
    P.C.slots[slot] = kVcCommitted | k;
}

__global__ __launch_bounds__(kVocabTile) void vocab_count_finish_kernel(const VocabCounterView C, uint64_t min_count) {
    const uint32_t slot = blockIdx.x * kVocabTile + threadIdx.x;
    if (slot >= C.n_slots) return;
    const uint64_t e = C.slots[slot];
    if (!(e & kVcCommitted)) return;
    const uint64_t k = e & ~kVcCommitted, count = C.counts[slot];
    if (k >= C.max_keys || count < min_count) return;
    const uint4 key = C.keys[k];
    const uint64_t i = vc_fetch_add(C.ctrl + kVcOut, 1);
    if (i < C.max_keys) C.out[i] = make_uint4(uint32_t(count), uint32_t(count >> 32), key.x, key.y);
}

}  // namespace

hipError_t launch_vocab_count(const VocabCountParams& P, hipStream_t stream) {
    if (P.n_docs == 0) return hipSuccess;
    const uint64_t blocks = P.capacity_in ? (P.capacity_in + kVocabTile - 1) / kVocabTile : 1;
    hipLaunchKernelGGL(vocab_count_keys_kernel, dim3(uint32_t(blocks)), dim3(kVocabTile), 0, stream, P);
    hipLaunchKernelGGL(vocab_count_insert_kernel, dim3(uint32_t(blocks)), dim3(kVocabTile), 0, stream, P);
    hipLaunchKernelGGL(vocab_count_commit_kernel, dim3(uint32_t(blocks)), dim3(kVocabTile), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_vocab_count_finish(const VocabCounterView& C, uint64_t min_count, hipStream_t stream) {
    hipLaunchKernelGGL(vocab_count_finish_kernel, dim3((C.n_slots + kVocabTile - 1) / kVocabTile), dim3(kVocabTile), 0, stream, C, min_count);
    return hipGetLastError();
}

}  // namespace vpt
