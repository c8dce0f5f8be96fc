// The tag stop filter behind the token spans: a compaction of the finished CSR (token_offsets, token_ends, token_tags of token_spans_kernel<true>)
// that drops every token one of whose slots carries a tag of the stop set, and writes for the kept ones what a dropped neighbour takes away:
// token_starts (the entry in front is no longer the token's start) and token_positions (an index is no longer a position).  A pass of its own --
// not fused into the span kernel, where a run's size would come to depend on its records --: a keep-flag count per workgroup, the chained scan
// (launch_scan, kernels_emit.hip), a scatter; the shape of the pattern tagger's merge, no sort and no atomics on anything that decides an order,
// so two runs give identical bytes.  A wave counts with ballots.  Without a stop set every token is kept: the same pass writes the trivial
// starts and positions.
// A workgroup takes kTokenFilterBlock consecutive tokens, a token a thread.  The number of tokens is on the device (token_offsets[n]); the grid
// is sized by the caller's bound and workgroups past the end do nothing.  Whatever the arrays hold, a token index is below min(token_offsets[n],
// capacity_in) before it indexes anything, a document index at most n, an output place below capacity_out.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"

namespace vpt {
namespace {

constexpr uint32_t kFilterWaves = kTokenFilterBlock / 64;

__device__ __forceinline__ uint64_t filter_tokens(const TokenFilterParams& P) {
    const uint64_t n = P.token_offsets[P.n_docs];
    return n < P.capacity_in ? n : P.capacity_in;
}
// a token is stopped when a slot's tag is in the slot's bitmap: ids of the predictor's vocabulary (>= 0), ids of the tagger's (-(2 + id)); None never
__device__ __forceinline__ bool filter_keep(const TokenFilterParams& P, uint64_t tok) {
    bool stop = false;
    for (uint32_t j = 0; j < P.n_tags; ++j) {
        const int32_t v = P.token_tags[tok * P.n_tags + j];
        if (v >= 0) {
            if (P.model_bits && uint32_t(v) < P.n_vocab) stop |= ((P.model_bits[size_t(j) * P.model_words + (uint32_t(v) >> 5)] >> (uint32_t(v) & 31u)) & 1u) != 0;
        } else if (v <= -2) {
            const uint32_t id = uint32_t(-2 - v);
            if (P.rule_bits && id < P.n_rule) stop |= ((P.rule_bits[size_t(j) * P.rule_words + (id >> 5)] >> (id & 31u)) & 1u) != 0;
        }
    }
    return !stop;
}
// the kept tokens of the workgroup in front of this thread's, and (*total) all of them
__device__ __forceinline__ uint32_t filter_rank(bool keep, uint32_t* wtot, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t bal = __ballot(keep);
    if (lane == 0) wtot[wave] = uint32_t(__popcll(bal));
    __syncthreads();
    uint32_t before = uint32_t(__popcll(bal & ((uint64_t(1) << lane) - 1u))), tot = 0;
    for (uint32_t k = 0; k < kFilterWaves; ++k) { const uint32_t u = wtot[k]; if (k < wave) before += u; tot += u; }
    *total = tot;
    return before;
}

__global__ __launch_bounds__(kTokenFilterBlock) void token_filter_count_kernel(const TokenFilterParams P) {
    __shared__ uint32_t wtot[kFilterWaves];
    const uint64_t n_tok = filter_tokens(P), tok = uint64_t(blockIdx.x) * kTokenFilterBlock + threadIdx.x;
    const bool keep = tok < n_tok && filter_keep(P, tok);
    uint32_t total;
    filter_rank(keep, wtot, &total);
    if (threadIdx.x == 0) P.counts[uint64_t(blockIdx.x) + 1] = total;
}

__global__ __launch_bounds__(kTokenFilterBlock) void token_filter_scatter_kernel(const TokenFilterParams P) {
    __shared__ uint32_t wtot[kFilterWaves];
    const uint64_t n_tok = filter_tokens(P), tok = uint64_t(blockIdx.x) * kTokenFilterBlock + threadIdx.x;
    const bool in = tok < n_tok, keep = in && filter_keep(P, tok);
    uint32_t total;
    const uint64_t rank = P.counts[blockIdx.x] + filter_rank(keep, wtot, &total);   // (counts: the scan's exclusive prefix of the workgroups)
    if (in) {
        // the token's document: the last one whose range starts at or in front of it
        uint64_t lo = 0, hi = P.n_docs;   // token_offsets[lo] <= tok as far as the offsets are offsets
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (P.token_offsets[mid] <= tok) lo = mid; else hi = mid - 1;
        }
        const uint64_t first = P.token_offsets[lo];
        if (first == tok)   // the document's first token: its range, and that of every empty document in front of it, starts at the token's rank
            for (uint64_t d = lo;; --d) {
                if (P.token_offsets[d] != tok) break;
                P.out_offsets[d] = rank;
                if (d == 0) break;
            }
        if (keep && rank < P.capacity_out) {
            P.out_starts[rank] = first < tok ? P.token_ends[tok - 1] : 0u;
            P.out_ends[rank] = P.token_ends[tok];
            P.out_positions[rank] = first <= tok ? uint32_t(tok - first) : 0u;
            for (uint32_t j = 0; j < P.n_tags; ++j) P.out_tags[rank * P.n_tags + j] = P.token_tags[tok * P.n_tags + j];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // the end, and the documents that begin there (empty ones behind the last token)
        const uint64_t kept = P.counts[P.n_blocks];
        for (uint64_t d = P.n_docs;; --d) {
            if (P.token_offsets[d] < n_tok) break;
            P.out_offsets[d] = kept;
            if (d == 0) break;
        }
        if (P.total_out) *P.total_out = kept;
    }
}

}  // namespace

hipError_t launch_token_filter(const TokenFilterParams& P, uint64_t* scan_part, hipStream_t stream) {
    hipLaunchKernelGGL(token_filter_count_kernel, dim3(uint32_t(P.n_blocks)), dim3(kTokenFilterBlock), 0, stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan(P.counts, P.n_blocks, scan_part, P.capacity_out, P.status, nullptr, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(token_filter_scatter_kernel, dim3(uint32_t(P.n_blocks)), dim3(kTokenFilterBlock), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
