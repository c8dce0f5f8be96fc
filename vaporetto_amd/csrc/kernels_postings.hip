// Postings of a batch (PostingsParams, kernels.hpp): term -> (document, tf) lists from the token ids of a FINISHED span CSR, term-major, by ONE
// stable sort of the batch's tokens by id and a run-length pass.  The call reads token_offsets and token_ids and nothing else: no text.
// The number of tokens is on the device; capacity_in bounds it, so every launch is over the capacity_in PLACES of the arrays, and a place that
// holds no indexed token carries the sentinel key n_terms: the stable sort leaves the indexed tokens in front, by (id, token index), which is
// (term, document, token index).
//   keys     a lane per place in tiles of kVocabTile: the token's owner (vocab_resolve.h: the last i with token_offsets[i] <= t), key = the id or
//            the sentinel, two u32 words {key, document} per place.  Dropped tokens (id < 0 or >= n_terms) are summed per wave with a ballot
//            before one integer atomic add to counts[1].  The offsets are checked once over the grid.
//   (sort)   train_radix_sort over the key word, as it is: ceil(bit_width(n_terms) / 8) passes.
//   heads    a lane per sorted place j: skey[j] = its key (contiguous from here on); a head when the key is below n_terms and j == 0 or the
//            (key, document) before it differs.
//   (scan)   train_scan over the head flags, as it is: scan[j] = the heads in front of j, scan[capacity_in] = the postings.
//   emit     a lane per sorted place: token_order[j]; a head with scan value q writes posting q -- its tf is the distance to the next head, found
//            by a bounded bisection over the scan (the last posting's: to the end of the indexed tokens, a bisection over skey).
//   terms    a lane per k in 0 .. n_terms: term_offsets[k] = the scan at the first sorted place whose key is >= k (a bounded bisection over
//            skey); the lane of n_terms also writes counts[0], post_first's last entry and the too-small bit.
// No atomic decides a value (the one atomic add sums integers), no loop's trip count depends on what another lane has not written, the launch
// boundaries are the only ordering relied on: two runs give identical bytes.  Every index is bounded before it indexes anything: a token below
// min(token_offsets[n], capacity_in), a document below n, a posting below capacity_out, a sorted index below capacity_in.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"
#include "vocab_resolve.h"

namespace vpt {
namespace {

// the first p in [lo, hi] with a[p] >= v, or hi when there is none in [lo, hi): a sorted (non-decreasing) array; at most 64 steps
template <typename T>
__device__ __forceinline__ uint64_t first_at_least(const T* a, uint64_t lo, uint64_t hi, uint64_t v) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (uint64_t(a[mid]) >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kVocabTile) void postings_keys_kernel(const PostingsParams P) {
    __shared__ uint64_t soff[kVocabLdsOffsets];   // token_offsets[d_lo ..]: the tile's documents and the end of the last
    __shared__ uint64_t edge[2];                  // d_lo, d_hi
    const uint32_t tid = threadIdx.x;
    uint32_t err = 0;
    const uint64_t gid = uint64_t(blockIdx.x) * kVocabTile + tid, gstride = uint64_t(gridDim.x) * kVocabTile;
    for (uint64_t i = gid; i < P.n_docs; i += gstride) {   // every entry once over the grid
        const uint64_t a = P.token_offsets[i], b = P.token_offsets[i + 1];
        if (a > b || b > P.capacity_in) err = kErrBadTokenCsr;
    }
    const uint64_t n_tok = vocab_token_count(P);
    const uint64_t t0 = uint64_t(blockIdx.x) * kVocabTile;
    uint64_t d_lo = 0;
    uint32_t n_own = 0;
    if (t0 < n_tok) n_own = vocab_tile_slice(P, n_tok, t0, soff, edge, &d_lo);   // (the whole workgroup or none of it)
    const uint64_t t = t0 + tid;
    bool dropped = false;
    if (t < P.capacity_in) {
        uint32_t key = P.n_terms, doc = 0;
        if (t < n_tok) {
            uint64_t d, first, next;
            if (n_own) {
                const uint32_t j = uint32_t(vocab_owner(soff, uint64_t(n_own), t));
                d = d_lo + j; first = soff[j]; next = soff[j + 1];
            } else {
                d = vocab_owner(P.token_offsets, P.n_docs, t);
                first = P.token_offsets[d]; next = P.token_offsets[d + 1];
            }
            if (first <= t && t < next) {
                const int32_t id = P.ids[t];
                doc = uint32_t(d);
                if (id >= 0 && uint32_t(id) < P.n_terms) key = uint32_t(id); else dropped = true;
            } else {
                err |= kErrBadTokenCsr;   // a token below token_offsets[n] that no document owns
            }
        }
        P.keydoc[2 * t] = key;
        P.keydoc[2 * t + 1] = doc;
    }
    const uint64_t m = __ballot(dropped);
    if ((tid & 63u) == 0 && m) atomicAdd(reinterpret_cast<unsigned long long*>(P.counts + 1), (unsigned long long)__popcll(m));
    if (err) atomicOr(P.status, err);
}

__global__ __launch_bounds__(kVocabTile) void postings_heads_kernel(const PostingsParams P) {
    const uint64_t j = uint64_t(blockIdx.x) * kVocabTile + threadIdx.x;
    if (j >= P.capacity_in) return;
    const uint32_t x = P.order[j];
    uint32_t key = P.n_terms, head = 0;
    if (x < P.capacity_in) {
        key = P.keydoc[2 * uint64_t(x)];
        if (key < P.n_terms) {
            head = 1;
            if (j > 0) {
                const uint32_t w = P.order[j - 1];
                if (w < P.capacity_in) head = (P.keydoc[2 * uint64_t(w)] != key || P.keydoc[2 * uint64_t(w) + 1] != P.keydoc[2 * uint64_t(x) + 1]) ? 1u : 0u;
            }
        }
    }
    P.skey[j] = key < P.n_terms ? key : P.n_terms;
    P.flags[j] = head;
}

__global__ __launch_bounds__(kVocabTile) void postings_emit_kernel(const PostingsParams P) {
    const uint64_t j = uint64_t(blockIdx.x) * kVocabTile + threadIdx.x;
    const uint64_t n = P.capacity_in;
    if (j >= n || P.skey[j] >= P.n_terms) return;   // (an indexed token: its sorted index is below capacity_in, heads_kernel saw to that)
    const uint32_t x = P.order[j];
    if (P.token_order) P.token_order[j] = x;
    if (!P.flags[j]) return;
    const uint64_t q = P.scan[j];
    if (q >= P.capacity_out) return;
    // the next head is the last place whose scan value is q + 1; none: the posting ends with the indexed tokens
    const uint64_t p = first_at_least(P.scan, j + 1, n + 1, q + 2);
    const uint64_t end = p <= n ? p - 1 : first_at_least(P.skey, j + 1, n, uint64_t(P.n_terms));
    P.post_docs[q] = uint32_t(P.doc_base + P.keydoc[2 * uint64_t(x) + 1]);
    P.post_tfs[q] = uint32_t(end - j);
    if (P.post_first) P.post_first[q] = j;
}

__global__ __launch_bounds__(kVocabTile) void postings_terms_kernel(const PostingsParams P) {
    const uint64_t k = uint64_t(blockIdx.x) * kVocabTile + threadIdx.x;
    if (k > P.n_terms) return;
    const uint64_t n = P.capacity_in;
    const uint64_t p = first_at_least(P.skey, 0, n, k);
    const uint64_t v = P.scan[p];
    P.term_offsets[k] = v;
    if (k == P.n_terms) {   // p: the indexed tokens; v: the postings
        P.counts[0] = v;
        if (v > P.capacity_out) atomicOr(P.status, kErrPostingsTooSmall);
        else if (P.post_first) P.post_first[v] = p;
    }
}

}  // namespace

hipError_t launch_postings_keys(const PostingsParams& P, hipStream_t stream) {
    const uint64_t blocks = P.capacity_in ? (P.capacity_in + kVocabTile - 1) / kVocabTile : 1;
    hipLaunchKernelGGL(postings_keys_kernel, dim3(uint32_t(blocks)), dim3(kVocabTile), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_heads(const PostingsParams& P, hipStream_t stream) {
    if (P.capacity_in == 0) return hipSuccess;
    hipLaunchKernelGGL(postings_heads_kernel, dim3(uint32_t((P.capacity_in + kVocabTile - 1) / kVocabTile)), dim3(kVocabTile), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_emit(const PostingsParams& P, hipStream_t stream) {
    if (P.capacity_in) hipLaunchKernelGGL(postings_emit_kernel, dim3(uint32_t((P.capacity_in + kVocabTile - 1) / kVocabTile)), dim3(kVocabTile), 0, stream, P);
    hipLaunchKernelGGL(postings_terms_kernel, dim3(uint32_t((uint64_t(P.n_terms) + 1 + kVocabTile - 1) / kVocabTile)), dim3(kVocabTile), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
