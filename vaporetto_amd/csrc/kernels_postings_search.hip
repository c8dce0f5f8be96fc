// BM25 top-k search of a batch of queries over one postings segment (PostingsSearchParams, kernels.hpp).  A query is a run of SLOTS {term,
// weight}; a CANDIDATE is a slot and one posting of its term.  The number of slots and of candidates is on the device; capacity_slots and
// capacity_candidates bound them, so every launch is over the slots, over the PLACES [0, capacity_candidates), over the n_queries + 1 query
// bounds or over the n_queries * k outputs.
//   slots    a lane per slot: its query (vocab_resolve.h: the last q with query_offsets[q] <= s, so runs of empty queries resolve), slot_df =
//            the term's df, 0 when the term is outside [0, n_terms) (counts[2], summed per wave with a ballot before one integer atomic add);
//            the weight's bits (<= 0x7F7FFFFF: finite, sign clear), the term's two bounds (ascending, inside capacity_postings); the query CSR
//            once over the grid.
//   (scan)   train_scan over slot_df: base[s] = the slot's first candidate place, base[capacity_slots] = the candidates.
//   expand   a lane per place p: its slot by a bounded bisection over base, its posting term_offsets[term] + (p - base[s]); tf != 0, the
//            document inside [doc_base, doc_base + n_docs) and above the posting before it in the list BEFORE doc_lens is read; the record
//            {document - doc_base, query, bits of c}.  A place that holds no candidate: the sentinel query n_queries.
//   (sort)   train_radix_sort over the document word, then the query word: stable, so the order is (query, document, slot).
//   heads    a lane per sorted place j: skey[j] = its query; a head when the query is below n_queries and the (query, document) before differs.
//   (scan)   train_scan over the heads: scan[j] = the hits in front of j, scan[places] = the matches of all queries.
//   sum      a head with scan value h adds its run in slot order, starting from the first c -- at most kSearchMaxQuerySlots steps, a valid
//            query has no more slots and a valid list a document once -- and writes hit h {query, document, ~bits of the score}; a lane whose
//            place is at or behind the hits writes the sentinel hit.
//   ranges   a lane per query bound q: qstart[q] = the scan at the first sorted place whose query is >= q (postings_terms_kernel's bisection);
//            match_counts[q] = qstart[q + 1] - qstart[q]; the lane of n_queries writes counts[1].
//   (sort)   train_radix_sort over the score word (scores are non-negative: ~bits ascending is the score descending), then the query word:
//            stable, so the order is (query, score descending, document ascending) and query q's hits are still [qstart[q], qstart[q + 1]).
//   take     a lane per (query, j < k): hit qstart[q] + j of the ranked order when j is below the matches; the lane of j == 0 writes hit_counts.
// No atomic decides a value (one integer add, the status OR), no loop's trip count depends on what another lane of the launch writes, the launch
// boundaries are the only ordering relied on: two runs give identical bytes.  Every index is bounded before it indexes anything: a term inside
// [0, n_terms), a posting below capacity_postings, a document below n_docs, a slot below capacity_slots, a sorted index below the places, an
// output below n_queries * k.  With one of error_mask (kSearchErrors; the clause search: kClauseErrors) in the status, ranges and take write
// nothing: the four outputs stay as they were.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"
#include "postings_score.h"
#include "vocab_resolve.h"

namespace vpt {
namespace {

constexpr uint32_t kSearchThreads = 256;

// s + c with both rounded: never fused with the product that made c
__device__ __forceinline__ float add_rounded(float s, float c) {
#pragma clang fp contract(off)
    return s + c;
}

__device__ __forceinline__ uint64_t slot_count(const PostingsSearchParams& P) {
    const uint64_t n_all = P.query_offsets[P.n_queries];
    return n_all < P.capacity_slots ? n_all : P.capacity_slots;
}

__global__ __launch_bounds__(kSearchThreads) void search_slots_kernel(const PostingsSearchParams P) {
    const uint64_t s = uint64_t(blockIdx.x) * kSearchThreads + threadIdx.x, gstride = uint64_t(gridDim.x) * kSearchThreads;
    uint32_t err = 0;
    for (uint64_t i = s; i < P.n_queries; i += gstride) {   // every entry once over the grid
        const uint64_t a = P.query_offsets[i], b = P.query_offsets[i + 1];
        if (a > b || b > P.capacity_slots) err |= kErrBadQueryCsr;
        else if (b - a > kSearchMaxQuerySlots) err |= kErrQueryTooLong;
    }
    bool skipped = false;
    if (s < P.capacity_slots) {
        uint64_t df = 0;
        uint32_t query = P.n_queries;
        if (s < slot_count(P)) {
            const uint64_t q = vocab_owner(P.query_offsets, uint64_t(P.n_queries), s);
            if (P.query_offsets[q] <= s && s < P.query_offsets[q + 1]) {
                query = uint32_t(q);
                const int32_t term = P.query_terms[s];
                if (bits_of(P.query_weights[s]) > 0x7F7FFFFFu) err |= kErrBadWeights;
                if (term >= 0 && uint32_t(term) < P.n_terms) {
                    const uint64_t a = P.term_offsets[term], b = P.term_offsets[uint32_t(term) + 1];
                    if (a > b || b > P.capacity_postings) err |= kErrBadSegment; else df = b - a;
                } else {
                    skipped = true;
                }
            } else {
                err |= kErrBadQueryCsr;   // a slot below query_offsets[n] that no query owns
            }
        }
        P.slot_df[s] = df;
        P.slot_query[s] = query;
    }
    const uint64_t m = __ballot(skipped);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(reinterpret_cast<unsigned long long*>(P.counts + 2), (unsigned long long)__popcll(m));
    if (err) atomicOr(P.status, err);
}

__global__ __launch_bounds__(kSearchThreads) void search_expand_kernel(const PostingsSearchParams P) {
    const uint64_t p = uint64_t(blockIdx.x) * kSearchThreads + threadIdx.x;
    const uint64_t total = P.base[P.capacity_slots];
    if (p == 0) {
        P.counts[0] = total;
        if (total > P.n_places) atomicOr(P.status, kErrCandidatesTooSmall);
    }
    if (p >= P.n_places) return;
    uint32_t err = 0, doc = 0, query = P.n_queries, cbits = 0;
    if (p < total && total <= P.n_places && P.capacity_slots) {
        const uint64_t s = vocab_owner(P.base, P.capacity_slots, p);   // the last slot whose base is <= p: the one with candidates there
        const uint64_t i = p - P.base[s];
        const int32_t term = P.query_terms[s];
        const uint32_t q = P.slot_query[s];
        if (P.base[s] <= p && i < P.slot_df[s] && term >= 0 && uint32_t(term) < P.n_terms && q < P.n_queries) {
            const uint64_t start = P.term_offsets[term], at = start + i;
            if (at >= start && at < P.capacity_postings) {
                const uint32_t d = P.post_docs[at], tf = P.post_tfs[at];
                const uint64_t rel = uint64_t(d) - P.doc_base;
                if (tf == 0 || uint64_t(d) < P.doc_base || rel >= P.n_docs || (i > 0 && P.post_docs[at - 1] >= d)) {
                    err = kErrBadSegment;
                } else {
                    doc = uint32_t(rel);
                    query = q;
                    cbits = bits_of(bm25_term(P.query_weights[s], tf, P.doc_lens[rel], P.k1, P.b, P.avgdl));
                }
            } else {
                err = kErrBadSegment;
            }
        }
    }
    P.rec[3 * p] = doc;
    P.rec[3 * p + 1] = query;
    P.rec[3 * p + 2] = cbits;
    if (err) atomicOr(P.status, err);
}

__global__ __launch_bounds__(kSearchThreads) void search_heads_kernel(const PostingsSearchParams P) {
    const uint64_t j = uint64_t(blockIdx.x) * kSearchThreads + threadIdx.x;
    if (j >= P.n_places) return;
    const uint32_t x = P.order[j];
    uint32_t key = P.n_queries, head = 0;
    if (x < P.n_places) {
        key = P.rec[3 * uint64_t(x) + 1];
        if (key < P.n_queries) {
            head = 1;
            if (j > 0) {
                const uint32_t w = P.order[j - 1];
                if (w < P.n_places) head = (P.rec[3 * uint64_t(w) + 1] != key || P.rec[3 * uint64_t(w)] != P.rec[3 * uint64_t(x)]) ? 1u : 0u;
            }
        }
    }
    P.skey[j] = key < P.n_queries ? key : P.n_queries;
    P.flags[j] = head;
}

__global__ __launch_bounds__(kSearchThreads) void search_sum_kernel(const PostingsSearchParams P) {
    const uint64_t j = uint64_t(blockIdx.x) * kSearchThreads + threadIdx.x;
    const uint64_t n = P.n_places;
    if (j >= n) return;
    if (j >= P.scan[n]) {   // at or behind the hits: no head writes here
        P.hit[3 * j] = P.n_queries;
        P.hit[3 * j + 1] = 0u;
        P.hit[3 * j + 2] = 0xFFFFFFFFu;
    }
    if (P.skey[j] >= P.n_queries || !P.flags[j]) return;
    const uint64_t h = P.scan[j];   // (heads in front of j: below j + 1 <= n)
    if (h >= n) return;
    const uint32_t x = P.order[j];
    if (x >= n) return;
    float score = float_of(P.rec[3 * uint64_t(x) + 2]);
    for (uint64_t t = j + 1; t < n && t - j < kSearchMaxQuerySlots; ++t) {
        if (P.flags[t] || P.skey[t] >= P.n_queries) break;
        const uint32_t y = P.order[t];
        if (y >= n) break;
        score = add_rounded(score, float_of(P.rec[3 * uint64_t(y) + 2]));
    }
    P.hit[3 * h] = P.skey[j];
    P.hit[3 * h + 1] = P.rec[3 * uint64_t(x)];
    P.hit[3 * h + 2] = ~bits_of(score);
}

__global__ __launch_bounds__(kSearchThreads) void search_ranges_kernel(const PostingsSearchParams P) {
    const uint64_t q = uint64_t(blockIdx.x) * kSearchThreads + threadIdx.x;
    if (q > P.n_queries) return;
    const uint64_t n = P.n_places;
    const uint64_t a = P.scan[first_at_least(P.skey, 0, n, q)];
    P.qstart[q] = a;
    if (q == P.n_queries) { P.counts[1] = a; return; }
    if (*P.status & P.error_mask) return;
    const uint64_t b = P.scan[first_at_least(P.skey, 0, n, q + 1)];
    P.match_counts[q] = b >= a ? b - a : 0;
}

__global__ __launch_bounds__(kSearchThreads) void search_take_kernel(const PostingsSearchParams P) {
    const uint64_t g = uint64_t(blockIdx.x) * kSearchThreads + threadIdx.x;
    if (g >= uint64_t(P.n_queries) * P.k || (*P.status & P.error_mask)) return;
    const uint32_t q = uint32_t(g / P.k), j = uint32_t(g % P.k);
    const uint64_t a = P.qstart[q], b = P.qstart[q + 1];
    const uint64_t matches = b >= a ? b - a : 0;
    if (j == 0) P.hit_counts[q] = matches < P.k ? uint32_t(matches) : P.k;
    if (j >= matches || a + j >= P.n_places) return;
    const uint32_t x = P.order[a + j];
    if (x >= P.n_places) return;
    P.hit_docs[g] = uint32_t(P.doc_base + P.hit[3 * uint64_t(x) + 1]);
    P.hit_scores[g] = float_of(~P.hit[3 * uint64_t(x) + 2]);
}

inline uint32_t blocks_of(uint64_t n) { return uint32_t((n + kSearchThreads - 1) / kSearchThreads); }

}  // namespace

hipError_t launch_postings_search_slots(const PostingsSearchParams& P, hipStream_t stream) {
    const uint64_t lanes = P.capacity_slots > P.n_queries ? P.capacity_slots : uint64_t(P.n_queries);
    hipLaunchKernelGGL(search_slots_kernel, dim3(blocks_of(lanes)), dim3(kSearchThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_search_expand(const PostingsSearchParams& P, hipStream_t stream) {
    hipLaunchKernelGGL(search_expand_kernel, dim3(blocks_of(P.n_places ? P.n_places : 1)), dim3(kSearchThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_search_heads(const PostingsSearchParams& P, hipStream_t stream) {
    if (P.n_places == 0) return hipSuccess;
    hipLaunchKernelGGL(search_heads_kernel, dim3(blocks_of(P.n_places)), dim3(kSearchThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_search_sum(const PostingsSearchParams& P, hipStream_t stream) {
    if (P.n_places) hipLaunchKernelGGL(search_sum_kernel, dim3(blocks_of(P.n_places)), dim3(kSearchThreads), 0, stream, P);
    hipLaunchKernelGGL(search_ranges_kernel, dim3(blocks_of(uint64_t(P.n_queries) + 1)), dim3(kSearchThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_search_take(const PostingsSearchParams& P, hipStream_t stream) {
    hipLaunchKernelGGL(search_take_kernel, dim3(blocks_of(uint64_t(P.n_queries) * P.k)), dim3(kSearchThreads), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
