// BM25 top-k search with MUST / SHOULD / MUST_NOT slots over one postings segment (PostingsBooleanParams, kernels.hpp; the definition is in
// include/vaporetto_hip.h).  A slot HAS a document when its term is inside [0, n_terms) and the term's list holds a posting for it.  A query's
// ANCHOR is its first MUST slot of the smallest df; a PLACE is a posting of the anchor or, in a query without a MUST slot, a posting of one
// of its SHOULD slots.  The three launches here stand where slots and expand stand in the OR search (kernels_postings_search.hip); the record
// they leave per place is that search's, and everything behind them is that search's launches as they stand.
//   queries  a lane per query: a walk over its slots (at most kSearchMaxQuerySlots): the occur values (<= 2), the anchor, whether a MUST_NOT
//            slot is there.  A MUST slot out of range or of df 0, or a query the CSR does not describe: the query is DEAD, it gets no place.
//   slots    a lane per slot: search_slots_kernel's checks (the CSR, the weight's bits, the term's two bounds; MUST_NOT slots too) and
//            counts[2]; slot_df = the slot's PLACES: its df when it is its query's anchor, or when the query has no anchor and the slot is
//            SHOULD, else 0.
//   (scan)   train_scan over slot_df: base[s] = the slot's first place, base[capacity_slots] = the places.
//   expand   a lane per place p: its slot by the bounded bisection over base, its posting with the OR search's checks (tf != 0, the document
//            inside the range and above the posting before it) BEFORE doc_lens is read.  ANCHORED: a walk over the query's slots in order; the
//            lane's own slot gives its own c, every other in-range slot is bisected (first_at_least over post_docs inside the term's clamped
//            bounds, at most 64 steps): MUST absent or MUST_NOT present is a veto, MUST or SHOULD present adds its c (a found tf of 0 is
//            kErrBadSegment) with the rounded add, left to right from the first c: the record's score word is the document's whole score
//            and its run behind the sort has length 1.  UNANCHORED: the lane's own c; only when the query has a MUST_NOT slot, a walk that
//            bisects those.  A vetoed or empty place: the sentinel query n_queries.
// Only the list that deals out the places is checked for ascent.  A bisected list that does not ascend gives some answer from inside its bounds.
// No atomic decides a value (one integer add, the status OR), every loop is bounded by kSearchMaxQuerySlots slots or 64 halvings, the launch
// boundaries are the only ordering relied on: two runs give identical bytes.  Every index is bounded before it indexes anything: a slot below
// capacity_slots, a term inside [0, n_terms), a posting below capacity_postings, a document below n_docs, a query below n_queries.
// ONE OR TWO SEGMENTS.  The three kernels are templates over kTwo, and every list they touch comes from term_list<kTwo>: <false> is the boolean
// search over the postings segment as it has always been; <true> (the clause search, n_lists > 0) takes a term inside [n_terms, n_terms +
// n_lists) as list term - n_terms of the derived segment {list_offsets, list_docs, list_tfs, capacity_lists} with the same checks against
// that segment's capacity: a list entry below capacity_lists.  The derived lists are the caller's arrays: what they hold is trusted no more
// than a segment is.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"
#include "postings_score.h"
#include "vocab_resolve.h"

namespace vpt {
namespace {

constexpr uint32_t kBoolThreads = 256;

// s + c with both rounded: never fused with the product that made c (search_sum_kernel's add)
__device__ __forceinline__ float add_rounded(float s, float c) {
#pragma clang fp contract(off)
    return s + c;
}

__device__ __forceinline__ uint64_t slot_count(const PostingsSearchParams& S) {
    const uint64_t n_all = S.query_offsets[S.n_queries];
    return n_all < S.capacity_slots ? n_all : S.capacity_slots;
}

// The list of a slot's term and the segment it lies in: {offsets, docs, tfs, capacity} of the postings segment for a term inside [0, n_terms),
// and, with kTwo (the clause search), those of the derived segment for a term inside [n_terms, n_terms + n_lists).  False: out of range.
struct TermList {
    const uint64_t* offsets;
    const uint32_t* docs;
    const uint32_t* tfs;
    uint64_t capacity;
    uint32_t index;   // the list's entry in offsets
};
// lists: whether the derived segment may be looked at (lists_usable); without it a term on that side is out of range.
template <bool kTwo>
__device__ __forceinline__ bool term_list(const PostingsBooleanParams& P, int32_t term, TermList* L, bool lists) {
    if (term < 0) return false;
    if (uint32_t(term) < P.S.n_terms) {
        *L = TermList{P.S.term_offsets, P.S.post_docs, P.S.post_tfs, P.S.capacity_postings, uint32_t(term)};
        return true;
    }
    if (kTwo && lists && uint32_t(term) - P.S.n_terms < P.n_lists) {
        *L = TermList{P.list_offsets, P.list_docs, P.list_tfs, P.capacity_lists, uint32_t(term) - P.S.n_terms};
        return true;
    }
    return false;
}

// A lists call enqueued in front of the clause search with no sync between them that found its 64-term limit or one of its capacities
// exceeded has written no list: the arrays hold what they held, and the status says so before the first launch here (kListsVoid: bits that
// no launch of the searches sets, so every lane of a launch reads the same).  The derived segment is then not looked at.
template <bool kTwo>
__device__ __forceinline__ bool lists_usable(const PostingsBooleanParams& P) {
    return kTwo && !(*P.S.status & kListsVoid);
}

// the clamped bounds of a list: [a, b) inside [0, its segment's capacity), empty when they are no list's
__device__ __forceinline__ void term_bounds(const TermList& L, uint64_t* a, uint64_t* b) {
    const uint64_t ta = L.offsets[L.index], tb = L.offsets[L.index + 1];
    const bool sound = ta <= tb && tb <= L.capacity;
    *a = sound ? ta : 0;
    *b = sound ? tb : 0;
}

// the slots [*a, *b) of query q when the CSR describes them, else false
__device__ __forceinline__ bool query_slots(const PostingsSearchParams& S, uint64_t q, uint64_t* a, uint64_t* b) {
    *a = S.query_offsets[q];
    *b = S.query_offsets[q + 1];
    return *a <= *b && *b <= S.capacity_slots && *b - *a <= kSearchMaxQuerySlots;
}

template <bool kTwo>
__global__ __launch_bounds__(kBoolThreads) void boolean_queries_kernel(const PostingsBooleanParams P) {
    const PostingsSearchParams& S = P.S;
    const uint64_t q = uint64_t(blockIdx.x) * kBoolThreads + threadIdx.x;
    if (q >= S.n_queries) return;
    const bool lists = lists_usable<kTwo>(P);
    uint64_t a, b, anchor = kBoolNoAnchor, best = ~uint64_t(0);
    uint32_t flags = 0, err = 0;
    bool dead = !query_slots(S, q, &a, &b);   // (what is wrong with the CSR: the slots launch says it)
    if (!dead) {
        for (uint64_t s = a; s < b; ++s) {
            const uint32_t occur = P.occurs[s];
            if (occur > kOccurMustNot) err = kErrBadOccur;
            if (occur == kOccurMustNot) flags |= kBoolHasNot;
            if (occur != kOccurMust) continue;
            const int32_t term = S.query_terms[s];
            uint64_t ta = 0, tb = 0;
            TermList L;
            if (term_list<kTwo>(P, term, &L, lists)) term_bounds(L, &ta, &tb);
            const uint64_t df = tb - ta;
            if (df == 0) dead = true;
            else if (df < best) { best = df; anchor = s; }
        }
    }
    P.q_anchor[q] = dead ? kBoolDead : anchor;
    P.q_flags[q] = flags;
    if (err) atomicOr(S.status, err);
}

template <bool kTwo>
__global__ __launch_bounds__(kBoolThreads) void boolean_slots_kernel(const PostingsBooleanParams P) {
    const PostingsSearchParams& S = P.S;
    const uint64_t s = uint64_t(blockIdx.x) * kBoolThreads + threadIdx.x, gstride = uint64_t(gridDim.x) * kBoolThreads;
    uint32_t err = 0;
    const bool lists = lists_usable<kTwo>(P);
    for (uint64_t i = s; i < S.n_queries; i += gstride) {   // every entry once over the grid
        const uint64_t a = S.query_offsets[i], b = S.query_offsets[i + 1];
        if (a > b || b > S.capacity_slots) err |= kErrBadQueryCsr;
        else if (b - a > kSearchMaxQuerySlots) err |= kErrQueryTooLong;
    }
    bool skipped = false;
    if (s < S.capacity_slots) {
        uint64_t places = 0;
        uint32_t query = S.n_queries;
        if (s < slot_count(S)) {
            const uint64_t q = vocab_owner(S.query_offsets, uint64_t(S.n_queries), s);
            if (q < S.n_queries && S.query_offsets[q] <= s && s < S.query_offsets[q + 1]) {
                query = uint32_t(q);
                const int32_t term = S.query_terms[s];
                const uint32_t occur = P.occurs[s];
                if (bits_of(S.query_weights[s]) > 0x7F7FFFFFu) err |= kErrBadWeights;
                TermList L;
                if (term_list<kTwo>(P, term, &L, lists)) {
                    const uint64_t a = L.offsets[L.index], b = L.offsets[L.index + 1];
                    if (a > b || b > L.capacity) {
                        err |= kErrBadSegment;
                    } else {
                        const uint64_t anchor = P.q_anchor[q];
                        if (anchor == kBoolNoAnchor ? occur == kOccurShould : anchor == s) places = b - a;
                    }
                } else {
                    skipped = true;
                }
            } else {
                err |= kErrBadQueryCsr;   // a slot below query_offsets[n] that no query owns
            }
        }
        S.slot_df[s] = places;
        S.slot_query[s] = query;
    }
    const uint64_t m = __ballot(skipped);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(reinterpret_cast<unsigned long long*>(S.counts + 2), (unsigned long long)__popcll(m));
    if (err) atomicOr(S.status, err);
}

template <bool kTwo>
__global__ __launch_bounds__(kBoolThreads) void boolean_expand_kernel(const PostingsBooleanParams P) {
    const PostingsSearchParams& S = P.S;
    const uint64_t p = uint64_t(blockIdx.x) * kBoolThreads + threadIdx.x;
    const uint64_t total = S.base[S.capacity_slots];
    if (p == 0) {
        S.counts[0] = total;
        if (total > S.n_places) atomicOr(S.status, kErrCandidatesTooSmall);
    }
    if (p >= S.n_places) return;
    const bool lists = lists_usable<kTwo>(P);
    uint32_t err = 0, doc = 0, query = S.n_queries, cbits = 0;
    if (p < total && total <= S.n_places && S.capacity_slots) {
        const uint64_t s = vocab_owner(S.base, S.capacity_slots, p);   // the last slot whose base is <= p: the one with places there
        const uint64_t i = p - S.base[s];
        const int32_t term = S.query_terms[s];
        const uint32_t q = S.slot_query[s];
        TermList L;
        if (S.base[s] <= p && i < S.slot_df[s] && term_list<kTwo>(P, term, &L, lists) && q < S.n_queries) {
            const uint64_t start = L.offsets[L.index], at = start + i;
            if (at >= start && at < L.capacity) {
                const uint32_t d = L.docs[at], tf = L.tfs[at];
                const uint64_t rel = uint64_t(d) - S.doc_base;
                if (tf == 0 || uint64_t(d) < S.doc_base || rel >= S.n_docs || (i > 0 && L.docs[at - 1] >= d)) {
                    err = kErrBadSegment;
                } else {
                    const uint32_t dl = S.doc_lens[rel];
                    const float own = bm25_term(S.query_weights[s], tf, dl, S.k1, S.b, S.avgdl);
                    const uint64_t anchor = P.q_anchor[q];
                    const bool anchored = anchor == s;
                    uint64_t qa, qb;
                    bool keep = anchored || anchor == kBoolNoAnchor;
                    float score = own;
                    if (keep && (anchored || (P.q_flags[q] & kBoolHasNot))) {
                        keep = query_slots(S, q, &qa, &qb);
                        bool first = true;
                        for (uint64_t t = qa; keep && t < qb; ++t) {
                            const uint32_t occur = P.occurs[t];
                            if (occur > kOccurMustNot || (!anchored && occur != kOccurMustNot)) continue;
                            float c = own;
                            if (t != s) {
                                const int32_t other = S.query_terms[t];
                                bool present = false;
                                uint32_t otf = 0;
                                TermList O;
                                if (term_list<kTwo>(P, other, &O, lists)) {
                                    uint64_t ta, tb;
                                    term_bounds(O, &ta, &tb);
                                    const uint64_t j = first_at_least(O.docs, ta, tb, uint64_t(d));
                                    if (j < tb && O.docs[j] == d) {
                                        present = true;
                                        otf = O.tfs[j];
                                    }
                                }
                                if (occur == kOccurMustNot ? present : (occur == kOccurMust && !present)) { keep = false; break; }
                                if (!present || occur == kOccurMustNot) continue;
                                if (otf == 0) { err = kErrBadSegment; keep = false; break; }
                                c = bm25_term(S.query_weights[t], otf, dl, S.k1, S.b, S.avgdl);
                            }
                            score = first ? c : add_rounded(score, c);
                            first = false;
                        }
                    }
                    if (keep) {
                        doc = uint32_t(rel);
                        query = q;
                        cbits = bits_of(score);
                    }
                }
            } else {
                err = kErrBadSegment;
            }
        }
    }
    S.rec[3 * p] = doc;
    S.rec[3 * p + 1] = query;
    S.rec[3 * p + 2] = cbits;
    if (err) atomicOr(S.status, err);
}

inline uint32_t blocks_of(uint64_t n) { return uint32_t((n + kBoolThreads - 1) / kBoolThreads); }

}  // namespace

hipError_t launch_postings_boolean_queries(const PostingsBooleanParams& P, hipStream_t stream) {
    if (P.n_lists)
        hipLaunchKernelGGL(boolean_queries_kernel<true>, dim3(blocks_of(P.S.n_queries)), dim3(kBoolThreads), 0, stream, P);
    else
        hipLaunchKernelGGL(boolean_queries_kernel<false>, dim3(blocks_of(P.S.n_queries)), dim3(kBoolThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_boolean_slots(const PostingsBooleanParams& P, hipStream_t stream) {
    const uint64_t lanes = P.S.capacity_slots > P.S.n_queries ? P.S.capacity_slots : uint64_t(P.S.n_queries);
    if (P.n_lists)
        hipLaunchKernelGGL(boolean_slots_kernel<true>, dim3(blocks_of(lanes)), dim3(kBoolThreads), 0, stream, P);
    else
        hipLaunchKernelGGL(boolean_slots_kernel<false>, dim3(blocks_of(lanes)), dim3(kBoolThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_boolean_expand(const PostingsBooleanParams& P, hipStream_t stream) {
    if (P.n_lists)
        hipLaunchKernelGGL(boolean_expand_kernel<true>, dim3(blocks_of(P.S.n_places ? P.S.n_places : 1)), dim3(kBoolThreads), 0, stream, P);
    else
        hipLaunchKernelGGL(boolean_expand_kernel<false>, dim3(blocks_of(P.S.n_places ? P.S.n_places : 1)), dim3(kBoolThreads), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
