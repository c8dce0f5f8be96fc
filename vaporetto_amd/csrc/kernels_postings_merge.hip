// Merge of K postings segments over one term id space (PostingsMergeParams, kernels.hpp): the union of the segments' lists of every term,
// ordered by document, a document that stands in several segments' lists of a term combined into one posting whose tf is the sum.
// The number of postings of a segment is on the device (term_offsets[n_terms]); its capacity bounds it, so the launches are over the PLACES of
// the segments' arrays laid end to end (n_places = the sum of the capacities), over the n_terms + 1 term bounds, or over the segments.
//   load     the descriptors from kernel arguments into the scratch, kPostingsMergeLoad a launch; the ranges' identities.
//   offsets  a lane per term bound k, a loop over the segments: term_offsets[0] == 0, no decrease, the end at most the capacity.  ORDERED: the
//            lane sums the segments' bounds (the merged term_offsets[k]: nothing combines) and leaves table[s][k], where segment s's list of
//            term k starts in the output; reads and writes are coalesced across the terms.  The lane of n_terms writes the counts.
//   ORDERED route
//   copy     a lane per place: its segment by a bisection over place_base, its term by a bisection over the segment's term_offsets, the
//            posting's checks (documents strictly ascend inside a term, tf != 0), posting table[s][k] + (i - term_offsets[k]) written; the
//            segment's smallest and largest document by an integer atomicMin / atomicMax, a wave of one segment reduced first.
//   check    one lane over the segments: every segment that has postings starts above the largest document of the one before.
//   GENERAL route
//   records  a lane per place: {term, document, tf} -- the sentinel term n_terms where the place holds no posting -- and the same checks.
//   (sort)   train_radix_sort over the document word (4 passes), then the term word (ceil(bit_width(n_terms) / 8) passes): stable, so the
//            order is (term, document, segment).
//   heads    a lane per sorted place j: skey[j] = its term; a head when the term is below n_terms and the (term, document) before differs.
//   (scan)   train_scan over the heads.
//   emit     a head with scan value q writes posting q: its run ends at the next head (a bounded bisection over the scan), its tf is the sum
//            of the run's tfs -- at most n_segs of them, a valid segment has a document once in a list.
//   terms    a lane per term bound: term_offsets[k] = the scan at the first sorted place whose term is >= k; the lane of n_terms writes
//            counts[0] and counts[1] = the places that hold a posting minus the postings written.
// No atomic decides a value (integer min / max and the status OR do not depend on order), no loop's trip count depends on what another lane of
// the launch writes; two runs give identical bytes.  Every index is bounded before it indexes anything: a term bound at most the segment's
// n_terms, a place below min(term_offsets[n_terms], capacity), a posting below capacity_out, a sorted index below n_places.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"

namespace vpt {
namespace {

constexpr uint32_t kMergeThreads = 256;

// the first p in [lo, hi] with a[p] >= v, or hi when there is none in [lo, hi): a sorted (non-decreasing) array; at most 64 steps
template <typename T>
__device__ __forceinline__ uint64_t first_at_least(const T* a, uint64_t lo, uint64_t hi, uint64_t v) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (uint64_t(a[mid]) >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// term bound k of a segment: term_offsets[min(k, n_terms)], at most the capacity
__device__ __forceinline__ uint64_t bound_of(const PostingsMergeSegment& S, uint32_t k) {
    const uint64_t v = S.term_offsets[k < S.n_terms ? k : S.n_terms];
    return v < S.capacity ? v : S.capacity;
}

// the segment of place p < n_places: the last s with place_base[s] <= p (place_base[0] = 0; at most 10 steps)
__device__ __forceinline__ uint32_t segment_of(const PostingsMergeSegment* segs, uint32_t n_segs, uint64_t p) {
    uint32_t lo = 0, hi = n_segs;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (segs[mid].place_base <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// What place p holds.  valid: a posting (i below the segment's postings, a term found); then s, k, i, doc, tf and the term's raw start.
struct Place {
    bool valid;
    uint32_t s, k, doc, tf;
    uint64_t i, start;
};

__device__ __forceinline__ Place place_of(const PostingsMergeParams& P, uint64_t p, uint32_t* err) {
    Place r{};
    if (p >= P.n_places) return r;
    r.s = segment_of(P.segs, P.n_segs, p);
    const PostingsMergeSegment S = P.segs[r.s];
    r.i = p - S.place_base;
    if (S.n_terms == 0 || r.i >= S.capacity || r.i >= bound_of(S, S.n_terms)) return r;
    uint32_t lo = 0, hi = S.n_terms;   // the last k in [0, n_terms) with term_offsets[k] <= i (term_offsets[0] = 0 in a segment)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (S.term_offsets[mid] <= r.i) lo = mid; else hi = mid;
    }
    r.k = lo;
    r.start = S.term_offsets[lo];
    if (r.start > r.i) { *err |= kErrBadSegment; return r; }   // (term_offsets[0] above 0: the offsets kernel reports it too)
    r.doc = S.docs[r.i];
    r.tf = S.tfs[r.i];
    if (r.tf == 0) *err |= kErrBadSegment;
    if (r.i > r.start && S.docs[r.i - 1] >= r.doc) *err |= kErrBadSegment;
    r.valid = true;
    return r;
}

__global__ __launch_bounds__(kPostingsMergeLoad) void merge_load_kernel(PostingsMergeSegment* segs, uint32_t* range, uint32_t first, uint32_t count,
                                                                        const PostingsMergeLoadArgs A) {
    const uint32_t i = threadIdx.x;
    if (i >= count) return;
    segs[first + i] = A.seg[i];
    if (range) { range[2 * (first + i)] = 0xFFFFFFFFu; range[2 * (first + i) + 1] = 0u; }
}

template <bool kOrdered>
__global__ __launch_bounds__(kMergeThreads) void merge_offsets_kernel(const PostingsMergeParams P) {
    const uint64_t g = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    if (g > P.n_terms) return;
    const uint32_t k = uint32_t(g);
    uint32_t err = 0;
    uint64_t total = 0;
    for (uint32_t s = 0; s < P.n_segs; ++s) {
        const PostingsMergeSegment S = P.segs[s];
        if (k <= S.n_terms) {
            const uint64_t a = S.term_offsets[k];
            if (k == 0 && a != 0) err = kErrBadSegment;
            if (k < S.n_terms) { if (a > S.term_offsets[k + 1]) err = kErrBadSegment; }
            else if (a > S.capacity) err = kErrBadSegment;
        }
        if (kOrdered) total += bound_of(S, k);
    }
    if (kOrdered) {
        const uint64_t row = uint64_t(P.n_terms) + 1;
        uint64_t at = total;
        for (uint32_t s = 0; s < P.n_segs; ++s) {
            const PostingsMergeSegment S = P.segs[s];
            const uint64_t a = bound_of(S, k), b = k < P.n_terms ? bound_of(S, k + 1) : a;
            P.table[uint64_t(s) * row + k] = at;
            at += b > a ? b - a : 0;
        }
        P.term_offsets[k] = total;
        if (k == P.n_terms) {
            P.counts[0] = total;
            P.counts[1] = 0;
            if (total > P.capacity_out) err |= kErrPostingsTooSmall;
        }
    }
    if (err) atomicOr(P.status, err);
}

__global__ __launch_bounds__(kMergeThreads) void merge_copy_kernel(const PostingsMergeParams P) {
    const uint64_t p = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    uint32_t err = 0;
    const Place c = place_of(P, p, &err);
    if (c.valid) {
        const uint64_t q = P.table[uint64_t(c.s) * (uint64_t(P.n_terms) + 1) + c.k] + (c.i - c.start);
        if (q < P.capacity_out) { P.post_docs[q] = c.doc; P.post_tfs[q] = c.tf; }
    }
    // the segment's document range: a wave whose postings are all of one segment is reduced first (every lane of the wave is here)
    const uint64_t m = __ballot(c.valid);
    if (m) {
        const uint32_t s0 = uint32_t(__shfl(int(c.s), __ffsll((long long)m) - 1));
        if (__ballot(c.valid && c.s != s0) == 0) {
            uint32_t lo = c.valid ? c.doc : 0xFFFFFFFFu, hi = c.valid ? c.doc : 0u;
            for (int w = 32; w; w >>= 1) {
                const uint32_t l2 = uint32_t(__shfl_xor(int(lo), w)), h2 = uint32_t(__shfl_xor(int(hi), w));
                lo = l2 < lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
            }
            if ((threadIdx.x & 63u) == 0) { atomicMin(P.range + 2 * s0, lo); atomicMax(P.range + 2 * s0 + 1, hi); }
        } else if (c.valid) {
            atomicMin(P.range + 2 * c.s, c.doc);
            atomicMax(P.range + 2 * c.s + 1, c.doc);
        }
    }
    if (err) atomicOr(P.status, err);
}

__global__ void merge_check_kernel(const PostingsMergeParams P) {
    if (blockIdx.x || threadIdx.x) return;
    bool have = false, bad = false;
    uint32_t top = 0;
    for (uint32_t s = 0; s < P.n_segs; ++s) {
        const uint32_t lo = P.range[2 * s], hi = P.range[2 * s + 1];
        if (lo > hi) continue;   // no posting
        if (have && lo <= top) bad = true;
        top = hi;
        have = true;
    }
    if (bad) atomicOr(P.status, kErrSegmentsOverlap);
}

__global__ __launch_bounds__(kMergeThreads) void merge_records_kernel(const PostingsMergeParams P) {
    const uint64_t p = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    if (p >= P.n_places) return;
    uint32_t err = 0;
    const Place c = place_of(P, p, &err);
    P.rec[3 * p] = c.valid ? c.k : P.n_terms;
    P.rec[3 * p + 1] = c.valid ? c.doc : 0u;
    P.rec[3 * p + 2] = c.valid ? c.tf : 0u;
    if (err) atomicOr(P.status, err);
}

__global__ __launch_bounds__(kMergeThreads) void merge_heads_kernel(const PostingsMergeParams P) {
    const uint64_t j = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    if (j >= P.n_places) return;
    const uint32_t x = P.order[j];
    uint32_t key = P.n_terms, head = 0;
    if (x < P.n_places) {
        key = P.rec[3 * uint64_t(x)];
        if (key < P.n_terms) {
            head = 1;
            if (j > 0) {
                const uint32_t w = P.order[j - 1];
                if (w < P.n_places) head = (P.rec[3 * uint64_t(w)] != key || P.rec[3 * uint64_t(w) + 1] != P.rec[3 * uint64_t(x) + 1]) ? 1u : 0u;
            }
        }
    }
    P.skey[j] = key < P.n_terms ? key : P.n_terms;
    P.flags[j] = head;
}

__global__ __launch_bounds__(kMergeThreads) void merge_emit_kernel(const PostingsMergeParams P) {
    const uint64_t j = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    const uint64_t n = P.n_places;
    if (j >= n || P.skey[j] >= P.n_terms || !P.flags[j]) return;
    const uint64_t q = P.scan[j];
    // the next head is the last place whose scan value is q + 1; none: the run ends with the places that hold a posting
    const uint64_t e = first_at_least(P.scan, j + 1, n + 1, q + 2);
    uint64_t end = e <= n ? e - 1 : first_at_least(P.skey, j + 1, n, uint64_t(P.n_terms));
    if (end - j > P.n_segs) end = j + P.n_segs;   // (a list that holds a document twice: the records kernel has reported it)
    uint64_t tf = 0;
    for (uint64_t t = j; t < end; ++t) {
        const uint32_t x = P.order[t];
        if (x < n) tf += P.rec[3 * uint64_t(x) + 2];
    }
    if (tf > 0xFFFFFFFFull) atomicOr(P.status, kErrTfOverflow);
    if (q >= P.capacity_out) return;
    const uint32_t x = P.order[j];
    P.post_docs[q] = x < n ? P.rec[3 * uint64_t(x) + 1] : 0u;
    P.post_tfs[q] = uint32_t(tf);
}

__global__ __launch_bounds__(kMergeThreads) void merge_terms_kernel(const PostingsMergeParams P) {
    const uint64_t k = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    if (k > P.n_terms) return;
    const uint64_t p = first_at_least(P.skey, 0, P.n_places, k);
    const uint64_t v = P.scan[p];
    P.term_offsets[k] = v;
    if (k == P.n_terms) {   // p: the places that hold a posting; v: the merged postings
        P.counts[0] = v;
        P.counts[1] = p - v;
        if (v > P.capacity_out) atomicOr(P.status, kErrPostingsTooSmall);
    }
}

inline uint32_t blocks_of(uint64_t n) { return uint32_t((n + kMergeThreads - 1) / kMergeThreads); }

}  // namespace

hipError_t launch_postings_merge_load(const PostingsMergeParams& P, const PostingsMergeSegment* host_segs, hipStream_t stream) {
    for (uint32_t first = 0; first < P.n_segs; first += kPostingsMergeLoad) {
        PostingsMergeLoadArgs A{};
        const uint32_t count = P.n_segs - first < kPostingsMergeLoad ? P.n_segs - first : kPostingsMergeLoad;
        for (uint32_t i = 0; i < count; ++i) A.seg[i] = host_segs[first + i];
        hipLaunchKernelGGL(merge_load_kernel, dim3(1), dim3(kPostingsMergeLoad), 0, stream, P.segs, P.range, first, count, A);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_postings_merge_ordered(const PostingsMergeParams& P, hipStream_t stream) {
    hipLaunchKernelGGL(merge_offsets_kernel<true>, dim3(blocks_of(uint64_t(P.n_terms) + 1)), dim3(kMergeThreads), 0, stream, P);
    if (P.n_places) hipLaunchKernelGGL(merge_copy_kernel, dim3(blocks_of(P.n_places)), dim3(kMergeThreads), 0, stream, P);
    hipLaunchKernelGGL(merge_check_kernel, dim3(1), dim3(64), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_merge_records(const PostingsMergeParams& P, hipStream_t stream) {
    hipLaunchKernelGGL(merge_offsets_kernel<false>, dim3(blocks_of(uint64_t(P.n_terms) + 1)), dim3(kMergeThreads), 0, stream, P);
    if (P.n_places) hipLaunchKernelGGL(merge_records_kernel, dim3(blocks_of(P.n_places)), dim3(kMergeThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_merge_heads(const PostingsMergeParams& P, hipStream_t stream) {
    if (P.n_places == 0) return hipSuccess;
    hipLaunchKernelGGL(merge_heads_kernel, dim3(blocks_of(P.n_places)), dim3(kMergeThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_merge_emit(const PostingsMergeParams& P, hipStream_t stream) {
    if (P.n_places) hipLaunchKernelGGL(merge_emit_kernel, dim3(blocks_of(P.n_places)), dim3(kMergeThreads), 0, stream, P);
    hipLaunchKernelGGL(merge_terms_kernel, dim3(blocks_of(uint64_t(P.n_terms) + 1)), dim3(kMergeThreads), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
