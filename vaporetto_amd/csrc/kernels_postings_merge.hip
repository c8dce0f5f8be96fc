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
// POSITIONAL segments (PostingsMergePosParams): the launches above write the three arrays as they do without positions; post_first and
// post_positions come from launches over the places, over the POSITION PLACES (the segments' capacity_positions laid end to end; place pp of
// segment s holds a position when pp - pplace_base[s] < min(post_first_s[postings_s], capacity_positions_s)) or over the term bounds.
//   pload     the position descriptors beside the descriptors; post_first[0] == 0 of every segment.
//   ORDERED route: the table applied to post_first
//   poffsets  a lane per term bound k: the positions of segment s in front of term k are post_first_s[term_offsets_s[k]]; their sum over the
//             segments is the merged position offset of term k (no scan), and ptable[s][k] is where segment s's positions of term k start.
//             The lane of n_terms writes post_first[postings] and counts[2].
//   copy      (merge_copy_first_kernel: the copy above through the same function) also post_first[q] = ptable[s][k] + (post_first_s[i] -
//             post_first_s[term start]); post_first_s[i + 1] - post_first_s[i] == tf, no descent, the end at most capacity_positions.
//   pcopy     a lane per position place: its segment by a bisection over pplace_base, its posting by a bisection over post_first_s, its term by
//             a bisection over term_offsets_s, the strict ascent against the position before it inside the posting, the position written at
//             ptable[s][k] + (j - post_first_s[term start]).
//   GENERAL route, behind heads
//   ranks     a lane per sorted place j: ptf[j] = the tf of the input posting there (0: none), inv[order[j]] = j, post_first against the tf.
//   (scan)    train_scan over ptf behind emit: pscan[j] = the positions of the input postings sorted in front of j.
//   first     a head with scan value q: post_first[q] = pscan at the head; the lane of n_places writes post_first[postings] and counts[2].
//   pcopy     a lane per position place: its segment and posting as above, the posting's sorted place t by inv, its run's head (at most
//             n_segs - 1 places in front), and over the other members of the run (at most n_segs) the number of their positions below its own,
//             a bisection each; an equal one is kErrBadPositions.  The position is written at pscan[head] + its rank.  A run of one: a copy.
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

// The copy of place p (every lane of the wave comes here): its posting written at *q, the segment's document range reduced.
__device__ __forceinline__ Place copy_place(const PostingsMergeParams& P, uint64_t p, uint32_t* err, uint64_t* q_out) {
    const Place c = place_of(P, p, err);
    if (c.valid) {
        const uint64_t q = P.table[uint64_t(c.s) * (uint64_t(P.n_terms) + 1) + c.k] + (c.i - c.start);
        if (q < P.capacity_out) { P.post_docs[q] = c.doc; P.post_tfs[q] = c.tf; }
        *q_out = q;
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
    return c;
}

__global__ __launch_bounds__(kMergeThreads) void merge_copy_kernel(const PostingsMergeParams P) {
    const uint64_t p = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    uint32_t err = 0;
    uint64_t q = 0;
    copy_place(P, p, &err, &q);
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

// ---- the position lists (PostingsMergePosParams)

// post_first of a segment at posting bound i <= capacity, at most capacity_positions
__device__ __forceinline__ uint64_t pfirst_of(const PostingsMergePosSegment& F, uint64_t i) {
    const uint64_t v = F.first[i];
    return v < F.capacity_positions ? v : F.capacity_positions;
}

// the segment of position place pp < n_pplaces: the last s with pplace_base[s] <= pp (pplace_base[0] = 0; at most 10 steps)
__device__ __forceinline__ uint32_t psegment_of(const PostingsMergePosSegment* psegs, uint32_t n_segs, uint64_t pp) {
    uint32_t lo = 0, hi = n_segs;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (psegs[mid].pplace_base <= pp) lo = mid; else hi = mid;
    }
    return lo;
}

// What position place pp holds.  valid: a position (j below the segment's positions, its posting found); then s, j, the posting i and its two
// bounds fs <= j < fe in post_first, and the position.  The strict ascent against the position before it inside the posting is checked here.
struct PosPlace {
    bool valid;
    uint32_t s, pos;
    uint64_t j, i, fs, fe;
};

__device__ __forceinline__ PosPlace pos_place_of(const PostingsMergePosParams& Q, uint64_t pp, uint32_t* err) {
    PosPlace r{};
    if (pp >= Q.n_pplaces) return r;
    r.s = psegment_of(Q.psegs, Q.M.n_segs, pp);
    const PostingsMergeSegment S = Q.M.segs[r.s];
    const PostingsMergePosSegment F = Q.psegs[r.s];
    r.j = pp - F.pplace_base;
    if (S.n_terms == 0) return r;
    const uint64_t n_post = bound_of(S, S.n_terms);
    if (n_post == 0 || r.j >= pfirst_of(F, n_post)) return r;
    uint64_t lo = 0, hi = n_post;   // the last i in [0, n_post) with post_first[i] <= j (post_first[0] = 0 in a segment)
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (F.first[mid] <= r.j) lo = mid; else hi = mid;
    }
    r.i = lo;
    r.fs = F.first[lo];
    r.fe = F.first[lo + 1];
    if (r.fs > r.j || r.fe <= r.j) { *err |= kErrBadSegment; return r; }   // (post_first that does not ascend: copy / ranks report it too)
    r.pos = F.positions[r.j];
    if (r.j > r.fs && F.positions[r.j - 1] >= r.pos) *err |= kErrBadPositions;
    r.valid = true;
    return r;
}

__global__ __launch_bounds__(kPostingsMergeLoad) void merge_pload_kernel(PostingsMergePosSegment* psegs, uint32_t* status, uint32_t first, uint32_t count,
                                                                         const PostingsMergePosLoadArgs A) {
    const uint32_t i = threadIdx.x;
    if (i >= count) return;
    psegs[first + i] = A.seg[i];
    if (A.seg[i].first[0] != 0) atomicOr(status, kErrBadSegment);
}

// ORDERED: a lane per term bound k.  The positions of segment s in front of term k are post_first_s[term_offsets_s[k]], so the merged position
// offset of term k is their sum over the segments -- the table applied to post_first, no scan.
__global__ __launch_bounds__(kMergeThreads) void merge_poffsets_kernel(const PostingsMergePosParams Q) {
    const PostingsMergeParams& P = Q.M;
    const uint64_t g = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    if (g > P.n_terms) return;
    const uint32_t k = uint32_t(g);
    uint32_t err = 0;
    uint64_t total = 0, posts = 0;
    for (uint32_t s = 0; s < P.n_segs; ++s) {
        const PostingsMergeSegment S = P.segs[s];
        const PostingsMergePosSegment F = Q.psegs[s];
        const uint64_t a = bound_of(S, k), f = F.first[a];
        if (f > F.capacity_positions) err = kErrBadSegment;
        if (k < P.n_terms && f > F.first[bound_of(S, k + 1)]) err = kErrBadSegment;
        total += f < F.capacity_positions ? f : F.capacity_positions;
        posts += a;
    }
    const uint64_t row = uint64_t(P.n_terms) + 1;
    uint64_t at = total;
    for (uint32_t s = 0; s < P.n_segs; ++s) {
        const PostingsMergeSegment S = P.segs[s];
        const PostingsMergePosSegment F = Q.psegs[s];
        const uint64_t a = pfirst_of(F, bound_of(S, k)), b = k < P.n_terms ? pfirst_of(F, bound_of(S, k + 1)) : a;
        Q.ptable[uint64_t(s) * row + k] = at;
        at += b > a ? b - a : 0;
    }
    if (k == P.n_terms) {   // posts: the merged postings (nothing combines)
        if (posts <= P.capacity_out) Q.post_first[posts] = total;
        P.counts[2] = total;
        if (total > Q.capacity_positions_out) err |= kErrPositionsTooSmall;
    }
    if (err) atomicOr(P.status, err);
}

// ORDERED: the copy of a place, and post_first of its posting; post_first against the tf
__global__ __launch_bounds__(kMergeThreads) void merge_copy_first_kernel(const PostingsMergePosParams Q) {
    const PostingsMergeParams& P = Q.M;
    const uint64_t p = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    uint32_t err = 0;
    uint64_t q = 0;
    const Place c = copy_place(P, p, &err, &q);
    if (c.valid) {
        const PostingsMergePosSegment F = Q.psegs[c.s];
        const uint64_t fs = F.first[c.i], fe = F.first[c.i + 1], f0 = F.first[c.start];   // (start <= i < capacity)
        if (fe < fs || fe - fs != c.tf || fe > F.capacity_positions || fs < f0) err |= kErrBadSegment;
        if (q < P.capacity_out) Q.post_first[q] = Q.ptable[uint64_t(c.s) * (uint64_t(P.n_terms) + 1) + c.k] + (fs > f0 ? fs - f0 : 0);
    }
    if (err) atomicOr(P.status, err);
}

// ORDERED: a lane per position place: its segment, its posting, its term, the position written behind the term's positions of the segments in front
__global__ __launch_bounds__(kMergeThreads) void merge_pcopy_ordered_kernel(const PostingsMergePosParams Q) {
    const PostingsMergeParams& P = Q.M;
    const uint64_t pp = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    uint32_t err = 0;
    const PosPlace c = pos_place_of(Q, pp, &err);
    if (c.valid) {
        const PostingsMergeSegment S = P.segs[c.s];
        const PostingsMergePosSegment F = Q.psegs[c.s];
        uint32_t lo = 0, hi = S.n_terms;   // the last k in [0, n_terms) with term_offsets[k] <= i
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (S.term_offsets[mid] <= c.i) lo = mid; else hi = mid;
        }
        const uint64_t start = S.term_offsets[lo];
        if (start > c.i) {
            err |= kErrBadSegment;
        } else {
            const uint64_t f0 = F.first[start];
            if (f0 > c.fs) {
                err |= kErrBadSegment;
            } else {
                const uint64_t o = Q.ptable[uint64_t(c.s) * (uint64_t(P.n_terms) + 1) + lo] + (c.j - f0);
                if (o < Q.capacity_positions_out) Q.post_positions[o] = c.pos;
            }
        }
    }
    if (err) atomicOr(P.status, err);
}

// GENERAL: a lane per sorted place j: the tf of its input posting for the scan, the inverse of order, post_first against the tf
__global__ __launch_bounds__(kMergeThreads) void merge_ranks_kernel(const PostingsMergePosParams Q) {
    const PostingsMergeParams& P = Q.M;
    const uint64_t j = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    if (j >= P.n_places) return;
    const uint64_t x = P.order[j];
    uint32_t tf = 0;
    if (x < P.n_places) {
        Q.inv[x] = uint32_t(j);
        if (P.rec[3 * x] < P.n_terms) {   // a posting: x - place_base is below the segment's postings and its capacity
            tf = P.rec[3 * x + 2];
            const uint32_t s = segment_of(P.segs, P.n_segs, x);
            const PostingsMergePosSegment F = Q.psegs[s];
            const uint64_t i = x - P.segs[s].place_base;
            const uint64_t fs = F.first[i], fe = F.first[i + 1];
            if (fe < fs || fe - fs != tf || fe > F.capacity_positions) atomicOr(P.status, kErrBadSegment);
        }
    }
    Q.ptf[j] = tf;
}

// GENERAL: a lane per sorted place and one more: post_first of a head is the positions of the input postings sorted in front of it
__global__ __launch_bounds__(kMergeThreads) void merge_first_kernel(const PostingsMergePosParams Q) {
    const PostingsMergeParams& P = Q.M;
    const uint64_t j = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    if (j > P.n_places) return;
    if (j < P.n_places) {
        if (!P.flags[j]) return;
        const uint64_t q = P.scan[j];
        if (q < P.capacity_out) Q.post_first[q] = Q.pscan[j];
        return;
    }
    const uint64_t posts = P.scan[j], total = Q.pscan[j];
    if (posts <= P.capacity_out) Q.post_first[posts] = total;
    P.counts[2] = total;
    if (total > Q.capacity_positions_out) atomicOr(P.status, kErrPositionsTooSmall);
}

// GENERAL: a lane per position place: its segment and its posting, the posting's sorted place by inv, its run (at most n_segs members); the
// position's rank in the merged posting = its rank in its own posting + the positions below it in every other member (a bisection each).
__global__ __launch_bounds__(kMergeThreads) void merge_pcopy_general_kernel(const PostingsMergePosParams Q) {
    const PostingsMergeParams& P = Q.M;
    const uint64_t pp = uint64_t(blockIdx.x) * kMergeThreads + threadIdx.x;
    uint32_t err = 0;
    const PosPlace c = pos_place_of(Q, pp, &err);
    const uint64_t n = P.n_places;
    if (c.valid) {
        const uint64_t p = P.segs[c.s].place_base + c.i;
        const uint64_t t = p < n ? Q.inv[p] : n;
        if (t < n && P.skey[t] < P.n_terms) {
            uint64_t h = t;   // the run's head: at most n_segs - 1 places in front
            for (uint32_t step = 0; step < P.n_segs && h > 0 && !P.flags[h]; ++step) --h;
            if (!P.flags[h]) {
                err |= kErrBadSegment;   // (a list that holds a document twice: the records kernel has reported it)
            } else {
                uint64_t rank = c.j - c.fs;
                for (uint64_t u = h; u < n && u - h < P.n_segs; ++u) {
                    if (u > h && (P.flags[u] || P.skey[u] >= P.n_terms)) break;
                    if (u == t) continue;
                    const uint64_t x = P.order[u];
                    if (x >= n) continue;
                    const uint32_t s2 = segment_of(P.segs, P.n_segs, x);
                    const PostingsMergeSegment S2 = P.segs[s2];
                    const PostingsMergePosSegment F2 = Q.psegs[s2];
                    const uint64_t i2 = x - S2.place_base;
                    if (i2 >= S2.capacity) continue;
                    const uint64_t a = pfirst_of(F2, i2);
                    uint64_t b = pfirst_of(F2, i2 + 1);
                    if (b < a) b = a;
                    const uint64_t at = first_at_least(F2.positions, a, b, uint64_t(c.pos));
                    if (at < b && F2.positions[at] == c.pos) err |= kErrBadPositions;   // one (term, document) holds a position twice
                    rank += at - a;
                }
                const uint64_t o = Q.pscan[h] + rank;
                if (o < Q.capacity_positions_out) Q.post_positions[o] = c.pos;
            }
        }
    }
    if (err) atomicOr(P.status, err);
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

hipError_t launch_postings_merge_positions_load(const PostingsMergePosParams& Q, const PostingsMergePosSegment* host_psegs, hipStream_t stream) {
    for (uint32_t first = 0; first < Q.M.n_segs; first += kPostingsMergeLoad) {
        PostingsMergePosLoadArgs A{};
        const uint32_t count = Q.M.n_segs - first < kPostingsMergeLoad ? Q.M.n_segs - first : kPostingsMergeLoad;
        for (uint32_t i = 0; i < count; ++i) A.seg[i] = host_psegs[first + i];
        hipLaunchKernelGGL(merge_pload_kernel, dim3(1), dim3(kPostingsMergeLoad), 0, stream, Q.psegs, Q.M.status, first, count, A);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_postings_merge_positions_ordered(const PostingsMergePosParams& Q, hipStream_t stream) {
    const PostingsMergeParams& P = Q.M;
    hipLaunchKernelGGL(merge_offsets_kernel<true>, dim3(blocks_of(uint64_t(P.n_terms) + 1)), dim3(kMergeThreads), 0, stream, P);
    hipLaunchKernelGGL(merge_poffsets_kernel, dim3(blocks_of(uint64_t(P.n_terms) + 1)), dim3(kMergeThreads), 0, stream, Q);
    if (P.n_places) hipLaunchKernelGGL(merge_copy_first_kernel, dim3(blocks_of(P.n_places)), dim3(kMergeThreads), 0, stream, Q);
    hipLaunchKernelGGL(merge_check_kernel, dim3(1), dim3(64), 0, stream, P);
    if (Q.n_pplaces) hipLaunchKernelGGL(merge_pcopy_ordered_kernel, dim3(blocks_of(Q.n_pplaces)), dim3(kMergeThreads), 0, stream, Q);
    return hipGetLastError();
}

hipError_t launch_postings_merge_positions_ranks(const PostingsMergePosParams& Q, hipStream_t stream) {
    if (Q.M.n_places == 0) return hipSuccess;
    hipLaunchKernelGGL(merge_ranks_kernel, dim3(blocks_of(Q.M.n_places)), dim3(kMergeThreads), 0, stream, Q);
    return hipGetLastError();
}

hipError_t launch_postings_merge_positions_general(const PostingsMergePosParams& Q, hipStream_t stream) {
    hipLaunchKernelGGL(merge_first_kernel, dim3(blocks_of(Q.M.n_places + 1)), dim3(kMergeThreads), 0, stream, Q);
    if (Q.n_pplaces) hipLaunchKernelGGL(merge_pcopy_general_kernel, dim3(blocks_of(Q.n_pplaces)), dim3(kMergeThreads), 0, stream, Q);
    return hipGetLastError();
}

}  // namespace vpt
