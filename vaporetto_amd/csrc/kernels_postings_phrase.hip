// The position lists of a postings segment and the exact-phrase BM25 top-k search over them (PostingsPositionsParams, PostingsPhraseParams:
// kernels.hpp).
//
// positions   one launch behind the postings pass, a lane per place j of capacity_in: below the indexed tokens post_first[postings],
//             post_positions[j] = the position of token token_order[j] -- the caller's token_positions, or the token's index inside its document
//             (its owner by vocab_resolve.h's bisection).  A place that is not the first of its posting compares with the place before it:
//             the positions of a posting strictly ascend, or kErrBadPositions.  The token CSR is checked once over the grid.
//
// A POSITIONAL segment is the postings pass's three arrays, post_first [postings + 1] and post_positions [indexed tokens]: posting x's positions
// are post_positions[post_first[x] .. post_first[x + 1]), strictly ascending, post_tfs[x] of them.  A query is ONE phrase, its slots in order;
// its ANCHOR is the slot whose term has the fewest indexed tokens (the first such slot); its PROBES are the anchor term's positions, one
// contiguous run of post_positions.  capacity_probes bounds the sum over the queries, so every launch is over the n_queries + 1 query bounds,
// over the PLACES [0, capacity_probes) or over the n_queries * k outputs.
//   queries  a lane per query: the CSR entry, the length limit, the weight's bits (<= 0x7F7FFFFF), every slot's term and its two bounds
//            (ascending, inside capacity_postings; the tokens between post_first of the two, ascending, inside capacity_positions), the anchor,
//            the probe count -- 0 for an empty query, a term outside [0, n_terms) (counts[2], summed per wave with a ballot before one integer
//            atomic add) or a term of df 0.
//   (scan)   train_scan over the probe counts: base[q] = the query's first place, base[n_queries] = the probes.
//   probe    a lane per place p: its query by vocab_owner over base, its place g in the anchor run, its posting x by bisection over post_first
//            inside the term's posting range; post_first[x] <= the place < post_first[x + 1] <= capacity_positions, the difference the tf, the
//            document inside [doc_base, doc_base + n_docs) and above the one before it in the list.  start = position - anchor slot (64-bit;
//            negative: no occurrence); for every other slot j the posting of that document in term j's list (bisection over post_docs) and
//            start + j in its positions (bisection).  flags[p] = 1 when every slot is found; plen[p] = the tf at the first place of a posting.
//   (scan)   train_scan over the flags.
//   heads    the first place of a posting: pf = the scan's difference over the posting; a head when pf > 0.
//   (scan)   train_scan over the heads: scan[p] = the hits in front of p, scan[places] = the matches of all queries.
//   emit     a head with scan value h writes hit h {query, document, ~bits of the score} and its pf; a lane at or behind the hits writes the
//            sentinel hit.  Hits are born in (query, document) order: no grouping sort.
//   ranges   a lane per query bound: qstart[q] = the head scan at the query's probe base; match_counts; the lane of n_queries writes counts[1].
//   (sort)   train_radix_sort over the score word, then the query word: stable, so (query, score descending, document ascending).
//   take     a lane per (query, j < k): hit qstart[q] + j of the ranked order; the lane of j == 0 writes hit_counts.
// The SLOPPY calls (vpt_postings_sloppy_phrase_search_device, .._lists_device) are the same launches with query_slops beside the queries and
// phrase_probe_kernel<true> in probe's place: flags[p] is then the number of occurrences the place OWNS, 0 .. 32 (see the kernel).
// The phrase LISTS (vpt_postings_phrase_lists_device) run queries .. the second heads scan as they stand, with no weights, and then
//   lists    a lane per place and per query bound: a head with scan value h writes list entry h {doc_base + document, pf} -- born in (phrase,
//            document) order, so every list ascends; list_offsets[q] = the head scan at the phrase's probe base (ranges' rule); counts[1] = the
//            entries.  More entries than capacity_lists (kErrListsTooSmall) or one of kPhraseErrors: the counts only.  No sort, no take.
// No atomic decides a value (one integer add, the status OR), every loop is bounded by kPhraseMaxTerms, by 64 bisection steps or (the sloppy walk) by 2 * kPhraseMaxSlop + 1 places, the launch
// boundaries are the only ordering relied on: two runs give identical bytes.  Every index is bounded before it indexes anything: a slot below
// capacity_slots, a term inside [0, n_terms), a posting below capacity_postings, a position place below capacity_positions, a document below
// n_docs, a place below capacity_probes, an output below n_queries * k.  Unsorted positions inside a posting are not seen here (positions
// reports them): the bisection then misses or finds, inside the same bounds.  With one of kPhraseErrors in the status, ranges and take write
// nothing: the five outputs stay as they were.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"
#include "postings_score.h"
#include "vocab_resolve.h"

namespace vpt {
namespace {

constexpr uint32_t kPhraseThreads = 256;

__global__ __launch_bounds__(kVocabTile) void postings_positions_kernel(const PostingsPositionsParams P) {
    const uint64_t j = uint64_t(blockIdx.x) * kVocabTile + threadIdx.x, gstride = uint64_t(gridDim.x) * kVocabTile;
    uint32_t err = 0;
    for (uint64_t i = j; i < P.n_docs; i += gstride) {   // every entry once over the grid
        const uint64_t a = P.token_offsets[i], b = P.token_offsets[i + 1];
        if (a > b || b > P.capacity_in) err = kErrBadTokenCsr;
    }
    const uint64_t n_tok = vocab_token_count(P);
    const uint64_t all_post = P.term_offsets[P.n_terms];
    const uint64_t n_post = all_post < P.capacity_postings ? all_post : P.capacity_postings;
    uint64_t n_idx = n_post ? P.post_first[n_post] : 0;
    if (n_idx > P.capacity_in) n_idx = P.capacity_in;
    if (j < n_idx) {
        const uint64_t t = P.token_order[j];
        bool ok = t < n_tok;
        uint32_t pos = 0;
        if (ok) {
            const uint64_t d = vocab_owner(P.token_offsets, P.n_docs, t);
            const uint64_t first = P.token_offsets[d], next = P.token_offsets[d + 1];
            ok = first <= t && t < next;
            if (ok) pos = P.positions ? P.positions[t] : uint32_t(t - first);
        }
        if (ok) {
            P.post_positions[j] = pos;
            // the neighbour in the same posting: post_first[x] < j for the last x with post_first[x] <= j
            const uint64_t x = vocab_owner(P.post_first, n_post, j);
            if (P.positions && j > 0 && P.post_first[x] < j) {
                const uint64_t u = P.token_order[j - 1];
                if (u < n_tok && P.positions[u] >= pos) err |= kErrBadPositions;
            }
        } else {
            err |= kErrBadTokenCsr;   // a token that the offsets do not hold or that no document owns
        }
    }
    if (err) atomicOr(P.status, err);
}

struct PhraseQuery {
    uint64_t a;   // its first slot
    uint32_t len; // 0: not a query to follow
};

// the query's slots, when the CSR entry is one: inside capacity_slots, at most kPhraseMaxTerms
__device__ __forceinline__ PhraseQuery phrase_query(const PostingsPhraseParams& P, uint64_t q) {
    const uint64_t a = P.query_offsets[q], b = P.query_offsets[q + 1];
    PhraseQuery r{a, 0u};
    if (a <= b && b <= P.capacity_slots && b - a <= kPhraseMaxTerms) r.len = uint32_t(b - a);
    return r;
}

// term's posting range [*ta, *tb) when the term is one and its bounds are a segment's
__device__ __forceinline__ bool phrase_term_range(const PostingsPhraseParams& P, int32_t term, uint64_t* ta, uint64_t* tb) {
    if (term < 0 || uint32_t(term) >= P.n_terms) return false;
    const uint64_t a = P.term_offsets[term], b = P.term_offsets[uint32_t(term) + 1];
    *ta = a; *tb = b;
    return a <= b && b <= P.capacity_postings;
}

__global__ __launch_bounds__(kPhraseThreads) void phrase_queries_kernel(const PostingsPhraseParams P) {
    const uint64_t q = uint64_t(blockIdx.x) * kPhraseThreads + threadIdx.x;
    uint32_t err = 0;
    bool skipped = false;
    if (q < P.n_queries) {
        uint32_t anchor = 0;
        uint64_t run = 0, probes = 0;
        const uint64_t a = P.query_offsets[q], b = P.query_offsets[q + 1];
        if (P.query_weights && bits_of(P.query_weights[q]) > 0x7F7FFFFFu) err |= kErrBadWeights;   // (the lists call has no weights)
        if (P.query_slops && P.query_slops[q] > kPhraseMaxSlop) err |= kErrBadSlop;                 // (the exact calls have no slops)
        if (a > b || b > P.capacity_slots) {
            err |= kErrBadQueryCsr;
        } else if (b - a > kPhraseMaxTerms) {
            err |= kErrPhraseTooLong;
        } else {
            const uint32_t len = uint32_t(b - a);
            bool can = len > 0;
            uint64_t best = ~uint64_t(0);
            for (uint32_t j = 0; j < len; ++j) {   // (at most kPhraseMaxTerms)
                const int32_t term = P.query_terms[a + j];
                if (term < 0 || uint32_t(term) >= P.n_terms) { skipped = true; can = false; continue; }
                uint64_t ta, tb;
                if (!phrase_term_range(P, term, &ta, &tb)) { err |= kErrBadSegment; can = false; continue; }
                if (ta == tb) { can = false; continue; }   // df 0
                const uint64_t fa = P.post_first[ta], fb = P.post_first[tb];
                if (fa > fb || fb > P.capacity_positions) { err |= kErrBadSegment; can = false; continue; }
                if (fb - fa < best) { best = fb - fa; anchor = j; run = fa; }
            }
            if (can) probes = best;
        }
        P.q_anchor[q] = anchor;
        P.q_run[q] = run;
        P.q_probes[q] = probes;
    }
    const uint64_t m = __ballot(skipped);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(reinterpret_cast<unsigned long long*>(P.counts + 2), (unsigned long long)__popcll(m));
    if (err) atomicOr(P.status, err);
}

// One slot of a sloppy probe: the adjusted positions p - j of posting (term_j, d) inside [lo, lo + 2 slop], as bits p - j - lo of the mask.
// One bisection to the first position >= max(lo + j, 0), then at most 2 slop + 1 places: the count of steps bounds the walk, whatever the
// positions hold.  false: the posting's bounds are no segment's (kErrBadSegment); *mask 0: the document has no posting of the term.
__device__ __forceinline__ bool sloppy_slot_mask(const PostingsPhraseParams& P, uint64_t ja, uint64_t jb, uint32_t d, uint32_t j, int64_t lo,
                                                 uint32_t reach, uint64_t* mask) {
    *mask = 0;
    const uint64_t y = first_at_least(P.post_docs, ja, jb, uint64_t(d));
    if (y >= jb || P.post_docs[y] != d) return true;
    const uint64_t y0 = P.post_first[y], y1 = P.post_first[y + 1];
    if (y0 > y1 || y1 > P.capacity_positions) return false;
    const int64_t from = lo + int64_t(j);   // (lo >= -94, j < 64: no wrap; above 2^32 - 1: the bisection ends at y1)
    uint64_t z = first_at_least(P.post_positions, y0, y1, from > 0 ? uint64_t(from) : 0u);
    uint64_t m = 0;
    for (uint32_t t = 0; t <= reach && z < y1; ++t, ++z) {   // (reach <= 2 slop; ascending positions end the walk by themselves)
        const int64_t off = int64_t(P.post_positions[z]) - int64_t(j) - lo;
        if (off > int64_t(reach)) break;
        if (off >= 0) m |= uint64_t(1) << off;   // (off <= reach <= 62)
    }
    *mask = m;
    return true;
}

// What the place of anchor position post_positions[i] (posting [f0, ..) of document d, anchor slot aj) owns: see phrase_probe_kernel.
__device__ __forceinline__ uint32_t sloppy_place_count(const PostingsPhraseParams& P, const PhraseQuery& Q, uint64_t q, uint32_t aj, uint64_t i,
                                                       uint64_t f0, uint32_t d, uint32_t* err) {
    uint32_t flag = 0;
    const uint32_t raw = P.query_slops ? P.query_slops[q] : 0u;
    const uint32_t slop = raw < kPhraseMaxSlop ? raw : kPhraseMaxSlop;   // (above it: kErrBadSlop, nothing is taken)
    const int64_t a = int64_t(P.post_positions[i]) - int64_t(aj);
    int64_t lo = a - int64_t(slop);
    if (i > f0) {
        const int64_t after = int64_t(P.post_positions[i - 1]) - int64_t(aj) + 1;
        if (after > lo) lo = after;
    }
    if (lo <= a) {   // (positions that do not ascend: the place owns nothing)
        const uint32_t own = uint32_t(a - lo);   // <= slop
        uint64_t all = ~uint64_t(0), any = 0;
        for (uint32_t j = 0; all && j < Q.len; ++j) {   // (at most kPhraseMaxTerms)
            uint64_t ja, jb, m;
            if (!phrase_term_range(P, P.query_terms[Q.a + j], &ja, &jb)) { all = 0; break; }
            if (!sloppy_slot_mask(P, ja, jb, d, j, lo, own + slop, &m)) { *err = kErrBadSegment; all = 0; break; }
            any |= m;
            uint64_t c = m;
            for (uint32_t left = slop, step = 1; left; step <<= 1) {   // smear down by 0 .. slop: 1, 2, 4, .. and the rest
                const uint32_t by = step < left ? step : left;
                c |= c >> by;
                left -= by;
            }
            all &= c;
        }
        flag = uint32_t(__popcll(all & any & ((uint64_t(2) << own) - 1)));
    }
    return flag;
}

// SLOPPY false: the exact probe, flags[p] = 1 at an occurrence.  SLOPPY true: the place's anchor position gives a = position - anchor slot, and
// the place OWNS the occurrences s in [lo, a], lo = max(a - slop, a_prev + 1) with a_prev the adjusted position of the place before it in the
// same posting (read from post_positions, whichever workgroup that place's lane is in): an occurrence has an anchor position in
// [s, s + slop] and belongs to the first one at or after s, so every occurrence is counted by exactly one lane.  Per slot j, the anchor's own
// included and a repeated term like any other, M_j = sloppy_slot_mask; C_j = M_j smeared down by 0 .. slop (bit s: an adjusted position in
// [s, s + slop]); flags[p] = popcount(AND C_j & OR M_j & bits [0, a - lo]), 0 .. 32.  Signed 64-bit throughout.
template <bool SLOPPY>
__global__ __launch_bounds__(kPhraseThreads) void phrase_probe_kernel(const PostingsPhraseParams P) {
    const uint64_t p = uint64_t(blockIdx.x) * kPhraseThreads + threadIdx.x;
    const uint64_t total = P.base[P.n_queries];
    if (p == 0) {
        P.counts[0] = total;
        if (total > P.n_places) atomicOr(P.status, kErrProbesTooSmall);
    }
    if (p >= P.n_places) return;
    uint32_t err = 0, flag = 0, plen = 0, doc = 0, query = P.n_queries;
    if (p < total && total <= P.n_places) {
        const uint64_t q = vocab_owner(P.base, uint64_t(P.n_queries), p);   // the last query whose base is <= p: the one with probes there
        const uint64_t g = p - P.base[q];
        const PhraseQuery Q = phrase_query(P, q);
        const uint32_t aj = P.q_anchor[q];
        uint64_t ta = 0, tb = 0;
        if (P.base[q] <= p && g < P.q_probes[q] && aj < Q.len && phrase_term_range(P, P.query_terms[Q.a + aj], &ta, &tb) && ta < tb) {
            const uint64_t i = P.q_run[q] + g;   // the probe's place in post_positions
            if (i >= g && i < P.capacity_positions) {
                const uint64_t x = ta + vocab_owner(P.post_first + ta, tb - ta, i);   // ta <= x < tb <= capacity_postings
                const uint64_t f0 = P.post_first[x], f1 = P.post_first[x + 1];
                const uint32_t d = P.post_docs[x], tf = P.post_tfs[x];
                const uint64_t rel = uint64_t(d) - P.doc_base;
                if (f0 > i || i >= f1 || f1 > P.capacity_positions || f1 - f0 != uint64_t(tf) || uint64_t(d) < P.doc_base || rel >= P.n_docs ||
                    (x > ta && P.post_docs[x - 1] >= d) || f1 - i > P.q_probes[q] - g) {
                    err = kErrBadSegment;
                } else {
                    doc = uint32_t(rel);
                    query = uint32_t(q);
                    if (i == f0) plen = tf;
                    if constexpr (SLOPPY) {
                        flag = sloppy_place_count(P, Q, q, aj, i, f0, d, &err);
                    } else {
                        const int64_t start = int64_t(P.post_positions[i]) - int64_t(aj);
                        bool found = start >= 0;
                        for (uint32_t j = 0; found && j < Q.len; ++j) {   // (at most kPhraseMaxTerms)
                            if (j == aj) continue;
                            uint64_t ja, jb;
                            found = phrase_term_range(P, P.query_terms[Q.a + j], &ja, &jb);
                            if (!found) break;
                            const uint64_t y = first_at_least(P.post_docs, ja, jb, uint64_t(d));
                            found = y < jb && P.post_docs[y] == d;
                            if (!found) break;
                            const uint64_t y0 = P.post_first[y], y1 = P.post_first[y + 1];
                            if (y0 > y1 || y1 > P.capacity_positions) { err = kErrBadSegment; found = false; break; }
                            const uint64_t want = uint64_t(start) + j;
                            const uint64_t z = first_at_least(P.post_positions, y0, y1, want);
                            found = z < y1 && uint64_t(P.post_positions[z]) == want;
                        }
                        flag = found ? 1u : 0u;
                    }
                }
            } else {
                err = kErrBadSegment;
            }
        }
    }
    P.flags[p] = flag;
    P.plen[p] = plen;
    P.pdoc[p] = doc;
    P.pq[p] = query;
    if (err) atomicOr(P.status, err);
}

__global__ __launch_bounds__(kPhraseThreads) void phrase_heads_kernel(const PostingsPhraseParams P) {
    const uint64_t p = uint64_t(blockIdx.x) * kPhraseThreads + threadIdx.x;
    const uint64_t n = P.n_places;
    if (p >= n) return;
    const uint64_t len = P.plen[p];
    uint64_t pf = 0;
    if (len) {
        const uint64_t end = n - p < len ? n : p + len;
        pf = P.scan[end] - P.scan[p];   // (exact: at most len, a u32; sloppy: at most 32 len)
    }
    P.plen[p] = pf < 0xFFFFFFFFull ? uint32_t(pf) : 0xFFFFFFFFu;
    P.flags[p] = pf ? 1u : 0u;   // (probe's flags are in the scan: no lane reads them here)
}

__global__ __launch_bounds__(kPhraseThreads) void phrase_emit_kernel(const PostingsPhraseParams P) {
    const uint64_t p = uint64_t(blockIdx.x) * kPhraseThreads + threadIdx.x;
    const uint64_t n = P.n_places;
    if (p >= n) return;
    if (p >= P.scan[n]) {   // at or behind the hits: no head writes here
        P.hit[3 * p] = P.n_queries;
        P.hit[3 * p + 1] = 0u;
        P.hit[3 * p + 2] = 0xFFFFFFFFu;
        P.hpf[p] = 0u;
    }
    if (!P.flags[p]) return;
    const uint64_t h = P.scan[p];   // (heads in front of p: below p + 1 <= n)
    const uint32_t q = P.pq[p], rel = P.pdoc[p], pf = P.plen[p];
    if (h >= n || q >= P.n_queries || uint64_t(rel) >= P.n_docs) return;
    const float score = bm25_term(P.query_weights[q], pf, P.doc_lens[rel], P.k1, P.b, P.avgdl);
    P.hit[3 * h] = q;
    P.hit[3 * h + 1] = rel;
    P.hit[3 * h + 2] = ~bits_of(score);
    P.hpf[h] = pf;
}

__global__ __launch_bounds__(kPhraseThreads) void phrase_ranges_kernel(const PostingsPhraseParams P) {
    const uint64_t q = uint64_t(blockIdx.x) * kPhraseThreads + threadIdx.x;
    if (q > P.n_queries) return;
    const uint64_t n = P.n_places;
    const uint64_t at = P.base[q] < n ? P.base[q] : n;
    const uint64_t a = P.scan[at];
    P.qstart[q] = a;
    if (q == P.n_queries) { P.counts[1] = a; return; }
    if (*P.status & kPhraseErrors) return;
    const uint64_t next = P.base[q + 1] < n ? P.base[q + 1] : n;
    const uint64_t b = P.scan[next];
    P.match_counts[q] = b >= a ? b - a : 0;
}

__global__ __launch_bounds__(kPhraseThreads) void phrase_take_kernel(const PostingsPhraseParams P) {
    const uint64_t g = uint64_t(blockIdx.x) * kPhraseThreads + threadIdx.x;
    if (g >= uint64_t(P.n_queries) * P.k || (*P.status & kPhraseErrors)) return;
    const uint32_t q = uint32_t(g / P.k), j = uint32_t(g % P.k);
    const uint64_t a = P.qstart[q], b = P.qstart[q + 1];
    const uint64_t matches = b >= a ? b - a : 0;
    if (j == 0) P.hit_counts[q] = matches < P.k ? uint32_t(matches) : P.k;
    if (j >= matches || a + j >= P.n_places) return;
    const uint32_t x = P.order[a + j];
    if (x >= P.n_places) return;
    P.hit_docs[g] = uint32_t(P.doc_base + P.hit[3 * uint64_t(x) + 1]);
    P.hit_scores[g] = float_of(~P.hit[3 * uint64_t(x) + 2]);
    if (P.hit_freqs) P.hit_freqs[g] = P.hpf[x];
}

// The lists call's one launch, behind the second heads scan: a lane per place and per query bound.  Whether the entries fit is read from
// the scan by every lane (no lane waits for the status word of its own launch); the status holds what the launches in front found.
__global__ __launch_bounds__(kPhraseThreads) void phrase_lists_kernel(const PostingsPhraseParams P) {
    const uint64_t p = uint64_t(blockIdx.x) * kPhraseThreads + threadIdx.x;
    const uint64_t n = P.n_places;
    const uint64_t entries = P.scan[n];
    const bool fits = entries <= P.capacity_lists;
    if (p == 0) {
        P.counts[1] = entries;
        if (!fits) atomicOr(P.status, kErrListsTooSmall);
    }
    if (!fits || (*P.status & kPhraseErrors)) return;   // (kErrListsTooSmall of this launch is `fits`; of an earlier call: the caller's to sync)
    if (p <= P.n_queries) {   // phrase_ranges_kernel's rule: the head scan at the query's probe base
        const uint64_t at = P.base[p] < n ? P.base[p] : n;
        P.list_offsets[p] = P.scan[at];
    }
    if (p >= n || !P.flags[p]) return;
    const uint64_t h = P.scan[p];   // (heads in front of p: below entries <= capacity_lists)
    if (h >= P.capacity_lists || uint64_t(P.pdoc[p]) >= P.n_docs) return;
    P.list_docs[h] = uint32_t(P.doc_base + P.pdoc[p]);
    P.list_tfs[h] = P.plen[p];
}

inline uint32_t blocks_of(uint64_t n) { return uint32_t((n + kPhraseThreads - 1) / kPhraseThreads); }

}  // namespace

hipError_t launch_postings_positions(const PostingsPositionsParams& P, hipStream_t stream) {
    if (P.capacity_in == 0 || P.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(postings_positions_kernel, dim3(uint32_t((P.capacity_in + kVocabTile - 1) / kVocabTile)), dim3(kVocabTile), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_phrase_queries(const PostingsPhraseParams& P, hipStream_t stream) {
    hipLaunchKernelGGL(phrase_queries_kernel, dim3(blocks_of(P.n_queries)), dim3(kPhraseThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_phrase_probe(const PostingsPhraseParams& P, hipStream_t stream) {
    hipLaunchKernelGGL((phrase_probe_kernel<false>), dim3(blocks_of(P.n_places ? P.n_places : 1)), dim3(kPhraseThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_phrase_sloppy_probe(const PostingsPhraseParams& P, hipStream_t stream) {
    hipLaunchKernelGGL((phrase_probe_kernel<true>), dim3(blocks_of(P.n_places ? P.n_places : 1)), dim3(kPhraseThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_phrase_heads(const PostingsPhraseParams& P, hipStream_t stream) {
    if (P.n_places == 0) return hipSuccess;
    hipLaunchKernelGGL(phrase_heads_kernel, dim3(blocks_of(P.n_places)), dim3(kPhraseThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_phrase_emit(const PostingsPhraseParams& P, hipStream_t stream) {
    if (P.n_places) hipLaunchKernelGGL(phrase_emit_kernel, dim3(blocks_of(P.n_places)), dim3(kPhraseThreads), 0, stream, P);
    hipLaunchKernelGGL(phrase_ranges_kernel, dim3(blocks_of(uint64_t(P.n_queries) + 1)), dim3(kPhraseThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_phrase_lists(const PostingsPhraseParams& P, hipStream_t stream) {
    const uint64_t lanes = P.n_places > P.n_queries ? P.n_places : uint64_t(P.n_queries) + 1;
    hipLaunchKernelGGL(phrase_lists_kernel, dim3(blocks_of(lanes)), dim3(kPhraseThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_postings_phrase_take(const PostingsPhraseParams& P, hipStream_t stream) {
    hipLaunchKernelGGL(phrase_take_kernel, dim3(blocks_of(uint64_t(P.n_queries) * P.k)), dim3(kPhraseThreads), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
