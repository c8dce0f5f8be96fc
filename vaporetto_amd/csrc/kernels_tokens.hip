// Token spans on the device: what vaporetto_tantivy's token_stream computes per document (vaporetto_tantivy/src/lib.rs:183-192) for a batch --
// `boundary_pos`: the byte index, in the caller's text, of every char that follows a WordBoundary, then the document's length.  Token k of a
// document is [boundary_pos[k - 1] or 0, boundary_pos[k]), its position k, position_length the number of entries.
//
// The writer's small sibling (emit_flat_kernel, kernels_emit.hip): the same partition into runs of sentences, the same reads, four bytes out
// per token instead of the token's text.  FLAT over bytes: a byte is a token's end-point iff it is a lead byte, not the first of its document,
// and the label in front of its char is 1; plus one end-point per document end.  A WORKGROUP takes a run of `per_block` documents.  Its size
// is a reduction over its labels alone (the ones + a document end each); ONE look-back per workgroup (place_run, emit_common.h) places the run;
// then the run is walked in pieces of 4 KB, sixteen bytes a thread: lead and document-start masks, one block prefix sum numbers the threads'
// chars and documents (which names their labels in the window of labels staged in LDS with the piece), a second one numbers their end-points,
// which are assembled in LDS and leave as consecutive dwords.  A document of any length spans pieces and runs of one; a run holds up to 512
// tiny ones.  No atomics on output positions, no sort; chainable behind the launch before it through EmitFuse::chain_in / chain_out.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"
#include "emit_common.h"
#include <type_traits>

namespace vpt {
namespace {

constexpr uint32_t kSpanPiece = kEmitThreads * 16;   // text bytes of a workgroup's step; a lead byte gives one end-point at most
struct alignas(16) SpanLds {
    uint32_t stage[kSpanPiece];               // the piece's end-points, in order
    uint32_t labs[(kSpanPiece + 64) / 4];     // the labels a piece's chars can ask for, from a 16-byte aligned address
    uint32_t starts[kSpanPiece / 32];         // one bit per byte of the piece: a document starts here
    uint32_t so[kEmitFlatMaxBlock + 1];       // the run's boundary offsets, relative to its first
    uint32_t sbo[kEmitFlatMaxBlock + 1];      // ... and its byte offsets
    uint32_t dump[kEmitThreads];              // where the stores of end-points that are not there go (nobody reads it)
    uint32_t wtot1[kEmitWaves], wtot2[kEmitWaves];
    uint32_t flags;                           // OR of the threads' "my offsets are no offsets"
    uint64_t red[kEmitWaves];
    uint64_t bcast[4];                        // ticket, B0, O0, base
};

// kTags: the tags of every token go out with its end-point.  The records of the run's chars are ONE slice of the sorted records (run_pref of
// its first and last front-end run, as for the tagged writer); per piece the records whose token ends at one of the piece's chars -- or at the
// char in front of it: an end-point is found at the char BEHIND its token -- are MARKED in LDS (a u16 per char: which record), every end-point
// leaves its char's number beside its value in the stage, and the loop that stores the end-points as consecutive dwords asks the mark of each
// and stores the token's n_tags words.  A record outside every token end of the run (labels that are not fill_tags' labels) makes the count of
// marked end-points differ from the slice's records in the run: kErrBadOffsets.
struct alignas(16) SpanMarks {
    uint16_t m[kSpanPiece + 16];              // m[k]: the record (its number from the piece's first + 1; 0: none) whose token ends at the piece's char k - 1
    uint16_t echar[kSpanPiece];               // beside stage[]: the piece's char at which the end-point was found
    uint16_t dump[kEmitThreads];
    uint32_t wtot[kEmitWaves];
};
struct NoSpanTags {};
// the tags of token `tok` from record `ri` (`has`: there is one); what is read of T by value (kernels_emit.hip, TagStrings)
__device__ __forceinline__ void store_token_tags(const uint4* records, const int32_t* rec_tags, uint32_t n_tags, int32_t* token_tags, const uint2* vocab_slot,
                                                 const uint32_t* vocab_ids, uint32_t n_models, uint32_t n_strings, uint64_t tok, uint64_t ri, bool has) {
    uint32_t word = 0;
    if (has) word = records[ri].z;
    const uint32_t model = word & kTokModelMask;   // 0: an empty record; kTokModelMask: a record the rules made
    for (uint32_t j = 0; j < n_tags; ++j) {
        int32_t v = -1;
        if (model) {
            const int32_t t = rec_tags[ri * n_tags + j];
            if (t < 0) v = t;
            else if (model != kTokModelMask && model - 1u < n_models) {
                const uint2 sl = vocab_slot[uint64_t(model - 1u) * n_tags + j];
                if (uint32_t(t) < sl.y && uint64_t(sl.x) + uint32_t(t) < n_strings) v = int32_t(vocab_ids[sl.x + uint32_t(t)]);
            }
        }
        token_tags[tok * n_tags + j] = v;
    }
}

template <bool kTags>
__global__ __launch_bounds__(kEmitThreads) void token_spans_kernel(const SpanParams P, const EmitFuse F, const std::conditional_t<kTags, SpanTags, NoSpanTags> T) {
    __shared__ SpanLds L;
    __shared__ std::conditional_t<kTags, SpanMarks, NoSpanTags> MK;   // (the untagged instance has none: its LDS is SpanLds alone)
    // the other array of state words, for the call after this one
    for (uint64_t k = uint64_t(blockIdx.x) * kEmitThreads + threadIdx.x; k < F.clear_n; k += uint64_t(gridDim.x) * kEmitThreads) F.clear[k] = 0;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
    if (tid == 0) { L.bcast[0] = atomicAdd(reinterpret_cast<unsigned long long*>(F.state + F.n_blocks), 1ull); L.flags = 0; }
    if (tid < kSpanPiece / 32) L.starts[tid] = 0;
    __syncthreads();
    const uint64_t blk = L.bcast[0];
    if (blk >= F.n_blocks) return;
    const uint64_t i0 = blk * F.per_block;
    const uint32_t ns = uint32_t(P.n_sent - i0 < F.per_block ? P.n_sent - i0 : F.per_block);
    // the run's offsets: thread j holds documents i0 + j and i0 + kEmitThreads + j (and their successors')
    constexpr uint32_t kMine = kEmitFlatMaxBlock / kEmitThreads;
    uint64_t my_b[kMine], my_o[kMine];
    bool mine[kMine];
    uint32_t err = 0;
#pragma unroll
    for (uint32_t j = 0; j < kMine; ++j) {
        const uint32_t s = tid + j * kEmitThreads;
        mine[j] = s < ns;
        uint64_t nx_b = 0, nx_o = 0;
        my_b[j] = ~uint64_t(0); my_o[j] = 0;
        if (mine[j]) { my_b[j] = P.boff[i0 + s]; my_o[j] = P.ooff[i0 + s]; nx_b = P.boff[i0 + s + 1]; nx_o = P.ooff[i0 + s + 1]; }
        if (s == 0) { L.bcast[1] = my_b[j]; L.bcast[2] = my_o[j]; }
        if (s == ns - 1) { L.red[0] = nx_b; L.red[1] = nx_o; }
        const bool empty = mine[j] && nx_b <= my_b[j], bad = mine[j] && (nx_o < my_o[j] || nx_o > P.total_boundaries);
        if (empty) err |= kErrEmptySentence;
        if (bad) err |= kErrBadOffsets;
        if (empty || bad) atomicOr(&L.flags, 1u);
    }
    __syncthreads();
    const uint64_t B0 = L.bcast[1], O0 = L.bcast[2], B1 = L.red[0], O1 = L.red[1];
    // (a run, and so a document, of 4 GB or more has no 32-bit spans: reported)
    const bool sane = L.flags == 0 && O1 - O0 < 0xFFFF0000ull && B1 - B0 < 0xFFFF0000ull;
    if (!sane) err |= kErrBadOffsets;
#pragma unroll
    for (uint32_t j = 0; j < kMine; ++j)
        if (mine[j]) { L.so[tid + j * kEmitThreads] = uint32_t(my_o[j] - O0); L.sbo[tid + j * kEmitThreads] = uint32_t(my_b[j] - B0); }
    if (tid == 0) { L.so[ns] = uint32_t(O1 - O0); L.sbo[ns] = uint32_t(B1 - B0); }
    __syncthreads();   // (red[] is used again below)

    // ---- the run's size = the ones of its label range + a document end each
    const uintptr_t l_all = reinterpret_cast<uintptr_t>(P.labels), l_end = l_all + P.total_boundaries;
    // with tags: the records of the run's chars [g0, g1) are the slice [r_lo, r_hi) of the sorted records
    const uint64_t g0 = O0 + i0, g1 = O1 + i0 + ns;
    uint64_t r_lo = 0, r_hi = 0;
    uint32_t n_exp = 0, n_hit = 0;   // the slice's records in the run; the end-points that found one
    if constexpr (kTags) {
        if (sane) {
            const uint64_t ra = i0 / T.tag.run_sent, rb = (i0 + ns + T.tag.run_sent - 1) / T.tag.run_sent;
            // (never a record past the arrays, whatever the counts say: tag_records.h; counts that had to be bent are no counts of this batch)
            if (!records_of_runs(T.tag, ra, rb, &r_lo, &r_hi)) err |= kErrBadOffsets;
            r_lo = wave_uniform64(r_lo); r_hi = wave_uniform64(r_hi);
            if (i0 != ra * T.tag.run_sent) {   // (the same in every thread) a run that starts inside a front-end run: its records begin further on
                for (;;) {
                    bool below = false;
                    if (r_lo + tid < r_hi) below = rec_pos(T.tag.records[r_lo + tid]) < g0;
                    uint32_t n_below;
                    flat_block_scan(below ? 1u : 0u, MK.wtot, lane, wave, &n_below);
                    r_lo += n_below;
                    if (n_below < uint32_t(kEmitThreads)) break;
                }
            }
            for (uint64_t r = r_lo + tid; r < r_hi; r += kEmitThreads) {
                const uint64_t pos = rec_pos(T.tag.records[r]);
                n_exp += pos >= g0 && pos < g1 ? 1u : 0u;
            }
        }
    }
    uint64_t size = 0;
    if (sane) {
        uint32_t ones = 0;
        const uintptr_t l_lo = l_all + O0, l_hi = l_all + O1;
        constexpr uint32_t kY = 4;   // loads in flight
        const uintptr_t lb = l_lo & ~uintptr_t(15);
        const uint32_t llo = uint32_t(l_lo - lb), lspan = l_hi > l_lo ? uint32_t(l_hi - lb) : 0u;   // (O1 - O0 < 4 GB: `sane`)
        for (uint32_t loff = 16u * tid; loff < lspan; loff += kY * kSpanPiece) {
            uint4 y[kY];
#pragma unroll
            for (uint32_t q = 0; q < kY; ++q) y[q] = loff + q * kSpanPiece < lspan ? *reinterpret_cast<const uint4*>(lb + loff + q * kSpanPiece) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (uint32_t q = 0; q < kY; ++q) {
                const uint32_t m = in_range16_rel(loff + q * kSpanPiece, llo, lspan);
                ones += uint32_t(__popc(one16(y[q]) & m));
                if (unk16(y[q]) & m) err |= kErrUnknownLabel;
            }
        }
        const uint64_t ws = wave_sum64(ones);
        if (lane == 0) L.red[wave] = ws;
        __syncthreads();
        size = ns;
#pragma unroll
        for (uint32_t k = 0; k < uint32_t(kEmitWaves); ++k) size += L.red[k];
    }
    // ---- the run's position: wave 0 looks back over the earlier runs' words, 64 per trip
    if (wave == 0) {
        if (lane == 0) publish_run_size(F, blk, size);
        const uint64_t base = place_run(F, blk, size, lane);
        if (lane == 0) L.bcast[3] = base;
    }
    __syncthreads();
    const uint64_t base = L.bcast[3], end = base + size;
    const bool store_ok = end <= P.capacity;   // (a run that does not fit writes nothing: nothing is written past `capacity`)
    if (blk == F.n_blocks - 1 && tid == 0) {
        P.token_offsets[P.n_sent] = end;
        if (end > P.capacity) err |= kErrOutputTooSmall;
        if (F.total_out) *F.total_out = end;
        if (F.chain_out) *F.chain_out = end;
    }
    if (!sane) {
#pragma unroll
        for (uint32_t j = 0; j < kMine; ++j) if (mine[j]) P.token_offsets[i0 + tid + j * kEmitThreads] = base;
        if (err) atomicOr(P.status, err);
        return;
    }

    // ---- the pieces: every end-point of the run to its place
    const uintptr_t t_lo = reinterpret_cast<uintptr_t>(P.text) + B0, t_hi = reinterpret_cast<uintptr_t>(P.text) + B1;
    const uintptr_t tb = t_lo & ~uintptr_t(15);   // (the run's bytes from a 16-byte aligned base, in 32 bits)
    const uint32_t lo_rel = uint32_t(t_lo - tb), span = uint32_t(t_hi - tb);
    uint32_t my_rel[kMine];   // where the thread's documents start, from tb (far away: none)
#pragma unroll
    for (uint32_t j = 0; j < kMine; ++j) my_rel[j] = mine[j] ? uint32_t(my_b[j] - B0) + lo_rel : 0xFFFFFFFFu;
    uint64_t at_out = base, cb = 0, sb = 0;   // output position, chars and document starts of the run in front of the piece
    bool fits = true;
    uint64_t rp = r_lo;   // with tags: the first record that is not in front of the char before the piece (the same in every thread)
    for (uint32_t p_off = 0; p_off < span; p_off += kSpanPiece) {
        if constexpr (kTags) {   // (the barrier behind the piece before: its marks are done with)
            reinterpret_cast<uint4*>(MK.m)[tid] = make_uint4(0, 0, 0, 0);
            reinterpret_cast<uint4*>(MK.m)[kEmitThreads + tid] = make_uint4(0, 0, 0, 0);
            if (tid < 2) reinterpret_cast<uint4*>(MK.m)[2 * kEmitThreads + tid] = make_uint4(0, 0, 0, 0);
        }
        const uint32_t vm = in_range16_rel(p_off + 16u * tid, lo_rel, span);
        const uint4 x = vm ? *reinterpret_cast<const uint4*>(tb + p_off + 16u * tid) : make_uint4(0, 0, 0, 0);
        // the labels the piece's chars can ask for: label (O0 + cb - sb) onwards (every char but a document's first has one in front)
        const uintptr_t lab_at = l_all + O0 + (cb - sb), lab_al = lab_at & ~uintptr_t(15);
        const uint32_t lab_head = uint32_t(lab_at - lab_al);
        {
            const uint32_t lim = l_end > lab_al ? (l_end - lab_al < 0xFFFFFFFFull ? uint32_t(l_end - lab_al) : 0xFFFFFFFFu) : 0u;
            const uint32_t a = 16u * tid, a2 = 16u * (uint32_t(kEmitThreads) + tid);
            reinterpret_cast<uint4*>(L.labs)[tid] = a < lim ? *reinterpret_cast<const uint4*>(lab_al + a) : make_uint4(0, 0, 0, 0);
            if (tid < 4) reinterpret_cast<uint4*>(L.labs)[kEmitThreads + tid] = a2 < lim ? *reinterpret_cast<const uint4*>(lab_al + a2) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (uint32_t j = 0; j < kMine; ++j) {
            if (mine[j] && my_rel[j] - p_off < kSpanPiece) {   // (unsigned: a start in front of the piece is far behind it)
                const uint32_t r = my_rel[j] - p_off;
                atomicOr(&L.starts[r >> 5], 1u << (r & 31u));
            }
        }
        __syncthreads();
        uint32_t sm = (L.starts[tid >> 1] >> (16 * (tid & 1))) & 0xFFFFu;
        const uint32_t lm = lead_mask16(x) & vm;
        if (sm & ~lm) err |= kErrBadOffsets;   // a document that starts inside a char (or outside the run)
        sm &= lm;
        const uint32_t nl = uint32_t(__popc(lm)), nst = uint32_t(__popc(sm));
        uint32_t tot;
        const uint32_t excl = flat_block_scan<false>(nl | (nst << 16), L.wtot1, lane, wave, &tot);   // (its barrier: every thread has read its starts)
        if (tid < kSpanPiece / 32) L.starts[tid] = 0;
        const uint32_t c_in = excl & 0xFFFFu, s_in = excl >> 16;   // chars / starts of the piece in front of this thread
        uint32_t n_done = 0;   // with tags: records in front of the piece's last char (the next piece begins behind them)
        if constexpr (kTags) {
            // mark the records whose token ends at char p_lo - 1 .. p_hi - 1: sorted, so they are the next ones -- coalesced reads of their positions.
            // A position is checked against the run, the piece and the arrays before it indexes anything.
            const uint64_t p_lo = g0 + cb, p_hi = p_lo + (tot & 0xFFFFu);
            for (uint64_t q = rp;; q += kEmitThreads) {
                const uint64_t r = q + tid;
                bool in = false, done = false;
                if (r < r_hi) {
                    const uint64_t pos = rec_pos(T.tag.records[r]);
                    in = pos < p_hi;
                    done = pos + 1 < p_hi;
                    if (in && pos + 1 >= p_lo && pos >= g0 && pos < T.tag.capacity && r - rp < 0xFFFFull) MK.m[uint32_t(pos + 1 - p_lo)] = uint16_t(r - rp + 1);
                }
                uint32_t n_in;
                flat_block_scan((in ? 1u : 0u) | (done ? 0x10000u : 0u), MK.wtot, lane, wave, &n_in);   // (its barriers: the marks are written)
                n_done += n_in >> 16;
                if ((n_in & 0xFFFFu) < uint32_t(kEmitThreads)) break;
            }
        }
        // the thread's chars that have a label in front take consecutive labels from (c_in - s_in) of the window on: label q of the thread = bit q of lab
        const uint32_t nm = lm & ~sm;
        uint32_t lab;
        {
            const uint32_t loff = lab_head + (c_in - s_in);           // byte offset in labs: <= 15 + 4096
            const uint32_t d = loff >> 2, r = loff & 3u;
            uint4 y;
            y.x = __builtin_amdgcn_alignbyte(L.labs[d + 1], L.labs[d], r); y.y = __builtin_amdgcn_alignbyte(L.labs[d + 2], L.labs[d + 1], r);
            y.z = __builtin_amdgcn_alignbyte(L.labs[d + 3], L.labs[d + 2], r); y.w = __builtin_amdgcn_alignbyte(L.labs[d + 4], L.labs[d + 3], r);
            lab = one16(y) & ((1u << uint32_t(__popc(nm))) - 1u);
        }
        // a document's end is written by the thread that holds the next one's first byte -- except the run's first document's start (the run
        // before this one wrote that end behind its last end-point); the run's last end comes behind the pieces
        uint32_t dm = sm;
        if (sb + s_in == 0 && sm) dm &= ~(sm & (0u - sm));
        const uint32_t t = uint32_t(__popc(lab)) + uint32_t(__popc(dm));
        uint32_t total;
        const uint32_t w = flat_block_scan<false>(t, L.wtot2, lane, wave, &total);
        if (at_out + total > end) { fits = false; break; }   // (the same in every thread)
        const uint32_t rel0 = p_off + 16u * tid - lo_rel;    // the thread's byte 0, from the run's first byte (bytes in front of the run: never looked at)
        const uint32_t n_before = uint32_t(sb) + s_in;       // documents of the run that start in front of the thread's bytes
        uint32_t* const dump = L.dump + tid;
        if (__ballot(sm != 0) == 0) {
            // (wave-uniform) no document starts in the wave's bytes: every end-point is a label's, from one document start per thread.  The value is
            // written where it WOULD stand, to a slot of the thread's own when there is none
            const uint32_t ds = n_before ? L.sbo[n_before - 1] : 0u;
            if (lm && !n_before) err |= kErrBadOffsets;      // chars in front of the run's first document
            uint32_t pos = w, bits = lab;
            [[maybe_unused]] uint32_t ci = c_in;   // with tags: the piece's char number of byte k (nm == lm here)
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const uint32_t nmk = (nm >> k) & 1u, e = nmk & bits;
                bits >>= nmk;
                *(e ? L.stage + pos : dump) = rel0 + k - ds;
                if constexpr (kTags) { *(e ? MK.echar + pos : MK.dump + tid) = uint16_t(ci); ci += nmk; }
                pos += e;
            }
        } else {
            // char by char: [the end of the document before] | the document's first token | [a label's end-point]
            uint32_t pos = w, bits = lab, cur = n_before, rem = lm;
            while (rem) {
                const uint32_t k = uint32_t(__ffs(int(rem))) - 1u, below = (1u << k) - 1u;
                rem &= rem - 1u;
                const uint32_t rel = rel0 + k;
                if ((sm >> k) & 1u) {
                    const uint32_t s = cur++;
                    if (s >= ns) { err |= kErrBadOffsets; continue; }
                    if (s > 0) {
                        if constexpr (kTags) MK.echar[pos] = uint16_t(c_in + uint32_t(__popc(lm & below)));
                        L.stage[pos++] = rel - L.sbo[s - 1];
                    }
                    P.token_offsets[i0 + s] = at_out + pos;
                    if (rel != L.sbo[s] || cb + c_in + uint32_t(__popc(lm & below)) != uint64_t(L.so[s]) + s) err |= kErrBadOffsets;   // not the char its offsets name
                } else {
                    const uint32_t e = bits & 1u;
                    bits >>= 1;
                    if (cur == 0 || cur > ns) { err |= kErrBadOffsets; continue; }
                    if (e) {
                        if constexpr (kTags) MK.echar[pos] = uint16_t(c_in + uint32_t(__popc(lm & below)));
                        L.stage[pos++] = rel - L.sbo[cur - 1];
                    }
                }
            }
            if (pos != w + t) err |= kErrBadOffsets;
        }
        __syncthreads();
        if constexpr (kTags) {
            // every end-point with its token's tags: the mark of the char it was found at names the record (or none)
            for (uint32_t d = tid; d < total; d += kEmitThreads) {
                const uint32_t ec = MK.echar[d];
                const uint32_t m = ec <= kSpanPiece ? MK.m[ec] : 0u;   // (a stage entry nobody wrote -- offsets that are none, reported below -- has any char)
                n_hit += m ? 1u : 0u;
                if (store_ok) {
                    P.token_ends[at_out + d] = L.stage[d];
                    store_token_tags(T.tag.records, T.tag.rec_tags, T.tag.n_tags, T.token_tags, T.vocab_slot, T.vocab_ids, T.n_models, T.n_strings, at_out + d,
                                     rp + (m ? m - 1u : 0u), m != 0);
                }
            }
            rp += n_done;
        } else {
            if (store_ok) for (uint32_t d = tid; d < total; d += kEmitThreads) P.token_ends[at_out + d] = L.stage[d];
        }
        __syncthreads();   // the next piece rewrites stage / labs / starts (and the marks)
        at_out += total;
        cb += tot & 0xFFFFu;
        sb += tot >> 16;
    }
    // the end of the run's last document
    if (fits && at_out < end) {
        if (store_ok && tid == 0) P.token_ends[at_out] = uint32_t(B1 - B0) - L.sbo[ns - 1];
        if constexpr (kTags) {
            if (tid == 0) {   // its token ends at the run's last char
                const uint64_t ri = records_lower_bound(T.tag.records, rp, r_hi, g1 - 1);
                const bool has = ri < r_hi && rec_pos(T.tag.records[ri]) == g1 - 1;
                n_hit += has ? 1u : 0u;
                if (store_ok) store_token_tags(T.tag.records, T.tag.rec_tags, T.tag.n_tags, T.token_tags, T.vocab_slot, T.vocab_ids, T.n_models, T.n_strings, at_out, ri, has);
            }
        }
        at_out += 1;
    }
    if constexpr (kTags) {   // a record of the run that no end-point met: the labels are not the ones fill_tags saw
        const uint64_t ws = wave_sum64(uint64_t(n_exp) | (uint64_t(n_hit) << 32));
        __syncthreads();
        if (lane == 0) L.red[wave] = ws;
        __syncthreads();
        uint64_t all = 0;
#pragma unroll
        for (uint32_t k = 0; k < uint32_t(kEmitWaves); ++k) all += L.red[k];
        if (uint32_t(all) != uint32_t(all >> 32)) err |= kErrBadOffsets;
    }
    // (what was written is what the size pass said: anything else means chars, labels and offsets do not belong together)
    if (!fits || at_out != end || cb != (O1 - O0) + ns || sb != ns) err |= kErrBadOffsets;
    if (err) atomicOr(P.status, err);
}

}  // namespace

hipError_t launch_token_spans(const SpanParams& P, const EmitFuse& F, hipStream_t stream) {   // a workgroup per run of documents
    hipLaunchKernelGGL(token_spans_kernel<false>, dim3(uint32_t(F.n_blocks)), dim3(kEmitThreads), 0, stream, P, F, NoSpanTags{});
    return hipGetLastError();
}
hipError_t launch_token_tags(const SpanParams& P, const SpanTags& T, const EmitFuse& F, hipStream_t stream) {   // the same runs, the tags beside the end-points
    hipLaunchKernelGGL(token_spans_kernel<true>, dim3(uint32_t(F.n_blocks)), dim3(kEmitThreads), 0, stream, P, F, T);
    return hipGetLastError();
}

}  // namespace vpt
