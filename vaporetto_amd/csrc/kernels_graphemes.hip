// ConcatGraphemeClustersFilter on the device (vaporetto_rules/src/sentence_filters/concat_grapheme_clusters.rs:10-36; the `G` of --wsconst and of
// the tantivy adapter): every label inside an extended grapheme cluster of the text AS IT WAS SCORED becomes 0.  The rules are UAX #29's, as
// include/vaporetto_grapheme.hpp states them one by one; the classes come from the two-stage table of tables.hpp (grapheme_class).
//
// POSITION-PARALLEL: a lane takes four consecutive chars of the batch's flat char array (the decode_chars words: char g of sentence i at
// out_offsets[i] + i + g) and decides the boundary in front of each from the two classes.  GB3 .. GB9b need the pair alone; where both classes
// are Other -- nearly every pair of Japanese text -- nothing is decided and nothing is stored.  GB9c, GB11 and GB12/13 need what the serial
// walk remembers of the text in front of the pair: ri & 1, pict in {0, 1, 2}, conj in {0, 1, 2} (grapheme_cluster_lengths).  Every char is a
// TRANSITION FUNCTION on that state, kept as three small maps in one word:
//   bits 0 .. 5    pict:  2 bits per incoming state 0, 1, 2 -> the state behind the char      (ExtPict: all 1; Extend: 1 -> 1; ZWJ: 1 -> 2)
//   bits 6 .. 11   conj:  the same                                                           (Consonant: all 1; Linker: 1, 2 -> 2; InCB Extend: identity)
//   bits 12, 13    ri:    the state behind the char for incoming 0, 1                         (Regional_Indicator: the swap)
//   bit 15         "a char here is not Other" (OR-ed along: a tile without it, behind a tile without it, has nothing to do)
//   bits 16 ..     sentence starts (added along: they number a char's sentence, which places its label)
// Any other char maps every state to 0 -- a CONSTANT function -- and so does a sentence's first char (the state is zero in front of it, so
// its function is the constant "what it makes of zero"): the segmented scan over sentences is a plain scan over these words.  Functions
// compose associatively (compose()), so the state in front of every char is an exclusive scan: inside a wave with __shfl_up, across the
// waves of a workgroup through LDS, across tiles through one SUMMARY word per tile.
//
// Two launches.  grapheme_classes_kernel: per tile of kGraphemeTile chars (cut by flat position: a sentence of any length spans tiles, a tile
// holds up to 1024 one-char sentences) the class bytes (| 0x80 at a sentence's first char), the tile's summary, and the number of sentences
// that start in front of it.  grapheme_apply_kernel: a tile composes the summaries of the tiles in front of it, 64 a trip, nearest first, back
// to the first trip that holds a constant summary (or the batch's start) -- no lane walks further back than that, and on ordinary text the
// tile in front is constant -- then scans its own chars and clears the labels.  Empty sentences and NUL chars set the status bits of the other
// text kernels; offsets that do not match the text are decode_chars' to report (it makes the words this kernel reads).
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"

namespace vpt {
namespace {

constexpr uint32_t kGThreads = 256, kGWaves = kGThreads / 64, kGPer = kGraphemeTile / kGThreads;
static_assert(kGPer == 4, "a lane's chars are the four bytes of one class word");
constexpr uint32_t kFnMask = 0x3FFFu, kFnIdent = 0x24u | (0x24u << 6) | 0x2000u, kFnWork = 0x8000u, kFnStart = 0x10000u;
enum : uint32_t { kOther = 0, kCR, kLF, kControl, kExtend, kZWJ, kRI, kPrepend, kSpacingMark, kL, kV, kT, kLV, kLVT };
constexpr uint32_t kExtPict = 16, kInCBMask = 96, kInCBConsonant = 32, kInCBExtend = 64, kInCBLinker = 96;

// g after f
__device__ __forceinline__ uint32_t compose(uint32_t f, uint32_t g) {
    uint32_t r = ((f | g) & kFnWork) | ((f & 0xFFFF0000u) + (g & 0xFFFF0000u));
#pragma unroll
    for (uint32_t s = 0; s < 3; ++s) {
        r |= ((g >> (2u * ((f >> (2u * s)) & 3u))) & 3u) << (2u * s);
        r |= ((g >> (6u + 2u * ((f >> (6u + 2u * s)) & 3u))) & 3u) << (6u + 2u * s);
    }
    r |= ((g >> (12u + ((f >> 12) & 1u))) & 1u) << 12;
    r |= ((g >> (12u + ((f >> 13) & 1u))) & 1u) << 13;
    return r;
}
__device__ __forceinline__ bool is_constant(uint32_t f) {
    const uint32_t p = f & 3u, c = (f >> 6) & 3u;
    return ((f >> 2) & 3u) == p && ((f >> 4) & 3u) == p && ((f >> 8) & 3u) == c && ((f >> 10) & 3u) == c && ((f >> 12) & 1u) == ((f >> 13) & 1u);
}
// the constant function "the state is (pict, conj, ri) = the low fields of f"
__device__ __forceinline__ uint32_t constant_of(uint32_t f) { return (f & 3u) * 0x15u | (((f >> 6) & 3u) * 0x15u) << 6 | ((f >> 12) & 1u) * 0x3000u; }

// a char's function from its class byte (bit 7: it starts a sentence)
__device__ __forceinline__ uint32_t char_fn(uint32_t c) {
    if ((c & 0xFFu) == 0) return 0;                       // Other inside a sentence: everything back to zero
    const uint32_t g = c & 15u, ic = c & kInCBMask;
    uint32_t f = (c & 0x7Fu) ? kFnWork : 0u;
    f |= (c & kExtPict) ? 0x15u : g == kExtend ? 0x04u : g == kZWJ ? 0x08u : 0u;
    f |= (ic == kInCBConsonant ? 0x15u : ic == kInCBLinker ? 0x28u : ic == kInCBExtend ? 0x24u : 0u) << 6;
    f |= g == kRI ? 0x1000u : 0u;
    if (c & 0x80u) f = (f & kFnWork) | constant_of(f) | kFnStart;
    return f;
}

// the function of a wave's chars in front of and including the lane's; *total: of all 64 lanes
__device__ __forceinline__ uint32_t wave_scan_fn(uint32_t x, uint32_t lane, uint32_t* total) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(x, d);
        if (lane >= d) x = compose(t, x);
    }
    *total = uint32_t(__shfl(int(x), 63));
    return x;
}

// does the boundary between classes p and c stay inside a cluster, the walk's state in front of c being the low fields of st (GB3 .. GB13)
__device__ __forceinline__ bool joined(uint32_t p, uint32_t c, uint32_t st) {
    const uint32_t g = c & 15u, pg = p & 15u;
    if (pg == kCR && g == kLF) return true;                                                   // GB3
    if (pg - kCR <= kControl - kCR || g - kCR <= kControl - kCR) return false;                // GB4, GB5
    if (pg == kL && (g == kL || g == kV || g == kLV || g == kLVT)) return true;               // GB6
    if ((pg == kLV || pg == kV) && (g == kV || g == kT)) return true;                         // GB7
    if ((pg == kLVT || pg == kT) && g == kT) return true;                                     // GB8
    if (g == kExtend || g == kZWJ || g == kSpacingMark || pg == kPrepend) return true;        // GB9, GB9a, GB9b
    if (((st >> 6) & 3u) == 2u && (c & kInCBMask) == kInCBConsonant) return true;             // GB9c
    if ((st & 3u) == 2u && (c & kExtPict)) return true;                                       // GB11
    return pg == kRI && g == kRI && ((st >> 12) & 1u);                                        // GB12, GB13; else GB999
}

__device__ __forceinline__ uint64_t chars_of(const GraphemeParams& P) {
    const uint64_t n = P.ooff[P.n_sent] + P.n_sent;
    return n < P.total_chars ? n : P.total_chars;
}

__global__ __launch_bounds__(kGThreads) void grapheme_classes_kernel(const GraphemeParams P) {
    __shared__ uint32_t starts[kGraphemeTile / 32];
    __shared__ uint32_t wtot[kGWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), tile = blockIdx.x;
    const uint64_t f0 = uint64_t(tile) * kGraphemeTile, N = chars_of(P);
    if (f0 >= N) {
        if (tid == 0) { P.summ[tile] = 0; P.first[tile] = 0; }
        return;
    }
    if (tid < kGraphemeTile / 32) starts[tid] = 0;
    __syncthreads();
    // the sentences that start inside the tile: at most one per char
    const uint64_t cnt = first_sentence_at(P.ooff, P.n_sent, 1, f0);
    uint32_t err = 0;
    for (uint64_t i = cnt + tid; i < P.n_sent && i < cnt + kGraphemeTile; i += kGThreads) {
        const uint64_t s = P.ooff[i] + i;
        if (s >= f0 + kGraphemeTile) break;
        if (s >= f0) atomicOr(&starts[uint32_t(s - f0) >> 5], 1u << (uint32_t(s - f0) & 31u));
        if (P.boff[i + 1] <= P.boff[i]) err |= kErrEmptySentence;
    }
    __syncthreads();
    const uint64_t f = f0 + kGPer * tid;
    const uint32_t sb = (starts[tid >> 3] >> (4u * (tid & 7u))) & 15u;
    uint32_t word = 0, fn = kFnIdent;
#pragma unroll
    for (uint32_t k = 0; k < kGPer; ++k) {
        uint32_t c = 0;
        if (f + k < N) {
            const uint32_t cp = P.cps[f + k] & 0x1FFFFFu;
            if (cp == 0) err |= kErrNulChar;
            c = grapheme_class(P.table, cp) | (((sb >> k) & 1u) << 7);
        }
        word |= c << (8u * k);
        fn = compose(fn, char_fn(c));
    }
    *reinterpret_cast<uint32_t*>(P.cls + f) = word;
    uint32_t total;
    wave_scan_fn(fn, lane, &total);
    if (lane == 0) wtot[wave] = total;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = wtot[0];
#pragma unroll
        for (uint32_t k = 1; k < kGWaves; ++k) t = compose(t, wtot[k]);
        P.summ[tile] = t;
        P.first[tile] = uint32_t(cnt);
    }
    if (err) atomicOr(P.status, err);
}

__global__ __launch_bounds__(kGThreads) void grapheme_apply_kernel(const GraphemeParams P) {
    __shared__ uint32_t wtot[kGWaves];
    __shared__ uint32_t incoming;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), tile = blockIdx.x;
    const uint64_t f0 = uint64_t(tile) * kGraphemeTile, N = chars_of(P);
    if (f0 >= N) return;
    // nothing but Other here and in the tile in front (whose last char could be a Prepend): every boundary of the tile stays as it is
    if (!((P.summ[tile] | (tile ? P.summ[tile - 1] : 0u)) & kFnWork)) return;
    if (wave == 0) {
        // the state in front of the tile: the summaries in front of it, nearest first, 64 a trip, up to a trip that holds a constant one
        uint32_t acc = kFnIdent;
        for (int64_t base = int64_t(tile) - 1;; base -= 64) {
            const int64_t idx = base - 63 + int64_t(lane);
            uint32_t r;
            wave_scan_fn(idx >= 0 ? P.summ[idx] & kFnMask : 0u, lane, &r);   // (in front of the batch: the constant zero)
            acc = compose(r, acc);
            if (is_constant(r)) break;
        }
        if (lane == 0) incoming = constant_of(acc);
    }
    const uint64_t f = f0 + kGPer * tid;
    const uint32_t word = *reinterpret_cast<const uint32_t*>(P.cls + f);
    uint32_t prev = f ? P.cls[f - 1] : 0u;
    uint32_t fn = kFnIdent;
#pragma unroll
    for (uint32_t k = 0; k < kGPer; ++k) fn = compose(fn, char_fn((word >> (8u * k)) & 0xFFu));
    uint32_t total;
    const uint32_t incl = wave_scan_fn(fn, lane, &total);
    if (lane == 0) wtot[wave] = total;
    uint32_t ex = __shfl_up(incl, 1);
    if (lane == 0) ex = kFnIdent;
    __syncthreads();
    uint32_t pre = incoming;
    for (uint32_t k = 0; k < wave; ++k) pre = compose(pre, wtot[k]);
    ex = compose(pre, ex);
    if (((word | (word >> 8) | (word >> 16) | (word >> 24) | prev) & 0x7Fu) == 0) return;   // Other next to Other only
    const uint64_t first = P.first[tile], lim_o = P.ooff[P.n_sent], lim = lim_o < P.total_boundaries ? lim_o : P.total_boundaries;
#pragma unroll
    for (uint32_t k = 0; k < kGPer; ++k) {
        const uint32_t c = (word >> (8u * k)) & 0xFFu;
        const uint32_t nx = compose(ex, char_fn(c));
        if (((prev | c) & 0x7Fu) != 0 && !(c & 0x80u) && f + k < N && joined(prev, c, ex)) {
            // the char's sentence is number first + (starts of the tile up to the char) - 1; its label sits that many + 1 in front of the char
            const uint64_t before = first + (nx >> 16);
            const uint64_t at = f + k - before;
            if (before != 0 && before <= f + k && at < lim) P.labels[at] = 0;
        }
        prev = c; ex = nx;
    }
}

}  // namespace

hipError_t launch_concat_graphemes(const GraphemeParams& P, hipStream_t stream) {
    if (P.n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(grapheme_classes_kernel, dim3(P.n_tiles), dim3(kGThreads), 0, stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grapheme_apply_kernel, dim3(P.n_tiles), dim3(kGThreads), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
