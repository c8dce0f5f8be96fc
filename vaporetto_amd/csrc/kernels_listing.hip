// The `predict` CLI's listings on the device (predict/src/main.rs:66-93, 122-176): per line the tokenized text T, the scores block of --scores
// ("{i}:{c}{c'} {score}\n" per boundary, then "\n") and the tag block of --tag-scores (per token its surface, "\t" + "tag:score,..." per slot of its
// tag model, "\n"; then "\n"), placed in ONE arena in the CLI's order.
//
// The output is a concatenation of ELEMENTS in output order: line i owns elements E(i) .. E(i + 1), E(i) = 2 * (ooff[i] + i) + i -- its T (with the
// newline behind it in the normalising order), one element per char for the scores block (char c: the line of boundary c; the last char: the block's
// "\n", and in the --no-norm order the newline that follows T and the scores there) and one per char for the tag block (the char's bytes; at a
// token's end its candidates and "\n"; at the last char the block's "\n").  A count pass sizes every element, the chained scan (launch_scan) turns
// the sizes into positions, the write pass formats every element where it belongs: no atomics on positions, the bytes depend on the input alone.
// The chars are the words decode_chars_kernel left (the scored scalar value: through KyteaFullwidthFilter when the flag is set), T is the text the
// writer (emit_flat_kernel) made for the same labels.  A workgroup of the write pass takes 256 consecutive elements, whose bytes are one range of
// the output: it assembles them in LDS and stores the range as aligned 16-byte pieces (a range larger than the staging area is stored directly).
// Every element is found by a search over ooff and then CHECKED against it (E(i) <= e < E(i + 1), the line inside the batch's arrays), so offsets
// that do not belong to the text give an error and never an access outside the arrays; an element writes exactly the bytes the count pass gave it.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"
#include "emit_common.h"

namespace vpt {
namespace {

constexpr uint32_t kLstThreads = 256;
constexpr uint32_t kLstWaves = kLstThreads / 64;
constexpr uint32_t kLstStage = 24576;   // bytes of a workgroup's range assembled in LDS (256 score lines take 8 KB at most; a T some hundred bytes)

__device__ __forceinline__ uint32_t dec_digits(uint32_t v) {   // 1 .. 10
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
__device__ __forceinline__ uint32_t magnitude(int32_t s) { return s < 0 ? 0u - uint32_t(s) : uint32_t(s); }   // (negated in unsigned: INT32_MIN)
__device__ __forceinline__ uint32_t utf8_len(uint32_t c) { return 1u + (c >= 0x80u) + (c >= 0x800u) + (c >= 0x10000u); }

// the bytes of an element, counted (W = false) or written to w as well
template <bool W>
struct Sink {
    uint8_t* w;
    uint64_t n = 0;
    __device__ __forceinline__ void put(uint32_t b) {
        if (W) w[n] = uint8_t(b);
        ++n;
    }
    __device__ __forceinline__ void dec(uint32_t v) {
        const uint32_t d = dec_digits(v);
        if (W) {
            for (uint32_t k = d; k-- > 0;) { w[n + k] = uint8_t('0' + v % 10u); v /= 10u; }
        }
        n += d;
    }
    __device__ __forceinline__ void sdec(int32_t s) {
        if (s < 0) put('-');
        dec(magnitude(s));
    }
    __device__ __forceinline__ void utf8(uint32_t c) {
        if (c < 0x80u) put(c);
        else if (c < 0x800u) { put(0xC0u | (c >> 6)); put(0x80u | (c & 0x3Fu)); }
        else if (c < 0x10000u) { put(0xE0u | (c >> 12)); put(0x80u | ((c >> 6) & 0x3Fu)); put(0x80u | (c & 0x3Fu)); }
        else { put(0xF0u | ((c >> 18) & 0x07u)); put(0x80u | ((c >> 12) & 0x3Fu)); put(0x80u | ((c >> 6) & 0x3Fu)); put(0x80u | (c & 0x3Fu)); }
    }
};

struct Loc {
    uint32_t kind;        // 0 T, 1 scores block, 2 tag block, 3 nothing
    uint64_t i, c, n, o0; // line, char, the line's chars, its first boundary
};

__device__ __forceinline__ uint64_t elem_of(const ListingParams& P, uint64_t i) { return 2u * P.ooff[i] + 3u * i; }
// the last line in [lo, hi] whose first element is not behind e (lo when there is none)
__device__ __forceinline__ uint64_t search_line(const ListingParams& P, uint64_t e, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (elem_of(P, mid) <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ Loc locate(const ListingParams& P, uint64_t e, uint64_t lo, uint64_t hi, uint32_t* err) {
    Loc L{3u, 0, 0, 0, 0};
    const uint64_t i = search_line(P, e, lo, hi);
    if (i >= P.n_sent) return L;   // behind the last line (total_boundaries may be an upper bound)
    const uint64_t o0 = P.ooff[i], o1 = P.ooff[i + 1], e0 = 2u * o0 + 3u * i;
    // the line's chars are [o0 + i, o1 + i + 1) of the batch's, its boundaries [o0, o1): checked before anything is read through them
    if (o1 < o0 || o1 > P.total_boundaries || e < e0 || e - e0 > 2u * (o1 - o0) + 2u) { *err |= kErrBadOffsets; return L; }
    const uint64_t r = e - e0, n = o1 - o0 + 1;
    L.i = i; L.n = n; L.o0 = o0;
    if (r == 0) L.kind = 0;
    else if (r <= n) { L.kind = 1; L.c = r - 1; }
    else { L.kind = 2; L.c = r - 1 - n; }
    return L;
}

// "\t" + "tag:score,..." per slot of the tag model of the token that ends at char g (Token::tag_candidates, sentence.rs:1228-1250)
template <bool W>
__device__ __forceinline__ void tag_candidates(const ListingParams& P, uint64_t g, Sink<W>& S) {
    const int32_t m = P.tag_models ? P.tag_models[g] : -1;
    if (m < 0 || uint32_t(m) >= P.n_models) return;
    const uint32_t first = P.models[12u * uint32_t(m) + 8u], ns = P.models[12u * uint32_t(m) + 9u];
    for (uint32_t s = first; s < first + ns; ++s) {
        const uint32_t cnt = P.slots[2u * s], zoff = P.slots[2u * s + 1u], k0 = P.slot_str[s];
        S.put('\t');
        for (uint32_t k = 0; k < cnt && k0 + k < P.n_strings; ++k) {
            if (k) S.put(',');
            // the predictor keeps its candidate strings escaped as write_tokenized_text writes them: a '\\' in front of ' ', '\\' and '/'
            for (uint32_t a = P.str_off[k0 + k], b = P.str_off[k0 + k + 1u]; a < b; ++a) {
                uint32_t ch = P.str_bytes[a];
                if (ch == '\\' && a + 1u < b) ch = P.str_bytes[++a];
                S.put(ch);
            }
            S.put(':');
            const int32_t score = (cnt >= 2u && P.tag_scores && zoff + k < P.score_stride) ? P.tag_scores[g * P.score_stride + zoff + k] : 0;
            S.sdec(score);
        }
    }
}

// an element of the scores block or of the tag block
template <bool W>
__device__ __forceinline__ uint64_t format_element(const ListingParams& P, const Loc& L, uint8_t* w) {
    Sink<W> S{w};
    const uint64_t g = L.o0 + L.i + L.c;
    const bool last = L.c + 1 == L.n;
    if (L.kind == 1) {
        if (!last) {
            if (P.flags & kListingScores) {   // print_scores, main.rs:66-75
                S.dec(uint32_t(L.c));
                S.put(':');
                S.utf8(P.cps[g] & kCharMaskTrain);
                S.utf8(P.cps[g + 1] & kCharMaskTrain);
                S.put(' ');
                S.sdec(P.scores[L.o0 + L.c]);
                S.put('\n');
            }
        } else {
            if (P.flags & kListingScores) S.put('\n');
            if (P.flags & kListingNoNormOrder) S.put('\n');   // main.rs:141: behind T and the scores
        }
    } else if (P.flags & kListingTagScores) {   // print_tag_scores, main.rs:77-93
        S.utf8(P.cps[g] & kCharMaskTrain);
        if (last || P.labels[L.o0 + L.c] == kWordBoundary) {
            tag_candidates<W>(P, g, S);
            S.put('\n');
        }
        if (last) S.put('\n');
    }
    return S.n;
}

// T of line i: where it is in the writer's text and its bytes; false: the writer's offsets are no offsets (its own verdict is in the status word)
__device__ __forceinline__ bool t_range(const ListingParams& P, uint64_t i, uint64_t* a, uint64_t* len) {
    const uint64_t t0 = P.t_off[i], t1 = P.t_off[i + 1];
    if (t1 < t0 || t1 > P.t_cap) return false;
    *a = t0; *len = t1 - t0;
    return true;
}

__device__ __forceinline__ void block_lines(const ListingParams& P, uint64_t e0, uint64_t* s_lines, uint64_t* lo, uint64_t* hi) {
    if (threadIdx.x == 0) {
        const uint64_t last = e0 + kLstThreads - 1 < P.n_elem ? e0 + kLstThreads - 1 : P.n_elem - 1;
        const uint64_t a = search_line(P, e0, 0, P.n_sent), b = search_line(P, last, 0, P.n_sent);
        s_lines[0] = a; s_lines[1] = b < a ? a : b;
    }
    __syncthreads();
    *lo = s_lines[0]; *hi = s_lines[1];
}

__global__ __launch_bounds__(kLstThreads) void listing_count_kernel(const ListingParams P) {
    __shared__ uint64_t s_lines[2];
    const uint64_t e0 = uint64_t(blockIdx.x) * kLstThreads, e = e0 + threadIdx.x;
    uint64_t lo, hi;
    block_lines(P, e0, s_lines, &lo, &hi);
    if (e >= P.n_elem) return;
    uint32_t err = 0;
    const Loc L = locate(P, e, lo, hi, &err);
    uint64_t n = 0;
    if (L.kind == 0) {
        uint64_t a, len;
        if (t_range(P, L.i, &a, &len)) n = len + ((P.flags & kListingNoNormOrder) ? 0u : 1u);
        else err |= kErrBadOffsets;
    } else if (L.kind != 3u) {
        n = format_element<false>(P, L, nullptr);
    }
    P.pos[e + 1] = n;
    if (err) atomicOr(P.status, err);
}

__global__ __launch_bounds__(kLstThreads) void listing_write_kernel(const ListingParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kLstStage];
    __shared__ uint64_t s_lines[2];
    __shared__ uint64_t s_tmask[kLstWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t e0 = uint64_t(blockIdx.x) * kLstThreads, e = e0 + tid;
    uint64_t lo, hi;
    block_lines(P, e0, s_lines, &lo, &hi);
    const uint64_t total = P.pos[P.n_elem];
    if (total > P.capacity) return;   // (the scan's verdict: kErrOutputTooSmall; nothing is written)
    if (e == 0) P.out_offsets[P.n_sent] = total;
    const uint64_t e1 = e0 + kLstThreads < P.n_elem ? e0 + kLstThreads : P.n_elem;
    const uint64_t p0 = P.pos[e0], span = P.pos[e1] - p0;
    const uint32_t mis = uint32_t((reinterpret_cast<uintptr_t>(P.out) + p0) & 15u);
    const bool staged = span + mis <= kLstStage;   // (the same in every thread)
    uint32_t err = 0;
    Loc L{3u, 0, 0, 0, 0};
    uint64_t at = 0, room = 0;
    if (e < P.n_elem) {
        L = locate(P, e, lo, hi, &err);
        at = P.pos[e]; room = P.pos[e + 1] - at;
    }
    uint8_t* const w = staged ? stage + (mis + (at - p0)) : P.out + at;
    bool is_t = false;
    if (L.kind == 0) {
        uint64_t a, len;
        const bool nl = !(P.flags & kListingNoNormOrder);
        is_t = t_range(P, L.i, &a, &len) && room == len + (nl ? 1u : 0u);
        if (is_t) {
            P.out_offsets[L.i] = at;
            if (nl) w[len] = '\n';
        } else err |= kErrBadOffsets;
    } else if (L.kind != 3u && room) {
        // exactly the bytes the count pass gave the element (anything else: the arrays changed between the passes)
        if (format_element<false>(P, L, nullptr) == room) format_element<true>(P, L, w);
        else err |= kErrBadOffsets;
    }
    // the T of the lines that start in the workgroup's elements: copied by all of its threads
    const uint64_t tm = __ballot(is_t);
    if (lane == 0) s_tmask[wave] = tm;
    __syncthreads();
    for (uint32_t q = 0; q < kLstWaves; ++q) {
        for (uint64_t rem = s_tmask[q]; rem; rem &= rem - 1) {
            const uint64_t et = e0 + 64u * q + uint32_t(__ffsll((long long)rem) - 1);
            uint32_t ignore = 0;
            const Loc T = locate(P, et, lo, hi, &ignore);
            uint64_t a = 0, len = 0;
            if (T.kind != 0 || !t_range(P, T.i, &a, &len)) continue;   // (never: the element's own thread found it)
            const uint64_t pt = P.pos[et];
            uint8_t* const d = staged ? stage + (mis + (pt - p0)) : P.out + pt;
            for (uint64_t k = tid; k < len; k += kLstThreads) d[k] = P.t_text[a + k];
        }
    }
    if (staged) {
        __syncthreads();
        // stage[0] stands at the 16-byte aligned address in front of the range: whole pieces as one store, the two ends byte by byte
        uint8_t* const base = P.out + p0 - mis;
        const uint32_t lim = mis + uint32_t(span);
        for (uint32_t off = 16u * tid; off < lim; off += 16u * kLstThreads) {
            if (off >= mis && off + 16u <= lim) *reinterpret_cast<uint4*>(base + off) = *reinterpret_cast<const uint4*>(stage + off);
            else for (uint32_t k = off < mis ? mis : off; k < off + 16u && k < lim; ++k) base[k] = stage[k];
        }
    }
    if (err) atomicOr(P.status, err);
}

// The caller's out_offsets as the launches of a listing take them: a copy when they are non-decreasing and inside the batch's arrays, else zeros
// (one char per line: in bounds for every kernel, and an error -- flagged here -- whatever the text is).  fill_tags' front end walks the batch in
// runs and trusts that the runs follow each other; offsets that decrease between two runs must not reach it.
__global__ __launch_bounds__(kLstThreads) void listing_check_offsets_kernel(const uint64_t* __restrict__ ooff, uint64_t n_sent, uint64_t total_boundaries,
                                                                            uint32_t* __restrict__ flag, uint32_t* __restrict__ status) {
    const uint64_t i = uint64_t(blockIdx.x) * kLstThreads + threadIdx.x;
    if (i >= n_sent) return;
    const uint64_t o0 = ooff[i], o1 = ooff[i + 1];
    if (o1 < o0 || o1 > total_boundaries) { atomicOr(flag, 1u); atomicOr(status, kErrBadOffsets); }
}
__global__ __launch_bounds__(kLstThreads) void listing_copy_offsets_kernel(const uint64_t* __restrict__ ooff, uint64_t n_sent, const uint32_t* __restrict__ flag,
                                                                           uint64_t* __restrict__ out) {
    const uint64_t i = uint64_t(blockIdx.x) * kLstThreads + threadIdx.x;
    if (i <= n_sent) out[i] = *flag ? 0ull : ooff[i];
}

}  // namespace

hipError_t launch_listing_offsets(const uint64_t* ooff, uint64_t n_sent, uint64_t total_boundaries, uint64_t* copy, uint32_t* flag, uint32_t* status,
                                  hipStream_t stream) {
    const uint32_t blocks = uint32_t((n_sent + kLstThreads) / kLstThreads);
    hipLaunchKernelGGL(listing_check_offsets_kernel, dim3(blocks), dim3(kLstThreads), 0, stream, ooff, n_sent, total_boundaries, flag, status);
    hipLaunchKernelGGL(listing_copy_offsets_kernel, dim3(blocks), dim3(kLstThreads), 0, stream, ooff, n_sent, flag, copy);
    return hipGetLastError();
}

hipError_t launch_listing(const ListingParams& P, uint64_t* scan_part, hipStream_t stream) {
    const uint64_t blocks = (P.n_elem + kLstThreads - 1) / kLstThreads;
    hipLaunchKernelGGL(listing_count_kernel, dim3(uint32_t(blocks)), dim3(kLstThreads), 0, stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan(P.pos, P.n_elem, scan_part, P.capacity, P.status, nullptr, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(listing_write_kernel, dim3(uint32_t(blocks)), dim3(kLstThreads), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
