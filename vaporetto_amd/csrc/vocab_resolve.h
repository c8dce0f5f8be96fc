// What the passes over a FINISHED span CSR share (kernels_vocab.hip: the id pass; kernels_vocab_count.hip: the counter's key pass): a token of
// the batch -> its document, its bytes in the caller's text, and its chars as they are looked up.  A workgroup takes kVocabTile consecutive
// tokens, a lane per token.
//   owner   the token's document is the last i with token_offsets[i] <= t.  Two lanes find the owners of the tile's first and last token by
//           bisection over token_offsets; the entries in between -- the tile's slice, at most kVocabLdsOffsets of them -- go to LDS and every lane
//           bisects there.  (A tile of one-token and empty documents can span more: its lanes bisect in global memory.)  "The last i" puts a
//           token behind a run of empty documents into the document that owns it, on either side of a tile edge.
//   span    start and end inside the document, start <= end, neither inside a char.
// Whatever the arrays hold: a token index is below min(token_offsets[n], capacity_in) before it indexes anything, a document index below n, a text
// byte inside [boff[0], boff[n]) and inside its document.  Reported (kErrBadTokenCsr) and never followed: token_offsets that decrease or exceed
// capacity_in, byte offsets that decrease, a token no document owns, start > end, end past the document, a start or an end inside a char.
// `Params` has text, boff, n_docs, token_offsets, token_starts, token_ends, capacity_in (VocabParams, VocabCountParams: kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace vpt {

// one char of p[*at .. end), strict UTF-8, as it is looked up; false: no valid sequence starts at *at (or it does not end in front of `end`)
__device__ __forceinline__ bool vocab_next_char(const uint8_t* __restrict__ p, uint64_t* at, uint64_t end, const uint32_t* __restrict__ cinfo, uint32_t* out) {
    const uint64_t a = *at;
    const uint32_t b0 = p[a];
    uint32_t cp, need;
    if (b0 < 0x80u) { cp = b0; need = 0; }
    else if (b0 >= 0xC2u && b0 < 0xE0u) { cp = b0 & 0x1Fu; need = 1; }
    else if (b0 >= 0xE0u && b0 < 0xF0u) { cp = b0 & 0x0Fu; need = 2; }
    else if (b0 >= 0xF0u && b0 < 0xF5u) { cp = b0 & 0x07u; need = 3; }
    else return false;
    if (end - a <= need) return false;
    for (uint32_t k = 1; k <= need; ++k) {
        const uint32_t b = p[a + k];
        if ((b & 0xC0u) != 0x80u) return false;
        cp = (cp << 6) | (b & 0x3Fu);
    }
    if ((need == 2 && (cp < 0x800u || (cp >= 0xD800u && cp < 0xE000u))) || (need == 3 && (cp < 0x10000u || cp > 0x10FFFFu))) return false;
    // KyteaFullwidthFilter's image: the table is asked only where the filter can differ from the identity (decode_chars_kernel)
    if (cinfo && cp < 0x10000u && (cp < 0x80u || (cp - 0x2000u) < 0x600u || (cp - 0xFF00u) < 0xF0u)) cp = cinfo[cp] & 0xFFFFu;
    *at = a + need + 1;
    *out = cp;
    return true;
}

// the last i in [0, n - 1] with off[i] <= t (0 when there is none: the caller checks what it gets)
template <typename Off>
__device__ __forceinline__ uint64_t vocab_owner(Off off, uint64_t n, uint64_t t) {
    uint64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The offsets, every entry once over the grid: non-decreasing, inside the arrays -> kErrBadTokenCsr or 0.
template <typename Params>
__device__ __forceinline__ uint32_t vocab_check_offsets(const Params& P) {
    uint32_t err = 0;
    const uint64_t gid = uint64_t(blockIdx.x) * kVocabTile + threadIdx.x, gstride = uint64_t(gridDim.x) * kVocabTile;
    for (uint64_t i = gid; i < P.n_docs; i += gstride) {
        const uint64_t a = P.token_offsets[i], b = P.token_offsets[i + 1];
        if (a > b || b > P.capacity_in || P.boff[i] > P.boff[i + 1]) err = kErrBadTokenCsr;
    }
    return err;
}

// the batch's tokens: what token_offsets[n] says, at most what the arrays hold
template <typename Params>
__device__ __forceinline__ uint64_t vocab_token_count(const Params& P) {
    const uint64_t n_all = P.token_offsets[P.n_docs];
    return n_all < P.capacity_in ? n_all : P.capacity_in;
}

// The tile's slice of token_offsets into LDS (soff [kVocabLdsOffsets], edge [2]); every lane of a workgroup whose first token t0 is below n_tok
// calls this.  -> the documents of the slice (0: the lanes bisect in global memory); *d_lo: its first document.
template <typename Params>
__device__ __forceinline__ uint32_t vocab_tile_slice(const Params& P, uint64_t n_tok, uint64_t t0, uint64_t* soff, uint64_t* edge, uint64_t* d_lo_out) {
    const uint32_t tid = threadIdx.x;
    const uint64_t t1 = n_tok - t0 > kVocabTile ? t0 + kVocabTile - 1 : n_tok - 1;
    if (tid == 0) edge[0] = vocab_owner(P.token_offsets, P.n_docs, t0);
    if (tid == 64) edge[1] = vocab_owner(P.token_offsets, P.n_docs, t1);
    __syncthreads();
    const uint64_t d_lo = edge[0], d_hi = edge[1];
    const bool in_lds = d_hi >= d_lo && d_hi - d_lo + 2 <= kVocabLdsOffsets;
    const uint32_t n_own = in_lds ? uint32_t(d_hi - d_lo + 1) : 0u;   // documents of the slice; it holds n_own + 1 entries (d_hi + 1 <= n_docs)
    for (uint32_t k = tid; in_lds && k <= n_own; k += kVocabTile) soff[k] = P.token_offsets[d_lo + k];
    __syncthreads();
    *d_lo_out = d_lo;
    return n_own;
}

// Token tok (< n_tok) -> its document's first byte *db in the text and its span [*start, *end) inside the document; false: the arrays do not
// describe it (kErrBadTokenCsr), and nothing of it may be read.
template <typename Params>
__device__ __forceinline__ bool vocab_token_span(const Params& P, uint64_t tok, uint32_t n_own, uint64_t d_lo, const uint64_t* soff, uint64_t* db_out,
                                                 uint32_t* start_out, uint32_t* end_out) {
    uint64_t d, first, next;
    if (n_own) {
        const uint32_t j = uint32_t(vocab_owner(soff, uint64_t(n_own), tok));
        d = d_lo + j; first = soff[j]; next = soff[j + 1];
    } else {
        d = vocab_owner(P.token_offsets, P.n_docs, tok);
        first = P.token_offsets[d]; next = P.token_offsets[d + 1];
    }
    bool ok = first <= tok && tok < next;
    uint64_t db = 0, dl = 0;
    uint32_t start = 0, end = 0;
    if (ok) {
        const uint64_t B0 = P.boff[0], B1 = P.boff[P.n_docs], de = P.boff[d + 1];
        db = P.boff[d];
        ok = B0 <= db && db <= de && de <= B1;
        dl = de - db;
    }
    if (ok) {
        end = P.token_ends[tok];
        start = P.token_starts ? P.token_starts[tok] : (tok > first ? P.token_ends[tok - 1] : 0u);
        ok = start <= end && uint64_t(end) <= dl;
    }
    // (start < dl, end < dl: bytes of the document.)  A span ends where a char ends: no continuation byte behind either end
    if (ok && uint64_t(start) < dl) ok = (P.text[db + start] & 0xC0u) != 0x80u;
    if (ok && uint64_t(end) < dl) ok = (P.text[db + end] & 0xC0u) != 0x80u;
    *db_out = db; *start_out = start; *end_out = end;
    return ok;
}

}  // namespace vpt
