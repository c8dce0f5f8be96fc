// Vocabulary ids of the token stream (vocab_table.hpp): a pass of its own over a FINISHED span CSR -- what vpt_token_spans_batch_device /
// vpt_token_tags_batch_device write (token_starts == nullptr: a token starts where the one in front of it in its document ends, or at 0) or what
// vpt_token_filter_batch_device writes (starts and ends; a document may own no token) -- that leaves one int32 per token: the id of the token's
// surface, or unk_id.  The surface is the token's bytes in the caller's text, or with `cinfo` their KyteaFullwidthFilter image char by char
// (decode_chars_kernel's map: the text as it was scored, the convention of the rule surfaces, kernels_pattern.hip).
//
// A workgroup takes kVocabTile consecutive tokens, a LANE PER TOKEN; adjacent tokens are adjacent in the text, so a wave's text reads fall into
// a few consecutive cache lines.
//   owner       the token's document is the last i with token_offsets[i] <= t.  Two lanes find the owners of the tile's first and last token by
//               bisection over token_offsets; the entries in between -- the tile's slice, at most kVocabLdsOffsets of them -- go to LDS and every lane
//               bisects there.  (A tile of one-token and empty documents can span more: its lanes bisect in global memory.)  "The last i" puts a
//               token behind a run of empty documents into the document that owns it, on either side of a tile edge.
//   length      a token of more bytes than 4 * max_len cannot be a key: unk_id, and its surface is not read.
//   lookup      the lane decodes at most max_len chars (strict UTF-8: a sequence no String can hold is no key), hashes them (pattern_tagger.hpp's
//               FNV-1a finished with the length), fetches its home slot as ONE aligned 16-byte load and walks the chain to the first empty slot; it
//               decodes the token again against the key's code points only where length and fingerprint agree.  No array of chars: no scratch.
// Nothing here decides an order and there is no atomic but the OR into the batch's status word: two runs give identical bytes.
//
// Whatever the arrays hold: a token index is below min(token_offsets[n], capacity_in) before it indexes anything, a document index below n, a text
// byte inside [boff[0], boff[n]) and inside its document.  Reported (kErrBadTokenCsr) and never followed: token_offsets that decrease or exceed
// capacity_in, byte offsets that decrease, a token no document owns, start > end, end past the document, a start or an end inside a char.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"
#include "pattern_tagger.hpp"

namespace vpt {
namespace {

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

__global__ __launch_bounds__(kVocabTile) void token_ids_kernel(const VocabParams P) {
    __shared__ uint64_t soff[kVocabLdsOffsets];   // token_offsets[d_lo ..]: the tile's documents and the end of the last
    __shared__ uint64_t edge[2];                  // d_lo, d_hi
    const uint32_t tid = threadIdx.x;
    uint32_t err = 0;
    // ---- the offsets, every entry once over the grid: non-decreasing, inside the arrays
    const uint64_t gid = uint64_t(blockIdx.x) * kVocabTile + tid, gstride = uint64_t(gridDim.x) * kVocabTile;
    for (uint64_t i = gid; i < P.n_docs; i += gstride) {
        const uint64_t a = P.token_offsets[i], b = P.token_offsets[i + 1];
        if (a > b || b > P.capacity_in || P.boff[i] > P.boff[i + 1]) err = kErrBadTokenCsr;
    }
    const uint64_t n_all = P.token_offsets[P.n_docs];
    const uint64_t n_tok = n_all < P.capacity_in ? n_all : P.capacity_in;
    const uint64_t t0 = uint64_t(blockIdx.x) * kVocabTile;
    if (t0 >= n_tok) {   // (the whole workgroup: nothing below is reached by a part of it)
        if (err) atomicOr(P.status, err);
        return;
    }
    const uint64_t t1 = n_tok - t0 > kVocabTile ? t0 + kVocabTile - 1 : n_tok - 1;
    if (tid == 0) edge[0] = vocab_owner(P.token_offsets, P.n_docs, t0);
    if (tid == 64) edge[1] = vocab_owner(P.token_offsets, P.n_docs, t1);
    __syncthreads();
    const uint64_t d_lo = edge[0], d_hi = edge[1];
    const bool in_lds = d_hi >= d_lo && d_hi - d_lo + 2 <= kVocabLdsOffsets;
    const uint32_t n_own = in_lds ? uint32_t(d_hi - d_lo + 1) : 0u;   // documents of the slice; it holds n_own + 1 entries (d_hi + 1 <= n_docs)
    for (uint32_t k = tid; in_lds && k <= n_own; k += kVocabTile) soff[k] = P.token_offsets[d_lo + k];
    __syncthreads();
    const uint64_t tok = t0 + tid;
    if (tok < n_tok) {
        uint64_t d, first, next;
        if (in_lds) {
            const uint32_t j = uint32_t(vocab_owner(soff, uint64_t(n_own), tok));
            d = d_lo + j; first = soff[j]; next = soff[j + 1];
        } else {
            d = vocab_owner(P.token_offsets, P.n_docs, tok);
            first = P.token_offsets[d]; next = P.token_offsets[d + 1];
        }
        int32_t id = P.unk_id;
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
        if (!ok) err = kErrBadTokenCsr;
        const uint64_t nbytes = uint64_t(end) - uint64_t(start);
        if (ok && nbytes != 0 && nbytes <= 4ull * P.max_len) {
            const uint64_t b_at = db + start, b_end = db + end;
            uint64_t at = b_at, h = kRuleHashSeed;
            uint32_t len = 0;
            bool key = true;
            while (at < b_end) {
                uint32_t cp;
                if (len == P.max_len || !vocab_next_char(P.text, &at, b_end, P.cinfo, &cp)) { key = false; break; }
                h = rule_hash_step(h, cp);
                ++len;
            }
            if (key) {
                h = rule_hash_finish(h, len);
                const uint32_t fp = uint32_t(h >> 32), mask = (1u << P.bits) - 1u;
                uint32_t slot = uint32_t(h) & mask;
                for (uint32_t tries = 0; tries <= mask; ++tries, slot = (slot + 1) & mask) {   // (at most half of the slots are taken: an empty one ends every chain)
                    const uint4 e = P.slots[slot];
                    if (e.x == 0) break;
                    if (e.y == len && e.z == fp) {
                        bool same = true;
                        uint64_t v = b_at;
                        for (uint32_t j = 0; j < len && same; ++j) {
                            uint32_t cp = 0;
                            same = vocab_next_char(P.text, &v, b_end, P.cinfo, &cp) && P.surf[e.w + j] == cp;
                        }
                        if (same) { id = int32_t(e.x - 1u); break; }
                    }
                }
            }
        }
        P.ids[tok] = id;
    }
    if (err) atomicOr(P.status, err);
}

}  // namespace

hipError_t launch_token_ids(const VocabParams& P, hipStream_t stream) {
    if (P.n_docs == 0) return hipSuccess;
    const uint64_t blocks = P.capacity_in ? (P.capacity_in + kVocabTile - 1) / kVocabTile : 1;
    hipLaunchKernelGGL(token_ids_kernel, dim3(uint32_t(blocks)), dim3(kVocabTile), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
