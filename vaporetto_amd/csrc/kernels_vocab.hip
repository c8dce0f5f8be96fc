// Vocabulary ids of the token stream (vocab_table.hpp): a pass of its own over a FINISHED span CSR -- what vpt_token_spans_batch_device /
// vpt_token_tags_batch_device write (token_starts == nullptr: a token starts where the one in front of it in its document ends, or at 0) or what
// vpt_token_filter_batch_device writes (starts and ends; a document may own no token) -- that leaves one int32 per token: the id of the token's
// surface, or unk_id.  The surface is the token's bytes in the caller's text, or with `cinfo` their KyteaFullwidthFilter image char by char
// (decode_chars_kernel's map: the text as it was scored, the convention of the rule surfaces, kernels_pattern.hip).
//
// A workgroup takes kVocabTile consecutive tokens, a LANE PER TOKEN; adjacent tokens are adjacent in the text, so a wave's text reads fall into
// a few consecutive cache lines.
//   owner       (vocab_resolve.h, shared with the counter's key pass) the token's document is the last i with token_offsets[i] <= t.  Two lanes find the owners of the tile's first and last token by
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
#include "vocab_resolve.h"

namespace vpt {
namespace {

__global__ __launch_bounds__(kVocabTile) void token_ids_kernel(const VocabParams P) {
    __shared__ uint64_t soff[kVocabLdsOffsets];   // token_offsets[d_lo ..]: the tile's documents and the end of the last
    __shared__ uint64_t edge[2];                  // d_lo, d_hi
    const uint32_t tid = threadIdx.x;
    uint32_t err = vocab_check_offsets(P);
    const uint64_t n_tok = vocab_token_count(P);
    const uint64_t t0 = uint64_t(blockIdx.x) * kVocabTile;
    if (t0 >= n_tok) {   // (the whole workgroup: nothing below is reached by a part of it)
        if (err) atomicOr(P.status, err);
        return;
    }
    uint64_t d_lo;
    const uint32_t n_own = vocab_tile_slice(P, n_tok, t0, soff, edge, &d_lo);
    const uint64_t tok = t0 + tid;
    if (tok < n_tok) {
        int32_t id = P.unk_id;
        uint64_t db;
        uint32_t start, end;
        const bool ok = vocab_token_span(P, tok, n_own, d_lo, soff, &db, &start, &end);
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
