// How the host-buffer pipelines (capi_host.cpp) cut a batch into chunks, and the sizes that follow from the cuts: plain arithmetic over the
// caller's offset arrays -- no HIP, no allocation -- so that tests/native/chunk_cut_test.cpp holds every bound below to random batches on the CPU.
// Three rules, each with its max_chunks and the pinned words its pipeline stages; they stay three because their cut points were measured
// (capi_host.cpp says where).  A chunk k that starts at sentence a keeps its n + 1 device offsets at a + k of the batch's arrays (offset_slots).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace vptcut {

enum class CutError { kNone, kEmptySentence, kBadOffsets };

// One sentence of a predict batch: its bytes and chars (boundaries + 1).  n chars take between n and 4n bytes: anything else cannot have come
// from vpt_count_boundaries, and is refused before any buffer is sized from these numbers.
inline CutError check_sentence(const uint64_t* byte_offsets, const uint64_t* out_offsets, size_t i, uint64_t* n_bytes, uint64_t* n_chars) {
    if (byte_offsets[i + 1] <= byte_offsets[i]) return CutError::kEmptySentence;
    *n_bytes = byte_offsets[i + 1] - byte_offsets[i];
    if (out_offsets[i + 1] < out_offsets[i] || out_offsets[i + 1] - out_offsets[i] + 1 > *n_bytes) return CutError::kBadOffsets;
    *n_chars = out_offsets[i + 1] - out_offsets[i] + 1;
    return CutError::kNone;
}

// Device offsets of a batch cut into chunks: chunk k of sentences [a, a + n) has its n + 1 entries at a + k.  Enough for max_chunks chunks:
// a + n <= n_sentences and k <= max_chunks - 1, so the last entry, a + k + n, is below n_sentences + max_chunks.
inline size_t offset_slots(size_t n_sentences, size_t max_chunks) { return n_sentences + max_chunks + 1; }

// ---- vpt_predict_batch, both schedules: sentences until `chunk_chars` chars are reached
// total_chars: what the ENDS of out_offsets claim (out_offsets[n] - out_offsets[0] + n).  Enough: every chunk but the last holds chunk_chars
// chars or more, which makes total_chars / chunk_chars + 1 chunks (and one to spare), and every chunk holds a sentence.  The count is of valid
// offsets; PredictCutter refuses the chunk after the last one this allows, which only offsets that contradict their own ends can ask for.
inline size_t predict_max_chunks(size_t n_sentences, uint64_t total_chars, uint64_t chunk_chars) {
    return std::min<size_t>(n_sentences, size_t(total_chars / chunk_chars) + 2);
}
// Pinned words of a call: a chunk of n sentences stages 2 (n + 1) offsets, and the chunks share the sentences out.
inline size_t predict_pinned_words(size_t n_sentences, size_t max_chunks) { return 2 * (n_sentences + max_chunks); }

struct PredictChunk {
    size_t a, n;                           // sentences [a, a + n); after an error: a + n is the sentence that has it
    uint64_t chars, max_bytes, max_chars;  // chars of the chunk, its longest sentence both ways
    uint64_t* off;                         // n + 1 byte offsets, then n + 1 boundary offsets, both from 0: in `staging`
    CutError error;
};
struct PredictCutter {
    const uint64_t *byte_offsets, *out_offsets;
    size_t n_sentences;
    uint64_t chunk_chars;
    size_t max_chunks;                     // predict_max_chunks
    uint64_t* staging;                     // predict_pinned_words
    size_t at = 0, k = 0, staged = 0;      // next sentence, next chunk, words staged

    bool done() const { return at >= n_sentences; }
    // the next chunk: its sentences validated, its offsets rebased into the staging words behind those of the chunks before
    PredictChunk next() {
        PredictChunk c{at, 0, 0, 0, 0, staging + staged, CutError::kNone};
        if (k == max_chunks) { c.error = CutError::kBadOffsets; return c; }   // more chars than the ends of out_offsets say
        size_t i = at;
        while (i < n_sentences && c.chars < chunk_chars) {
            uint64_t nby = 0, nch = 0;
            if ((c.error = check_sentence(byte_offsets, out_offsets, i, &nby, &nch)) != CutError::kNone) { c.n = i - at; return c; }
            c.max_bytes = std::max(c.max_bytes, nby); c.max_chars = std::max(c.max_chars, nch);
            c.chars += nch;
            ++i;
        }
        c.n = i - at;
        const uint64_t t0 = byte_offsets[at], o0 = out_offsets[at];
        uint64_t* ho = c.off + (c.n + 1);
        for (size_t j = 0; j <= c.n; ++j) { c.off[j] = byte_offsets[at + j] - t0; ho[j] = out_offsets[at + j] - o0; }
        staged += 2 * (c.n + 1);
        at = i; ++k;
        return c;
    }
};

// ---- what both tokenize rules return
struct TokenizeChunk { size_t a, n; uint64_t tb, nby, mb; };   // sentences [a, a + n); first text byte (from the batch's), bytes, longest sentence

// ---- vpt_tokenize_batch without tags, vpt_token_stream_batch: chunk k of n_cuts should end at (k + 1) * chunk_bytes
inline size_t stream_cuts(uint64_t nbytes, uint64_t chunk_bytes) { return size_t((nbytes + chunk_bytes - 1) / chunk_bytes); }
// Enough by construction: StreamCutter::next gives its chunk the rest of the batch once max_chunks - 1 are out.  (A chunk per cut point, fewer
// where sentences longer than a chunk swallow some, one to spare.)
inline size_t stream_max_chunks(size_t n_sentences, uint64_t nbytes, uint64_t chunk_bytes) {
    return std::min<size_t>(n_sentences, stream_cuts(nbytes, chunk_bytes)) + 1;
}
// Pinned words of a call: the n + 1 offsets relative to the batch's text, where every chunk's text ends (a word per chunk and one), the two
// workspaces' status words.
inline size_t stream_pinned_words(size_t n_sentences, size_t max_chunks) { return n_sentences + 1 + max_chunks + 1 + 2; }

// Incremental: next() is called when a copy in is due, and rebases the offsets of its chunk only (h_boff[0 .. a + n] are then filled).
struct StreamCutter {
    const uint64_t* byte_offsets;
    size_t n_sentences;
    uint64_t chunk_bytes;
    uint64_t* h_boff;                      // n_sentences + 1 words: byte_offsets relative to byte_offsets[0]
    uint64_t nbytes;
    size_t n_cuts, max_chunks;
    size_t at = 0, cut_k = 0, k = 0;       // next sentence, next cut point, next chunk

    StreamCutter(const uint64_t* byte_offsets_, size_t n_sentences_, uint64_t chunk_bytes_, uint64_t* h_boff_)
        : byte_offsets(byte_offsets_), n_sentences(n_sentences_), chunk_bytes(chunk_bytes_), h_boff(h_boff_),
          nbytes(byte_offsets_[n_sentences_] - byte_offsets_[0]), n_cuts(stream_cuts(nbytes, chunk_bytes_)),
          max_chunks(stream_max_chunks(n_sentences_, nbytes, chunk_bytes_)) {
        h_boff[0] = 0;
    }
    bool done() const { return at >= n_sentences; }
    uint64_t cut_end(size_t c) const { return std::min<uint64_t>(nbytes, (c + 1) * chunk_bytes); }   // where chunk c of n_cuts should end
    TokenizeChunk next() {
        const size_t a = at;
        const uint64_t t0 = byte_offsets[0];
        uint64_t want = cut_end(cut_k++);
        while (want <= h_boff[a] && cut_k < n_cuts) want = cut_end(cut_k++);   // (a sentence longer than a chunk took these)
        size_t i = a;
        uint64_t mb = 0;
        do {
            h_boff[i + 1] = byte_offsets[i + 1] - t0;
            mb = std::max<uint64_t>(mb, h_boff[i + 1] - h_boff[i]);
            ++i;
        } while (i < n_sentences && (h_boff[i] < want || k + 1 >= max_chunks));
        at = i; ++k;
        return {a, i - a, h_boff[a], h_boff[i] - h_boff[a], mb};
    }
};

// ---- vpt_tokenize_batch with tags: greedy, sentences until `chunk_bytes` bytes are reached
// Enough: every chunk but the last holds chunk_bytes bytes or more (nbytes / chunk_bytes + 1 chunks, one to spare), and every chunk a sentence.
inline size_t tagged_max_chunks(size_t n_sentences, uint64_t nbytes, uint64_t chunk_bytes) {
    return std::min<size_t>(n_sentences, size_t(nbytes / chunk_bytes) + 2);
}
// Pinned words of a call: the n + 1 offsets relative to the batch's text, then one total per chunk.
inline size_t tagged_pinned_words(size_t n_sentences, size_t max_chunks) { return n_sentences + 1 + max_chunks; }
// the chunk that starts at sentence a; h_boff: all n_sentences + 1 offsets, relative to the batch's text
inline TokenizeChunk tagged_chunk(const uint64_t* h_boff, size_t n_sentences, size_t a, uint64_t chunk_bytes) {
    size_t i = a;
    uint64_t mb = 0;
    while (i < n_sentences && h_boff[i] - h_boff[a] < chunk_bytes) { mb = std::max<uint64_t>(mb, h_boff[i + 1] - h_boff[i]); ++i; }
    return {a, i - a, h_boff[a], h_boff[i] - h_boff[a], mb};
}

}  // namespace vptcut
