// TEST INFRASTRUCTURE: vaporetto_amd/csrc/host_chunks.hpp -- the three rules that cut a host batch into chunks and the sizes the pipelines take
// from them -- over seeded random batches, on the CPU (tests/test_chunk_cut_native.py builds this file alone, with the address and
// undefined-behaviour sanitizers: every staging array below is exactly as long as the header's bound says, so a word past it is a report).
//
// argv[1]: the number of batches.  Exit status 0 and one line "ok <batches> <cuts> <chunks>", or the first failed check on stderr and 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_chunks.hpp"

namespace {
using namespace vptcut;

uint64_t g_state;
uint64_t rnd(uint64_t n) {   // [0, n): splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) % n;
}

#define CHECK(cond)                                                                                                        \
    do {                                                                                                                   \
        if (!(cond)) {                                                                                                     \
            std::fprintf(stderr, "batch %llu, chunk size %llu, line %d: %s\n", g_batch, g_chunk, __LINE__, #cond);         \
            std::exit(1);                                                                                                  \
        }                                                                                                                  \
    } while (0)
unsigned long long g_batch, g_chunk, g_cuts, g_chunks;

struct Batch {
    std::vector<uint64_t> bytes, chars;   // per sentence
    std::vector<uint64_t> boff, ooff;     // what a caller passes: neither starts at 0
    size_t n() const { return bytes.size(); }
    void offsets() {
        boff.assign(1, 11); ooff.assign(1, 5);
        for (size_t i = 0; i < n(); ++i) { boff.push_back(boff[i] + bytes[i]); ooff.push_back(ooff[i] + chars[i] - 1); }
    }
};

// 1 .. 60 sentences of 1 .. 300 bytes, 1 .. 4 bytes per char.  kind 1: one sentence; 2: the first longer than three chunks; 3 / 4: sentence j
// ends where the batch's bytes / chars reach a multiple of the chunk size
Batch make_batch(int kind, uint64_t chunk) {
    Batch b;
    const size_t n = kind == 1 ? 1 : 1 + rnd(60);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t by = 1 + rnd(rnd(4) ? 30 : 300);
        b.bytes.push_back(by);
        b.chars.push_back((by + 3) / 4 + rnd(by - (by + 3) / 4 + 1));
    }
    if (kind == 2) { b.bytes[0] = std::min<uint64_t>(300, 3 * chunk + 1 + rnd(20)); b.chars[0] = b.bytes[0]; }
    if (kind == 3 || kind == 4) {
        const size_t j = rnd(n);
        uint64_t before = 0;
        for (size_t i = 0; i < j; ++i) before += kind == 3 ? b.bytes[i] : b.chars[i];
        const uint64_t len = chunk - before % chunk;   // 1 .. chunk
        if (len <= 300) { b.bytes[j] = len; b.chars[j] = len; }
    }
    b.offsets();
    return b;
}

void check_predict(const Batch& b, uint64_t chunk) {
    const size_t n = b.n();
    const size_t max_chunks = predict_max_chunks(n, b.ooff[n] - b.ooff[0] + n, chunk);
    std::vector<uint64_t> staging(predict_pinned_words(n, max_chunks));
    PredictCutter cutter{b.boff.data(), b.ooff.data(), n, chunk, max_chunks, staging.data()};
    size_t at = 0, k = 0;
    for (; !cutter.done(); ++k) {
        const PredictChunk c = cutter.next();
        CHECK(c.error == CutError::kNone && c.a == at && c.n >= 1 && at + c.n <= n);
        CHECK(k < max_chunks && cutter.staged <= staging.size() && c.off + 2 * (c.n + 1) == staging.data() + cutter.staged);
        CHECK(c.a + k + c.n + 1 <= offset_slots(n, max_chunks));
        uint64_t chars = 0, mb = 0, mc = 0;
        for (size_t j = 0; j < c.n; ++j) { chars += b.chars[at + j]; mb = std::max(mb, b.bytes[at + j]); mc = std::max(mc, b.chars[at + j]); }
        CHECK(c.chars == chars && c.max_bytes == mb && c.max_chars == mc);
        CHECK(chars - b.chars[at + c.n - 1] < chunk && (chars >= chunk || at + c.n == n));   // the rule: sentences until chunk chars are reached
        for (size_t j = 0; j <= c.n; ++j)
            CHECK(c.off[j] == b.boff[at + j] - b.boff[at] && c.off[c.n + 1 + j] == b.ooff[at + j] - b.ooff[at]);
        at += c.n;
    }
    CHECK(at == n && k >= 1);
    g_chunks += k;
}

// kind 0: sentence j is empty; 1: it claims more chars than it has bytes; 2: its boundary offsets go backwards; 3: the last offset claims fewer
// chars than the sentences in front of it hold (the ends of out_offsets size the staging)
void check_predict_errors(Batch b, uint64_t chunk, int kind) {
    const size_t n = b.n();
    size_t j = rnd(n);
    if (kind == 0) { b.bytes[j] = 0; b.chars[j] = 1; }
    if (kind == 1) b.chars[j] = b.bytes[j] + 1 + rnd(3);
    b.offsets();
    if (kind == 2) { for (size_t i = j + 1; i <= n; ++i) b.ooff[i] -= b.chars[j]; }   // ooff[j + 1] = ooff[j] - 1
    if (kind == 3) { j = n - 1; if (b.ooff[n - 1] == b.ooff[0]) return; b.ooff[n] = b.ooff[0]; }
    const size_t max_chunks = predict_max_chunks(n, b.ooff[n] - b.ooff[0] + n, chunk);
    std::vector<uint64_t> staging(predict_pinned_words(n, max_chunks));
    PredictCutter cutter{b.boff.data(), b.ooff.data(), n, chunk, max_chunks, staging.data()};
    for (size_t at = 0;;) {
        CHECK(!cutter.done());
        const PredictChunk c = cutter.next();
        CHECK(c.a == at && cutter.staged <= staging.size());
        at += c.n;
        if (c.error == CutError::kNone) { CHECK(c.n >= 1 && at <= j); continue; }
        CHECK(c.error == (kind == 0 ? CutError::kEmptySentence : CutError::kBadOffsets));
        CHECK(kind == 3 ? at <= j : at == j);   // (kind 3: refused at the latest where the sentence is; before it where the chunks run out)
        break;
    }
}

void check_stream(const Batch& b, uint64_t chunk) {
    const size_t n = b.n();
    const uint64_t nbytes = b.boff[n] - b.boff[0];
    const size_t max_chunks = stream_max_chunks(n, nbytes, chunk);
    std::vector<uint64_t> pinned(stream_pinned_words(n, max_chunks));
    StreamCutter cutter(b.boff.data(), n, chunk, pinned.data());
    CHECK(cutter.max_chunks == max_chunks && cutter.nbytes == nbytes);
    size_t at = 0, k = 0;
    for (; !cutter.done(); ++k) {
        const TokenizeChunk c = cutter.next();
        CHECK(c.a == at && c.n >= 1 && at + c.n <= n && k < max_chunks);
        CHECK(c.a + k + c.n + 1 <= offset_slots(n, max_chunks));
        uint64_t mb = 0;
        for (size_t j = 0; j < c.n; ++j) mb = std::max(mb, b.bytes[at + j]);
        CHECK(c.tb == b.boff[at] - b.boff[0] && c.nby == b.boff[at + c.n] - b.boff[at] && c.mb == mb);
        for (size_t j = 0; j <= at + c.n; ++j) CHECK(pinned[j] == b.boff[j] - b.boff[0]);
        // the rule: a chunk that is not the last ends with the sentence that reaches or crosses a multiple of the chunk size
        if (at + c.n < n && k + 1 < max_chunks) CHECK((c.tb + c.nby) / chunk > (c.tb + c.nby - b.bytes[at + c.n - 1]) / chunk);
        at += c.n;
    }
    CHECK(at == n && n + 1 + (k + 1) + 2 <= pinned.size());   // offsets, where every chunk's text ends, two status words
    g_chunks += k;
}

void check_tagged(const Batch& b, uint64_t chunk) {
    const size_t n = b.n();
    const uint64_t nbytes = b.boff[n] - b.boff[0];
    const size_t max_chunks = tagged_max_chunks(n, nbytes, chunk);
    std::vector<uint64_t> pinned(tagged_pinned_words(n, max_chunks));
    for (size_t i = 0; i <= n; ++i) pinned[i] = b.boff[i] - b.boff[0];
    size_t at = 0, k = 0;
    for (; at < n; ++k) {
        const TokenizeChunk c = tagged_chunk(pinned.data(), n, at, chunk);
        CHECK(c.a == at && c.n >= 1 && at + c.n <= n && k < max_chunks);
        CHECK(c.a + k + c.n + 1 <= offset_slots(n, max_chunks));
        uint64_t mb = 0;
        for (size_t j = 0; j < c.n; ++j) mb = std::max(mb, b.bytes[at + j]);
        CHECK(c.tb == pinned[at] && c.nby == pinned[at + c.n] - pinned[at] && c.mb == mb);
        CHECK(c.nby - b.bytes[at + c.n - 1] < chunk && (c.nby >= chunk || at + c.n == n));   // the rule: sentences until chunk bytes are reached
        at += c.n;
    }
    CHECK(n + 1 + k <= pinned.size());   // offsets, one total per chunk
    g_chunks += k;
}

}  // namespace

int main(int argc, char** argv) {
    const unsigned long long batches = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 3000;
    for (g_batch = 0; g_batch < batches; ++g_batch) {
        g_state = 0x5EED0000ull + g_batch;
        static const uint64_t sizes[4] = {1, 7, 50, 0};   // 0: larger than the batch
        g_chunk = sizes[g_batch % 4];
        const int kind = int(g_batch / 4 % 5);
        Batch b = make_batch(kind, g_chunk ? g_chunk : 50);
        if (!g_chunk) g_chunk = b.boff[b.n()] + 1 + rnd(1000);
        check_predict(b, g_chunk);
        check_stream(b, g_chunk);
        check_tagged(b, g_chunk);
        for (int e = 0; e < 4; ++e) check_predict_errors(b, g_chunk, e);
        ++g_cuts;
    }
    std::printf("ok %llu %llu %llu\n", batches, 3 * g_cuts, g_chunks);
    return 0;
}
