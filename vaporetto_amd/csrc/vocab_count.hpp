// The vocabulary counter's host side (kernels_vocab_count.hip counts; this orders): the sizes of a counter, and what vpt_vocab_counter_finish
// hands out -- the counted surfaces, most frequent first, in the form vpt_vocab_create takes.  No item of the reference: what a caller does with
// a dict over VaporettoTokenStream's Token::text (vaporetto_tantivy/src/lib.rs:204-219) before it can make a term dictionary or a model's vocabulary.
// Host only, header only: no HIP type in here, so it compiles into a stand-alone program as well (tests/native/vocab_count_test.cpp).
//
// The device leaves one entry per counted key -- {count, where its code points start in the arena, chars} -- in the order its lanes happened to
// commit and compact them.  finish_vocab_count sorts them by count descending, then by code points ascending (a surface that is a prefix of
// another comes first): a TOTAL order, surfaces being distinct, so two runs give identical bytes whatever order the device had.  It keeps the
// first max_entries (0: all) and packs the surfaces as UTF-8: surfaces [offsets[n]] bytes, offsets [n + 1], counts [n].
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vpt {

constexpr uint64_t kVocabCounterMaxKeys = uint64_t(1) << 24;
constexpr uint64_t kVocabCounterMaxSurfaceChars = uint64_t(1) << 24;   // 4 * max_surface_chars is a byte length of 32 bits
constexpr uint64_t kVocabCounterMaxArenaChars = 0xFFFFFFF0ull;         // a key's first code point is a 32-bit index

// the smallest power of two >= 2 * max_keys: load factor at most 1/2, an empty slot ends every chain of a counter that is not full
inline uint32_t vocab_counter_slots(uint64_t max_keys) {
    uint32_t n = 2;
    while (uint64_t(n) < 2 * max_keys) n <<= 1;
    return n;
}
inline uint64_t vocab_counter_arena_chars(uint64_t max_keys, uint64_t arena_chars) { return arena_chars ? arena_chars : 8 * max_keys; }

struct VocabCountEntry {
    uint64_t count;
    uint32_t first, chars;   // arena[first .. first + chars)
};

struct VocabCountResult {
    std::vector<uint8_t> surfaces;
    std::vector<uint64_t> offsets;   // [n + 1]
    std::vector<uint64_t> counts;    // [n]
};

inline void vocab_count_put_utf8(uint32_t cp, std::vector<uint8_t>* out) {
    if (cp < 0x80u) {
        out->push_back(uint8_t(cp));
    } else if (cp < 0x800u) {
        out->push_back(uint8_t(0xC0u | (cp >> 6)));
        out->push_back(uint8_t(0x80u | (cp & 0x3Fu)));
    } else if (cp < 0x10000u) {
        out->push_back(uint8_t(0xE0u | (cp >> 12)));
        out->push_back(uint8_t(0x80u | ((cp >> 6) & 0x3Fu)));
        out->push_back(uint8_t(0x80u | (cp & 0x3Fu)));
    } else {
        out->push_back(uint8_t(0xF0u | (cp >> 18)));
        out->push_back(uint8_t(0x80u | ((cp >> 12) & 0x3Fu)));
        out->push_back(uint8_t(0x80u | ((cp >> 6) & 0x3Fu)));
        out->push_back(uint8_t(0x80u | (cp & 0x3Fu)));
    }
}

// entries [n] as the device left them (an entry that reaches outside arena[0 .. arena_len), or has no char, is dropped: the device writes none);
// min_count: entries below it are dropped (the device has dropped them already); max_entries: 0 keeps all.
inline VocabCountResult finish_vocab_count(const VocabCountEntry* entries, size_t n, const uint32_t* arena, size_t arena_len, uint64_t min_count,
                                           uint64_t max_entries) {
    std::vector<VocabCountEntry> kept;
    kept.reserve(n);
    for (size_t k = 0; k < n; ++k) {
        const VocabCountEntry& e = entries[k];
        if (e.count < min_count || e.chars == 0 || uint64_t(e.first) + e.chars > arena_len) continue;
        kept.push_back(e);
    }
    std::sort(kept.begin(), kept.end(), [arena](const VocabCountEntry& a, const VocabCountEntry& b) {
        if (a.count != b.count) return a.count > b.count;
        const uint32_t m = std::min(a.chars, b.chars);
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t x = arena[a.first + j], y = arena[b.first + j];
            if (x != y) return x < y;
        }
        if (a.chars != b.chars) return a.chars < b.chars;
        return a.first < b.first;   // (equal surfaces: the device holds a surface once)
    });
    if (max_entries && kept.size() > max_entries) kept.resize(size_t(max_entries));
    VocabCountResult R;
    size_t total_chars = 0;
    for (const VocabCountEntry& e : kept) total_chars += e.chars;
    R.surfaces.reserve(3 * total_chars);
    R.offsets.reserve(kept.size() + 1);
    R.counts.reserve(kept.size());
    R.offsets.push_back(0);
    for (const VocabCountEntry& e : kept) {
        for (uint32_t j = 0; j < e.chars; ++j) vocab_count_put_utf8(arena[e.first + j], &R.surfaces);
        R.offsets.push_back(uint64_t(R.surfaces.size()));
        R.counts.push_back(e.count);
    }
    return R;
}

}  // namespace vpt
