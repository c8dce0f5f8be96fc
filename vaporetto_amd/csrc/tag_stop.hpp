// The tag stop set of the token stream, resolved on the host: a list of (slot, tag string) pairs becomes one bitmap per slot over the ids of a
// vocabulary -- the predictor's (tag_vocab.hpp) and, when a pattern tagger is given, the tagger's.  A string found in a vocabulary sets its bit in
// the pair's slot; one found in neither matches nothing and is not an error.  Host only, no HIP type: compiles into a stand-alone program as well
// (tests/native/tag_stop_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

namespace vpt {
struct StopError : std::runtime_error { using std::runtime_error::runtime_error; };
struct StopBitmap {
    uint32_t words = 0;            // per slot: ceil(n_ids / 32), at least 1
    std::vector<uint32_t> bits;    // [n_tags * words]
};
// vocab_off [n_ids + 1] / vocab_bytes: the raw strings of the ids.  The error messages follow the pattern tagger's (pattern_tagger.cpp).
inline StopBitmap build_stop_bitmap(const uint32_t* slots, const uint8_t* tag_bytes, const uint64_t* tag_offsets, size_t n_entries, uint32_t n_tags,
                                    const uint32_t* vocab_off, const uint8_t* vocab_bytes, uint32_t n_ids) {
    auto reject = [](const char* what, size_t e) -> void { throw StopError(std::string("InvalidArgumentError: stop tags: ") + what + " (entry " + std::to_string(e) + ")"); };
    StopBitmap B;
    B.words = n_ids ? (n_ids + 31) / 32 : 1;
    B.bits.assign(size_t(n_tags) * B.words, 0u);
    std::unordered_map<std::string, uint32_t> ids;
    for (uint32_t k = 0; k < n_ids; ++k) ids.emplace(std::string(reinterpret_cast<const char*>(vocab_bytes) + vocab_off[k], vocab_off[k + 1] - vocab_off[k]), k);
    for (size_t e = 0; e < n_entries; ++e) {
        if (slots[e] >= n_tags) reject("a slot must be smaller than the predictor's n_tags", e);
        if (tag_offsets[e + 1] < tag_offsets[e]) reject("tag_offsets must be non-decreasing", e);
        const std::string tag(reinterpret_cast<const char*>(tag_bytes) + tag_offsets[e], size_t(tag_offsets[e + 1] - tag_offsets[e]));
        if (tag.find('\0') != std::string::npos) reject("a tag must not contain NULL", e);
        const auto it = ids.find(tag);
        if (it != ids.end()) B.bits[size_t(slots[e]) * B.words + (it->second >> 5)] |= 1u << (it->second & 31u);
    }
    return B;
}
}  // namespace vpt
