// The tag vocabulary of a predictor: the distinct RAW tag strings of its tag models, numbered in order of first appearance over
// Model::tag_models, then slots, then candidates -- which is the order of the candidate strings in HostTagTables (tables.hpp: slot_str, str_off,
// str_bytes; the strings there are escaped the way Sentence::write_tokenized_text writes a tag, sentence.rs:871-880: a '\' in front of ' ',
// '\' and '/').  Built from those tables alone, so a predictor loaded from its compiled form has the same vocabulary, id for id.
// Host only, no HIP type: the builder compiles into a stand-alone program as well (tests/native/tag_vocab_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace vpt {
struct TagVocab {
    std::vector<uint32_t> raw_off{0};   // [n + 1] string `id` = raw_bytes[raw_off[id] .. raw_off[id + 1])
    std::vector<uint8_t> raw_bytes;
    std::vector<uint32_t> ids;          // [n_strings] candidate string k -> id
    std::vector<uint32_t> slot;         // [n_models * n_tags * 2] {the slot's first candidate string, its candidates} (0, 0: the model has no such slot)
    uint32_t size() const { return uint32_t(raw_off.size() - 1); }
};
// models: 12 words a tag model ([8] its first slot, [9] its slots); slots: 2 words a slot ([0] candidates); slot_str: a slot's first candidate
// string; str_off [n_strings + 1].  Whatever the arrays hold, nothing is read outside them: a model, slot or string that does not fit is left out.
inline TagVocab build_tag_vocab(const uint32_t* models, size_t n_models, const uint32_t* slots, size_t n_slot_words, const uint32_t* slot_str,
                                size_t n_slot_str, const uint32_t* str_off, size_t n_str_off, const uint8_t* str_bytes, size_t n_bytes, uint32_t n_tags) {
    TagVocab V;
    const size_t n_strings = n_str_off ? n_str_off - 1 : 0;
    V.ids.assign(n_strings, 0u);
    V.slot.assign(n_models * size_t(n_tags) * 2, 0u);
    std::unordered_map<std::string, uint32_t> seen;
    std::vector<bool> visited(n_strings, false);
    std::string raw;
    for (size_t m = 0; m < n_models; ++m) {
        const uint64_t first = models[12 * m + 8], ns = models[12 * m + 9];
        for (uint64_t j = 0; j < ns && j < n_tags; ++j) {
            const uint64_t s = first + j;
            if (2 * s + 1 >= n_slot_words || s >= n_slot_str) continue;
            const uint64_t cnt = slots[2 * s], k0 = slot_str[s];
            if (k0 + cnt > n_strings) continue;
            V.slot[(m * n_tags + j) * 2] = uint32_t(k0);
            V.slot[(m * n_tags + j) * 2 + 1] = uint32_t(cnt);
            for (uint64_t k = k0; k < k0 + cnt; ++k) {
                if (visited[k]) continue;   // (slots never share strings; a table that says so is walked once)
                visited[k] = true;
                const uint64_t a = str_off[k], b = str_off[k + 1];
                raw.clear();
                for (uint64_t q = a; q < b && q < n_bytes; ++q) {
                    if (str_bytes[q] == '\\' && q + 1 < b && q + 1 < n_bytes) ++q;   // the writer's escape: the byte behind it is the tag's
                    raw.push_back(char(str_bytes[q]));
                }
                const auto it = seen.find(raw);
                if (it != seen.end()) { V.ids[k] = it->second; continue; }
                const uint32_t id = V.size();
                seen.emplace(raw, id);
                V.ids[k] = id;
                V.raw_bytes.insert(V.raw_bytes.end(), raw.begin(), raw.end());
                V.raw_off.push_back(uint32_t(V.raw_bytes.size()));
            }
        }
    }
    return V;
}
}  // namespace vpt
