// vaporetto_amd/csrc/tag_vocab.hpp alone, under the address and undefined-behaviour sanitizers (tests/test_tag_vocab_native.py): seeded random tag
// tables in arrays exactly as long as they say -- well-formed ones, whose vocabulary is checked against a plain walk, and hostile ones (slot
// numbers, string numbers and byte ranges past the arrays), which must be walked without a read outside them.  Prints "ok <cases>".
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "tag_vocab.hpp"

static void fail(const char* what, int c) { std::fprintf(stderr, "case %d: %s\n", c, what); std::exit(1); }

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 500;
    std::mt19937 rng(12345);
    const std::string alphabet[] = {"a", "b", "/", " ", "\\", "名", ""};
    for (int c = 0; c < cases; ++c) {
        const bool hostile = c % 3 == 2;
        const uint32_t n_tags = 1 + rng() % 3, n_models = rng() % 6;
        std::vector<uint32_t> models, slots, slot_str, str_off;
        std::vector<uint8_t> bytes;
        std::vector<std::string> want;            // the plain walk
        std::map<std::string, uint32_t> seen;
        std::vector<uint32_t> want_ids;
        for (uint32_t m = 0; m < n_models; ++m) {
            const uint32_t ns = rng() % (n_tags + 1);
            std::vector<uint32_t> rec(12, 0);
            rec[8] = uint32_t(slots.size() / 2); rec[9] = ns;
            models.insert(models.end(), rec.begin(), rec.end());
            for (uint32_t j = 0; j < ns; ++j) {
                const uint32_t cnt = rng() % 4;
                slots.push_back(cnt); slots.push_back(0);
                slot_str.push_back(uint32_t(str_off.size()));
                for (uint32_t k = 0; k < cnt; ++k) {
                    std::string raw;
                    for (uint32_t q = rng() % 4; q > 0; --q) raw += alphabet[rng() % 7];
                    str_off.push_back(uint32_t(bytes.size()));
                    for (char ch : raw) { if (ch == ' ' || ch == '\\' || ch == '/') bytes.push_back('\\'); bytes.push_back(uint8_t(ch)); }
                    auto it = seen.find(raw);
                    if (it == seen.end()) { it = seen.emplace(raw, uint32_t(want.size())).first; want.push_back(raw); }
                    want_ids.push_back(it->second);
                }
            }
        }
        str_off.push_back(uint32_t(bytes.size()));
        if (hostile) {   // numbers that point past the arrays
            for (auto& v : models) if (rng() % 5 == 0) v = rng();
            for (auto& v : slots) if (rng() % 5 == 0) v = rng();
            for (auto& v : slot_str) if (rng() % 5 == 0) v = rng();
            for (auto& v : str_off) if (rng() % 5 == 0) v = rng();
        }
        // arrays of exactly their sizes on the heap: a read past one is the sanitizer's
        std::vector<uint32_t> a(models), b(slots), s(slot_str), o(str_off);
        std::vector<uint8_t> y(bytes);
        a.shrink_to_fit(); b.shrink_to_fit(); s.shrink_to_fit(); o.shrink_to_fit(); y.shrink_to_fit();
        const vpt::TagVocab V = vpt::build_tag_vocab(a.data(), n_models, b.data(), b.size(), s.data(), s.size(), o.data(), o.size(), y.data(), y.size(), n_tags);
        if (V.ids.size() != o.size() - 1 || V.slot.size() != size_t(n_models) * n_tags * 2 || V.raw_off.size() != size_t(V.size()) + 1) fail("shape", c);
        for (uint32_t id : V.ids) if (V.size() ? id >= V.size() : id != 0) fail("an id past the vocabulary", c);
        if (hostile) continue;
        if (V.size() != want.size()) fail("size", c);
        for (uint32_t k = 0; k < V.size(); ++k)
            if (std::string(V.raw_bytes.begin() + V.raw_off[k], V.raw_bytes.begin() + V.raw_off[k + 1]) != want[k]) fail("string", c);
        if (V.ids != want_ids) fail("ids", c);
    }
    std::printf("ok %d\n", cases);
    return 0;
}
