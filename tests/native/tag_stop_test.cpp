// vaporetto_amd/csrc/tag_stop.hpp alone, under the address and undefined-behaviour sanitizers (tests/test_tag_stop_native.py): seeded random
// vocabularies and (slot, tag) lists in arrays exactly as long as they say -- every bit of the bitmaps against a plain search, strings outside
// the vocabulary, the empty string, an empty vocabulary, no entries; the three rejections by message.  Prints "ok <cases>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "tag_stop.hpp"

static void fail(const char* what, int c) { std::fprintf(stderr, "case %d: %s\n", c, what); std::exit(1); }

template <typename F>
static bool rejects(F f, const char* text) {
    try { f(); } catch (const vpt::StopError& e) { return std::string(e.what()).find(text) != std::string::npos; }
    return false;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 500;
    std::mt19937 rng(777);
    const std::string pieces[] = {"a", "b", "/", " ", "名", "助詞", ""};
    for (int c = 0; c < cases; ++c) {
        const uint32_t n_tags = 1 + rng() % 3, n_ids = c % 7 == 0 ? 0 : rng() % 70;
        std::vector<std::string> vocab;
        while (vocab.size() < n_ids) {   // distinct strings
            std::string s;
            for (uint32_t q = rng() % 4; q > 0; --q) s += pieces[rng() % 7];
            s += std::to_string(vocab.size());
            if (vocab.empty() && rng() % 2) s.clear();   // the empty string is a tag
            vocab.push_back(s);
        }
        std::vector<uint32_t> voff(1, 0);
        std::vector<uint8_t> vbytes;
        for (const auto& s : vocab) { vbytes.insert(vbytes.end(), s.begin(), s.end()); voff.push_back(uint32_t(vbytes.size())); }
        const size_t n_entries = c % 5 == 0 ? 0 : rng() % 40;
        std::vector<uint32_t> slots;
        std::vector<std::string> tags;
        for (size_t e = 0; e < n_entries; ++e) {
            slots.push_back(rng() % n_tags);
            tags.push_back(!vocab.empty() && rng() % 3 ? vocab[rng() % vocab.size()] : std::string("nowhere") + std::to_string(rng() % 9));
        }
        std::vector<uint64_t> toff(1, 0);
        std::vector<uint8_t> tbytes;
        for (const auto& s : tags) { tbytes.insert(tbytes.end(), s.begin(), s.end()); toff.push_back(tbytes.size()); }
        // arrays of exactly their sizes on the heap (one spare byte where data() of an empty vector would be null)
        std::vector<uint8_t> vb(vbytes), tb(tbytes);
        if (vb.empty()) vb.push_back(0);
        if (tb.empty()) tb.push_back(0);
        std::vector<uint32_t> sl(slots);
        if (sl.empty()) sl.push_back(0);
        const vpt::StopBitmap B = vpt::build_stop_bitmap(sl.data(), tb.data(), toff.data(), n_entries, n_tags, voff.data(), vb.data(), n_ids);
        if (B.words != (n_ids ? (n_ids + 31) / 32 : 1) || B.bits.size() != size_t(n_tags) * B.words) fail("shape", c);
        for (uint32_t j = 0; j < n_tags; ++j)
            for (uint32_t id = 0; id < B.words * 32; ++id) {
                bool want = false;
                for (size_t e = 0; e < n_entries; ++e) want |= slots[e] == j && id < n_ids && tags[e] == vocab[id];
                if ((((B.bits[size_t(j) * B.words + (id >> 5)] >> (id & 31u)) & 1u) != 0) != want) fail("bit", c);
            }
    }
    // the rejections
    const uint32_t voff[2] = {0, 1};
    const uint8_t vb[1] = {'x'};
    const uint32_t slots[2] = {0, 3};
    const uint8_t tb[3] = {'x', 0, 'y'};
    const uint64_t ok_off[3] = {0, 1, 1}, nul_off[3] = {0, 1, 3}, down_off[3] = {0, 1, 0};
    if (!rejects([&] { vpt::build_stop_bitmap(slots, tb, ok_off, 2, 3, voff, vb, 1); }, "a slot must be smaller than the predictor's n_tags (entry 1)")) fail("slot", -1);
    if (!rejects([&] { vpt::build_stop_bitmap(slots, tb, nul_off, 2, 4, voff, vb, 1); }, "a tag must not contain NULL (entry 1)")) fail("nul", -1);
    if (!rejects([&] { vpt::build_stop_bitmap(slots, tb, down_off, 2, 4, voff, vb, 1); }, "tag_offsets must be non-decreasing (entry 1)")) fail("offsets", -1);
    std::printf("ok %d\n", cases);
    return 0;
}
