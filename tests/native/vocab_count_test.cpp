// vaporetto_amd/csrc/vocab_count.hpp as a stand-alone program (tests/test_vocab_count_native.py builds it with the address and
// undefined-behaviour sanitizers): seeded key sets with tied counts and surfaces of 1- to 4-byte chars, in a shuffled "device" order, against an
// independent ordering (std::map over UTF-32 strings); the cuts; output arrays of exactly the sizes the header states (exact-size heap copies of
// the inputs, so that a read past either end is the sanitizer's).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>

#include "vocab_count.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (case %d)\n", __FILE__, __LINE__, #c, g_case); std::exit(1); } } while (0)
static int g_case = -1;

static std::string utf8_of(const std::u32string& s) {
    std::vector<uint8_t> b;
    for (char32_t c : s) vpt::vocab_count_put_utf8(uint32_t(c), &b);
    return std::string(b.begin(), b.end());
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
    static const char32_t alphabet[] = {U'a', U'b', U'z', 0xE9, 0x3B1, 0x3042, 0x3044, 0x6F22, 0xFF21, 0x1F90C, 0x20BB7, 0x10FFFF, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000};
    for (g_case = 0; g_case < cases; ++g_case) {
        std::mt19937_64 rng(1234 + g_case);
        const size_t n_keys = g_case == 0 ? 0 : 1 + rng() % 60;
        std::map<std::u32string, uint64_t> keys;
        while (keys.size() < n_keys) {
            std::u32string s;
            for (size_t k = 0, n = 1 + rng() % 4; k < n; ++k) s += alphabet[rng() % (sizeof(alphabet) / sizeof(alphabet[0]))];
            keys[s] = 1 + rng() % 4 + (rng() % 50 == 0 ? (uint64_t(1) << 40) : 0);   // many ties; a few counts above 32 bits
        }
        // the "device": the keys in a random order, their code points anywhere in the arena, unused gaps between them
        std::vector<std::pair<std::u32string, uint64_t>> order(keys.begin(), keys.end());
        std::shuffle(order.begin(), order.end(), rng);
        std::vector<uint32_t> arena;
        std::vector<vpt::VocabCountEntry> entries;
        for (const auto& kv : order) {
            for (size_t g = rng() % 3; g > 0; --g) arena.push_back(0x41);
            entries.push_back({kv.second, uint32_t(arena.size()), uint32_t(kv.first.size())});
            for (char32_t c : kv.first) arena.push_back(uint32_t(c));
        }
        uint32_t* a = static_cast<uint32_t*>(std::malloc(4 * arena.size() + 1));
        vpt::VocabCountEntry* e = static_cast<vpt::VocabCountEntry*>(std::malloc(sizeof(vpt::VocabCountEntry) * entries.size() + 1));
        for (size_t k = 0; k < arena.size(); ++k) a[k] = arena[k];
        for (size_t k = 0; k < entries.size(); ++k) e[k] = entries[k];
        const uint64_t min_count = 1 + rng() % 4, max_entries = rng() % 3 == 0 ? 0 : 1 + rng() % 70;
        // the order, independently: count descending, then the map's (code point) order
        std::vector<std::pair<std::u32string, uint64_t>> want;
        for (const auto& kv : keys) if (kv.second >= min_count) want.push_back(kv);
        std::stable_sort(want.begin(), want.end(), [](const auto& x, const auto& y) { return x.second > y.second; });
        if (max_entries && want.size() > max_entries) want.resize(size_t(max_entries));
        const vpt::VocabCountResult R = vpt::finish_vocab_count(e, entries.size(), a, arena.size(), min_count, max_entries);
        CHECK(R.counts.size() == want.size() && R.offsets.size() == want.size() + 1 && R.offsets[0] == 0);
        CHECK(R.surfaces.size() == R.offsets.back());
        for (size_t k = 0; k < want.size(); ++k) {
            const std::string s = utf8_of(want[k].first);
            CHECK(R.counts[k] == want[k].second);
            CHECK(R.offsets[k + 1] - R.offsets[k] == s.size());
            CHECK(std::string(R.surfaces.begin() + long(R.offsets[k]), R.surfaces.begin() + long(R.offsets[k + 1])) == s);
        }
        // twice: identical bytes, whatever order the device had
        std::shuffle(e, e + entries.size(), rng);
        const vpt::VocabCountResult R2 = vpt::finish_vocab_count(e, entries.size(), a, arena.size(), min_count, max_entries);
        CHECK(R2.surfaces == R.surfaces && R2.offsets == R.offsets && R2.counts == R.counts);
        std::free(a);
        std::free(e);
    }
    CHECK(vpt::vocab_counter_slots(1) == 2 && vpt::vocab_counter_slots(4) == 8 && vpt::vocab_counter_slots(5) == 16 &&
          vpt::vocab_counter_slots(vpt::kVocabCounterMaxKeys) == (1u << 25));
    CHECK(vpt::vocab_counter_arena_chars(4, 0) == 32 && vpt::vocab_counter_arena_chars(4, 7) == 7);
    std::printf("ok %d\n", cases);
    return 0;
}
