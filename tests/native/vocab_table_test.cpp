// vaporetto_amd/csrc/vocab_table.hpp -- the host builder of the id pass's vocabulary -- as a stand-alone program: seeded random vocabularies, the
// load-factor bounds, every key found under its id and every non-key not found (the probe the kernel makes, vocab_find), the surfaces' bytes
// back, and the rejections by message.  Built with the address and undefined-behaviour sanitizers by tests/test_vocab_table_native.py.
//   vocab_table_test CASES  ->  "ok CASES"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "vocab_table.hpp"

namespace {

int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); if (++failures > 20) std::exit(1); } } while (0)

void put_utf8(std::string* s, uint32_t cp) {
    if (cp < 0x80) s->push_back(char(cp));
    else if (cp < 0x800) { s->push_back(char(0xC0 | (cp >> 6))); s->push_back(char(0x80 | (cp & 0x3F))); }
    else if (cp < 0x10000) { s->push_back(char(0xE0 | (cp >> 12))); s->push_back(char(0x80 | ((cp >> 6) & 0x3F))); s->push_back(char(0x80 | (cp & 0x3F))); }
    else { s->push_back(char(0xF0 | (cp >> 18))); s->push_back(char(0x80 | ((cp >> 12) & 0x3F))); s->push_back(char(0x80 | ((cp >> 6) & 0x3F))); s->push_back(char(0x80 | (cp & 0x3F))); }
}

using Word = std::vector<uint32_t>;

Word random_word(std::mt19937_64& rng) {
    static const uint32_t pool[] = {'A', 'B', '0', 0xE9, 0x3042, 0x3044, 0x6F22, 0x5B57, 0xFF21, 0x20BB7, 0x1F90C};
    Word w(1 + rng() % 5);
    for (uint32_t& c : w) c = pool[rng() % (sizeof(pool) / sizeof(pool[0]))];
    return w;
}

struct Packed {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off{0};
    void add(const std::string& s) { bytes.insert(bytes.end(), s.begin(), s.end()); off.push_back(bytes.size()); }
    void add(const Word& w) { std::string s; for (uint32_t c : w) put_utf8(&s, c); add(s); }
    const uint8_t* data() const { static const uint8_t none = 0; return bytes.empty() ? &none : bytes.data(); }
    size_t n() const { return off.size() - 1; }
};

void one_case(uint64_t seed) {
    std::mt19937_64 rng(seed);
    const size_t want = seed % 7 == 0 ? 1 + rng() % 3 : 1 + rng() % 300;
    std::set<Word> seen;
    std::vector<Word> keys;
    while (keys.size() < want) {
        Word w = random_word(rng);
        if (seen.insert(w).second) keys.push_back(w);
    }
    Packed P;
    for (const Word& w : keys) P.add(w);
    const vpt::HostVocabTable T = vpt::build_vocab_table(P.data(), P.off.data(), P.n());
    CHECK(T.n_keys == keys.size());
    CHECK(T.slots.size() == (size_t(4) << T.bits));
    CHECK(T.load() <= 0.5);
    CHECK(T.load() > 0.25);
    CHECK(T.off.size() == keys.size() + 1 && T.bytes == P.bytes);
    uint32_t longest = 0, taken = 0;
    for (size_t k = 0; k < keys.size(); ++k) {
        CHECK(vpt::vocab_find(T, keys[k].data(), uint32_t(keys[k].size())) == int64_t(k));
        CHECK(T.off[k] == P.off[k]);
        if (keys[k].size() > longest) longest = uint32_t(keys[k].size());
    }
    CHECK(T.max_len == longest);
    for (size_t s = 0; s < (size_t(1) << T.bits); ++s) taken += T.slots[4 * s] != 0;
    CHECK(taken == keys.size());
    for (int k = 0; k < 200; ++k) {   // non-keys: other words, a key with one char more, a key with its last char changed
        Word w = k % 3 == 0 ? random_word(rng) : keys[rng() % keys.size()];
        if (k % 3 == 1) w.push_back('A');
        if (k % 3 == 2) w.back() ^= 1u;
        if (seen.count(w)) continue;
        CHECK(vpt::vocab_find(T, w.data(), uint32_t(w.size())) == -1);
    }
}

void expect_error(const Packed& P, const char* want) {
    try {
        (void)vpt::build_vocab_table(P.data(), P.off.data(), P.n());
        std::fprintf(stderr, "no error, wanted: %s\n", want);
        ++failures;
    } catch (const vpt::VocabError& e) {
        if (std::strcmp(e.what(), want) != 0) { std::fprintf(stderr, "got: %s\nwanted: %s\n", e.what(), want); ++failures; }
    }
}

void rejections() {
    { Packed P; P.add(std::string("a")); P.add(std::string("b")); P.add(std::string("a")); P.add(std::string("b"));
      expect_error(P, "InvalidArgumentError: vocab: a surface must not repeat an earlier entry's (entry 2)"); }
    { Packed P; P.add(std::string("a")); P.add(std::string("")); P.add(std::string(""));
      expect_error(P, "InvalidArgumentError: vocab: a surface must contain at least one character (entry 1)"); }
    { Packed P; P.add(std::string("ab")); P.add(std::string("a\0b", 3));
      expect_error(P, "InvalidArgumentError: vocab: a surface must not contain NULL (entry 1)"); }
    const char* bad[] = {"\xC0\xAF", "\xE3\x81", "\xED\xA0\x80", "\xF4\x90\x80\x80", "\x80", "\xE0\x80\x80", "a\xFF"};
    for (const char* b : bad) {
        Packed P; P.add(std::string("ok")); P.add(std::string("x")); P.add(std::string(b)); P.add(std::string(""));
        expect_error(P, "InvalidArgumentError: vocab: a surface is not valid UTF-8 (entry 2)");
    }
    { Packed P;   // no entry: an empty table of two slots, nothing found
      const vpt::HostVocabTable T = vpt::build_vocab_table(P.data(), P.off.data(), 0);
      const uint32_t a = 'a';
      CHECK(T.n_keys == 0 && T.max_len == 0 && T.slots.size() == 8 && vpt::vocab_find(T, &a, 1) == -1); }
}

}  // namespace

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 2000;
    for (int k = 0; k < cases; ++k) one_case(1000 + uint64_t(k));
    rejections();
    if (failures) return 1;
    std::printf("ok %d\n", cases);
    return 0;
}
