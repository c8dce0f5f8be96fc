// The host builder of PatternMatchTagger's rule table (vaporetto_amd/csrc/pattern_tagger.cpp) as a stand-alone program: every key is found
// again by the probe the kernel makes, a duplicate keeps the last rule, the errors name their rule.  Built by tests/test_pattern_tagger_table.py
// with g++ (and, by hand, with -fsanitize=address,undefined: it has its own main and needs no device).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../vaporetto_amd/csrc/pattern_tagger.hpp"

namespace {
int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

struct Rules {
    std::vector<uint8_t> surf, tags, present;
    std::vector<uint64_t> off{0}, toff{0};
    std::vector<uint32_t> counts;
    void add(const std::string& s, const std::vector<const char*>& list, const std::vector<size_t>& lens = {}) {
        surf.insert(surf.end(), s.begin(), s.end());
        off.push_back(surf.size());
        counts.push_back(uint32_t(list.size()));
        for (size_t k = 0; k < list.size(); ++k) {
            present.push_back(list[k] ? 1 : 0);
            if (list[k]) { const size_t n = k < lens.size() ? lens[k] : std::strlen(list[k]); tags.insert(tags.end(), list[k], list[k] + n); }
            toff.push_back(tags.size());
        }
    }
    vpt::HostRuleTable build(uint32_t n_tags) {
        surf.push_back(0); tags.push_back(0); present.push_back(0);
        return vpt::build_rule_table(surf.data(), off.data(), counts.size(), counts.data(), present.data(), tags.data(), toff.data(), n_tags);
    }
};

std::vector<uint32_t> decode(const std::string& s) {   // (valid UTF-8 only)
    std::vector<uint32_t> out;
    for (size_t i = 0; i < s.size();) {
        const uint8_t b = uint8_t(s[i]);
        const int n = b < 0x80 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
        uint32_t c = n == 1 ? b : b & (0xFFu >> (n + 1));
        for (int k = 1; k < n; ++k) c = (c << 6) | (uint8_t(s[i + k]) & 0x3Fu);
        out.push_back(c);
        i += n;
    }
    return out;
}

// the kernel's probe: rule + 1, or 0
uint32_t find(const vpt::HostRuleTable& T, const std::vector<uint32_t>& cps) {
    uint64_t h = vpt::kRuleHashSeed;
    for (uint32_t c : cps) h = vpt::rule_hash_step(h, c);
    h = vpt::rule_hash_finish(h, uint32_t(cps.size()));
    const uint32_t mask = (1u << T.bits) - 1u;
    for (uint32_t slot = uint32_t(h) & mask;; slot = (slot + 1) & mask) {
        const uint32_t* e = &T.slots[size_t(slot) * 4];
        if (e[0] == 0) return 0;
        if (e[1] == cps.size() && e[2] == uint32_t(h >> 32)) {
            bool same = true;
            for (size_t k = 0; k < cps.size() && same; ++k) same = T.cps[e[3] + k] == cps[k];
            if (same) return e[0];
        }
    }
}

void expect_error(Rules r, const char* msg) {
    try {
        r.build(2);
        std::printf("FAILED: no error, expected %s\n", msg);
        ++failures;
    } catch (const vpt::RuleError& e) {
        if (std::string(e.what()) != std::string("InvalidArgumentError: rules: ") + msg) { std::printf("FAILED: got '%s', expected '%s'\n", e.what(), msg); ++failures; }
    }
}
}  // namespace

int main() {
    {   // the semantics of one small table
        Rules r;
        r.add("\xe6\x9d\xb1\xe4\xba\xac", {"a", nullptr, "c"});
        r.add("b", {"x/y", ""});
        r.add("\xe6\x9d\xb1\xe4\xba\xac", {"last"});
        r.add("\xf0\x9f\xa4\x8c", {});
        const vpt::HostRuleTable T = r.build(2);
        CHECK(T.n_keys == 3 && T.n_rules == 4 && T.max_len == 2 && T.n_tags == 2);
        CHECK(find(T, decode("\xe6\x9d\xb1\xe4\xba\xac")) == 3 && find(T, decode("b")) == 2 && find(T, decode("\xf0\x9f\xa4\x8c")) == 4);
        CHECK(find(T, decode("\xe6\x9d\xb1")) == 0 && find(T, decode("bb")) == 0);
        CHECK(T.rule_tags[2 * 2] >= 0 && T.rule_tags[2 * 2 + 1] == -1 && T.rule_tags[0] >= 0 && T.rule_tags[1] == -1);
        CHECK(T.n_ids == 5);   // a, c, x/y, "", last -- c is kept as a string though its slot is past n_tags
        const int32_t xy = T.rule_tags[1 * 2], empty = T.rule_tags[1 * 2 + 1];
        CHECK(xy >= 0 && empty >= 0 && T.str_off[xy + 1] - T.str_off[xy] == 4 && T.raw_off[xy + 1] - T.raw_off[xy] == 3 && T.str_off[empty + 1] == T.str_off[empty]);
        CHECK(T.max_suffix == 2 + 4);   // "/x\/y/"
        CHECK(T.load() > 0.0 && T.load() <= 0.5);
    }
    {   // no rules
        Rules r;
        const vpt::HostRuleTable T = r.build(3);
        CHECK(T.n_keys == 0 && T.max_len == 0 && T.n_ids == 0 && find(T, {0x41}) == 0);
    }
    {   // many keys: chains, every key found, the load factor
        std::mt19937 rng(7);
        Rules r;
        std::vector<std::string> keys;
        for (int k = 0; k < 100000; ++k) {
            std::string s;
            for (int n = 1 + int(rng() % 5); n > 0; --n) { const uint32_t c = 0x3041 + rng() % 40; s += char(0xE0 | (c >> 12)); s += char(0x80 | ((c >> 6) & 0x3F)); s += char(0x80 | (c & 0x3F)); }
            keys.push_back(s);
            r.add(s, {(k % 3) ? "t" : nullptr, "u"});
        }
        const vpt::HostRuleTable T = r.build(2);
        CHECK(T.load() > 0.0 && T.load() <= 0.5 && T.max_probe >= 2);
        std::vector<uint32_t> last(keys.size());
        bool all = true;
        for (size_t k = 0; k < keys.size(); ++k) {
            const uint32_t got = find(T, decode(keys[k]));
            all = all && got != 0 && keys[got - 1] == keys[k] && got - 1 >= k;   // the rule found is the last with this surface
        }
        CHECK(all);
    }
    {
        Rules r; r.add("ok", {"t"}); r.add("\xe3\x81", {"t"});
        expect_error(r, "a surface is not valid UTF-8 (rule 1)");
    }
    { Rules r; r.add("\xc0\xaf", {"t"}); expect_error(r, "a surface is not valid UTF-8 (rule 0)"); }
    { Rules r; r.add("\xed\xa0\x80", {"t"}); expect_error(r, "a surface is not valid UTF-8 (rule 0)"); }
    { Rules r; r.add("\xf4\x90\x80\x80", {"t"}); expect_error(r, "a surface is not valid UTF-8 (rule 0)"); }
    { Rules r; r.add("ok", {}); r.add("", {"t"}); expect_error(r, "a surface must contain at least one character (rule 1)"); }
    { Rules r; r.add(std::string("a\0b", 3), {"t"}); expect_error(r, "a surface must not contain NULL (rule 0)"); }
    { Rules r; r.add("ok", {nullptr, nullptr, "t\0u"}, {0, 0, 3}); expect_error(r, "a tag must not contain NULL (rule 0)"); }
    if (failures) return 1;
    std::printf("rule table ok\n");
    return 0;
}
