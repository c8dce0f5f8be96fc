// The host builder of PatternMatchTagger's rule table (pattern_tagger.hpp).
#include "pattern_tagger.hpp"

#include <unordered_map>

namespace vpt {
namespace {

// strict UTF-8 (what a Rust String holds): no overlong forms, no surrogates, nothing above U+10FFFF
bool decode_utf8(const uint8_t* s, size_t n, std::vector<uint32_t>* out) {
    for (size_t i = 0; i < n;) {
        const uint32_t b0 = s[i];
        uint32_t cp, need;
        if (b0 < 0x80u) { cp = b0; need = 0; }
        else if (b0 >= 0xC2u && b0 < 0xE0u) { cp = b0 & 0x1Fu; need = 1; }
        else if (b0 >= 0xE0u && b0 < 0xF0u) { cp = b0 & 0x0Fu; need = 2; }
        else if (b0 >= 0xF0u && b0 < 0xF5u) { cp = b0 & 0x07u; need = 3; }
        else return false;
        if (n - i <= need) return false;
        for (uint32_t k = 1; k <= need; ++k) {
            const uint32_t b = s[i + k];
            if ((b & 0xC0u) != 0x80u) return false;
            cp = (cp << 6) | (b & 0x3Fu);
        }
        if ((need == 2 && (cp < 0x800u || (cp >= 0xD800u && cp < 0xE000u))) || (need == 3 && (cp < 0x10000u || cp > 0x10FFFFu))) return false;
        out->push_back(cp);
        i += need + 1;
    }
    return true;
}

[[noreturn]] void reject(const char* what, size_t rule) {
    throw RuleError(std::string("InvalidArgumentError: rules: ") + what + " (rule " + std::to_string(rule) + ")");
}

}  // namespace

HostRuleTable build_rule_table(const uint8_t* surfaces, const uint64_t* offsets, size_t n_rules, const uint32_t* slot_counts, const uint8_t* present,
                               const uint8_t* tag_bytes, const uint64_t* tag_offsets, uint32_t n_tags) {
    HostRuleTable T;
    if (n_rules > (size_t(1) << 30)) throw RuleError("InvalidArgumentError: rules: at most 2^30 rules");   // (2 slots per rule, 32-bit slot numbers: bits <= 31)
    T.n_rules = uint32_t(n_rules); T.n_tags = n_tags;
    while ((size_t(1) << T.bits) < 2 * n_rules) ++T.bits;
    const uint32_t mask = (1u << T.bits) - 1u;
    T.slots.assign(size_t(4) << T.bits, 0u);
    T.rule_tags.assign(n_rules * size_t(n_tags), -1);
    T.str_off.push_back(0); T.raw_off.push_back(0);
    std::unordered_map<std::string, uint32_t> ids;
    std::vector<uint32_t> cps;
    size_t entry = 0;   // the (rule, slot) entries in front of the rule
    for (size_t r = 0; r < n_rules; ++r) {
        if (offsets[r + 1] < offsets[r]) reject("offsets must be non-decreasing", r);
        const uint8_t* s = surfaces + offsets[r];
        const size_t len = size_t(offsets[r + 1] - offsets[r]);
        if (len == 0) reject("a surface must contain at least one character", r);
        cps.clear();
        if (!decode_utf8(s, len, &cps)) reject("a surface is not valid UTF-8", r);
        for (uint32_t c : cps) if (c == 0) reject("a surface must not contain NULL", r);
        // the rule's tags: ids for the slots below n_tags; every tag is checked
        uint32_t bytes = 0, last = 0;
        for (uint32_t j = 0; j < slot_counts[r]; ++j, ++entry) {
            if (!present[entry]) continue;
            if (tag_offsets[entry + 1] < tag_offsets[entry]) reject("tag_offsets must be non-decreasing", r);
            const uint8_t* t = tag_bytes + tag_offsets[entry];
            const size_t tl = size_t(tag_offsets[entry + 1] - tag_offsets[entry]);
            for (size_t k = 0; k < tl; ++k) if (t[k] == 0) reject("a tag must not contain NULL", r);
            if (tl >= 0x10000u) reject("a tag must be shorter than 65536 bytes", r);
            std::string key(reinterpret_cast<const char*>(t), tl);
            auto it = ids.find(key);
            if (it == ids.end()) {
                it = ids.emplace(std::move(key), uint32_t(ids.size())).first;
                T.raw_bytes.insert(T.raw_bytes.end(), t, t + tl);
                T.raw_off.push_back(uint32_t(T.raw_bytes.size()));
                for (size_t k = 0; k < tl; ++k) {   // sentence.rs:871-880
                    if (t[k] == ' ' || t[k] == '\\' || t[k] == '/') T.str_bytes.push_back('\\');
                    T.str_bytes.push_back(t[k]);
                }
                T.str_off.push_back(uint32_t(T.str_bytes.size()));
                if (T.str_bytes.size() >= 0x7FFFFFFFull) reject("the tags take 2 GB or more", r);
            }
            if (j < n_tags) {
                T.rule_tags[r * size_t(n_tags) + j] = int32_t(it->second);
                bytes += T.str_off[it->second + 1] - T.str_off[it->second];
                last = j + 1;
            }
        }
        if (bytes + last > T.max_suffix) T.max_suffix = bytes + last;
        if (cps.size() >= 0x40000000ull) reject("a surface is too long", r);
        // the surface's slot: its own when it is a key already (the last rule wins), else the first empty one of its chain
        uint64_t h = kRuleHashSeed;
        for (uint32_t c : cps) h = rule_hash_step(h, c);
        h = rule_hash_finish(h, uint32_t(cps.size()));
        const uint32_t fp = uint32_t(h >> 32);
        uint32_t slot = uint32_t(h) & mask, probes = 1;
        for (;; slot = (slot + 1) & mask, ++probes) {
            uint32_t* e = &T.slots[size_t(slot) * 4];
            if (e[0] == 0) {
                e[0] = uint32_t(r) + 1; e[1] = uint32_t(cps.size()); e[2] = fp; e[3] = uint32_t(T.cps.size());
                T.cps.insert(T.cps.end(), cps.begin(), cps.end());
                if (T.cps.size() >= 0xFFFFFFF0ull) reject("the surfaces take 2^32 chars or more", r);
                ++T.n_keys;
                if (probes > T.max_probe) T.max_probe = probes;
                if (cps.size() > T.max_len) T.max_len = uint32_t(cps.size());
                break;
            }
            if (e[1] == cps.size() && e[2] == fp) {
                bool same = true;
                for (size_t k = 0; k < cps.size() && same; ++k) same = T.cps[e[3] + k] == cps[k];
                if (same) { e[0] = uint32_t(r) + 1; break; }
            }
        }
    }
    T.n_ids = uint32_t(ids.size());
    return T;
}

}  // namespace vpt
