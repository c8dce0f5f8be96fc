// The vocabulary of the token stream's id pass as the device reads it (kernels_vocab.hip): token surface -> int32 id.  No item of the reference:
// what a caller who feeds a model or a term dictionary does with VaporettoTokenStream's tokens (vaporetto_tantivy/src/lib.rs:204-219) on the host.
// Host only, header only: no HIP type in here, so the builder compiles into a stand-alone program as well (tests/native/vocab_table_test.cpp).
//
// The layout is the rule table's (pattern_tagger.hpp), with the hash of a surface shared with it:
//   slots   open addressing (linear probing), 2^bits slots of 16 bytes -- ONE aligned 16-byte load is all a lane fetches for a token that is no
//           key: {id + 1 (0: empty), chars, high 32 bits of the surface's hash, where its code points start in `cps`}.  A lane goes on to `cps`
//           only when length and fingerprint agree, and verifies char by char.  2^bits is the smallest power of two >= 2 * keys: the load
//           factor is in (1/4, 1/2] for any vocabulary of at least one key (HostVocabTable::load()), so an empty slot ends every chain.
//   cps     the surfaces' code points, back to back, in the order of the ids
//   off     [n_keys + 1]: the bytes of surface `id` in `bytes`, as the caller gave them (vpt_vocab_surface)
// Entry k gets id k.  A surface names ONE id: a duplicate is an error here (the rules' last-wins has no meaning for ids).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "pattern_tagger.hpp"

namespace vpt {

struct VocabError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

constexpr size_t kVocabMaxEntries = size_t(1) << 24;

struct HostVocabTable {
    uint32_t bits = 1, n_keys = 0;
    uint32_t max_len = 0;      // the longest surface, in chars (0: no key)
    uint32_t max_probe = 0;    // the longest probe chain of a key (statistics)
    std::vector<uint32_t> slots, cps;
    std::vector<uint64_t> off;
    std::vector<uint8_t> bytes;
    double load() const { return double(n_keys) / double(size_t(1) << bits); }
};

// strict UTF-8 (what a Rust String holds): no overlong forms, no surrogates, nothing above U+10FFFF
inline bool vocab_decode_utf8(const uint8_t* s, size_t n, std::vector<uint32_t>* out) {
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

// the hash of a surface's code points (pattern_tagger.hpp): the slot it belongs to is the low `bits` bits, its fingerprint the high 32
inline uint64_t vocab_hash(const uint32_t* cps, uint32_t n) {
    uint64_t h = kRuleHashSeed;
    for (uint32_t k = 0; k < n; ++k) h = rule_hash_step(h, cps[k]);
    return rule_hash_finish(h, n);
}

// surfaces / offsets [n_entries + 1]: the entries' surfaces, packed UTF-8.
// Throws VocabError "InvalidArgumentError: vocab: <reason> (entry k)" for the first failing entry: invalid UTF-8, an empty surface, a NUL, a
// surface an earlier entry has.
inline HostVocabTable build_vocab_table(const uint8_t* surfaces, const uint64_t* offsets, size_t n_entries) {
    HostVocabTable T;
    if (n_entries > kVocabMaxEntries) throw VocabError("InvalidArgumentError: vocab: at most 2^24 entries");
    auto reject = [](const char* what, size_t k) -> void {
        throw VocabError(std::string("InvalidArgumentError: vocab: ") + what + " (entry " + std::to_string(k) + ")");
    };
    while ((size_t(1) << T.bits) < 2 * n_entries) ++T.bits;
    const uint32_t mask = (1u << T.bits) - 1u;
    T.slots.assign(size_t(4) << T.bits, 0u);
    T.off.reserve(n_entries + 1);
    T.off.push_back(0);
    std::vector<uint32_t> cps;
    for (size_t k = 0; k < n_entries; ++k) {
        if (offsets[k + 1] < offsets[k]) reject("offsets must be non-decreasing", k);
        const uint8_t* s = surfaces + offsets[k];
        const size_t len = size_t(offsets[k + 1] - offsets[k]);
        if (len == 0) reject("a surface must contain at least one character", k);
        cps.clear();
        if (!vocab_decode_utf8(s, len, &cps)) reject("a surface is not valid UTF-8", k);
        for (uint32_t c : cps) if (c == 0) reject("a surface must not contain NULL", k);
        if (cps.size() >= 0x40000000ull) reject("a surface is too long", k);
        const uint64_t h = vocab_hash(cps.data(), uint32_t(cps.size()));
        const uint32_t fp = uint32_t(h >> 32);
        uint32_t slot = uint32_t(h) & mask, probes = 1;
        for (;; slot = (slot + 1) & mask, ++probes) {
            uint32_t* e = &T.slots[size_t(slot) * 4];
            if (e[0] == 0) {
                if (T.cps.size() + cps.size() >= 0xFFFFFFF0ull) reject("the surfaces take 2^32 chars or more", k);
                e[0] = uint32_t(k) + 1; e[1] = uint32_t(cps.size()); e[2] = fp; e[3] = uint32_t(T.cps.size());
                T.cps.insert(T.cps.end(), cps.begin(), cps.end());
                break;
            }
            if (e[1] == cps.size() && e[2] == fp) {
                bool same = true;
                for (size_t j = 0; j < cps.size() && same; ++j) same = T.cps[e[3] + j] == cps[j];
                if (same) reject("a surface must not repeat an earlier entry's", k);
            }
        }
        ++T.n_keys;
        if (probes > T.max_probe) T.max_probe = probes;
        if (cps.size() > T.max_len) T.max_len = uint32_t(cps.size());
        T.bytes.insert(T.bytes.end(), s, s + len);
        T.off.push_back(uint64_t(T.bytes.size()));
    }
    return T;
}

// the id of a surface given as code points, or -1: the probe the kernel makes, on the host (the stand-alone test, and nothing on the product path)
inline int64_t vocab_find(const HostVocabTable& T, const uint32_t* cps, uint32_t n) {
    const uint32_t mask = (1u << T.bits) - 1u;
    const uint64_t h = vocab_hash(cps, n);
    for (uint32_t slot = uint32_t(h) & mask, tries = 0; tries <= mask; slot = (slot + 1) & mask, ++tries) {
        const uint32_t* e = &T.slots[size_t(slot) * 4];
        if (e[0] == 0) return -1;
        if (e[1] == n && e[2] == uint32_t(h >> 32)) {
            bool same = true;
            for (uint32_t j = 0; j < n && same; ++j) same = T.cps[e[3] + j] == cps[j];
            if (same) return int64_t(e[0]) - 1;
        }
    }
    return -1;
}

}  // namespace vpt
