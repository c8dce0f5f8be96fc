// PatternMatchTagger's rule table (vaporetto_rules/src/sentence_filters/pattern_match_tagger.rs): HashMap<String, Vec<Option<String>>> as the
// device reads it (kernels_pattern.hip).  Host only: no HIP type in here, so the builder compiles into a stand-alone program as well.
//
//   slots      open addressing (linear probing) over the rule surfaces, 2^bits slots of 16 bytes -- ONE aligned 16-byte load, one L2 request, is all a
//              lane fetches for a token that is no key (most are not): {rule + 1 (0: empty), chars, high 32 bits of the surface's hash, where
//              its code points start in `cps`}.  A lane goes on to `cps` only when length and fingerprint agree, and verifies char by char.
//              The table holds at least two slots per key: the load factor is in (1/4, 1/2] (HostRuleTable::load()).
//   cps        the surfaces' code points, back to back
//   rule_tags  [n_rules * n_tags]: the rule's entry for slot j < n_tags -- the tag's id, or -1 (None: a None entry, or a list shorter than
//              j + 1).  Entries at j >= n_tags are dropped here (pattern_match_tagger.rs:26: the loop runs over the token's n_tags slots).
//   str_off    [n_ids + 1]: the bytes of tag `id` in str_bytes, ESCAPED the way Sentence::write_tokenized_text writes a tag (sentence.rs:871-880)
//   raw_off    ... and in raw_bytes as the caller gave them (vpt_pattern_tagger_tag)
// Ids: the distinct tag strings in the order the rules name them first (rule by rule, slot by slot; overridden duplicates included).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "layout.h"

namespace vpt {

// The hash of a surface: FNV-1a over its code points, finished with the length (the kernel computes the same from the decoded chars).
constexpr uint64_t kRuleHashSeed = 0xCBF29CE484222325ull;
VPT_HD uint64_t rule_hash_step(uint64_t h, uint32_t cp) { return (h ^ cp) * 0x100000001B3ull; }
VPT_HD uint64_t rule_hash_finish(uint64_t h, uint32_t len) {
    uint64_t x = h ^ len;
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    return x ^ (x >> 33);
}

struct RuleError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

struct HostRuleTable {
    uint32_t bits = 4, n_rules = 0, n_keys = 0, n_ids = 0, n_tags = 0;
    uint32_t max_len = 0;        // the longest surface, in chars (0: no rule)
    uint32_t max_suffix = 0;     // the most bytes one rule's tags take in the tokenized text: a '/' per slot up to the last Some + the escaped strings
    uint32_t max_probe = 0;      // the longest probe chain of a key (statistics)
    std::vector<uint32_t> slots, cps, str_off, raw_off;
    std::vector<int32_t> rule_tags;
    std::vector<uint8_t> str_bytes, raw_bytes;
    double load() const { return double(n_keys) / double(size_t(1) << bits); }
};

// surfaces / offsets [n_rules + 1]: the rules' surfaces, packed UTF-8; slot_counts [n_rules]: the length of every rule's list; present /
// tag_offsets: one entry per (rule, slot) in order -- present != 0: Some(tag_bytes[tag_offsets[k] .. tag_offsets[k + 1])), else None (its
// range is ignored).  A duplicate surface: the last rule wins (HashMap::insert).
// Throws RuleError "InvalidArgumentError: rules: ... (rule i)": invalid UTF-8, an empty surface, a NUL in a surface or in a tag.
HostRuleTable build_rule_table(const uint8_t* surfaces, const uint64_t* offsets, size_t n_rules, const uint32_t* slot_counts, const uint8_t* present,
                               const uint8_t* tag_bytes, const uint64_t* tag_offsets, uint32_t n_tags);

}  // namespace vpt
