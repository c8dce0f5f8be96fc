// vaporetto_hip.hpp -- C++ mirror of the `vaporetto` crate's boundary-scoring API on top of the C ABI (vaporetto_hip.h).
//
// The reference is compiled code (Rust) and has no FFI; INTEGRATION.md shows the Rust binding a maintainer would add.  This
// header is the same host side in C++, for callers that are not Rust: the names, argument meaning and error behaviour of
// vaporetto::{Model, Predictor, Sentence, CharacterBoundary, CharacterType, VaporettoError} (lib.rs:82-91) for the path this
// library accelerates -- Predictor::predict -- and the calls around it (fill_tags, iter_tokens, write_tokenized_text).
// Header only; link with -lvaporetto_hip.  There is no CPU path: every predict goes to the device.
//
//   auto model = vaporetto_hip::Model::read_slice(bytes.data(), bytes.size()).first;     // model.rs:127-135
//   vaporetto_hip::Predictor predictor(model, /*predict_tags=*/true);                     // predictor.rs:450
//   auto s = vaporetto_hip::Sentence::from_raw("まぁ社長は火星猫だ");                        // sentence.rs:217
//   predictor.predict(s);                                                                 // predictor.rs:518
//   s.fill_tags();                                                                        // sentence.rs:1144
//   std::string out = s.write_tokenized_text();                                           // sentence.rs:850
//
// One sentence per call costs two kernel launches and a synchronisation: anything with more than a handful of sentences
// belongs in Predictor::predict_batch (one launch for all of them) or Predictor::tokenize (lines in, tokenized lines out).
#ifndef VAPORETTO_HIP_HPP
#define VAPORETTO_HIP_HPP

#include <algorithm>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "vaporetto_grapheme.hpp"
#include "vaporetto_hip.h"

namespace vaporetto_hip {

// errors.rs:15-38.  `what()` is the reference's Display text where it defines one.
class VaporettoError : public std::runtime_error {
public:
    enum Kind { InvalidModel, InvalidArgument, Device };
    VaporettoError(Kind kind, const std::string& msg) : std::runtime_error(msg), kind_(kind) {}
    Kind kind() const { return kind_; }

private:
    Kind kind_;
};

namespace detail {
inline void check(vpt_status st) {
    if (st == VPT_OK) return;
    const std::string msg = vpt_last_error();
    throw VaporettoError(st == VPT_INVALID_MODEL ? VaporettoError::InvalidModel
                                                 : st == VPT_INVALID_ARGUMENT ? VaporettoError::InvalidArgument : VaporettoError::Device,
                         msg);
}
// What a Predictor and the sentences it predicted share: the library handle and the store_tag_scores flag (predictor.rs:436).
struct Shared {
    vpt_predictor* raw = nullptr;
    bool store_tag_scores = false;
    ~Shared() { if (raw) vpt_predictor_destroy(raw); }
};
}  // namespace detail

// sentence.rs:70-82
enum class CharacterBoundary : uint8_t { NotWordBoundary = VPT_NOT_WORD_BOUNDARY, WordBoundary = VPT_WORD_BOUNDARY, Unknown = VPT_BOUNDARY_UNKNOWN };

// sentence.rs:24-48 (the discriminants the models are trained with)
enum class CharacterType : uint8_t { Digit = 1, Roman = 2, Hiragana = 3, Katakana = 4, Kanji = 5, Other = 6 };

// CharacterType::get_type, sentence.rs:50-67
inline CharacterType get_type(char32_t c) {
    if ((c >= 0x30 && c <= 0x39) || (c >= 0xFF10 && c <= 0xFF19)) return CharacterType::Digit;
    if ((c >= 0x41 && c <= 0x5A) || (c >= 0x61 && c <= 0x7A) || (c >= 0xFF21 && c <= 0xFF3A) || (c >= 0xFF41 && c <= 0xFF5A)) return CharacterType::Roman;
    if (c >= 0x3040 && c <= 0x3096) return CharacterType::Hiragana;
    if ((c >= 0x30A0 && c <= 0x30FA) || (c >= 0x30FC && c <= 0x30FF) || (c >= 0xFF66 && c <= 0xFF9F)) return CharacterType::Katakana;
    if ((c >= 0x3400 && c <= 0x4DBF) || (c >= 0x4E00 && c <= 0x9FFF) || (c >= 0xF900 && c <= 0xFAFF) || (c >= 0x20000 && c <= 0x2A6DF) ||
        (c >= 0x2A700 && c <= 0x2B73F) || (c >= 0x2B740 && c <= 0x2B81F) || (c >= 0x2B820 && c <= 0x2CEAF) || (c >= 0x2F800 && c <= 0x2FA1F))
        return CharacterType::Kanji;
    return CharacterType::Other;
}

// model.rs:58-70: the bytes of a model ("VaporettoTokenizer 0.5.0\n" + bincode), validated by the library's decoder.
class Model {
public:
    // Model::read_slice (model.rs:127-135): the model and how many bytes it took (the rest belongs to the caller).
    static std::pair<Model, size_t> read_slice(const uint8_t* data, size_t len) {
        size_t used = 0;
        detail::check(vpt_model_read_len(data, len, &used));
        return {Model(std::vector<uint8_t>(data, data + used)), used};
    }
    const std::vector<uint8_t>& to_vec() const { return bytes_; }   // model.rs:99-104

private:
    explicit Model(std::vector<uint8_t> b) : bytes_(std::move(b)) {}
    std::vector<uint8_t> bytes_;
};

class Predictor;
class PatternMatchTagger;

// sentence.rs:85-101, raw-text path: the text, its character types, and after `predict` the boundary scores and labels.
class Sentence {
public:
    Sentence() { set_default(); }                                   // Sentence::default: a single space (sentence.rs:116)
    static Sentence from_raw(const std::string& text) {             // sentence.rs:217-245
        Sentence s;
        s.parse_raw(text);
        return s;
    }
    void update_raw(const std::string& text) {                      // sentence.rs:264-283: on error the sentence becomes " "
        try {
            parse_raw(text);
        } catch (const VaporettoError&) {
            set_default();
            throw;
        }
    }
    const std::string& as_raw_text() const { return text_; }                         // sentence.rs:782
    size_t len() const { return char_types_.size(); }                                // chars
    const std::vector<uint8_t>& char_types() const { return char_types_; }           // sentence.rs:1034
    const std::vector<uint8_t>& boundaries() const { return boundaries_; }           // sentence.rs:993 (CharacterBoundary values)
    std::vector<uint8_t>& boundaries_mut() { return boundaries_; }                   // sentence.rs:1016
    const std::vector<int32_t>& boundary_scores() const { return scores_; }          // sentence.rs:1040-1046 (empty before predict)
    const std::vector<size_t>& char_to_str_pos() const { return char_pos_; }         // len() + 1 byte positions
    uint32_t n_tags() const { return n_tags_; }                                      // sentence.rs:1161
    // Candidate indices per (char, slot), -1 = None; an entry is set on a token's LAST char (sentence.rs:1068 holds the strings:
    // the C ABI hands out indices, write_tokenized_text the strings).
    const std::vector<int32_t>& tag_indices() const { return tags_; }
    // Token::tag_candidates' numbers (sentence.rs:1218-1250) for the token that ENDS at char `c`: the tag model it matched (index
    // in Model::tag_models order, -1: none) and its score vector, slot after slot over the slots with >= 2 candidates.  Like the
    // reference this needs Predictor::store_tag_scores(true) before fill_tags (it throws otherwise, where the reference panics).
    int32_t tag_model(size_t c) const { need_scores(); return tag_models_.at(c); }
    std::vector<int32_t> tag_scores(size_t c) const {
        need_scores();
        return std::vector<int32_t>(tag_scores_.begin() + c * score_stride_, tag_scores_.begin() + (c + 1) * score_stride_);
    }
    // tagger: a PatternMatchTagger whose rules fill the slots fill_tags leaves None, on the device behind it (a rule tag is -(2 + id) in
    // tag_indices(); PatternMatchTagger::tag gives its string); the writer prints them when it is given the same tagger
    inline void fill_tags(const PatternMatchTagger* tagger = nullptr);               // sentence.rs:1144-1148
    inline std::string write_tokenized_text(const PatternMatchTagger* tagger = nullptr) const;   // sentence.rs:850-886

    // TokenIterator (sentence.rs:1265-1309), surfaces only: tokens next to an Unknown boundary are skipped.
    std::vector<std::string> iter_tokens() const {
        std::vector<std::string> out;
        const size_t n = len();
        size_t start = 0;
        bool valid = true;
        for (size_t e = 0; e < n; ++e) {
            const uint8_t b = e == n - 1 ? uint8_t(VPT_WORD_BOUNDARY) : boundaries_[e];
            if (b == VPT_BOUNDARY_UNKNOWN) valid = false;
            else if (b == VPT_WORD_BOUNDARY) {
                if (valid) out.push_back(text_.substr(char_pos_[start], char_pos_[e + 1] - char_pos_[start]));
                start = e + 1;
                valid = true;
            }
        }
        return out;
    }

private:
    friend class Predictor;
    void need_scores() const {
        if (tag_models_.empty()) throw VaporettoError(VaporettoError::InvalidArgument, "Predictor::store_tag_scores() must be set to true to use this function.");
    }
    void set_default() {                                            // sentence.rs:140-158
        text_ = " ";
        char_types_.assign(1, uint8_t(CharacterType::Other));
        char_pos_ = {0, 1};
        boundaries_.clear(); scores_.clear(); tags_.clear(); tag_scores_.clear(); tag_models_.clear();
        n_tags_ = 0; predictor_.reset();
    }
    void parse_raw(const std::string& text) {                       // sentence.rs:160-196
        if (text.find('\0') != std::string::npos) throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: text: must not contain NULL");
        if (text.empty()) throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: text: must contain at least one character");
        std::vector<uint8_t> types;
        std::vector<size_t> pos;
        for (size_t i = 0; i < text.size();) {                      // (a Rust &str is valid UTF-8; here: lead bytes delimit the chars)
            const unsigned char b0 = static_cast<unsigned char>(text[i]);
            size_t n = b0 < 0x80 ? 1 : b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4;
            if (i + n > text.size()) n = text.size() - i;
            char32_t c = n == 1 ? b0 : n == 2 ? (b0 & 0x1F) : n == 3 ? (b0 & 0x0F) : (b0 & 0x07);
            for (size_t k = 1; k < n; ++k) c = (c << 6) | (static_cast<unsigned char>(text[i + k]) & 0x3F);
            pos.push_back(i);
            types.push_back(uint8_t(get_type(c)));
            i += n;
        }
        pos.push_back(text.size());
        text_ = text;
        char_types_ = std::move(types);
        char_pos_ = std::move(pos);
        boundaries_.assign(char_types_.size() - 1, uint8_t(VPT_BOUNDARY_UNKNOWN));
        scores_.clear(); tags_.clear(); tag_scores_.clear(); tag_models_.clear();
        n_tags_ = 0; predictor_.reset();
    }

    std::string text_;
    std::vector<uint8_t> char_types_;
    std::vector<size_t> char_pos_;
    std::vector<uint8_t> boundaries_;
    std::vector<int32_t> scores_;
    std::vector<int32_t> tags_;
    std::vector<int32_t> tag_scores_, tag_models_;   // only with store_tag_scores (sentence.rs:96)
    uint32_t n_tags_ = 0, score_stride_ = 0;
    // predictor.rs:542: the predictor that last predicted this sentence.  The reference ties the two with a lifetime
    // (`Sentence<'_, 'a>` borrows `&'a Predictor`); here the sentence SHARES the library handle, so fill_tags() and
    // write_tokenized_text() stay valid when the Predictor object has been moved from or destroyed in the meantime.
    std::shared_ptr<detail::Shared> predictor_;
};

// predictor.rs:433-665.  Immutable after construction; `predict` takes `&self`, any number of threads may share one.
class Predictor {
public:
    Predictor(const Model& model, bool predict_tags, int device_id = 0) : predict_tags_(predict_tags) {   // Predictor::new, predictor.rs:450-508
        raw_ = std::make_shared<detail::Shared>();
        detail::check(vpt_predictor_create(model.to_vec().data(), model.to_vec().size(), predict_tags ? 1 : 0, device_id, &raw_->raw));
    }
    // the handle is reference-counted (sentences that were predicted hold it too): moving is cheap, copying is not offered
    // -- the reference's Predictor is not Clone either
    Predictor(const Predictor&) = delete;
    Predictor& operator=(const Predictor&) = delete;
    Predictor(Predictor&&) noexcept = default;
    Predictor& operator=(Predictor&&) noexcept = default;

    const vpt_predictor* raw() const { return raw_->raw; }
    uint32_t n_tags() const { uint32_t n = 0; detail::check(vpt_predictor_n_tags(raw_->raw, &n)); return n; }
    void store_tag_scores(bool flag) { raw_->store_tag_scores = flag; }   // predictor.rs:510-514

    // Predictor::predict (predictor.rs:518-543): scores and labels of one sentence.
    void predict(Sentence& s) const {
        const size_t n = s.len();
        std::vector<int32_t> scores(n > 1 ? n - 1 : 1);
        std::vector<uint8_t> labels(n > 1 ? n - 1 : 1);
        size_t nb = 0;
        detail::check(vpt_predict_one(raw_->raw, reinterpret_cast<const uint8_t*>(s.text_.data()), s.text_.size(), scores.data(), labels.data(), &nb));
        scores.resize(nb); labels.resize(nb);
        s.scores_ = std::move(scores); s.boundaries_ = std::move(labels);
        s.tags_.clear(); s.tag_scores_.clear(); s.tag_models_.clear(); s.n_tags_ = 0; s.predictor_ = raw_;   // tags and their scores go together (sentence.rs:96, predictor.rs:599-601)
    }

    // The same for many sentences with one launch (flags: VPT_FLAG_*).
    void predict_batch(std::vector<Sentence>& sentences, unsigned flags = 0) const {
        if (sentences.empty()) return;
        std::string text;
        std::vector<uint64_t> boff(1, 0), ooff(1, 0);
        for (const Sentence& s : sentences) {
            text += s.text_;
            boff.push_back(text.size());
            ooff.push_back(ooff.back() + (s.len() - 1));
        }
        std::vector<int32_t> scores(size_t(ooff.back()) + 1);
        std::vector<uint8_t> labels(size_t(ooff.back()) + 1);
        detail::check(vpt_predict_batch_flags(raw_->raw, reinterpret_cast<const uint8_t*>(text.data()), boff.data(), sentences.size(), scores.data(),
                                              labels.data(), ooff.data(), flags));
        for (size_t i = 0; i < sentences.size(); ++i) {
            Sentence& s = sentences[i];
            s.scores_.assign(scores.begin() + ooff[i], scores.begin() + ooff[i + 1]);
            s.boundaries_.assign(labels.begin() + ooff[i], labels.begin() + ooff[i + 1]);
            s.tags_.clear(); s.tag_scores_.clear(); s.tag_models_.clear(); s.n_tags_ = 0; s.predictor_ = raw_;   // tags and their scores go together (sentence.rs:96, predictor.rs:599-601)
        }
    }

    // Lines in, tokenized lines out: the CLI's loop (predict/src/main.rs:122-176) for a batch, everything on the device.
    // tagger (with tagged): PatternMatchTagger behind fill_tags, in the same one call (vpt_tokenize_batch_rules).
    inline std::vector<std::string> tokenize(const std::vector<std::string>& lines, bool tagged = false, unsigned flags = 0,
                                             const PatternMatchTagger* tagger = nullptr) const;

    // The `predict` CLI's stdout per line with --scores / --tag-scores (predict/src/main.rs:66-93, 122-176), formatted on the device:
    // listing = VPT_LISTING_* bits, flags = VPT_FLAG_* (vpt_predict_listing_batch).
    std::vector<std::string> predict_listing(const std::vector<std::string>& lines, unsigned listing, unsigned flags = VPT_FLAG_KYTEA_FULLWIDTH) const {
        std::vector<std::string> out;
        if (lines.empty()) return out;
        std::string text;
        std::vector<uint64_t> boff(1, 0);
        size_t chars = 0;
        for (const std::string& l : lines) { text += l; boff.push_back(text.size()); }
        for (unsigned char c : text) chars += (c & 0xC0) != 0x80;
        uint32_t sfx = 0, cand = 0;
        if (listing & VPT_LISTING_TAGGED) detail::check(vpt_predictor_max_tag_suffix(raw_->raw, &sfx));
        if (listing & VPT_LISTING_TAG_SCORES) detail::check(vpt_predictor_max_tag_listing(raw_->raw, &cand));
        const size_t S = lines.size(), B = text.size();
        size_t cap = 3 * B + S + chars * sfx;
        if (listing & VPT_LISTING_SCORES) cap += 32 * (chars - S) + S;
        if (listing & VPT_LISTING_TAG_SCORES) cap += 3 * B + chars + S + chars * size_t(cand);
        std::vector<uint8_t> buf(cap + 16);
        std::vector<uint64_t> off(S + 1);
        detail::check(vpt_predict_listing_batch(raw_->raw, reinterpret_cast<const uint8_t*>(text.data()), boff.data(), S, flags, listing, nullptr, nullptr,
                                                buf.data(), cap, off.data()));
        for (size_t i = 0; i < S; ++i) out.emplace_back(buf.begin() + off[i], buf.begin() + off[i + 1]);
        return out;
    }

    // The tag vocabulary (vpt_predictor_n_tag_strings / vpt_predictor_tag_string): the distinct raw tag strings of the tag models in order of
    // first appearance over tag models, slots, candidates -- what the ids >= 0 of the tagged token stream name.  Empty without predict_tags.
    std::vector<std::string> tag_strings() const {
        uint32_t n = 0;
        detail::check(vpt_predictor_n_tag_strings(raw_->raw, &n));
        std::vector<std::string> out;
        for (uint32_t k = 0; k < n; ++k) {
            const uint8_t* p = nullptr;
            size_t len = 0;
            detail::check(vpt_predictor_tag_string(raw_->raw, k, &p, &len));
            out.emplace_back(reinterpret_cast<const char*>(p), len);
        }
        return out;
    }

private:
    friend class Sentence;
    friend class PatternMatchTagger;
    friend class TagStopFilter;
    friend class Vocabulary;
    friend class VocabularyCounter;
    std::shared_ptr<detail::Shared> raw_;
    bool predict_tags_;
};

// vaporetto_rules' PatternMatchTagger (sentence_filters/pattern_match_tagger.rs:10-41) on the device: rules[surface] fills the tag slots
// fill_tags left None (never one that is Some; entries past the predictor's n_tags are ignored; nullopt stays None, "" is a tag).  The table
// is built and uploaded once, for ONE predictor (its device, its n_tags); a repeated surface keeps the last rule, like HashMap::insert.
// Pass it to Sentence::fill_tags / write_tokenized_text or Predictor::tokenize.  Keeps the predictor's handle alive.
class PatternMatchTagger {
public:
    using Rules = std::vector<std::pair<std::string, std::vector<std::optional<std::string>>>>;
    PatternMatchTagger(const Predictor& predictor, const Rules& rules) : predictor_(predictor.raw_) {   // PatternMatchTagger::new
        std::string surf, tags;
        std::vector<uint64_t> off(1, 0), toff(1, 0);
        std::vector<uint32_t> counts;
        std::vector<uint8_t> present;
        for (const auto& r : rules) {
            surf += r.first;
            off.push_back(surf.size());
            counts.push_back(uint32_t(r.second.size()));
            for (const auto& t : r.second) {
                present.push_back(t ? 1 : 0);
                if (t) tags += *t;
                toff.push_back(tags.size());
            }
        }
        surf.push_back('\0'); tags.push_back('\0'); counts.push_back(0); present.push_back(0);   // (no empty array's data() is handed over)
        detail::check(vpt_pattern_tagger_create(predictor_->raw, reinterpret_cast<const uint8_t*>(surf.data()), off.data(), rules.size(), counts.data(),
                                                present.data(), reinterpret_cast<const uint8_t*>(tags.data()), toff.data(), &raw_));
    }
    ~PatternMatchTagger() { vpt_pattern_tagger_destroy(raw_); }
    PatternMatchTagger(const PatternMatchTagger&) = delete;
    PatternMatchTagger& operator=(const PatternMatchTagger&) = delete;

    const void* raw() const { return raw_; }
    uint32_t n_tags() const { uint32_t n = 0; detail::check(vpt_pattern_tagger_n_tags(raw_, &n)); return n; }   // the distinct tag strings: the ids
    std::string tag(uint32_t id) const {                                                                          // the string of rule tag -(2 + id)
        const uint8_t* p = nullptr;
        size_t n = 0;
        detail::check(vpt_pattern_tagger_tag(raw_, id, &p, &n));
        return std::string(reinterpret_cast<const char*>(p), n);
    }
    uint32_t max_tag_suffix() const { uint32_t n = 0; detail::check(vpt_pattern_tagger_max_tag_suffix(raw_, &n)); return n; }

private:
    std::shared_ptr<detail::Shared> predictor_;
    void* raw_ = nullptr;
};

// A stop set for the tagged token stream (vpt_tag_stop_create): (slot, tag string) pairs -- a token is dropped when, for some pair, its slot's tag
// equals the pair's string, a tag model's or (with `tagger`) a rule's; None never matches; a string in neither vocabulary matches nothing.
// Tied to ONE predictor (and the tagger's ids); immutable.  Keeps the predictor's handle alive.
class TagStopFilter {
public:
    using Pairs = std::vector<std::pair<uint32_t, std::string>>;
    TagStopFilter(const Predictor& predictor, const Pairs& pairs, const PatternMatchTagger* tagger = nullptr) : predictor_(predictor.raw_) {
        std::string tags;
        std::vector<uint64_t> toff(1, 0);
        std::vector<uint32_t> slots;
        for (const auto& p : pairs) {
            slots.push_back(p.first);
            tags += p.second;
            toff.push_back(tags.size());
        }
        slots.push_back(0);   // (no empty array's data() is handed over; std::string::data() is never null)
        detail::check(vpt_tag_stop_create(predictor_->raw, tagger ? tagger->raw() : nullptr, slots.data(), reinterpret_cast<const uint8_t*>(tags.data()),
                                          toff.data(), pairs.size(), &raw_));
    }
    ~TagStopFilter() { vpt_tag_stop_destroy(raw_); }
    TagStopFilter(const TagStopFilter&) = delete;
    TagStopFilter& operator=(const TagStopFilter&) = delete;
    const void* raw() const { return raw_; }

private:
    std::shared_ptr<detail::Shared> predictor_;
    void* raw_ = nullptr;
};

// A vocabulary for the token stream's ids (vpt_vocab_create): entry k of `surfaces` gets id k, a token that is no entry unk_id.  An empty surface,
// a NUL, invalid UTF-8 and a repeated surface throw, naming the entry.  Tied to ONE predictor; immutable.  Keeps the predictor's handle alive.
class Vocabulary {
public:
    Vocabulary(const Predictor& predictor, const std::vector<std::string>& surfaces, int32_t unk_id = -1) : predictor_(predictor.raw_), unk_id_(unk_id) {
        std::string bytes;
        std::vector<uint64_t> off(1, 0);
        for (const std::string& s : surfaces) { bytes += s; off.push_back(bytes.size()); }
        detail::check(vpt_vocab_create(predictor_->raw, reinterpret_cast<const uint8_t*>(bytes.data()), off.data(), surfaces.size(), unk_id, &raw_));
    }
    ~Vocabulary() { vpt_vocab_destroy(raw_); }
    Vocabulary(const Vocabulary&) = delete;
    Vocabulary& operator=(const Vocabulary&) = delete;
    const void* raw() const { return raw_; }
    int32_t unk_id() const { return unk_id_; }
    size_t size() const { uint32_t n = 0; detail::check(vpt_vocab_info(raw_, &n, nullptr, nullptr)); return n; }
    std::string surface(uint32_t id) const {
        const uint8_t* b = nullptr;
        size_t n = 0;
        detail::check(vpt_vocab_surface(raw_, id, &b, &n));
        return std::string(reinterpret_cast<const char*>(b), n);
    }

private:
    std::shared_ptr<detail::Shared> predictor_;
    void* raw_ = nullptr;
    int32_t unk_id_;
};

// A vocabulary counter (vpt_vocab_counter_create): token surface -> count, accumulated on the predictor's device; entries() is what Vocabulary
// takes.  max_keys distinct surfaces (1 .. 2^24), tokens of more than max_surface_chars chars are skipped, arena_chars code points over all keys
// (0: 8 * max_keys).  Tied to ONE predictor, whose handle it keeps alive.  MUTABLE: one call at a time, in stream order.  A counter that has
// become full throws "vocab counter: full" from count calls and entries() until reset().
class VocabularyCounter {
public:
    struct Info { uint64_t n_keys, n_counted, n_skipped; uint32_t n_slots; bool full; };
    VocabularyCounter(const Predictor& predictor, uint64_t max_keys, uint64_t max_surface_chars = 64, uint64_t arena_chars = 0) : predictor_(predictor.raw_) {
        detail::check(vpt_vocab_counter_create(predictor_->raw, max_keys, max_surface_chars, arena_chars, &raw_));
    }
    ~VocabularyCounter() { vpt_vocab_counter_destroy(raw_); }
    VocabularyCounter(const VocabularyCounter&) = delete;
    VocabularyCounter& operator=(const VocabularyCounter&) = delete;
    void* raw() const { return raw_; }
    void reset() { detail::check(vpt_vocab_counter_reset(raw_)); }
    Info info() const {
        Info i{};
        uint32_t full = 0;
        detail::check(vpt_vocab_counter_info(raw_, &i.n_keys, &i.n_counted, &i.n_skipped, &i.n_slots, &full));
        i.full = full != 0;
        return i;
    }
    // A snapshot: {surface, count} of the keys of count >= min_count, by count descending, then by code points ascending; the first
    // max_entries of them (0: all).  Copies of the handle's arrays.
    std::vector<std::pair<std::string, uint64_t>> entries(uint64_t min_count = 1, uint64_t max_entries = 0) const {
        const uint8_t* s = nullptr;
        const uint64_t *off = nullptr, *cnt = nullptr;
        size_t n = 0;
        detail::check(vpt_vocab_counter_finish(raw_, min_count, max_entries, &s, &off, &cnt, &n));
        std::vector<std::pair<std::string, uint64_t>> out;
        out.reserve(n);
        for (size_t k = 0; k < n; ++k) out.emplace_back(std::string(reinterpret_cast<const char*>(s) + off[k], size_t(off[k + 1] - off[k])), cnt[k]);
        return out;
    }

private:
    std::shared_ptr<detail::Shared> predictor_;
    void* raw_ = nullptr;
};

// The postings of one batch of documents (a segment), term-major (vpt_token_stream_postings_batch): term k's postings are
// [term_offsets[k], term_offsets[k + 1]) of docs (doc_base + the document's index, ascending within a term) and tfs; its document frequency is
// the difference of the two offsets.  n_dropped: the tokens whose id was no term.
struct Postings {
    std::vector<uint64_t> term_offsets;   // [n_terms + 1]
    std::vector<uint32_t> docs, tfs;
    // A positional segment (VaporettoTokenizer::index with positions) also has first [postings + 1] and positions [indexed tokens]: posting q's
    // positions are positions[first[q] .. first[q + 1]), strictly ascending; both empty otherwise.
    std::vector<uint64_t> first;
    std::vector<uint32_t> positions;
    uint64_t n_dropped = 0;
    size_t n_terms() const { return term_offsets.size() - 1; }
    uint64_t df(size_t term) const { return term_offsets[term + 1] - term_offsets[term]; }
    uint64_t n_combined = 0;   // merge: the input postings that were combined into another
    // The merge of segments that share a term id space (vpt_postings_merge): per term the union of their lists by document, a document that
    // stands in several of them one posting whose tf is the sum; n_dropped the segments' sum.  ordered: the promise that every segment's
    // documents are above those of the one before -- checked on the device, no sort.  n_terms: the merged term count (0: the largest of the
    // segments').  No token lists: token indices are local to a segment.  positions: the position lists are merged too
    // (vpt_postings_merge_positional; every segment must be positional): the result has first and positions, a merged posting's list the
    // ascending union of its inputs', and phrase_search runs on it; without it both stay empty.
    static Postings merge(const Predictor& predictor, const std::vector<Postings>& segments, bool ordered = false, size_t n_terms = 0,
                          bool positions = false);
    // BM25 top-k of every query over this segment (vpt_postings_search; the definition is in vaporetto_hip.h).  queries: term ids, a slot per
    // id, ids outside [0, n_terms) score nothing.  doc_lens[i]: the length of document doc_base + i (VaporettoTokenizer::doc_lens).  weights:
    // shaped as queries, or nullptr for vpt_okapi_idf(n_documents, df(term)) per slot.  avgdl = float(sum(doc_lens) / n_documents), in double.
    struct Hit { uint32_t document; float score; };
    struct SearchResult {
        std::vector<std::vector<Hit>> hits;   // per query at most k, by score descending, then document ascending
        std::vector<uint64_t> match_counts;   // per query
        uint64_t counts[3] = {0, 0, 0};       // candidates, matches, skipped slots
    };
    SearchResult search(const Predictor& predictor, const std::vector<std::vector<int32_t>>& queries, const std::vector<uint32_t>& doc_lens,
                        uint64_t doc_base = 0, uint32_t k = 10, float k1 = 1.2f, float b = 0.75f,
                        const std::vector<std::vector<float>>* weights = nullptr) const;
    // BM25 top-k of every boolean query over this segment (vpt_postings_boolean_search; the definition is in vaporetto_hip.h).  A slot is a
    // term and an occur (VPT_OCCUR_SHOULD / VPT_OCCUR_MUST / VPT_OCCUR_MUST_NOT): a document matches when every MUST slot has it, no MUST_NOT
    // slot has it and, without a MUST slot, some SHOULD slot has it.  weights: shaped as queries, or nullptr for vpt_okapi_idf(n_documents,
    // df(term)) per MUST / SHOULD slot and 0 per MUST_NOT slot.  counts[0] of the result: the places.
    struct Clause { int32_t term; uint8_t occur; };
    SearchResult boolean_search(const Predictor& predictor, const std::vector<std::vector<Clause>>& queries, const std::vector<uint32_t>& doc_lens,
                                uint64_t doc_base = 0, uint32_t k = 10, float k1 = 1.2f, float b = 0.75f,
                                const std::vector<std::vector<float>>* weights = nullptr) const;
    // Exact-phrase BM25 top-k of every phrase over this POSITIONAL segment (vpt_postings_phrase_search; the definition is in vaporetto_hip.h).
    // phrases: term ids, each vector ONE phrase, its ids at consecutive positions in order; an id outside [0, n_terms) makes it match nothing.
    // weights: one per phrase, or nullptr for tantivy's phrase weight (the float sum, in slot order, of vpt_okapi_idf over the slots).
    // slop: the slop of every phrase, 0 .. 31 (tantivy's set_slop; the definition is in vaporetto_hip.h); 0 is the exact call, anything else
    // vpt_postings_sloppy_phrase_search.
    struct PhraseHit { uint32_t document; float score; uint32_t freq; };
    struct PhraseResult {
        std::vector<std::vector<PhraseHit>> hits;   // per phrase at most k, by score descending, then document ascending
        std::vector<uint64_t> match_counts;         // per phrase
        uint64_t counts[3] = {0, 0, 0};             // probes, matches, skipped phrases
    };
    PhraseResult phrase_search(const Predictor& predictor, const std::vector<std::vector<int32_t>>& phrases, const std::vector<uint32_t>& doc_lens,
                               uint64_t doc_base = 0, uint32_t k = 10, float k1 = 1.2f, float b = 0.75f,
                               const std::vector<float>* weights = nullptr, uint32_t slop = 0) const;
    // BM25 top-k of every boolean query of CLAUSES over this POSITIONAL segment (vpt_postings_clause_search; the definition is in
    // vaporetto_hip.h).  A clause of one term is a slot of that term, as in boolean_search; every other clause is ONE exact phrase scored by
    // its phrase frequency (an id outside [0, n_terms) makes it match nothing, and so does an empty clause).  weights: shaped as queries, or
    // nullptr for the phrase weight of phrase_search per MUST / SHOULD clause and 0 per MUST_NOT clause.  counts of the result: the places, the
    // matches, the skipped clauses.  slop: the slop of every clause that is a phrase (vpt_postings_sloppy_clause_search when not 0).
    struct PhraseClause { std::vector<int32_t> terms; uint8_t occur; };
    SearchResult clause_search(const Predictor& predictor, const std::vector<std::vector<PhraseClause>>& queries, const std::vector<uint32_t>& doc_lens,
                               uint64_t doc_base = 0, uint32_t k = 10, float k1 = 1.2f, float b = 0.75f,
                               const std::vector<std::vector<float>>* weights = nullptr, uint32_t slop = 0) const;
};

inline Postings::SearchResult Postings::clause_search(const Predictor& predictor, const std::vector<std::vector<PhraseClause>>& queries,
                                                      const std::vector<uint32_t>& doc_lens, uint64_t doc_base, uint32_t k, float k1, float b,
                                                      const std::vector<std::vector<float>>* weights, uint32_t slop) const {
    SearchResult out;
    if (queries.empty()) return out;
    if (first.size() != docs.size() + 1)
        throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: clause_search: the postings were made without positions");
    if (term_offsets.empty() || doc_lens.empty() || (weights && weights->size() != queries.size()) || docs.size() != tfs.size() ||
        term_offsets.back() != docs.size() || first.back() != positions.size())
        throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: clause_search: the arrays do not belong together");
    double total = 0;
    for (uint32_t l : doc_lens) total += double(l);
    const float avgdl = float(total / double(doc_lens.size()));
    std::vector<uint64_t> qoff(1, 0), coff(1, 0);
    std::vector<int32_t> terms;
    std::vector<float> w;
    std::vector<uint8_t> occurs;
    for (size_t q = 0; q < queries.size(); ++q) {
        if (weights && (*weights)[q].size() != queries[q].size())
            throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: weights: not shaped as the queries");
        for (size_t j = 0; j < queries[q].size(); ++j) {
            const PhraseClause& c = queries[q][j];
            float sum = 0.0f;
            bool any = false;
            for (const int32_t t : c.terms) {
                terms.push_back(t);
                if (weights || c.occur == VPT_OCCUR_MUST_NOT || t < 0 || size_t(t) >= n_terms()) continue;
                float x = 0.0f;
                detail::check(vpt_okapi_idf(doc_lens.size(), df(size_t(t)), &x));
                sum = any ? sum + x : x;
                any = true;
            }
            w.push_back(weights ? (*weights)[q][j] : sum);
            occurs.push_back(c.occur);
            coff.push_back(terms.size());
        }
        qoff.push_back(occurs.size());
    }
    terms.push_back(0); w.push_back(0.0f); occurs.push_back(0);   // (data() of an empty vector may be NULL)
    std::vector<uint32_t> pos(positions);
    pos.push_back(0);
    const size_t n_out = queries.size() * size_t(k) + 1;
    std::vector<uint32_t> hd(n_out), hc(queries.size());
    std::vector<float> hs(n_out);
    out.match_counts.assign(queries.size(), 0);
    if (slop == 0) {
        detail::check(vpt_postings_clause_search(predictor.raw(), term_offsets.data(), docs.data(), tfs.data(), first.data(), pos.data(),
                                                 uint32_t(n_terms()), doc_base, doc_lens.size(), doc_lens.data(), qoff.data(), coff.data(), terms.data(),
                                                 w.data(), occurs.data(), uint32_t(queries.size()), k1, b, avgdl, k, hd.data(), hs.data(), hc.data(),
                                                 out.match_counts.data(), out.counts));
    } else {
        const std::vector<uint32_t> slops(occurs.size(), slop);
        detail::check(vpt_postings_sloppy_clause_search(predictor.raw(), term_offsets.data(), docs.data(), tfs.data(), first.data(), pos.data(),
                                                        uint32_t(n_terms()), doc_base, doc_lens.size(), doc_lens.data(), qoff.data(), coff.data(),
                                                        terms.data(), w.data(), occurs.data(), slops.data(), uint32_t(queries.size()), k1, b, avgdl, k,
                                                        hd.data(), hs.data(), hc.data(), out.match_counts.data(), out.counts));
    }
    out.hits.resize(queries.size());
    for (size_t q = 0; q < queries.size(); ++q)
        for (uint32_t j = 0; j < hc[q]; ++j) out.hits[q].push_back(Hit{hd[q * size_t(k) + j], hs[q * size_t(k) + j]});
    return out;
}

inline Postings::PhraseResult Postings::phrase_search(const Predictor& predictor, const std::vector<std::vector<int32_t>>& phrases,
                                                      const std::vector<uint32_t>& doc_lens, uint64_t doc_base, uint32_t k, float k1, float b,
                                                      const std::vector<float>* weights, uint32_t slop) const {
    PhraseResult out;
    if (phrases.empty()) return out;
    if (first.size() != docs.size() + 1)
        throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: phrase_search: the postings were made without positions");
    if (term_offsets.empty() || doc_lens.empty() || (weights && weights->size() != phrases.size()) || docs.size() != tfs.size() ||
        term_offsets.back() != docs.size() || first.back() != positions.size())
        throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: phrase_search: the arrays do not belong together");
    double total = 0;
    for (uint32_t l : doc_lens) total += double(l);
    const float avgdl = float(total / double(doc_lens.size()));
    std::vector<uint64_t> qoff(1, 0);
    std::vector<int32_t> terms;
    std::vector<float> w;
    for (size_t q = 0; q < phrases.size(); ++q) {
        float sum = 0.0f;
        bool any = false;
        for (const int32_t t : phrases[q]) {
            terms.push_back(t);
            if (weights || t < 0 || size_t(t) >= n_terms()) continue;
            float x = 0.0f;
            detail::check(vpt_okapi_idf(doc_lens.size(), df(size_t(t)), &x));
            sum = any ? sum + x : x;
            any = true;
        }
        w.push_back(weights ? (*weights)[q] : sum);
        qoff.push_back(terms.size());
    }
    terms.push_back(0);   // (data() of an empty vector may be NULL)
    std::vector<uint32_t> pos(positions);
    pos.push_back(0);
    const size_t n_out = phrases.size() * size_t(k) + 1;
    std::vector<uint32_t> hd(n_out), hf(n_out), hc(phrases.size());
    std::vector<float> hs(n_out);
    out.match_counts.assign(phrases.size(), 0);
    if (slop == 0) {
        detail::check(vpt_postings_phrase_search(predictor.raw(), term_offsets.data(), docs.data(), tfs.data(), first.data(), pos.data(),
                                                 uint32_t(n_terms()), doc_base, doc_lens.size(), doc_lens.data(), qoff.data(), terms.data(), w.data(),
                                                 uint32_t(phrases.size()), k1, b, avgdl, k, hd.data(), hs.data(), hf.data(), hc.data(),
                                                 out.match_counts.data(), out.counts));
    } else {
        const std::vector<uint32_t> slops(phrases.size(), slop);
        detail::check(vpt_postings_sloppy_phrase_search(predictor.raw(), term_offsets.data(), docs.data(), tfs.data(), first.data(), pos.data(),
                                                        uint32_t(n_terms()), doc_base, doc_lens.size(), doc_lens.data(), qoff.data(), terms.data(),
                                                        w.data(), slops.data(), uint32_t(phrases.size()), k1, b, avgdl, k, hd.data(), hs.data(),
                                                        hf.data(), hc.data(), out.match_counts.data(), out.counts));
    }
    out.hits.resize(phrases.size());
    for (size_t q = 0; q < phrases.size(); ++q)
        for (uint32_t j = 0; j < hc[q]; ++j) out.hits[q].push_back(PhraseHit{hd[q * size_t(k) + j], hs[q * size_t(k) + j], hf[q * size_t(k) + j]});
    return out;
}

inline Postings::SearchResult Postings::search(const Predictor& predictor, const std::vector<std::vector<int32_t>>& queries, const std::vector<uint32_t>& doc_lens,
                                               uint64_t doc_base, uint32_t k, float k1, float b, const std::vector<std::vector<float>>* weights) const {
    SearchResult out;
    if (queries.empty()) return out;
    if (term_offsets.empty() || doc_lens.empty() || (weights && weights->size() != queries.size()))
        throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: search: the arrays do not belong together");
    double total = 0;
    for (uint32_t l : doc_lens) total += double(l);
    const float avgdl = float(total / double(doc_lens.size()));
    std::vector<uint64_t> qoff(1, 0);
    std::vector<int32_t> terms;
    std::vector<float> w;
    for (size_t q = 0; q < queries.size(); ++q) {
        if (weights && (*weights)[q].size() != queries[q].size())
            throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: weights: not shaped as the queries");
        for (size_t j = 0; j < queries[q].size(); ++j) {
            const int32_t t = queries[q][j];
            float x = 0.0f;
            if (weights) x = (*weights)[q][j];
            else if (t >= 0 && size_t(t) < n_terms()) detail::check(vpt_okapi_idf(doc_lens.size(), df(size_t(t)), &x));
            terms.push_back(t);
            w.push_back(x);
        }
        qoff.push_back(terms.size());
    }
    terms.push_back(0); w.push_back(0.0f);   // (data() of an empty vector may be NULL)
    const size_t n_out = queries.size() * size_t(k) + 1;
    std::vector<uint32_t> hd(n_out), hc(queries.size());
    std::vector<float> hs(n_out);
    out.match_counts.assign(queries.size(), 0);
    detail::check(vpt_postings_search(predictor.raw(), term_offsets.data(), docs.data(), tfs.data(), uint32_t(n_terms()), doc_base, doc_lens.size(),
                                      doc_lens.data(), qoff.data(), terms.data(), w.data(), uint32_t(queries.size()), k1, b, avgdl, k, hd.data(), hs.data(),
                                      hc.data(), out.match_counts.data(), out.counts));
    out.hits.resize(queries.size());
    for (size_t q = 0; q < queries.size(); ++q)
        for (uint32_t j = 0; j < hc[q]; ++j) out.hits[q].push_back(Hit{hd[q * size_t(k) + j], hs[q * size_t(k) + j]});
    return out;
}

inline Postings::SearchResult Postings::boolean_search(const Predictor& predictor, const std::vector<std::vector<Clause>>& queries,
                                                       const std::vector<uint32_t>& doc_lens, uint64_t doc_base, uint32_t k, float k1, float b,
                                                       const std::vector<std::vector<float>>* weights) const {
    SearchResult out;
    if (queries.empty()) return out;
    if (term_offsets.empty() || doc_lens.empty() || (weights && weights->size() != queries.size()))
        throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: boolean_search: the arrays do not belong together");
    double total = 0;
    for (uint32_t l : doc_lens) total += double(l);
    const float avgdl = float(total / double(doc_lens.size()));
    std::vector<uint64_t> qoff(1, 0);
    std::vector<int32_t> terms;
    std::vector<float> w;
    std::vector<uint8_t> occurs;
    for (size_t q = 0; q < queries.size(); ++q) {
        if (weights && (*weights)[q].size() != queries[q].size())
            throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: weights: not shaped as the queries");
        for (size_t j = 0; j < queries[q].size(); ++j) {
            const int32_t t = queries[q][j].term;
            float x = 0.0f;
            if (weights) x = (*weights)[q][j];
            else if (queries[q][j].occur != VPT_OCCUR_MUST_NOT && t >= 0 && size_t(t) < n_terms())
                detail::check(vpt_okapi_idf(doc_lens.size(), df(size_t(t)), &x));
            terms.push_back(t);
            w.push_back(x);
            occurs.push_back(queries[q][j].occur);
        }
        qoff.push_back(terms.size());
    }
    terms.push_back(0); w.push_back(0.0f); occurs.push_back(0);   // (data() of an empty vector may be NULL)
    const size_t n_out = queries.size() * size_t(k) + 1;
    std::vector<uint32_t> hd(n_out), hc(queries.size());
    std::vector<float> hs(n_out);
    out.match_counts.assign(queries.size(), 0);
    detail::check(vpt_postings_boolean_search(predictor.raw(), term_offsets.data(), docs.data(), tfs.data(), uint32_t(n_terms()), doc_base, doc_lens.size(),
                                              doc_lens.data(), qoff.data(), terms.data(), w.data(), occurs.data(), uint32_t(queries.size()), k1, b, avgdl, k,
                                              hd.data(), hs.data(), hc.data(), out.match_counts.data(), out.counts));
    out.hits.resize(queries.size());
    for (size_t q = 0; q < queries.size(); ++q)
        for (uint32_t j = 0; j < hc[q]; ++j) out.hits[q].push_back(Hit{hd[q * size_t(k) + j], hs[q * size_t(k) + j]});
    return out;
}

inline Postings Postings::merge(const Predictor& predictor, const std::vector<Postings>& segments, bool ordered, size_t n_terms, bool positions) {
    std::vector<vpt_postings_segment> segs(segments.size());
    std::vector<vpt_postings_positional_segment> psegs(positions ? segments.size() : 0);
    size_t cap = 0, cap_pos = 0;
    Postings out;
    for (size_t k = 0; k < segments.size(); ++k) {
        const Postings& s = segments[k];
        if (s.term_offsets.empty() || s.docs.size() != s.tfs.size())
            throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: merge: a segment's arrays do not belong together");
        segs[k] = vpt_postings_segment{s.term_offsets.data(), s.docs.data(), s.tfs.data(), uint32_t(s.n_terms()), uint64_t(s.docs.size())};
        if (positions) {
            if (s.first.empty())
                throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: merge: a segment was made without positions");
            if (s.first.size() != s.docs.size() + 1)
                throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: merge: a segment's arrays do not belong together");
            psegs[k] = vpt_postings_positional_segment{s.term_offsets.data(), s.docs.data(), s.tfs.data(), s.first.data(), s.positions.data(),
                                                       uint32_t(s.n_terms()), uint64_t(s.docs.size()), uint64_t(s.positions.size())};
            cap_pos += s.positions.size();
        }
        n_terms = std::max(n_terms, s.n_terms());
        cap += s.docs.size();
        out.n_dropped += s.n_dropped;
    }
    out.term_offsets.assign(n_terms + 1, 0);
    out.docs.resize(cap + 1);
    out.tfs.resize(cap + 1);
    uint64_t n_postings = 0;
    const unsigned flags = ordered ? unsigned(VPT_POSTINGS_MERGE_ORDERED) : 0u;
    if (positions) {
        uint64_t n_positions = 0;
        out.first.resize(cap + 1);
        out.positions.resize(cap_pos + 1);
        detail::check(vpt_postings_merge_positional(predictor.raw(), psegs.data(), psegs.size(), uint32_t(n_terms), flags, out.term_offsets.data(),
                                                    out.docs.data(), out.tfs.data(), out.first.data(), cap, out.positions.data(), cap_pos, &n_postings,
                                                    &out.n_combined, &n_positions));
        out.first.resize(size_t(n_postings) + 1);
        out.positions.resize(size_t(n_positions));
    } else {
        detail::check(vpt_postings_merge(predictor.raw(), segs.data(), segs.size(), uint32_t(n_terms), flags, out.term_offsets.data(), out.docs.data(),
                                         out.tfs.data(), cap, &n_postings, &out.n_combined));
    }
    out.docs.resize(size_t(n_postings));
    out.tfs.resize(size_t(n_postings));
    return out;
}

inline std::vector<std::string> Predictor::tokenize(const std::vector<std::string>& lines, bool tagged, unsigned flags, const PatternMatchTagger* tagger) const {
    std::vector<std::string> out;
    if (lines.empty()) return out;
    std::string text;
    std::vector<uint64_t> boff(1, 0);
    for (const std::string& l : lines) { text += l; boff.push_back(text.size()); }
    uint32_t sfx = 0;
    if (tagged) detail::check(vpt_predictor_max_tag_suffix(raw_->raw, &sfx));
    if (tagged && tagger) sfx += tagger->max_tag_suffix();
    std::vector<uint8_t> buf(3 * text.size() + text.size() * sfx + 16);
    std::vector<uint64_t> toff(lines.size() + 1);
    if (tagger)
        detail::check(vpt_tokenize_batch_rules(raw_->raw, reinterpret_cast<const uint8_t*>(text.data()), boff.data(), lines.size(), flags, tagged ? 1 : 0,
                                               buf.data(), buf.size(), toff.data(), tagger->raw()));
    else
        detail::check(vpt_tokenize_batch(raw_->raw, reinterpret_cast<const uint8_t*>(text.data()), boff.data(), lines.size(), flags, tagged ? 1 : 0, buf.data(),
                                         buf.size(), toff.data()));
    for (size_t i = 0; i < lines.size(); ++i) out.emplace_back(buf.begin() + toff[i], buf.begin() + toff[i + 1]);
    return out;
}

// vaporetto_tantivy's VaporettoTokenizer (vaporetto_tantivy/src/lib.rs:62-229) for callers that are not Rust: KyteaFullwidthFilter always,
// Predictor::new(model, false), SplitLinebreaksFilter first, then one filter per char of `wsconst` -- D R H T K O: KyteaWsConstFilter of that type,
// G: ConcatGraphemeClustersFilter; anything else throws "Could not parse a wsconst value" (lib.rs:69-86).  A Token is tantivy's as
// VaporettoTokenStream fills it (lib.rs:204-219): byte offsets into the caller's text.  A batch is ONE call (vpt_token_stream_batch: the text
// goes to the device, the spans come back), G included: VPT_FLAG_CONCAT_GRAPHEMES runs last on the device, which is the adapter's result for any
// place of G in the string.
// Beyond the adapter (which predicts no tags): with predict_tags a Token carries `tags`, one entry per slot (nullopt: None) -- the tag models'
// and, behind them, the rules' of `rules` (PatternMatchTagger) --, and the tokens of `stop_tags` ((slot, tag string) pairs, TagStopFilter) are
// dropped: a kept token's `position` is then its index BEFORE filtering and `position_length` the count before filtering (what position
// increments need).  ONE call per batch (vpt_token_stream_tagged_batch); under a stop filter a second, untagged one (vpt_token_stream_batch:
// scoring and spans again, no tags) gives the counts before filtering.  Without predict_tags the class is the adapter's, token for token.
struct Token {
    std::string text;
    size_t offset_from, offset_to, position, position_length;
    std::vector<std::optional<std::string>> tags;
};
class VaporettoTokenizer {
public:
    VaporettoTokenizer(const Model& model, const std::string& wsconst, int device_id = 0, bool predict_tags = false,
                       const PatternMatchTagger::Rules& rules = {}, const TagStopFilter::Pairs& stop_tags = {})
        : predictor_(model, predict_tags, device_id), tagged_(predict_tags) {
        for (char c : wsconst) {
            const char* at = std::char_traits<char>::find("DRHTKO", 6, c);
            if (c == 'G') flags_ |= VPT_FLAG_CONCAT_GRAPHEMES;
            else if (at) flags_ |= VPT_FLAG_WSCONST(unsigned(at - "DRHTKO") + 1);
            else throw VaporettoError(VaporettoError::InvalidArgument, "Could not parse a wsconst value");
        }
        if (!predict_tags && (!rules.empty() || !stop_tags.empty()))
            throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: rules / stop_tags: need predict_tags = true");
        if (!rules.empty()) tagger_ = std::make_unique<PatternMatchTagger>(predictor_, rules);
        if (!stop_tags.empty()) stop_ = std::make_unique<TagStopFilter>(predictor_, stop_tags, tagger_.get());
    }
    const Predictor& predictor() const { return predictor_; }

    // token_stream for every document of a batch (lib.rs:160-192); an empty document has no tokens
    std::vector<std::vector<Token>> token_stream_batch(const std::vector<std::string>& texts) const {
        std::vector<std::vector<Token>> out(texts.size());
        std::string text;
        std::vector<uint64_t> boff(1, 0);
        std::vector<size_t> doc;   // the documents that have text
        for (size_t i = 0; i < texts.size(); ++i) {
            if (texts[i].empty()) continue;
            text += texts[i];
            boff.push_back(text.size());
            doc.push_back(i);
        }
        if (doc.empty()) return out;
        const uint8_t* utf8 = reinterpret_cast<const uint8_t*>(text.data());
        std::vector<uint64_t> toff(doc.size() + 1);
        std::vector<uint32_t> ends(text.size());
        if (tagged_) {
            uint32_t nt = 0;
            detail::check(vpt_predictor_n_tags(predictor_.raw(), &nt));
            std::vector<uint32_t> starts(text.size()), pos(text.size());
            std::vector<int32_t> tags(text.size() * size_t(nt) + 1);
            detail::check(vpt_token_stream_tagged_batch(predictor_.raw(), utf8, boff.data(), doc.size(), flags_, tagger_ ? tagger_->raw() : nullptr,
                                                        stop_ ? stop_->raw() : nullptr, toff.data(), starts.data(), ends.data(), pos.data(), tags.data(),
                                                        ends.size()));
            std::vector<uint64_t> full(toff);   // the documents' tokens before filtering
            if (stop_) {
                std::vector<uint32_t> all_ends(text.size());
                detail::check(vpt_token_stream_batch(predictor_.raw(), utf8, boff.data(), doc.size(), flags_, full.data(), all_ends.data(), all_ends.size()));
            }
            const std::vector<std::string> vocab = predictor_.tag_strings();
            for (size_t k = 0; k < doc.size(); ++k) {
                const std::string& t = texts[doc[k]];
                for (size_t j = size_t(toff[k]); j < size_t(toff[k + 1]); ++j) {
                    Token tok{t.substr(starts[j], ends[j] - starts[j]), starts[j], ends[j], pos[j], size_t(full[k + 1] - full[k]), {}};
                    for (uint32_t q = 0; q < nt; ++q) {
                        const int32_t v = tags[j * nt + q];
                        if (v >= 0) tok.tags.emplace_back(vocab.at(size_t(v)));
                        else if (v <= -2 && tagger_) tok.tags.emplace_back(tagger_->tag(uint32_t(-2 - v)));
                        else tok.tags.emplace_back(std::nullopt);
                    }
                    out[doc[k]].push_back(std::move(tok));
                }
            }
            return out;
        }
        detail::check(vpt_token_stream_batch(predictor_.raw(), utf8, boff.data(), doc.size(), flags_, toff.data(), ends.data(), ends.size()));
        for (size_t k = 0; k < doc.size(); ++k) {
            const std::string& t = texts[doc[k]];
            const size_t n = size_t(toff[k + 1] - toff[k]);
            size_t from = 0;
            for (size_t j = 0; j < n; ++j) {
                const size_t to = ends[size_t(toff[k]) + j];
                out[doc[k]].push_back(Token{t.substr(from, to - from), from, to, j, n, {}});
                from = to;
            }
        }
        return out;
    }
    std::vector<Token> token_stream(const std::string& text) const { return token_stream_batch({text})[0]; }

    // The stream's vocabulary ids and nothing else (vpt_token_stream_ids_batch; beyond the adapter): {token_offsets [n + 1], ids} -- document i
    // owns ids[token_offsets[i] .. token_offsets[i + 1]), the tokens this tokenizer streams (tags and stop set included), each the id of its
    // surface in `vocab` (made for predictor()) or vocab.unk_id().  normalize: the surface looked up is the KyteaFullwidthFilter image of the
    // token -- the text as it was scored --, else the caller's bytes.  No token string is built on the way.
    std::pair<std::vector<uint64_t>, std::vector<int32_t>> encode(const std::vector<std::string>& texts, const Vocabulary& vocab, bool normalize = true) const {
        std::string text;
        std::vector<uint64_t> boff(1, 0);
        for (const std::string& t : texts) { text += t; boff.push_back(text.size()); }
        std::vector<uint64_t> toff(texts.size() + 1, 0);
        const size_t cap = text.size() + 1;
        std::vector<uint32_t> starts(cap), ends(cap), pos(cap);
        std::vector<int32_t> ids(cap), tags;
        if (tagged_) {
            uint32_t nt = 0;
            detail::check(vpt_predictor_n_tags(predictor_.raw(), &nt));
            tags.resize(cap * size_t(nt) + 1);
        }
        detail::check(vpt_token_stream_ids_batch(predictor_.raw(), reinterpret_cast<const uint8_t*>(text.data()), boff.data(), texts.size(), flags_,
                                                 tagger_ ? tagger_->raw() : nullptr, stop_ ? stop_->raw() : nullptr, vocab.raw(),
                                                 normalize ? unsigned(VPT_FLAG_KYTEA_FULLWIDTH) : 0u, toff.data(), starts.data(), ends.data(), pos.data(),
                                                 tagged_ ? tags.data() : nullptr, ids.data(), cap));
        ids.resize(size_t(toff[texts.size()]));
        return {std::move(toff), std::move(ids)};
    }

    // Every token this tokenizer streams for `texts` (tagger and stop set included) into `counter` (made for predictor()), on the device
    // (vpt_token_stream_count_batch); normalize as in encode.  Nothing comes back.
    void count(const std::vector<std::string>& texts, VocabularyCounter& counter, bool normalize = true) const {
        std::string text;
        std::vector<uint64_t> boff(1, 0);
        for (const std::string& t : texts) { text += t; boff.push_back(text.size()); }
        detail::check(vpt_token_stream_count_batch(predictor_.raw(), reinterpret_cast<const uint8_t*>(text.data()), boff.data(), texts.size(), flags_,
                                                   tagger_ ? tagger_->raw() : nullptr, stop_ ? stop_->raw() : nullptr, counter.raw(),
                                                   normalize ? unsigned(VPT_FLAG_KYTEA_FULLWIDTH) : 0u));
    }

    // The postings of `texts` (a segment) over `vocab` (made for predictor()): term = vocabulary id, document = doc_base + the text's index,
    // empty texts included, tf = the term's tokens among those this tokenizer streams (vpt_token_stream_postings_batch); normalize as in encode.
    // positions: a positional segment (first, positions: the stream's token positions; vpt_token_stream_positional_postings_batch).
    Postings index(const std::vector<std::string>& texts, const Vocabulary& vocab, uint64_t doc_base = 0, bool normalize = true,
                   bool positions = false) const {
        std::string text;
        std::vector<uint64_t> boff(1, 0);
        for (const std::string& t : texts) { text += t; boff.push_back(text.size()); }
        Postings out;
        out.term_offsets.assign(vocab.size() + 1, 0);
        const size_t cap = text.size() + 1;   // (a token has a byte at least, a posting a token)
        out.docs.resize(cap);
        out.tfs.resize(cap);
        uint64_t n_postings = 0;
        if (positions) {
            uint64_t n_positions = 0;
            out.first.resize(cap + 1);
            out.positions.resize(cap);
            detail::check(vpt_token_stream_positional_postings_batch(
                predictor_.raw(), reinterpret_cast<const uint8_t*>(text.data()), boff.data(), texts.size(), flags_, tagger_ ? tagger_->raw() : nullptr,
                stop_ ? stop_->raw() : nullptr, vocab.raw(), normalize ? unsigned(VPT_FLAG_KYTEA_FULLWIDTH) : 0u, doc_base, out.term_offsets.data(),
                out.docs.data(), out.tfs.data(), out.first.data(), cap, out.positions.data(), cap, &n_postings, &out.n_dropped, &n_positions));
            out.first.resize(size_t(n_postings) + 1);
            out.positions.resize(size_t(n_positions));
        } else {
            detail::check(vpt_token_stream_postings_batch(predictor_.raw(), reinterpret_cast<const uint8_t*>(text.data()), boff.data(), texts.size(), flags_,
                                                          tagger_ ? tagger_->raw() : nullptr, stop_ ? stop_->raw() : nullptr, vocab.raw(),
                                                          normalize ? unsigned(VPT_FLAG_KYTEA_FULLWIDTH) : 0u, doc_base, out.term_offsets.data(),
                                                          out.docs.data(), out.tfs.data(), cap, &n_postings, &out.n_dropped));
        }
        out.docs.resize(size_t(n_postings));
        out.tfs.resize(size_t(n_postings));
        return out;
    }

    // The postings of a corpus given as batches of texts: every batch a segment (index above) with a running doc_base, the segments merged on
    // the device by the ordered route (Postings::merge).  Equal to index of the concatenation.  positions: positional segments, merged with
    // their position lists -- equal to index of the concatenation with positions; phrase_search runs on it.
    Postings index(const std::vector<std::vector<std::string>>& batches, const Vocabulary& vocab, uint64_t doc_base = 0, bool normalize = true,
                   bool positions = false) const {
        std::vector<Postings> segments;
        for (const std::vector<std::string>& texts : batches) {
            segments.push_back(index(texts, vocab, doc_base, normalize, positions));
            doc_base += texts.size();
        }
        if (segments.empty()) return index(std::vector<std::string>(), vocab, doc_base, normalize, positions);
        return Postings::merge(predictor_, segments, true, vocab.size(), positions);
    }

    // The lengths Postings::search takes: the tokens this tokenizer streams per text (those without a vocabulary entry included).
    std::vector<uint32_t> doc_lens(const std::vector<std::string>& texts, const Vocabulary& vocab, bool normalize = true) const {
        const auto enc = encode(texts, vocab, normalize);
        std::vector<uint32_t> out(texts.size());
        for (size_t i = 0; i < texts.size(); ++i) out[i] = uint32_t(enc.first[i + 1] - enc.first[i]);
        return out;
    }

    // BM25 top-k of query TEXTS over `postings` (of this tokenizer and `vocab`): the texts are tokenised and encoded as documents are, every
    // token a slot -- nothing is dropped, a token without a vocabulary entry scores nothing -- then Postings::search with the idf weights.
    Postings::SearchResult search(const Postings& postings, const Vocabulary& vocab, const std::vector<std::string>& texts,
                                  const std::vector<uint32_t>& doc_lens, uint64_t doc_base = 0, uint32_t k = 10, float k1 = 1.2f, float b = 0.75f,
                                  bool normalize = true) const {
        const auto enc = encode(texts, vocab, normalize);
        std::vector<std::vector<int32_t>> queries(texts.size());
        for (size_t i = 0; i < texts.size(); ++i) queries[i].assign(enc.second.begin() + enc.first[i], enc.second.begin() + enc.first[i + 1]);
        return postings.search(predictor_, queries, doc_lens, doc_base, k, k1, b);
    }

    // BM25 top-k of boolean query TEXTS over `postings`.  A text is split on ASCII spaces into clauses: one that starts with `+` is MUST, one
    // that starts with `-` is MUST_NOT, any other is SHOULD; the rest of the clause is tokenised and encoded as documents are, and every token
    // of it is a slot of the clause's occur; an empty clause adds nothing; then Postings::boolean_search with the idf weights.  phrases (what
    // tantivy's query parser does; `postings` indexed with positions): a clause of several tokens is ONE exact phrase -- a token without a
    // vocabulary entry makes it match nothing -- a clause of one token a term slot, a clause without a token adds nothing; then
    // Postings::clause_search with the phrase weights and `slop` for every phrase clause (a `~` in a text stays a character of its clause).
    Postings::SearchResult boolean_search(const Postings& postings, const Vocabulary& vocab, const std::vector<std::string>& texts,
                                          const std::vector<uint32_t>& doc_lens, uint64_t doc_base = 0, uint32_t k = 10, float k1 = 1.2f,
                                          float b = 0.75f, bool normalize = true, bool phrases = false, uint32_t slop = 0) const {
        std::vector<std::string> clauses;
        std::vector<std::pair<size_t, uint8_t>> owner;
        for (size_t i = 0; i < texts.size(); ++i) {
            const std::string& text = texts[i];
            for (size_t a = 0; a <= text.size();) {
                size_t e = text.find(' ', a);
                if (e == std::string::npos) e = text.size();
                uint8_t occur = VPT_OCCUR_SHOULD;
                if (a < e && (text[a] == '+' || text[a] == '-')) occur = text[a++] == '+' ? VPT_OCCUR_MUST : VPT_OCCUR_MUST_NOT;
                if (a < e) {
                    clauses.push_back(text.substr(a, e - a));
                    owner.emplace_back(i, occur);
                }
                a = e + 1;
            }
        }
        std::vector<std::vector<Postings::Clause>> queries(texts.size());
        if (!clauses.empty()) {
            const auto enc = encode(clauses, vocab, normalize);
            for (size_t c = 0; c < clauses.size(); ++c)
                for (uint64_t t = enc.first[c]; t < enc.first[c + 1]; ++t) queries[owner[c].first].push_back(Postings::Clause{enc.second[t], owner[c].second});
        }
        if (phrases) {
            std::vector<std::vector<Postings::PhraseClause>> cq(texts.size());
            if (!clauses.empty()) {
                const auto enc = encode(clauses, vocab, normalize);
                for (size_t c = 0; c < clauses.size(); ++c)
                    if (enc.first[c] < enc.first[c + 1])
                        cq[owner[c].first].push_back(Postings::PhraseClause{
                            std::vector<int32_t>(enc.second.begin() + enc.first[c], enc.second.begin() + enc.first[c + 1]), owner[c].second});
            }
            return postings.clause_search(predictor_, cq, doc_lens, doc_base, k, k1, b, nullptr, slop);
        }
        return postings.boolean_search(predictor_, queries, doc_lens, doc_base, k, k1, b);
    }

    // Exact-phrase BM25 top-k of query TEXTS over a positional `postings` (index with positions): each text is tokenised and encoded as
    // documents are and is ONE phrase -- a token without a vocabulary entry makes it match nothing -- then Postings::phrase_search (slop: its).
    Postings::PhraseResult phrase_search(const Postings& postings, const Vocabulary& vocab, const std::vector<std::string>& texts,
                                         const std::vector<uint32_t>& doc_lens, uint64_t doc_base = 0, uint32_t k = 10, float k1 = 1.2f,
                                         float b = 0.75f, bool normalize = true, uint32_t slop = 0) const {
        const auto enc = encode(texts, vocab, normalize);
        std::vector<std::vector<int32_t>> phrases(texts.size());
        for (size_t i = 0; i < texts.size(); ++i) phrases[i].assign(enc.second.begin() + enc.first[i], enc.second.begin() + enc.first[i + 1]);
        return postings.phrase_search(predictor_, phrases, doc_lens, doc_base, k, k1, b, nullptr, slop);
    }

private:
    Predictor predictor_;
    unsigned flags_ = 0;
    bool tagged_ = false;
    std::unique_ptr<PatternMatchTagger> tagger_;
    std::unique_ptr<TagStopFilter> stop_;
};

inline void Sentence::fill_tags(const PatternMatchTagger* tagger) {
    if (!predictor_) throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: sentence: predict() has not been called");
    const uint64_t boff[2] = {0, text_.size()}, ooff[2] = {0, len() - 1};
    uint32_t nt = 0, stride = 0;
    detail::check(vpt_predictor_n_tags(predictor_->raw, &nt));
    std::vector<int32_t> tags(len() * size_t(nt) + 1);
    tag_scores_.clear(); tag_models_.clear();
    if (tagger && predictor_->store_tag_scores)
        throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: tagger: not with store_tag_scores (rule tags have no scores)");
    if (tagger) {
        detail::check(vpt_fill_tags_batch_rules(predictor_->raw, reinterpret_cast<const uint8_t*>(text_.data()), boff, 1, ooff, boundaries_.data(), tags.data(),
                                                0u, tagger->raw()));
    } else if (predictor_->store_tag_scores && nt != 0) {   // predictor.rs:563-566
        detail::check(vpt_predictor_tag_score_stride(predictor_->raw, &stride));
        std::vector<int32_t> sc(len() * size_t(stride) + 1), md(len(), -1);
        detail::check(vpt_fill_tags_scores_batch(predictor_->raw, reinterpret_cast<const uint8_t*>(text_.data()), boff, 1, ooff, boundaries_.data(), 0u,
                                                 tags.data(), sc.data(), md.data()));
        sc.resize(len() * size_t(stride));
        tag_scores_ = std::move(sc); tag_models_ = std::move(md); score_stride_ = stride;
    } else {
        detail::check(vpt_fill_tags_batch(predictor_->raw, reinterpret_cast<const uint8_t*>(text_.data()), boff, 1, ooff, boundaries_.data(), tags.data()));
    }
    tags.resize(len() * size_t(nt));
    tags_ = std::move(tags);
    n_tags_ = nt;
}

inline std::string Sentence::write_tokenized_text(const PatternMatchTagger* tagger) const {
    // The writer is the device's (the same bytes Sentence::write_tokenized_text produces): with tags when fill_tags has been
    // called, which is when the reference's Sentence holds any.
    const uint64_t boff[2] = {0, text_.size()}, ooff[2] = {0, len() - 1};
    uint64_t toff[2] = {0, 0};
    const bool tagged = n_tags_ != 0 && predictor_ != nullptr;
    uint32_t sfx = 0;
    if (tagged) detail::check(vpt_predictor_max_tag_suffix(predictor_->raw, &sfx));
    if (tagged && tagger) sfx += tagger->max_tag_suffix();
    std::vector<uint8_t> buf(3 * text_.size() + text_.size() * sfx + 16);
    if (tagged && tagger) {
        detail::check(vpt_write_tagged_batch_rules(predictor_->raw, reinterpret_cast<const uint8_t*>(text_.data()), boff, 1, ooff, boundaries_.data(), 0u,
                                                   buf.data(), buf.size(), toff, tagger->raw()));
    } else if (tagged) {
        detail::check(vpt_write_tagged_batch(predictor_->raw, reinterpret_cast<const uint8_t*>(text_.data()), boff, 1, ooff, boundaries_.data(), 0u,
                                             buf.data(), buf.size(), toff));
    } else {
        if (!predictor_) throw VaporettoError(VaporettoError::InvalidArgument, "InvalidArgumentError: sentence: predict() has not been called");
        detail::check(vpt_write_tokenized_batch(predictor_->raw, reinterpret_cast<const uint8_t*>(text_.data()), boff, 1, ooff, boundaries_.data(),
                                                buf.data(), buf.size(), toff));
    }
    return std::string(buf.begin(), buf.begin() + toff[1]);
}

}  // namespace vaporetto_hip

#endif  // VAPORETTO_HIP_HPP
