// What the files of the C ABI share (capi.cpp: predictors and workspaces; capi_device.cpp: the device-resident entry points; capi_host.cpp:
// the host-buffer pipelines): the handles' structs, the knobs, and the small helpers -- those in an unnamed namespace, a copy per file.
#pragma once
#include "../../include/vaporetto_hip.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "host_chunks.hpp"
#include "kernels.hpp"
#include "model.hpp"
#include "pattern_tagger.hpp"
#include "scratch_carve.hpp"
#include "tables.hpp"
#include "tag_stop.hpp"
#include "tag_vocab.hpp"

extern thread_local std::string vpt_g_last_error;   // (capi.cpp) the calling thread's message: vpt_last_error

namespace {

vpt_status fail(vpt_status st, const std::string& msg) {
    vpt_g_last_error = msg;
    return st;
}

#define VPT_HIP(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(VPT_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr); \
    } while (0)
#define VPT_TRY(expr)                       \
    do {                                    \
        const vpt_status s_ = (expr);       \
        if (s_ != VPT_OK) return s_;        \
    } while (0)

// Experiment / test knobs from the environment (tools/README.md).  Read ONCE -- the table-level ones when a predictor is made
// (bind_predictor), together with the launch-level ones of the workspaces its host entry points make for themselves (a pooled
// workspace is created lazily, inside predict / fill_tags / tokenize, possibly from several host threads at once: it copies the
// predictor's snapshot); a workspace the CALLER makes (vpt_batch_create) reads the launch-level ones then -- never on the launch
// path: getenv is not thread-safe against setenv, and a drop-in library must not change behaviour under a running host.
struct PredictorKnobs {
    bool force_window_table = false;    // VPT_FORCE_WINDOW_TABLE: the 8^(2W) type table instead of the type rows
    int pipe_lanes = -1;                // VPT_PIPE_LANES (-1: the size rule)
    uint64_t chunk_chars = 0;           // VPT_CHUNK_CHARS (0: the size rule)
    uint64_t tokenize_chunk_bytes = uint64_t(256) << 20;   // VPT_TOKENIZE_CHUNK_BYTES (the tagged pipeline's default; the untagged one: a sixth of the batch, 2 .. 8 MB)
    bool tokenize_chunk_bytes_set = false;
    uint64_t eval_chunk_bytes = uint64_t(64) << 20;        // VPT_EVAL_CHUNK_BYTES: vpt_evaluate_batch's chunks of tokenized text (~22 device bytes per byte)
};
struct BatchKnobs {
    bool force_generic = false;         // VPT_FORCE_GENERIC
    int force_cut = 0;                  // VPT_FORCE_CUT_TILES: 1 = cut tiles for every batch, -1 = whole-sentence tiles whenever they fit (tests, A/B)
    uint32_t tile_flat = 0;             // VPT_TILE_FLAT: flat positions per tile (tests: cuts at many places; never above what fits)
    uint32_t debug_ablate = 0;          // VPT_DEBUG_ABLATE
    bool profile_phases = false;        // VPT_PROFILE_PHASES
    uint32_t emit_per_block = 0;        // VPT_EMIT_PER_BLOCK: sentences a workgroup of the writer takes (1..512; 0: from the mean sentence length) -- tests: runs of any size
    int text_policy = -1;               // VPT_TEXT_POLICY=plain|nt: how the specialised kernel loads the text, 0 / 1 (-1, unset: text_policy_for decides per launch)
};
PredictorKnobs read_predictor_knobs() {
    PredictorKnobs k;
    k.force_window_table = std::getenv("VPT_FORCE_WINDOW_TABLE") != nullptr;
    if (const char* v = std::getenv("VPT_PIPE_LANES")) k.pipe_lanes = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("VPT_CHUNK_CHARS")) { const long long n = std::atoll(v); if (n > 0) k.chunk_chars = uint64_t(n); }
    if (const char* v = std::getenv("VPT_TOKENIZE_CHUNK_BYTES")) { const long long n = std::atoll(v); if (n > 0) { k.tokenize_chunk_bytes = uint64_t(n); k.tokenize_chunk_bytes_set = true; } }
    if (const char* v = std::getenv("VPT_EVAL_CHUNK_BYTES")) { const long long n = std::atoll(v); if (n > 0) k.eval_chunk_bytes = uint64_t(n); }
    return k;
}
BatchKnobs read_batch_knobs() {
    BatchKnobs k;
    k.force_generic = std::getenv("VPT_FORCE_GENERIC") != nullptr;
    if (const char* v = std::getenv("VPT_FORCE_CUT_TILES")) k.force_cut = std::atoi(v);
    if (const char* v = std::getenv("VPT_TILE_FLAT")) k.tile_flat = uint32_t(std::max(0, std::atoi(v)));
    if (const char* v = std::getenv("VPT_EMIT_PER_BLOCK")) k.emit_per_block = uint32_t(std::min(512, std::max(0, std::atoi(v))));
    if (const char* v = std::getenv("VPT_DEBUG_ABLATE")) k.debug_ablate = uint32_t(std::atoi(v));
    k.profile_phases = std::getenv("VPT_PROFILE_PHASES") != nullptr;
    if (const char* v = std::getenv("VPT_TEXT_POLICY")) k.text_policy = std::strcmp(v, "nt") == 0 ? 1 : std::strcmp(v, "plain") == 0 ? 0 : -1;
    return k;
}

// How the specialised scoring kernel loads a launch's text (ScoreParams::text_nt): plain, or non-temporal -- around the vector L1, and marked
// in the L2 as the line to give up first.  What decides is how much the launch streams through the L2 and the Infinity Cache beside the table
// gathers that need them: its text and its outputs (4 bytes of score and 1 of label a boundary).  A launch that streams less than the caches
// hold gains nothing from sparing them and, scored again on the same buffers, finds its text still there; one that streams far more evicts
// table lines with text it reads once.  Measured on MI355X over 100 K .. 10 M sentences of 64 chars, configs[3]'s model and whole documents
// (profiles/text_policy_sweep.jsonl): the threshold lies between the largest batch on which plain was not slower (300 K
// sentences: 58 MB + 95 MB, plain 2.9 % faster) and the smallest on which `nt` won by more than the rounds' spread (1 M: 192 MB + 315 MB,
// `nt` 3.2 % faster) -- at the size of the Infinity Cache, 256 MiB.
constexpr uint64_t kTextNtMinStreamBytes = uint64_t(256) << 20;
inline uint64_t launch_output_bytes(uint64_t total_boundaries, bool want_scores, bool want_labels) {
    return total_boundaries * ((want_scores ? 4u : 0u) + (want_labels ? 1u : 0u));
}
inline uint32_t text_policy_for(uint64_t text_bytes, uint64_t output_bytes) { return text_bytes + output_bytes > kTextNtMinStreamBytes ? 1u : 0u; }

constexpr size_t kTimingRing = 256;     // timed launches remembered per vpt_batch
constexpr size_t kTablePadBytes = 256;  // probes read whole 16-byte chunks; keep the tail of every table readable

// Every table of a predictor lives in ONE device allocation (the arena), each in a section of its own, 256-byte aligned
// and followed by kTablePadBytes of zeros.  With the fixed-size description below (PredictorMeta) the arena IS the compiled
// predictor: it can be written out and read back (vpt_predictor_save / _load: the analogue of Predictor::serialize_to_vec /
// deserialize_from_slice_unchecked, predictor.rs:640-664, in a format of our own) and copied to another GPU device to
// device (vpt_predictor_clone_to_device) without compiling the model again.
enum Section : int {
    kSecCShort, kSecCUni, kSecCEdges, kSecCWdata,              // general char tables
    kSecTShort, kSecTUni, kSecTEdges, kSecTWdata,              // general type tables (type_kind == pattern tables)
    kSecPUni, kSecPBi, kSecPTri, kSecPDeep, kSecPXrows, kSecPTrow, kSecPCpid, kSecPXcid,   // packed tables: contiguous, addressed from kSecPUni
    kSecTypeTable, kSecCtype, kSecCinfo, kSecCid,
    kSecTagTokTab, kSecTagModels, kSecTagMfilt, kSecTagNgrams, kSecTagNrec, kSecTagSyms, kSecTagSlots, kSecTagWeights, kSecTagSlotStr, kSecTagStrOff, kSecTagStrBytes,
    kSectionCount
};
struct TableGeom {
    uint32_t present, short_bits, edge_bits, stride_dw, uni_dw, uni_n, ext_slot, has_long;
    int32_t window, lo[3], len[3];
};
constexpr char kCompiledMagic[16] = "VaporettoHIP-C\x01";   // 15 chars + NUL
constexpr uint32_t kCompiledVersion = 12;                    // bump whenever layout.h or a kernel's reading of it changes
struct PredictorMeta {                                      // plain data: written and read as is (little-endian hosts)
    char magic[16];
    uint32_t version, meta_bytes;
    uint64_t arena_bytes, checksum;                         // checksum: of the arena's bytes (0 in a description: vpt_predictor_describe)
    uint64_t meta_checksum;                                 // of this block with both checksum fields zero
    uint64_t sec_off[kSectionCount], sec_bytes[kSectionCount];
    int32_t bias, pad, type_kind, type_window, chunks;
    uint32_t predict_tags, has_tags, n_tags, tok_bits, max_tag_suffix, tag_use_char, tag_use_type, n_tag_models, n_tag_strings, max_tag_scores;
    TableGeom geom[2];                                      // chars, types
    uint32_t pk_present, pk_n_uni, pk_n_tri, pk_bi_shift, pk_wl, pk_trow_mode, pk_trow_levels, pk_xcid_bits;
    vpt_model_info info;
};

uint64_t arena_checksum(const unsigned char* p, size_t n) {   // n is a multiple of 256
    const uint64_t* w = reinterpret_cast<const uint64_t*>(p);
    uint64_t a = 0x9E3779B97F4A7C15ull, b = 0xC2B2AE3D27D4EB4Full, c = 0x165667B19E3779F9ull, d = 0x27D4EB2F165667C5ull;
    for (size_t i = 0; i + 4 <= n / 8; i += 4) {   // four independent lanes: memory-bound, not multiply-bound
        a = (a ^ w[i]) * 0x100000001B3ull; b = (b ^ w[i + 1]) * 0x100000001B3ull;
        c = (c ^ w[i + 2]) * 0x100000001B3ull; d = (d ^ w[i + 3]) * 0x100000001B3ull;
    }
    return a ^ (b << 1 | b >> 63) ^ (c << 2 | c >> 62) ^ (d << 3 | d >> 61) ^ uint64_t(n);
}

// Field by field: hashing the struct's raw bytes would take in its padding (vpt_model_info has 4 bytes of it in front of
// device_table_bytes and 4 at its tail), which only a memcpy of the whole block preserves.  The two checksum fields are left out.
struct MetaHash {
    uint64_t h = 0xCBF29CE484222325ull;
    template <typename T>
    void add(const T& v) {
        static_assert(std::is_arithmetic<T>::value, "scalars only: no padding inside");
        const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
        for (size_t i = 0; i < sizeof(T); ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    }
    template <typename T, size_t N>
    void add(const T (&a)[N]) { for (const T& v : a) add(v); }
};
uint64_t meta_checksum_of(const PredictorMeta& m) {
    MetaHash f;
    f.add(m.magic); f.add(m.version); f.add(m.meta_bytes); f.add(m.arena_bytes);
    f.add(m.sec_off); f.add(m.sec_bytes);
    f.add(m.bias); f.add(m.pad); f.add(m.type_kind); f.add(m.type_window); f.add(m.chunks);
    f.add(m.predict_tags); f.add(m.has_tags); f.add(m.n_tags); f.add(m.tok_bits); f.add(m.max_tag_suffix); f.add(m.tag_use_char); f.add(m.tag_use_type);
    f.add(m.n_tag_models); f.add(m.n_tag_strings); f.add(m.max_tag_scores);
    for (const TableGeom& g : m.geom) {
        f.add(g.present); f.add(g.short_bits); f.add(g.edge_bits); f.add(g.stride_dw); f.add(g.uni_dw); f.add(g.uni_n); f.add(g.ext_slot); f.add(g.has_long);
        f.add(g.window); f.add(g.lo); f.add(g.len);
    }
    f.add(m.pk_present); f.add(m.pk_n_uni); f.add(m.pk_n_tri); f.add(m.pk_bi_shift); f.add(m.pk_wl); f.add(m.pk_trow_mode); f.add(m.pk_trow_levels); f.add(m.pk_xcid_bits);
    const vpt_model_info& i = m.info;
    f.add(i.n_char_ngrams); f.add(i.n_type_ngrams); f.add(i.n_dict_words); f.add(i.n_tag_models); f.add(i.bias); f.add(i.char_window); f.add(i.type_window);
    f.add(i.max_pattern_chars); f.add(i.n_short_entries); f.add(i.n_long_nodes); f.add(i.type_kind); f.add(i.device_table_bytes); f.add(i.hot_table_bytes);
    f.add(i.packed); f.add(i.n_displaced); f.add(i.type_rows); f.add(i.n_overflow_children); f.add(i.predict_tags);
    return f.h ^ 0x5A17EDull;
}
// (a field added to PredictorMeta / TableGeom / vpt_model_info must be added above: these sizes are the reminder)
static_assert(sizeof(TableGeom) == 60 && sizeof(vpt_model_info) == 88, "meta_checksum_of lists every field");

// What the kernels assume of the scalars and section sizes of a compiled predictor that did not come from compile_model in
// this process (vpt_predictor_load, vpt_predictor_adopt_device): a flipped bit in the description must not become an
// out-of-bounds device read or a silently different score.  The arena's CONTENT is covered by its own checksum.
const char* validate_meta(const PredictorMeta& m) {
    auto sz = [&](int sec) { return m.sec_bytes[sec]; };
    if (m.pad < 1 || m.pad > vpt::kMaxWindow || m.chunks < 1 || m.chunks > 16) return "pad / chunks";
    if (m.type_kind < 0 || m.type_kind > 2 || m.type_window < 0 || m.type_window > vpt::kMaxWindow) return "type scorer";
    if (sz(kSecCtype) != 65536 || sz(kSecCinfo) != 2ull * 65536 * 4) return "char class tables";
    if (sz(kSecCid) != (m.pk_present ? 2ull * 65536 * 4 : 0ull)) return "char id table";
    if (m.type_kind == vpt::kTypeWindowTable && (m.type_window > 3 || sz(kSecTypeTable) < (4ull << (6 * m.type_window)))) return "type window table";
    for (int t = 0; t < 2; ++t) {
        const TableGeom& g = m.geom[t];
        if (!g.present) continue;
        const int first = t == 0 ? kSecCShort : kSecTShort;
        if (g.short_bits < 2 || g.short_bits > 30 || g.edge_bits < 3 || g.edge_bits > 30) return "table geometry (bits)";
        if (g.stride_dw < 4 || g.stride_dw > 64 || g.stride_dw % 4 || g.uni_dw < 4 || g.uni_dw > 64 || g.uni_dw % 4) return "table geometry (strides)";
        if (g.window < 0 || g.window > vpt::kMaxWindow || g.ext_slot + 2 > g.stride_dw) return "table geometry (window)";
        if (g.uni_n > (t == 0 ? vpt::kUniDirectChars : vpt::kUniDirectTypes)) return "table geometry (direct rows)";
        for (int i = 0; i < 3; ++i)
            if (g.len[i] < 0 || g.len[i] > 2 * vpt::kMaxWindow + 2 || g.lo[i] > 0 || g.lo[i] < -vpt::kMaxWindow - 1 || uint32_t(g.len[i]) + 2 > g.stride_dw || uint32_t(g.len[i]) > g.uni_dw + (i ? 64u : 0u)) return "table geometry (rows)";
        if (sz(first) < (4ull << g.short_bits) * g.stride_dw || sz(first + 1) < 4ull * g.uni_n * g.uni_dw || sz(first + 2) < (16ull << g.edge_bits)) return "table geometry (sections)";
    }
    if (m.type_kind == vpt::kTypePatternTable && !m.geom[1].present) return "type pattern tables";
    if (m.pk_present) {
        if (m.pk_wl < 3 || m.pk_wl > uint32_t(vpt::kMaxWindow)) return "packed tables (row window)";
        const int wl = int(m.pk_wl);
        if (m.pk_n_uni < 2 || sz(kSecPUni) < 4ull * vpt::pk_uni_dw(wl) * m.pk_n_uni || sz(kSecPCpid) < 4ull * m.pk_n_uni || sz(kSecPTri) < 4ull * vpt::pk_tri_dw(wl) * m.pk_n_tri) return "packed tables";
        if (m.pk_bi_shift > 16 || sz(kSecPBi) < 4ull * vpt::pk_bi_dw(wl) || sz(kSecPDeep) < 64) return "packed tables (bigram level)";
        if (m.pk_trow_mode > vpt::kTypeRowsGlobal) return "type rows";
        if (m.pk_trow_mode == vpt::kTypeRowsLds && (m.pk_trow_levels != 3 || sz(kSecPTrow) < 4ull * vpt::pk_trow_dw(wl) * vpt::kTypeRowCount)) return "type rows";
        if (m.pk_trow_mode == vpt::kTypeRowsGlobal && (m.pk_trow_levels < 3 || m.pk_trow_levels > uint32_t(vpt::kMaxTypeRowLevels) ||
                                                      sz(kSecPTrow) < 4ull * vpt::pk_trow_global_dw(wl) * vpt::type_row_count(int(m.pk_trow_levels)))) return "type rows";
        if (m.pk_xcid_bits > 20 || sz(kSecPXcid) != (m.pk_xcid_bits ? 8ull + (8ull << m.pk_xcid_bits) : 0ull)) return "packed tables (chars outside the BMP)";
        if (m.sec_off[kSecPXcid] + sz(kSecPXcid) - m.sec_off[kSecPUni] >= (1ull << 32)) return "packed tables (32-bit offsets)";
    }
    if (m.has_tags) {
        if (m.n_tags == 0 || m.n_tags > 4096 || m.tok_bits < 2 || m.tok_bits > 30 || m.max_tag_scores > vpt::kTagMaxZ) return "tag tables";
        if (sz(kSecTagTokTab) < (16ull << m.tok_bits) || sz(kSecTagModels) < 48ull * m.n_tag_models || sz(kSecTagMfilt) < 4ull * vpt::kTagFiltStride * m.n_tag_models) return "tag tables (sections)";
        if (sz(kSecTagStrOff) < 4ull * (uint64_t(m.n_tag_strings) + 1)) return "tag strings";
    } else if (m.predict_tags > 1) return "predict_tags";
    return nullptr;
}

TableGeom geom_of(const vpt::HostPatternTable& h) {
    TableGeom g{};
    g.present = h.present ? 1u : 0u;
    if (!h.present) return g;
    g.short_bits = h.short_bits; g.edge_bits = h.edge_bits; g.stride_dw = h.stride_dw; g.uni_dw = h.uni_dw; g.uni_n = h.uni_n;
    g.ext_slot = h.ext_slot; g.has_long = h.has_long ? 1u : 0u; g.window = h.window;
    for (int i = 0; i < 3; ++i) { g.lo[i] = h.lo[i]; g.len[i] = h.len[i]; }
    return g;
}

void fill_info(const vpt::CompiledModel& c, vpt_model_info* info) {
    std::memset(info, 0, sizeof(*info));
    info->n_char_ngrams = c.n_char_ngrams; info->n_type_ngrams = c.n_type_ngrams;
    info->n_dict_words = c.n_dict_words; info->n_tag_models = c.n_tag_models;
    info->bias = c.bias;
    info->char_window = c.chars.present ? uint32_t(c.char_window) : 0;
    info->type_window = uint32_t(c.type_window);
    info->max_pattern_chars = c.chars.max_pattern;
    info->n_short_entries = c.chars.n_short; info->n_long_nodes = c.chars.n_long_nodes;
    info->type_kind = uint32_t(c.type_kind);
    info->packed = c.packed.present ? 1u : 0u;
    info->n_displaced = c.packed.present ? 0u : c.chars.n_displaced_short;
    info->type_rows = c.packed.present ? c.packed.trow_mode : 0u;
    info->n_overflow_children = 0u;
    // the specialised kernel reads only the packed tables; the general ones stay resident for oversized sentences
    info->device_table_bytes = (c.chars.present ? c.chars.bytes() : 0) + (c.types.present ? c.types.bytes() : 0) +
                               4ull * c.type_table.size() + (c.packed.present ? c.packed.bytes() : 0);
    info->hot_table_bytes = c.packed.present ? c.packed.bytes() + (c.packed.trow_mode == vpt::kTypeRowsNone ? 4ull * c.type_table.size() : 0) : info->device_table_bytes;
}

}  // namespace

// PatternMatchTagger's rule table on the predictor's device (pattern_tagger.hpp; kernels_pattern.hip): immutable, shared by any number of workspaces
// of ITS predictor.  One allocation; `arena` = the predictor's tag strings followed by the rules' (escaped), so that the writer copies either kind
// from one base: a record's strings are {start, length} in it (the predictor's keep their places at its front).
struct vpt_pattern_tagger {
    const vpt_predictor* pred = nullptr;
    int device = 0;
    unsigned char* mem = nullptr;
    const uint4* slots = nullptr; const uint32_t* surf = nullptr; const int32_t* rule_tags = nullptr; const uint2* id_str = nullptr;
    const uint8_t* arena = nullptr;
    uint32_t bits = 4, max_len = 0, n_tags = 0, n_ids = 0, max_suffix = 0, n_keys = 0;
    std::vector<uint32_t> raw_off;     // vpt_pattern_tagger_tag: the tags as the caller gave them
    std::vector<uint8_t> raw_bytes;
};

// A tag stop set on the predictor's device (tag_stop.hpp; kernels_token_filter.hip): one bitmap per slot over the predictor's vocabulary ids and,
// when it was made with a tagger, one over the tagger's ids.  Immutable, tied to its predictor, shared by workspaces and host threads.
struct vpt_tag_stop {
    const vpt_predictor* pred = nullptr;
    const vpt_pattern_tagger* tagger = nullptr;
    int device = 0;
    unsigned char* mem = nullptr;
    const uint32_t *model_bits = nullptr, *rule_bits = nullptr;
    uint32_t model_words = 0, rule_words = 0, n_vocab = 0, n_rule = 0;
};

// A vocabulary on the predictor's device (vocab_table.hpp; kernels_vocab.hip): the hashed surface table and the surfaces' code points in one
// allocation; the surfaces' bytes stay on the host (vpt_vocab_surface).  Immutable, tied to its predictor's device, shared by workspaces and host threads.
struct vpt_vocab {
    const vpt_predictor* pred = nullptr;
    int device = 0;
    unsigned char* mem = nullptr;
    const uint4* slots = nullptr; const uint32_t* surf = nullptr;
    uint32_t bits = 1, max_len = 0, n_keys = 0;
    int32_t unk_id = -1;
    std::vector<uint64_t> off;         // [n_keys + 1]
    std::vector<uint8_t> bytes;
};

// A vocabulary counter on the predictor's device (vocab_count.hpp; kernels_vocab_count.hip): control words, slots, counts, key records, the
// arena and finish's output in ONE allocation.  MUTABLE, unlike a vocabulary: one call on it at a time, in stream order.  What the last finish
// handed out lives here until the next finish, reset or destroy.
struct vpt_vocab_counter {
    const vpt_predictor* pred = nullptr;
    int device = 0;
    unsigned char* mem = nullptr;
    size_t state_bytes = 0;            // control words, slots and counts: what reset clears
    vpt::VocabCounterView view{};
    hipStream_t last_stream = nullptr; // of the last count call that may still be running
    bool in_flight = false;
    bool known_full = false;           // the host has seen the full word (info / finish): count calls refuse at once
    std::vector<uint8_t> surfaces;
    std::vector<uint64_t> offsets, counts;
};
constexpr const char* kVocabCounterFull = "InvalidArgumentError: vocab counter: full (max_keys / arena_chars)";
constexpr const char* kPostingsTooSmall = "InvalidArgumentError: capacity: smaller than the number of postings";
constexpr const char* kCandidatesTooSmall = "InvalidArgumentError: capacity_candidates: smaller than the number of candidates";
constexpr const char* kProbesTooSmall = "InvalidArgumentError: capacity_probes: smaller than the number of probes";
constexpr const char* kListsTooSmall = "InvalidArgumentError: capacity_lists: smaller than the number of list entries";
constexpr const char* kPositionsTooSmall = "InvalidArgumentError: capacity_positions: smaller than the number of indexed tokens";

// A device allocation that a workspace owns: freed with it.  cap: elements (grow) -- the allocation has 64 bytes more -- or bytes / sizeof(T) (alloc).
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)hipFree(p); }
    operator T*() const { return p; }
    void release() { (void)hipFree(p); p = nullptr; cap = 0; }
    vpt_status alloc(size_t bytes) {   // exactly `bytes`; the contents are gone
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes);
        if (e != hipSuccess) { vpt_g_last_error = std::string("HIP error: ") + hipGetErrorString(e) + " at hipMalloc"; return VPT_RUNTIME_ERROR; }
        cap = bytes / sizeof(T);
        return VPT_OK;
    }
    vpt_status grow(size_t need) {     // room for `need` elements: by half as much again at least; the contents are gone
        if (need <= cap && p) return VPT_OK;
        const size_t ncap = std::max<size_t>(std::max<size_t>(need, cap + cap / 2), 64);
        const vpt_status st = alloc(ncap * sizeof(T) + 64);
        if (st == VPT_OK) cap = ncap;
        return st;
    }
};
// Two buffers indexed alike (grown by the same needs, they have the same capacity); each knows its own, so a failure between the two leaves
// nothing behind that a later call could overrun.
template <typename A, typename B>
vpt_status grow_pair(DevBuf<A>& a, DevBuf<B>& b, size_t need) {
    const vpt_status st = a.grow(need);
    return st != VPT_OK ? st : b.grow(need);
}

struct vpt_batch {
    const vpt_predictor* pred = nullptr;
    int device = 0;
    BatchKnobs knobs;                  // read once, when the workspace was made
    // per-call device tables
    DevBuf<uint32_t> d_tile_first, d_slow_list;   // (one capacity: grow_pair)
    DevBuf<vpt::TileDesc> d_tiles;     // the specialised kernel's tiles
    DevBuf<uint32_t> d_cut_local;      // ... and, for cut tiles, the lead-byte index of the text
    DevBuf<uint64_t> d_cut_super;
    DevBuf<uint32_t> d_ctrl;           // [0] status bits, [1] slow tile count
    DevBuf<uint64_t> d_prof;           // 8 per-phase cycle counters + 8 node-read counters (only with VPT_PROFILE_PHASES set)
    DevBuf<unsigned char> d_scratch;
    DevBuf<uint32_t> d_cps;            // decoded scalar values for vpt_fill_tags_batch_device
    // the batch whose chars d_cps holds because the scoring kernel of a predict call on this workspace wrote them (all 0: none)
    const void* cps_text = nullptr; const void* cps_ooff = nullptr; size_t cps_sentences = 0; uint64_t cps_boundaries = 0; unsigned cps_flags = 0;
    uint64_t max_chars = 0;            // caller's bound on chars per sentence (0 = unknown)
    unsigned flags = 0;                // VPT_FLAG_*
    // (vpt_tokenize_batch) the scoring launch of the next predict call goes on split_stream, behind split_event recorded after the tile search:
    // the caller's next chunk can then have its chars counted and its tiles found (other workspace, the call's stream) while this one is scored
    hipStream_t split_stream = nullptr; hipEvent_t split_event = nullptr;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;        // ring of (start, stop) pairs around the scoring kernel
    size_t ev_calls = 0;               // timed calls since the last vpt_batch_kernel_ms
    uint32_t last_tiles = 0, last_tile_flat = 0, last_plan = 0;   // last_plan: 0 general kernels, 1 whole-sentence tiles, 2 cut tiles
    uint32_t last_text_policy = 0;     // the text's cache policy in the last scoring launch: 0 plain (the general kernels: always), 1 non-temporal
    hipStream_t last_stream = nullptr; bool pending = false;
    // staging for the host-buffer entry points
    hipStream_t own_stream = nullptr;
    DevBuf<uint8_t> d_text;
    DevBuf<uint64_t> d_boff, d_ooff;                                // (one capacity: grow_pair)
    DevBuf<int32_t> d_scores; DevBuf<uint8_t> d_labels;             // (one capacity: grow_pair)
    DevBuf<int32_t> d_tags;                                         // vpt_fill_tags_batch
    DevBuf<int32_t> d_tag_scores, d_tag_models;                     // vpt_fill_tags_scores_batch
    DevBuf<uint8_t> d_tok;                                          // vpt_write_tokenized_batch
    DevBuf<uint8_t> d_tlab;                                         // vpt_tokenize_batch: the labels of the whole batch (no scores are kept)
    DevBuf<uint64_t> d_toff;
    DevBuf<uint32_t> d_tends;                                       // vpt_token_spans_batch / vpt_token_stream_batch: the tokens' end-points
    // vpt_token_stream_tagged_batch: the unfiltered tags beside d_tends, the filter's five arrays, and its counts + scan state (vpt_token_filter_batch_device)
    DevBuf<int32_t> d_ttags, d_ftags;
    DevBuf<uint32_t> d_fstarts, d_fends, d_fpos;
    DevBuf<uint64_t> d_ftoff, d_filt;
    DevBuf<int32_t> d_fids;                                         // vpt_token_stream_ids_batch: the ids beside the filter's arrays
    DevBuf<uint4> d_vrec;                                           // vpt_vocab_count_batch_device: two words per token (VocabCountParams::rec)
    DevBuf<unsigned char> d_post;                                   // (the layouts: scratch_carve.hpp) vpt_postings_batch_device: keys, documents, index arrays, flags, scan, histograms (PostingsParams); vpt_postings_merge_device: PostingsMergeParams; vpt_postings_merge_positional_device: PostingsMergePosParams (32 bytes more a segment; ordered a second table, general 16 bytes more a place); vpt_postings_search_device: PostingsSearchParams; vpt_postings_phrase_search_device: PostingsPhraseParams (36 bytes a query, 48 bytes a probe place, the histograms)
    DevBuf<uint64_t> d_chain;                                       // vpt_tokenize_batch: where a chunk's tokenized text starts (EmitOut::chain_in / chain_out)
    // what the last fill_tags on this workspace left (TagParams, kernels.hpp): a record per token that has a tag model, sorted by position
    DevBuf<uint4> d_tag_records;
    DevBuf<int32_t> d_rec_tags;
    DevBuf<uint64_t> d_tag_ctl;                                     // the scan's state, run_pref [n_runs + 1]: zeroed as one range per call
    DevBuf<uint2> d_rec_str;
    DevBuf<uint4> d_tag_cands;
    DevBuf<uint32_t> d_tag_summary;
    // What that call hands to the readers of its records (tag_records.h; tag_records_for).  own: fill_tags' (what evaluate takes: its CLI runs no
    // PatternMatchTagger); merged: the pattern tagger's merge when the workspace has one, else own again (the writer, expand_tags)
    struct TagHandOver {
        vpt::TagRecordsView own{}, merged{};
        uint64_t chars = 0, sentences = 0;                          // the batch they belong to (0 chars: none)
    } tag_out;
    // vpt_batch_set_pattern_tagger: the rules applied behind every fill_tags on this workspace (nullptr: none), and what they are merged into.
    const vpt_pattern_tagger* tagger = nullptr;
    DevBuf<uint4> d_pm_records;
    DevBuf<int32_t> d_pm_rec_tags;
    DevBuf<uint2> d_pm_rec_str, d_pm_hits;
    DevBuf<uint64_t> d_pm_ctl;
    std::vector<uint64_t> h_boff, h_ooff;                           // rebased offsets of the call in flight (copied asynchronously)
    DevBuf<uint8_t> d_types;                                        // vpt_char_types_batch
    DevBuf<uint64_t> d_scan_part;                                   // per-workgroup partials of the prefix sums (kernels_emit.hip)
    // the writer's state words (EmitFuse): two arrays of emit_state_cap words in one allocation, used in turn; a call zeroes what the call
    // before it left in the other one (emit_dirty = how many words that is)
    DevBuf<uint64_t> d_emit_state; size_t emit_state_cap = 0; size_t emit_dirty[2] = {0, 0}; int emit_flip = 0;
    // the pipelined host-buffer path (predict_pipelined): two sets of device buffers, copy streams, pinned offset staging
    struct PipeSet {
        DevBuf<uint8_t> text;
        DevBuf<uint64_t> off;                             // byte offsets, then boundary offsets: one copy
        DevBuf<int32_t> scores; DevBuf<uint8_t> labels;
        hipEvent_t ev_in = nullptr, ev_k = nullptr, ev_out = nullptr;   // chunk copied in / scored / copied out
    } pipe[2];   // (four sets, i.e. the host running further ahead, measured no faster at 2 M-char chunks and slower at 1 M: profiles/r02_c7_e2e.txt)
    // ONE copy stream per direction: a single hipMemcpyAsync stream moves 56 GB/s each way and 84 GB/s both ways at once on
    // this link; two streams per direction were slower (profiles/r02_c6_pcie_microbench.txt)
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipStream_t s_tok_in = nullptr, s_tok_out = nullptr;            // tokenize_chunked's copy streams, in and out
    uint64_t* h_off = nullptr; size_t h_off_cap = 0;                // pinned (pinned_words): the offsets and totals of every chunk of the call in flight
    // vpt_parse_tokenized_batch_device's per-line tag counts (ParseParams::tag_off / tb_off) and vpt_evaluate_batch's buffers (one allocation)
    DevBuf<uint64_t> d_parse_tmp;
    DevBuf<unsigned char> d_eval;
    std::vector<hipEvent_t> chunk_ev;                               // vpt_tokenize_batch: one per chunk in flight (chunk_events)
    // vpt_predict_listing_batch[_device]: the elements' sizes / positions and the scan's state (kernels_listing.hip); the host variant's output
    DevBuf<uint64_t> d_lst_pos;
    DevBuf<uint8_t> d_lst_out;
    DevBuf<uint64_t> d_lst_off;
    // VPT_FLAG_CONCAT_GRAPHEMES (kernels_graphemes.hip): the class bytes and, in one array, the tiles' summaries and first sentences
    DevBuf<uint8_t> d_gcls;
    DevBuf<uint32_t> d_gsum;
};

struct DeviceTags {   // views into the arena
    const uint32_t *tok_tab = nullptr, *models = nullptr, *mfilt = nullptr, *ngrams = nullptr, *nrec = nullptr, *syms = nullptr, *slots = nullptr, *slot_str = nullptr, *str_off = nullptr;
    const uint8_t* str_bytes = nullptr;
    const int32_t* weights = nullptr;
    uint32_t n_models = 0, n_strings = 0;
};

struct vpt_predictor {
    int device = 0;
    PredictorKnobs knobs;              // read once, when the predictor was made (bind_predictor)
    BatchKnobs pool_knobs;             // ... and what the workspaces of its pool are made with
    unsigned char* arena = nullptr;    // the one device allocation that holds every table
    PredictorMeta meta{};
    // what the launches use, bound from meta + arena (bind_predictor)
    bool predict_tags = false;
    bool has_tags = false;
    uint32_t n_tags = 0, tok_bits = 0, max_tag_suffix = 0, max_tag_scores = 0;
    bool tag_use_char = false, tag_use_type = false;
    DeviceTags dtag;
    vpt_model_info info{};
    int32_t bias = 0; int pad = 1; int type_kind = 0; int type_window = 0; int chunks = 2;
    uint32_t tile_slots = 0;           // workgroups of the scoring kernel the device runs at a time (0 = unknown)
    uint32_t n_cus = 0;                // compute units of the device (0 = unknown)
    vpt::PackedView pk{};
    const int32_t* d_type_table = nullptr;
    const uint8_t* d_ctype = nullptr;
    const uint32_t* d_cinfo = nullptr; // [0, 65536): plain; [65536, 131072): through KyteaFullwidthFilter
    const uint32_t* d_cid = nullptr;   // the same two tables for the specialised kernel: id | type << 16 | linebreak << 19
    vpt::PatternTableView ct{}, tt{};
    mutable std::mutex pool_mu;
    mutable std::vector<vpt_batch*> pool;  // idle workspaces for the host-buffer entry points
    mutable std::atomic<int64_t> max_tag_listing{-1};  // vpt_predictor_max_tag_listing: a constant of the tables, computed by the first call
    // The tag vocabulary (bind_predictor, from the tables the predictor holds; only with predict_tags and tag models): the distinct raw tag strings
    // in order of first appearance over tag models, slots, candidates -- vpt_predictor_tag_string -- and, on the device in one allocation of its
    // own, what token_spans_kernel<true> turns a record's candidate into an id with (SpanTags, kernels.hpp).
    vpt::TagVocab vocab;
    std::string vocab_error;           // why there is none although there should be one (a HIP error while it was made)
    unsigned char* vocab_mem = nullptr;
    const uint2* d_vocab_slot = nullptr;
    const uint32_t* d_vocab_ids = nullptr;
};

namespace {

// The argument checks that the postings calls repeat (capi_device.cpp, capi_host.cpp): one per concept, each with its one message.
inline vpt_status bad_argument(bool bad, const char* msg) { return bad ? fail(VPT_INVALID_ARGUMENT, msg) : VPT_OK; }
vpt_status check_batch(const vpt_predictor* p, const vpt_batch* b) {
    return bad_argument(!p || !b || b->pred != p, "InvalidArgumentError: batch: does not belong to this predictor");
}
vpt_status check_n_terms(uint32_t n_terms) {
    return bad_argument(n_terms == 0 || n_terms > vpt::kPostingsMaxTerms, "InvalidArgumentError: n_terms: must be between 1 and 2^24");
}
vpt_status check_n_queries(uint32_t n_queries) {
    return bad_argument(n_queries == 0 || n_queries > vpt::kSearchMaxQueries, "InvalidArgumentError: n_queries: must be between 1 and 2^24");
}
vpt_status check_top_k(uint32_t n_queries, uint32_t k) {
    return bad_argument(k == 0 || uint64_t(n_queries) * k >= (1ull << 32), "InvalidArgumentError: k: must be at least 1, and n_queries * k below 2^32");
}
vpt_status check_doc_range(uint64_t doc_base, uint64_t n_documents) {
    return bad_argument(doc_base > (1ull << 32) || n_documents > (1ull << 32) - doc_base,
                        "InvalidArgumentError: doc_base: doc_base + n_documents must not exceed 2^32");
}
vpt_status check_n_segments(size_t n_segments) {
    return bad_argument(n_segments == 0 || n_segments > vpt::kPostingsMergeMaxSegments, "InvalidArgumentError: n_segments: must be between 1 and 1024");
}
vpt_status check_pass_tokens(uint64_t capacity_in) {
    return bad_argument(capacity_in >= (1ull << 32), "InvalidArgumentError: capacity: the postings pass takes fewer than 2^32 tokens per call");
}
// a segment's places (positions) behind the `sum` of those in front of it
vpt_status check_merge_places(uint64_t sum, uint64_t n) {
    return bad_argument(n >= (1ull << 32) || sum + n >= (1ull << 32),
                        "InvalidArgumentError: capacity: the postings merge takes fewer than 2^32 input places per call");
}
vpt_status check_merge_positions(uint64_t sum, uint64_t n) {
    return bad_argument(n >= (1ull << 32) || sum + n >= (1ull << 32),
                        "InvalidArgumentError: capacity_positions: the postings merge takes fewer than 2^32 positions per call");
}
// segment s of a merge's `segments`, a plain one as a positional one without position arrays
vpt_postings_positional_segment merge_segment(const void* segments, bool positional, size_t s) {
    if (positional) return static_cast<const vpt_postings_positional_segment*>(segments)[s];
    const vpt_postings_segment& in = static_cast<const vpt_postings_segment*>(segments)[s];
    return vpt_postings_positional_segment{in.d_term_offsets, in.d_post_docs, in.d_post_tfs, nullptr, nullptr, in.n_terms, in.capacity, 0};
}
// two of a search's sizes (slots, postings, positions, candidates, places, probes); phrase: the phrase search's words
vpt_status check_search_sizes(bool phrase, uint64_t a, uint64_t b = 0) {
    return bad_argument(a >= (1ull << 32) || b >= (1ull << 32),
                        phrase ? "InvalidArgumentError: capacity: the phrase search takes fewer than 2^32 slots and probes per call"
                               : "InvalidArgumentError: capacity: the postings search takes fewer than 2^32 slots and candidates per call");
}
// the derived lists beside a segment's n_terms: a term value names a term or a list, and a list entry has a 32-bit place
vpt_status check_clause_lists(uint32_t n_terms, uint32_t n_lists, uint64_t capacity_lists) {
    VPT_TRY(bad_argument(n_lists > vpt::kPostingsMaxTerms || n_terms + uint64_t(n_lists) > vpt::kPostingsMaxTerms,
                         "InvalidArgumentError: n_lists: n_terms + n_lists must not exceed 2^24"));
    return bad_argument(capacity_lists >= (1ull << 32), "InvalidArgumentError: capacity_lists: must be below 2^32");
}

vpt_status compile(const uint8_t* bytes, size_t len, int predict_tags, vpt::CompiledModel* out) {
    if (!bytes) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: model_bytes: must not be NULL");
    try {
        vpt::ModelData m = vpt::parse_model(bytes, len, nullptr);
        *out = vpt::compile_model(m, predict_tags != 0);
    } catch (const vpt::ModelError& e) {
        return fail(VPT_INVALID_MODEL, e.what());
    } catch (const std::bad_alloc&) {
        return fail(VPT_RUNTIME_ERROR, "out of host memory while compiling the model");
    }
    return VPT_OK;
}

// (the device buffers free themselves: DevBuf)
void batch_release(vpt_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    for (auto& ps : b->pipe)
        for (hipEvent_t e : {ps.ev_in, ps.ev_k, ps.ev_out})
            if (e) (void)hipEventDestroy(e);
    if (b->h_off) (void)hipHostFree(b->h_off);
    for (hipEvent_t e : b->chunk_ev) (void)hipEventDestroy(e);
    for (hipStream_t s : {b->s_in, b->s_tok_in, b->s_tok_out, b->s_out})
        if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : b->ev) (void)hipEventDestroy(e);
    if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
    delete b;
}

vpt_status status_from_bits(uint32_t bits) {
    if (bits == 0) return VPT_OK;
    if (bits & vpt::kErrEmptySentence)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: text: must contain at least one character");
    if (bits & vpt::kErrNulChar) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: text: must not contain NULL");
    if (bits & vpt::kErrBadOffsets)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: out_offsets: do not match the text (or the text is not valid UTF-8)");
    if (bits & vpt::kErrUnknownLabel)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: labels: only NotWordBoundary (0) and WordBoundary (1) can be written as tokenized text");
    if (bits & vpt::kErrOutputTooSmall)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: text_capacity: smaller than the tokenized text");
    if (bits & vpt::kErrBadLabel)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: labels: not a CharacterBoundary (0, 1 or 2)");
    if (bits & vpt::kErrBadTokenCsr)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: token_offsets / token_starts / token_ends: do not describe the documents' tokens");
    if (bits & vpt::kErrVocabCounterFull) return fail(VPT_INVALID_ARGUMENT, kVocabCounterFull);
    if (bits & vpt::kErrBadQueryCsr)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: query_offsets: do not describe the queries' slots");
    if (bits & vpt::kErrBadSegment)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: segment: term_offsets or postings are not a segment's");
    if (bits & vpt::kErrBadWeights) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: weights: negative or not finite");
    if (bits & vpt::kErrQueryTooLong) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: query: more than 1024 slots");
    if (bits & vpt::kErrBadOccur) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: occurs: a value above 2");
    if (bits & vpt::kErrCandidatesTooSmall) return fail(VPT_INVALID_ARGUMENT, kCandidatesTooSmall);
    if (bits & vpt::kErrPhraseTooLong) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: query: a phrase of more than 64 terms");
    if (bits & vpt::kErrBadSlop) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: query: a slop above 31");
    if (bits & vpt::kErrProbesTooSmall) return fail(VPT_INVALID_ARGUMENT, kProbesTooSmall);
    if (bits & vpt::kErrListsTooSmall) return fail(VPT_INVALID_ARGUMENT, kListsTooSmall);
    if (bits & vpt::kErrBadPositions)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: positions: do not strictly ascend inside a document's list");
    if (bits & vpt::kErrSegmentsOverlap)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: segments: document ranges overlap or descend");
    if (bits & vpt::kErrTfOverflow) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: tf: sum exceeds 32 bits");
    if (bits & vpt::kErrPostingsTooSmall) return fail(VPT_INVALID_ARGUMENT, kPostingsTooSmall);
    if (bits & vpt::kErrPositionsTooSmall) return fail(VPT_INVALID_ARGUMENT, kPositionsTooSmall);
    return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: max_sentence_bytes / max_sentence_chars: smaller than the longest sentence");
}

// what a cutter of host_chunks.hpp refused, in the words the device has for the same finding
vpt_status cut_fail(vptcut::CutError e) {
    return status_from_bits(e == vptcut::CutError::kEmptySentence ? vpt::kErrEmptySentence : vpt::kErrBadOffsets);
}

// A line that parse_tokenized rejects (sentence.rs:285-400): the reference's message for the kParseErr* reason and the batch's line.
vpt_status parse_fail(uint32_t reason, uint64_t line) {
    static const char* const msg[7] = {"", "must contain at least one character", "must not start with a whitespace", "must not contain consecutive whitespaces", "must not end with a whitespace", "a slash must follow a character", "must not contain NULL"};
    return fail(VPT_INVALID_ARGUMENT, std::string("InvalidArgumentError: tokenized_text: ") + msg[reason] + " (line " + std::to_string(line) + ")");
}
// The device's verdict on tokenized text (kErrParse): the smallest failing line over the reason words (kernels.hpp); line_base: the first line of the call's batch.
vpt_status parse_status(const uint32_t* ctrl, uint64_t line_base) {
    uint32_t best = 0, reason = 0;
    for (uint32_t r = 1; r <= 6; ++r)
        if (ctrl[vpt::kParseErrWord + r] > best) { best = ctrl[vpt::kParseErrWord + r]; reason = r; }
    if (!reason) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: tokenized_text: rejected");
    return parse_fail(reason, line_base + (0xFFFFFFFFu - best));
}

// A line that parse_partial_annotation rejects (sentence.rs:516-631): the reference's message and the batch's line.  offender: the code point of
// kPartialErrChar (the message is a C string: a NUL offender ends it).
vpt_status partial_fail(uint32_t reason, const std::string& offender, uint64_t line) {
    static const char* const msg[5] = {"rejected", "must contain at least one character", "must not contain NULL",
                                       "contains an invalid boundary character: '", "invalid annotation"};
    std::string m = std::string("InvalidArgumentError: partial_annotation_text: ") + msg[reason <= 4 ? reason : 0];
    if (reason == vpt::kPartialErrChar) m += offender + "'";
    return fail(VPT_INVALID_ARGUMENT, m + " (line " + std::to_string(line) + ")");
}
// The device's verdict on partially annotated text (kErrParsePartial): the smallest failing line over the reason words, and for the
// invalid-boundary-character reason the offender's bytes (kernels.hpp).
vpt_status partial_status(const uint32_t* ctrl, uint64_t line_base) {
    uint32_t best = 0, reason = 0;
    for (uint32_t r = 1; r <= 4; ++r)
        if (ctrl[vpt::kPartialErrWord + r] > best) { best = ctrl[vpt::kPartialErrWord + r]; reason = r; }
    std::string offender;
    if (reason == vpt::kPartialErrChar) {
        const uint32_t w = ctrl[vpt::kPartialErrBytesWord];
        offender.push_back(char(w & 0xFFu));
        for (int k = 1; k < 4 && ((w >> (8 * k)) & 0xC0u) == 0x80u; ++k) offender.push_back(char((w >> (8 * k)) & 0xFFu));
    }
    return partial_fail(reason, offender, line_base + (0xFFFFFFFFu - best));
}

// An idle workspace of the predictor's pool for one host-buffer call (created, with a stream of its own, when the
// pool is empty); goes back to the pool when the guard dies.
// Every stream a host-buffer call may have used on this workspace has run dry.
void drain(vpt_batch* b) {
    (void)hipStreamSynchronize(b->own_stream);
    for (hipStream_t s : {b->s_in, b->s_tok_in, b->s_tok_out, b->s_out})
        if (s) (void)hipStreamSynchronize(s);
}
struct Workspace {
    const vpt_predictor* p = nullptr;
    vpt_batch* b = nullptr;
    ~Workspace() {
        if (!b) return;
        drain(b);              // an error return may leave copies from the caller's buffers in flight
        b->tagger = nullptr;   // (the *_rules pipelines bind one for their call)
        std::lock_guard<std::mutex> g(p->pool_mu);
        p->pool.push_back(b);
    }
};
vpt_status batch_create_with(const vpt_predictor* p, const BatchKnobs& knobs, vpt_batch** out) {
    *out = nullptr;
    VPT_HIP(hipSetDevice(p->device));
    vpt_batch* b = new (std::nothrow) vpt_batch();
    if (!b) return fail(VPT_RUNTIME_ERROR, "out of host memory");
    b->pred = p; b->device = p->device;
    b->knobs = knobs;
    hipError_t e = hipSuccess;
    vpt_status st = b->d_ctrl.alloc(64);
    if (st == VPT_OK) e = hipMemset(b->d_ctrl, 0, 64);
    if (st == VPT_OK && e == hipSuccess && b->knobs.profile_phases && (st = b->d_prof.alloc(128)) == VPT_OK) e = hipMemset(b->d_prof, 0, 128);
    if (e != hipSuccess) st = fail(VPT_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
    if (st != VPT_OK) { batch_release(b); return st; }
    *out = b;
    return VPT_OK;
}

vpt_status acquire(const vpt_predictor* p, Workspace* w) {
    w->p = p;
    {
        std::lock_guard<std::mutex> g(p->pool_mu);
        if (!p->pool.empty()) { w->b = p->pool.back(); p->pool.pop_back(); }
    }
    if (w->b) { w->b->cps_text = nullptr; return VPT_OK; }   // a pooled workspace remembers nothing of the call before
    vpt_batch* b = nullptr;
    vpt_status st = batch_create_with(p, p->pool_knobs, &b);   // (the knobs the predictor was made under: no getenv from a host thread's first call)
    if (st != VPT_OK) return st;
    if (hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking) != hipSuccess) {
        batch_release(b);
        return fail(VPT_RUNTIME_ERROR, "HIP error: cannot create a stream");
    }
    w->b = b;
    return VPT_OK;
}

// b->h_off holds `need` pinned words (by half as much again when it has to be made anew: its contents are then gone).
vpt_status pinned_words(vpt_batch* b, size_t need) {
    if (need <= b->h_off_cap) return VPT_OK;
    if (b->h_off) (void)hipHostFree(b->h_off);
    b->h_off = nullptr; b->h_off_cap = 0;
    VPT_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->h_off), (need + need / 2) * sizeof(uint64_t), hipHostMallocDefault));
    b->h_off_cap = need + need / 2;
    return VPT_OK;
}

// The caller's batch -> the workspace's staging buffers, on its stream: text, offsets rebased so that the device sees
// text and outputs starting at 0, and (when given) the labels.  `max_bytes` / `max_chars`: the longest sentence.
vpt_status stage(vpt_batch* b, const uint8_t* utf8, const uint64_t* byte_offsets, const uint64_t* out_offsets, size_t n_sentences,
                 const uint8_t* labels, uint64_t* total_b_out, uint64_t* max_bytes_out, uint64_t* max_chars_out) {
    b->cps_text = nullptr;   // d_text is about to be rewritten: whatever chars a predict call left decoded are another batch's
    const uint64_t t0 = byte_offsets[0], t1 = byte_offsets[n_sentences];
    if (t1 < t0) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: byte_offsets: must be non-decreasing");
    const size_t nbytes = size_t(t1 - t0);
    const uint64_t total_b = out_offsets[n_sentences] - out_offsets[0];
    uint64_t max_bytes = 0, max_chars = 0;
    for (size_t i = 0; i < n_sentences; ++i) {   // (checked before any buffer is sized from these numbers)
        uint64_t nb = 0, nc = 0;
        const vptcut::CutError bad = vptcut::check_sentence(byte_offsets, out_offsets, i, &nb, &nc);
        if (bad != vptcut::CutError::kNone) return cut_fail(bad);
        max_bytes = std::max(max_bytes, nb);
        max_chars = std::max(max_chars, nc);
    }
    vpt_status st;
    if ((st = b->d_text.grow(nbytes + 32)) != VPT_OK) return st;
    if ((st = grow_pair(b->d_boff, b->d_ooff, n_sentences + 1)) != VPT_OK) return st;
    if ((st = grow_pair(b->d_scores, b->d_labels, size_t(total_b) + 1)) != VPT_OK) return st;
    std::vector<uint64_t>&boff = b->h_boff, &ooff = b->h_ooff;   // they outlive the asynchronous copies: the call ends with a sync
    boff.resize(n_sentences + 1); ooff.resize(n_sentences + 1);
    for (size_t i = 0; i <= n_sentences; ++i) { boff[i] = byte_offsets[i] - t0; ooff[i] = out_offsets[i] - out_offsets[0]; }
    hipStream_t s = b->own_stream;
    VPT_HIP(hipMemcpyAsync(b->d_text, utf8 + t0, nbytes, hipMemcpyHostToDevice, s));
    VPT_HIP(hipMemcpyAsync(b->d_boff, boff.data(), 8 * (n_sentences + 1), hipMemcpyHostToDevice, s));
    VPT_HIP(hipMemcpyAsync(b->d_ooff, ooff.data(), 8 * (n_sentences + 1), hipMemcpyHostToDevice, s));
    if (labels && total_b) VPT_HIP(hipMemcpyAsync(b->d_labels, labels + out_offsets[0], size_t(total_b), hipMemcpyHostToDevice, s));
    *total_b_out = total_b;
    if (max_bytes_out) *max_bytes_out = max_bytes;
    if (max_chars_out) *max_chars_out = max_chars;
    return VPT_OK;
}

// The records the fill_tags call on this workspace left for THIS batch -- n_sentences and, where the caller knows them, total_boundaries
// (kBoundariesUnknown: any batch of that many sentences) -- merged with the pattern tagger's or fill_tags' own; an error when there are none.
constexpr uint64_t kBoundariesUnknown = ~uint64_t(0);
vpt_status tag_records_for(const vpt_batch* b, size_t n_sentences, uint64_t total_boundaries, bool merged, vpt::TagRecordsView* out) {
    const vpt_batch::TagHandOver& h = b->tag_out;
    if (h.sentences != n_sentences || (total_boundaries == kBoundariesUnknown ? h.chars == 0 : h.chars != total_boundaries + n_sentences))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: call vpt_fill_tags_batch_device on this workspace for this batch first");
    *out = merged ? h.merged : h.own;
    return VPT_OK;
}

}  // namespace

// the pieces of the device-resident path that the host pipelines drive as well (capi_device.cpp)
namespace vptc {
vpt_status emit_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                       const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries, const uint8_t* d_labels,
                       bool tagged, uint8_t* d_text_out, uint64_t text_capacity, uint64_t* d_text_offsets_out,
                       hipStream_t stream, uint64_t* total_out = nullptr, const uint64_t* chain_in = nullptr, uint64_t* chain_out = nullptr);
vpt_status spans_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                        const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries, const uint8_t* d_labels,
                        uint64_t* d_token_offsets, uint32_t* d_token_ends, uint64_t capacity, hipStream_t stream, uint64_t* total_out,
                        const uint64_t* chain_in, uint64_t* chain_out);
// ... with the tokens' tags (vpt_token_tags_batch_device), and the stop filter behind them (vpt_token_filter_batch_device; stop: or nullptr --
// every token is kept); total_out: an optional device-writable host word for the number of tokens written
vpt_status token_tags_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                             const uint64_t* d_out_offsets, size_t n_documents, uint64_t total_boundaries, const uint8_t* d_labels,
                             uint64_t* d_token_offsets, uint32_t* d_token_ends, int32_t* d_token_tags, uint64_t capacity, hipStream_t stream,
                             uint64_t* total_out);
vpt_status token_filter_device(const vpt_predictor* p, vpt_batch* b, const vpt_tag_stop* stop, const uint64_t* d_token_offsets,
                               const uint32_t* d_token_ends, const int32_t* d_token_tags, size_t n_documents, uint64_t capacity_in,
                               uint64_t* d_offsets_out, uint32_t* d_starts_out, uint32_t* d_ends_out, uint32_t* d_positions_out, int32_t* d_tags_out,
                               uint64_t capacity, hipStream_t stream, uint64_t* total_out, bool with_tags = true);
// The id pass over a finished CSR (vpt_token_ids_batch_device; kernels_vocab.hip)
vpt_status token_ids_device(const vpt_predictor* p, vpt_batch* b, const vpt_vocab* vocab, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                            size_t n_documents, const uint64_t* d_token_offsets, const uint32_t* d_token_starts, const uint32_t* d_token_ends,
                            uint64_t capacity_in, unsigned flags, int32_t* d_token_ids, hipStream_t stream);
// A count call over a finished CSR (vpt_vocab_count_batch_device; kernels_vocab_count.hip)
vpt_status vocab_count_device(const vpt_predictor* p, vpt_batch* b, vpt_vocab_counter* counter, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                              size_t n_documents, const uint64_t* d_token_offsets, const uint32_t* d_token_starts, const uint32_t* d_token_ends,
                              uint64_t capacity_in, unsigned flags, hipStream_t stream);
// The postings pass over a finished CSR's ids (vpt_postings_batch_device; kernels_postings.hip)
vpt_status postings_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_token_offsets, size_t n_documents, const int32_t* d_token_ids,
                           uint64_t capacity_in, uint32_t n_terms, uint64_t doc_base, uint64_t* d_term_offsets, uint32_t* d_post_docs, uint32_t* d_post_tfs,
                           uint64_t capacity_out, uint64_t* d_post_first, uint32_t* d_token_order, uint64_t* d_counts, hipStream_t stream);
// The merge of postings segments (vpt_postings_merge_device; kernels_postings_merge.hip)
vpt_status postings_merge_device(const vpt_predictor* p, vpt_batch* b, const vpt_postings_segment* segments, size_t n_segments, uint32_t n_terms_out,
                                 unsigned flags, uint64_t* d_term_offsets_out, uint32_t* d_post_docs_out, uint32_t* d_post_tfs_out, uint64_t capacity_out,
                                 uint64_t* d_counts, hipStream_t stream);
// The merge of positional segments (vpt_postings_merge_positional_device; kernels_postings_merge.hip)
vpt_status postings_merge_positional_device(const vpt_predictor* p, vpt_batch* b, const vpt_postings_positional_segment* segments, size_t n_segments,
                                            uint32_t n_terms_out, unsigned flags, uint64_t* d_term_offsets_out, uint32_t* d_post_docs_out,
                                            uint32_t* d_post_tfs_out, uint64_t* d_post_first_out, uint64_t capacity_out, uint32_t* d_post_positions_out,
                                            uint64_t capacity_positions_out, uint64_t* d_counts, hipStream_t stream);
// The BM25 top-k search over a segment (vpt_postings_search_device; kernels_postings_search.hip)
vpt_status postings_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs, const uint32_t* d_post_tfs,
                                  uint32_t n_terms, uint64_t capacity_postings, uint64_t doc_base, uint64_t n_documents, const uint32_t* d_doc_lens,
                                  const uint64_t* d_query_offsets, const int32_t* d_query_terms, const float* d_query_weights, uint32_t n_queries,
                                  uint64_t capacity_slots, float k1, float bm_b, float avgdl, uint32_t k, uint64_t capacity_candidates,
                                  uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_counts, uint64_t* d_match_counts, uint64_t* d_counts,
                                  hipStream_t stream);
// The BM25 top-k search with MUST / SHOULD / MUST_NOT slots (vpt_postings_boolean_search_device; kernels_postings_boolean.hip)
vpt_status postings_boolean_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                          const uint32_t* d_post_tfs, uint32_t n_terms, uint64_t capacity_postings, uint64_t doc_base, uint64_t n_documents,
                                          const uint32_t* d_doc_lens, const uint64_t* d_query_offsets, const int32_t* d_query_terms,
                                          const float* d_query_weights, const uint8_t* d_query_occurs, uint32_t n_queries, uint64_t capacity_slots, float k1,
                                          float bm_b, float avgdl, uint32_t k, uint64_t capacity_candidates, uint32_t* d_hit_docs, float* d_hit_scores,
                                          uint32_t* d_hit_counts, uint64_t* d_match_counts, uint64_t* d_counts, hipStream_t stream);
// The position lists of a segment and the exact-phrase search over them (vpt_postings_positions_device, vpt_postings_phrase_search_device;
// kernels_postings_phrase.hip)
vpt_status postings_positions_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_token_offsets, size_t n_documents, uint64_t capacity_in,
                                     const uint32_t* d_token_positions, const uint64_t* d_term_offsets, uint32_t n_terms, const uint64_t* d_post_first,
                                     uint64_t capacity_postings, const uint32_t* d_token_order, uint32_t* d_post_positions, hipStream_t stream);
vpt_status postings_phrase_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                         const uint32_t* d_post_tfs, const uint64_t* d_post_first, const uint32_t* d_post_positions, uint32_t n_terms,
                                         uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base, uint64_t n_documents,
                                         const uint32_t* d_doc_lens, const uint64_t* d_query_offsets, const int32_t* d_query_terms,
                                         const float* d_query_weights, uint32_t n_queries, uint64_t capacity_slots, float k1, float bm_b, float avgdl,
                                         uint32_t k, uint64_t capacity_probes, uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_freqs,
                                         uint32_t* d_hit_counts, uint64_t* d_match_counts, uint64_t* d_counts, bool sloppy,
                                         const uint32_t* d_query_slops, hipStream_t stream);   // sloppy: the sloppy probe; slops NULL: all 0
// Phrases to posting lists and the boolean search over a segment and such lists (vpt_postings_phrase_lists_device,
// vpt_postings_clause_search_device; kernels_postings_phrase.hip, kernels_postings_boolean.hip)
vpt_status postings_phrase_lists_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                        const uint32_t* d_post_tfs, const uint64_t* d_post_first, const uint32_t* d_post_positions, uint32_t n_terms,
                                        uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base, uint64_t n_documents,
                                        const uint64_t* d_phrase_offsets, const int32_t* d_phrase_terms, uint32_t n_phrases, uint64_t capacity_slots,
                                        uint64_t capacity_probes, uint64_t* d_list_offsets, uint32_t* d_list_docs, uint32_t* d_list_tfs,
                                        uint64_t capacity_lists, uint64_t* d_counts, bool sloppy, const uint32_t* d_phrase_slops, hipStream_t stream);
vpt_status postings_clause_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                         const uint32_t* d_post_tfs, uint32_t n_terms, uint64_t capacity_postings, const uint64_t* d_list_offsets,
                                         const uint32_t* d_list_docs, const uint32_t* d_list_tfs, uint32_t n_lists, uint64_t capacity_lists,
                                         uint64_t doc_base, uint64_t n_documents, const uint32_t* d_doc_lens, const uint64_t* d_query_offsets,
                                         const int32_t* d_query_terms, const float* d_query_weights, const uint8_t* d_query_occurs, uint32_t n_queries,
                                         uint64_t capacity_slots, float k1, float bm_b, float avgdl, uint32_t k, uint64_t capacity_candidates,
                                         uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_counts, uint64_t* d_match_counts, uint64_t* d_counts,
                                         hipStream_t stream);
vpt_status predict_device_impl(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                               const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries,
                               uint64_t max_sentence_bytes, int32_t* d_scores, uint8_t* d_labels, void* hip_stream);
vpt_status count_boundaries_impl(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                 size_t n_sentences, uint64_t* d_out_offsets, void* hip_stream, uint64_t text_bytes_hint);
// ConcatGraphemeClustersFilter on d_labels (kernels_graphemes.hip), the classes those of the text under b->flags' VPT_FLAG_KYTEA_FULLWIDTH; have_cps:
// b->d_cps holds this batch's chars already (the scoring launch in front left them there), else they are decoded here
vpt_status concat_graphemes_impl(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                 const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries, uint8_t* d_labels, bool have_cps,
                                 hipStream_t stream);
}  // namespace vptc
using namespace vptc;
