// Kernel-side parameter block and launchers (kernels.hip), used by the C ABI (capi.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "../../include/vaporetto_hip.h"
#include "layout.h"
#include "tables.hpp"
#include "tag_records.h"

namespace vpt {

constexpr int kThreads = 256;                    // 4 waves per workgroup
constexpr int kCap = 2048;                       // flat positions (chars + separators) one LDS tile can hold
constexpr int kTileFlat = 1024;                  // flat positions a tile is cut at (a tile ends with the sentence
                                                 // that crosses the cut, so it needs kCap - kTileFlat of slack)
constexpr int kMargin = 8;                       // zeroed slack past the tile for the s+1, s+2 look-ahead
// The specialised kernel's tile per ROW WINDOW wl (layout.h): fast_cap(wl) flat positions, fast_wg(wl) workgroups per CU.  Window 3
// (every distributed model): 1280 / 8, the best of the geometries measured on MI355X (profiles/r02_c5_ab*.jsonl, r03_d_ab_m1.jsonl;
// LDS-resident caches in front of the char table and the unigram nodes, a dense matrix for the bigram nodes of frequent second
// chars and a stage-major walk were measured in round 3 and are gone: profiles/r03_d/f/h_ab_*.jsonl).  Wider windows have wider
// nodes in flight and wider type rows in LDS: 1024 positions at 6 (5 for window 8) workgroups per CU.  Round 4 measured one more LDS table
// -- the symbol words of ASCII, U+3000..30FF and U+FF00..FFEF, direct-indexed, in the idle W queues during classify -- 2-3 % SLOWER on
// every workload (profiles/r04_f_ctab_*.jsonl; the fill and the range tests cost more than the gathers they save) and tiles of 960 /
// 640 positions (more rounds on a 100 K-sentence batch) 2 % / 13 % slower: out again.
// (-D overrides: A/B builds of tools/build_variants.sh.)
#ifndef VPT_FAST_CAP
#define VPT_FAST_CAP 1280
#endif
#ifndef VPT_FAST_WG
#define VPT_FAST_WG 8
#endif
#ifndef VPT_FAST_CAP_WIDE
#define VPT_FAST_CAP_WIDE 1024
#endif
constexpr int fast_cap(int wl) { return wl <= 3 ? VPT_FAST_CAP : VPT_FAST_CAP_WIDE; }
constexpr int fast_wg(int wl) { return wl <= 3 ? VPT_FAST_WG : wl <= 7 ? 6 : 5; }
constexpr int kFastCapMax = VPT_FAST_CAP > VPT_FAST_CAP_WIDE ? VPT_FAST_CAP : VPT_FAST_CAP_WIDE;
// Two ways of cutting a batch into tiles ("Tiles"):
//   whole sentences   a tile = the sentences whose flat start lies in its range; needs every sentence to fit beside tile_flat
//   cut anywhere      a tile = a range of flat positions plus a halo of max(pattern length) chars on either side, so a sentence
//                     of ANY length is scored by as many tiles as it spans (the reference scores any length in one loop,
//                     char_scorer/boundary_scorer.rs:93-113; its tantivy adapter passes whole documents as one Sentence)
constexpr int fast_whole_max_chars(int wl) { return fast_cap(wl) / 2 - 2 * pk_pad(wl); }   // batches whose longest sentence has more chars are cut
                                                 // anywhere (a whole-sentence tile holds tile_flat >= cap / 2 positions plus the sentence that crosses its end)
constexpr int kCutBlockShift = 8;                // cut tiles find their text through lead-byte counts per 256-byte block
constexpr int kFastStageSlack = 136;             // flat positions a cut tile leaves unused so that its text always fits the staging area
                                                 // (a tile of n chars stages at most 4 n + 2 * 256 bytes; the area holds 4 * cap + 32)
constexpr int kBitmapWords = 4 * kCap / 32 + 4;  // one bit per text byte of a tile (UTF-8: <= 4 bytes per char)

// device status word (OR of bits)
constexpr uint32_t kErrEmptySentence = 1u;    // "text: must contain at least one character" (sentence.rs:181-186)
constexpr uint32_t kErrNulChar = 2u;          // "text: must not contain NULL"               (sentence.rs:174-179)
constexpr uint32_t kErrBadOffsets = 4u;       // out_offsets do not match the text (or invalid UTF-8)
constexpr uint32_t kErrScratchTooSmall = 8u;  // max_sentence_bytes was understated
constexpr uint32_t kErrUnknownLabel = 16u;    // token emission: a label that is neither 0 nor 1
constexpr uint32_t kErrOutputTooSmall = 32u;  // token emission: text_capacity is smaller than the tokenized text
constexpr uint32_t kErrParse = 64u;           // tokenized text that parse_tokenized rejects: the reason / line in status words kParseErrWord + reason
// the reasons (sentence.rs:285-400), each with the smallest failing line as 0xFFFFFFFF - line (atomicMax) in status word kParseErrWord + reason
constexpr uint32_t kParseErrNoChar = 1u, kParseErrStartSpace = 2u, kParseErrDoubleSpace = 3u, kParseErrEndSpace = 4u, kParseErrSlash = 5u,
                   kParseErrNul = 6u, kParseErrWord = 8u;
constexpr uint32_t kErrParsePartial = 128u;   // partially annotated text that parse_partial_annotation rejects (sentence.rs:516-631)
// its reasons, each with the smallest failing line as 0xFFFFFFFF - line (atomicMax) in status word kPartialErrWord + reason; for kPartialErrChar the
// offending code point's bytes (little-endian, lead first) of THAT line in status word kPartialErrBytesWord, stored by the write pass
constexpr uint32_t kPartialErrNoChar = 1u, kPartialErrNul = 2u, kPartialErrChar = 3u, kPartialErrEnd = 4u, kPartialErrWord = 1u, kPartialErrBytesWord = 7u;
constexpr uint32_t kErrBadLabel = 256u;       // the partial-annotation writer: a label that is no CharacterBoundary (above 2)
constexpr uint32_t kErrBadTokenCsr = 512u;    // the id pass: token_offsets / starts / ends that do not describe the documents (kernels_vocab.hip)
constexpr uint32_t kErrVocabCounterFull = 1024u;   // the vocabulary counter: more keys or chars than it was made for (kernels_vocab_count.hip)
constexpr uint32_t kErrPostingsTooSmall = 2048u;   // the postings pass: more postings than capacity_out (kernels_postings.hip)
constexpr uint32_t kErrBadSegment = 4096u;         // the postings merge: term_offsets or postings that are not a segment's (kernels_postings_merge.hip)
constexpr uint32_t kErrSegmentsOverlap = 8192u;    // the postings merge, ordered: the segments' document ranges overlap or descend
constexpr uint32_t kErrTfOverflow = 16384u;        // the postings merge: a combined tf above 32 bits
constexpr uint32_t kErrBadQueryCsr = 32768u;          // the postings search: query_offsets that decrease, exceed capacity_slots or leave a slot unowned
constexpr uint32_t kErrBadWeights = 65536u;           // the postings search: a weight that is negative or not finite
constexpr uint32_t kErrQueryTooLong = 131072u;        // the postings search: a query of more than kSearchMaxQuerySlots slots
constexpr uint32_t kErrCandidatesTooSmall = 262144u;  // the postings search: more candidates than capacity_candidates
constexpr uint32_t kErrBadPositions = 524288u;        // the positions of a segment: a posting's positions do not strictly ascend (kernels_postings_phrase.hip)
constexpr uint32_t kErrPhraseTooLong = 1048576u;      // the phrase search: a phrase of more than kPhraseMaxTerms slots
constexpr uint32_t kErrProbesTooSmall = 2097152u;     // the phrase search: more probes than capacity_probes
constexpr uint32_t kErrPositionsTooSmall = 4194304u;  // the positional merge: more merged positions than capacity_positions_out
constexpr uint32_t kErrBadOccur = 8388608u;           // the boolean search: an occur value above 2 (kernels_postings_boolean.hip)
constexpr uint32_t kErrListsTooSmall = 16777216u;     // the phrase lists: more list entries than capacity_lists (kernels_postings_phrase.hip)
constexpr uint32_t kErrBadSlop = 33554432u;           // the sloppy phrase search: a slop above kPhraseMaxSlop


struct ScoreParams {
    PatternTableView ct;        // characters: n-grams + dictionary words
    PatternTableView tt;        // character types, when type_kind == kTypePatternTable
    PackedView pk;              // characters again, as the double-array trie of the specialised kernel (if eligible)
    const int32_t* type_table;  // 8^(2W) window scores, when type_kind == kTypeWindowTable
    const uint8_t* ctype;       // CharacterType of every BMP scalar value (65536 bytes)
    const uint32_t* cinfo;      // only with VPT_FLAG_KYTEA_FULLWIDTH, else nullptr: per BMP scalar value the char it is
                                // scored as (KyteaFullwidthFilter's image) | CharacterType of that char << 16
    const uint32_t* cid;        // specialised kernel: per BMP scalar value id | CharacterType << 16 | linebreak << 19 of the char it is
                                // scored as (layout.h, "ids"; the plain table or the one through KyteaFullwidthFilter)
    int32_t type_window;
    int32_t type_kind;
    int32_t bias;
    int32_t pad;
    const uint8_t* text;
    const uint64_t* boff;       // [S+1] byte offsets
    const uint64_t* ooff;       // [S+1] output (boundary) offsets
    const uint32_t* tile_first; // [n_tiles+1] (general kernel)
    const struct TileDesc* tiles; // [n_tiles] (specialised kernel, cut tiles; nullptr: whole-sentence tiles from tile_first)
    uint64_t n_sent;
    uint32_t tile_flat, n_tiles;
    int32_t* scores;
    uint8_t* labels;
    uint32_t* status;
    uint32_t* slow_list;        // tiles deferred to the global-scratch path
    uint32_t* slow_count;
    unsigned char* scratch;     // slabs for score_slow_kernel
    uint64_t scratch_stride;    // bytes per workgroup slab
    uint32_t scratch_cap;       // flat positions per slab
    uint32_t* cps_out;          // specialised kernel, optional: the batch's chars flat (char g of sentence i at ooff[i] + i + g) as scored
                                // scalar value | CharacterType << 24 -- what decode_chars_kernel makes for the tag kernel
    uint64_t total_chars;       // what cps_out holds: total boundaries + sentences of the call
    uint32_t post;              // label post-filters: bits 1..6 KyteaWsConstFilter per CharacterType, bit 7 SplitLinebreaksFilter, bit 8: that one FIRST
    uint32_t force_window_table;// experiment knob (read when the predictor is made): the 8^(2W) type table although type rows exist
    uint32_t debug;             // profiling ablation bits (VPT_DEBUG_ABLATE env, 0 in production)
    uint32_t text_nt;           // specialised kernel: the text is loaded non-temporal (1) or plain (0) -- the launch's choice (capi_internal.hpp, text_policy_for)
    uint64_t* prof;             // per-phase shader-cycle counters (VPT_PROFILE_PHASES env), else nullptr
};

// What a workgroup of the specialised kernel needs to know of its tile, made by the assign kernels (kernels_fast.hip).  The tile's
// text is bytes [byte0, byte0 + nbytes); lead number ci of it (0-based) in tile-local sentence si sits at LDS position
// c_off + ci + pad * si, si = sib0 + (sentence starts at or before its byte); positions outside [pad, flat_len) are not kept.
struct TileDesc {
    uint32_t i0, nsent;         // sentences [i0, i0 + nsent): every sentence with a byte in the staged text
    uint32_t byte0_lo, byte0_hi;
    uint32_t nbytes;
    int32_t c_off;
    int32_t sib0;               // -1: byte0 starts sentence i0; 0: it lies inside sentence i0
    uint32_t own_lo, own_hi;    // the boundaries (and chars) at LDS positions [own_lo, own_hi) are this tile's to write
    uint32_t flat_len;
    uint32_t g0_lo, g0_hi;      // global char number (out_offsets[i] + i + char index) of the first staged lead
    uint32_t expect_chars;      // leads the staged text must hold (whole-sentence tiles), 0xFFFFFFFF: not checked
    uint32_t strict_end;        // a lead at or past flat_len is an error (the text ends with the tile)
    uint32_t rsv0, rsv1;
};
static_assert(sizeof(TileDesc) == 64, "four 16-byte scalar loads");
static_assert(sizeof(ScoreParams) == 488, "the scoring kernels' parameter block (DESIGN.md 4.1; text_nt sits in what was padding in front of `prof`)");

// tag prediction (kernels_tags.hip); table layouts: HostTagTables in tables.hpp
struct TagParams {
    const uint32_t *tok_tab, *models, *mfilt, *ngrams, *nrec, *syms, *slots;
    const int32_t* weights;
    const uint32_t* cinfo;      // as in ScoreParams
    uint32_t tok_bits, n_tags, use_char, use_type;
    const uint32_t* cps;        // the batch's chars, flat (decode_chars_kernel): scored scalar value | CharacterType << 24
    const uint64_t* ooff;       // [S+1]
    const uint8_t* labels;      // [total boundaries] CharacterBoundary values (0, 1, 2 = Unknown)
    uint64_t n_sent;
    uint64_t total_chars;       // total boundaries + S: what `cps` holds (below 2^32 - 256: capi_device.cpp)
    const uint32_t *slot_str, *str_off;   // the tag strings' lengths (HostTagTables): what a token's tags take in the tokenized text
    uint32_t n_strings;
    // What fill_tags LEAVES (round 6): one RECORD per token that can have a tag model -- the reference holds None for every other char
    // (predictor.rs:558-573) and so nothing is stored for them -- sorted by the token's last char:
    //   records[k]  = {flat index of the token's last char (2 dwords), its tok_model word (layout.h: tag model + 1 | the bytes its tags take in
    //                  the tokenized text << 24; 0: the token table's filter let the token through but it has no tag model: an empty record),
    //                  slots of its "/tag" suffix (up to the last Some)}
    //                  (between the lookups and the passes: {last char, context clip, tag model + 1 | record form << 31, 0});
    //   rec_tags[k * n_tags + j] = the candidate chosen for slot j, -1 = None;   rec_str[k * n_tags + j] = {where that candidate's string starts in
    //                  the predictor's str_bytes, its length}: the writer copies bytes, it looks nothing up
    // The front end walks the batch in RUNS of `run_sent` consecutive sentences, a wave per run, in order, and numbers the run's CANDIDATES (the
    // token ends the filter lets through) as it meets them: candidate i of run r is record run_pref[r] + i.  run_pref [n_runs + 1]: zero in front of
    // the launches; the front end leaves run r's candidate count in entry r + 1; a chained scan turns it into the exclusive prefix (entry
    // n_runs: all records).  cands [total_chars]: run r's candidates at [first char of r, + count): {char in the run, token length, chars
    // before | after << 8 inside the sentence (clipped to the context), 0} -- plain stores, nothing the front end waits for.
    uint4* records;
    int32_t* rec_tags;
    uint2* rec_str;
    uint64_t* run_pref;
    uint64_t* scan_state;       // scan_part_entries(n_runs) words of that scan, zero in front of the launches
    uint64_t n_runs;
    uint32_t run_sent;
    uint4* cands;
    // the dense arrays of the C ABI, all optional (nullptr: not wanted), indexed by char; the caller has set them to None (-1) / left them alone:
    int32_t* tags;              // [(total boundaries + S) * n_tags] candidate index per slot: written at the last char of a token with a tag model
    int32_t* scores_out;        // [(total boundaries + S) * score_stride]: Predictor::store_tag_scores (predictor.rs:510-514,599-601): there, entries
                                // [0, bias.len()) = the scores the reference keeps in sentence.tag_scores[i]
    int32_t* model_out;         // [total boundaries + S]: there, the index of the tag model (Model::tag_models order)
    uint32_t score_stride;
    uint32_t n_cus;             // the device's CUs: the grids are what it holds at a time
    const uint32_t* summary;    // 2^(kTagSumLog2 - 5) words for the summary of the token filter (tag_filter_summary_kernel writes it, the front end reads it)
    uint32_t* status;           // the batch's control word; with kErrBadOffsets in it the front end accepts no run (THE RUNS' BOUND, tag_records.h)
};
// the records of P as their readers take them (the passes of fill_tags itself among them); str_bytes: the arena of the strings rec_str points into
VPT_HD TagRecordsView records_view(const TagParams& P, const uint8_t* str_bytes = nullptr) { return {P.records, P.rec_tags, P.rec_str, P.run_pref, str_bytes, P.n_runs, P.total_chars, P.run_sent, P.n_tags}; }
// sentences of a front-end run for a batch of this shape (about VPT_TAG_RUN_CHARS chars, at most 256 sentences); words of TagParams::summary
uint32_t tag_run_sentences(uint64_t n_sent, uint64_t total_chars);
size_t tag_summary_words();
// `fullwidth`: cinfo is the table that looks through KyteaFullwidthFilter (else the identity: no word of it is read)
hipError_t launch_decode_chars(const uint8_t* text, const uint64_t* boff, const uint64_t* ooff, uint64_t n_sent, uint64_t total_chars,
                               const uint32_t* cinfo, uint32_t* cps, uint8_t* types, uint32_t* status, hipStream_t stream, bool fullwidth);
hipError_t launch_tag_tokens(const TagParams& P, hipStream_t stream);

// token emission (kernels_emit.hip): Sentence::write_tokenized_text, boundary part
struct EmitParams {
    const uint8_t* text;
    const uint64_t* boff;       // [S+1]
    const uint64_t* ooff;       // [S+1]
    const uint8_t* labels;      // [total boundaries] 0 / 1
    uint64_t n_sent, total_boundaries;
    uint8_t* out_text;          // [capacity]
    uint64_t* out_offsets;      // [S+1] byte range of every sentence's tokenized text in out_text
    uint64_t capacity;
    uint32_t* status;
    TagRecordsView tag;         // "/tag" suffixes (sentence.rs:866-881), from the records the fill_tags call on this workspace left; records == nullptr: none
};
// scan_part: workspace of scan_part_entries(n_sent) uint64 (the prefix sum's per-workgroup partials)
size_t scan_part_entries(uint64_t n);
// The writer's launch (emit_flat_kernel): a WORKGROUP per run of `per_block` consecutive sentences (1 .. kEmitFlatMaxBlock)
constexpr uint32_t kEmitFlatMaxBlock = 512;   // (two sentences a thread)
struct EmitFuse {
    uint64_t* state;        // n_blocks + 1 words, ZERO when the kernel starts: the blocks' sizes / positions and the ticket
    uint64_t* clear;        // the state words of the NEXT call (the other of two arrays), zeroed by this one: [0, clear_n)
    uint64_t clear_n, n_blocks;
    uint32_t per_block;
    uint64_t* total_out;    // optional device-writable HOST address that receives the output's total size
    // calls enqueued one after the other on one stream write ONE contiguous text (vpt_tokenize_batch's chunks): a device word that holds the
    // output position in front of this call's text / receives the position behind it; nullptr: the text starts at 0
    const uint64_t* chain_in;
    uint64_t* chain_out;
};
// inclusive prefix sum over offsets[1 .. n] in place, offsets[0] = 0 (a chained scan, one launch; part: scan_part_entries(n) zero words)
// (a total above `capacity` raises `overflow_err` in *status, when there is one)
hipError_t launch_scan(uint64_t* offsets, uint64_t n, uint64_t* part, uint64_t capacity, uint32_t* status, uint64_t* total_out, hipStream_t stream,
                       uint32_t overflow_err = kErrOutputTooSmall);
// vpt_expand_tags_batch_device: the dense tags array from the records (None everywhere else)
hipError_t launch_expand_tags(const TagRecordsView& V, int32_t* tags, uint32_t n_cus, hipStream_t stream);
hipError_t launch_emit_tokenized(const EmitParams& P, const EmitFuse& F, hipStream_t stream);
// token spans (kernels_tokens.hip): vaporetto_tantivy's boundary_pos per document (vaporetto_tantivy/src/lib.rs:183-192), the writer's runs
struct SpanParams {
    const uint8_t* text;
    const uint64_t* boff;       // [S+1]
    const uint64_t* ooff;       // [S+1]
    const uint8_t* labels;      // [total boundaries] 0 / 1
    uint64_t n_sent, total_boundaries;
    uint32_t* token_ends;       // [capacity] byte offset, from the document's first byte, behind every token
    uint64_t* token_offsets;    // [S+1] the documents' ranges in token_ends
    uint64_t capacity;
    uint32_t* status;
};
hipError_t launch_token_spans(const SpanParams& P, const EmitFuse& F, hipStream_t stream);
// ... with every token's tags (token_spans_kernel<true>): n_tags int32 per token at token_tags[token * n_tags + slot] -- >= 0 an id of the
// predictor's tag vocabulary, -1 None (no record, an empty record, a slot left None), -(2 + id) a rule tag of the pattern tagger, as in the records.
// The records are those the fill_tags call on the workspace left for the same batch and labels (a slice per run, through tag_records.h).
struct SpanTags {
    TagRecordsView tag;
    int32_t* token_tags;          // [capacity * tag.n_tags]
    const uint2* vocab_slot;      // [n_models * tag.n_tags] {the slot's first string (HostTagTables::slot_str), its candidates}
    const uint32_t* vocab_ids;    // [n_strings] candidate string -> vocabulary id
    uint32_t n_models, n_strings;
};
hipError_t launch_token_tags(const SpanParams& P, const SpanTags& T, const EmitFuse& F, hipStream_t stream);
// The tag stop filter behind them (kernels_token_filter.hip): the kept tokens of the CSR, with starts and positions.  A count per workgroup of
// kTokenFilterBlock tokens, the chained scan, a scatter.  model_bits / rule_bits: one bitmap per slot over the predictor's vocabulary ids / the
// tagger's ids (nullptr: nothing of that kind is stopped; both nullptr: every token is kept).
constexpr uint32_t kTokenFilterBlock = 256;   // tokens a workgroup takes (vpt_token_filter_tile)
struct TokenFilterParams {
    const uint64_t* token_offsets;  // [n_docs + 1]
    const uint32_t* token_ends;     // [capacity_in]
    const int32_t* token_tags;      // [capacity_in * n_tags]
    uint64_t n_docs, capacity_in;
    uint32_t n_tags;
    const uint32_t *model_bits, *rule_bits;   // [n_tags * model_words], [n_tags * rule_words]
    uint32_t model_words, rule_words, n_vocab, n_rule;
    uint64_t* out_offsets;          // [n_docs + 1]
    uint32_t *out_starts, *out_ends, *out_positions;   // [capacity_out]
    int32_t* out_tags;              // [capacity_out * n_tags]
    uint64_t capacity_out;
    uint64_t* counts;               // workspace [n_blocks + 1], zero in front of the launches
    uint64_t n_blocks;              // ceil(bound of the tokens / kTokenFilterBlock), at least 1
    uint64_t* total_out;            // optional device-writable host address: the kept tokens
    uint32_t* status;
};
// scan_part: scan_part_entries(n_blocks) zero words
hipError_t launch_token_filter(const TokenFilterParams& P, uint64_t* scan_part, hipStream_t stream);
// Vocabulary ids of a finished span CSR (kernels_vocab.hip): one int32 per token, the id of its surface in the table of vocab_table.hpp or unk_id.
// A workgroup takes kVocabTile consecutive tokens, a lane per token.  starts == nullptr: a token's start is the entry before it in its
// document, or 0 (what the span kernels write); else starts / ends are the filter's.  cinfo: nullptr, or the KyteaFullwidthFilter image of the
// BMP (decode_chars_kernel's table): the surface looked up is then that of the text as it was scored.
constexpr uint32_t kVocabTile = 256;       // tokens a workgroup takes (vpt_vocab_tile)
constexpr uint32_t kVocabLdsOffsets = 512; // token_offsets entries of a tile's documents kept in LDS; a tile that spans more bisects in global memory
struct VocabParams {
    const uint8_t* text;
    const uint64_t* boff;           // [n_docs + 1]
    uint64_t n_docs;
    const uint64_t* token_offsets;  // [n_docs + 1]
    const uint32_t* token_starts;   // [capacity_in] or nullptr
    const uint32_t* token_ends;     // [capacity_in]
    uint64_t capacity_in;
    const uint4* slots;             // 2^bits slots {id + 1, chars, fingerprint, first code point in surf}
    const uint32_t* surf;
    const uint32_t* cinfo;
    uint32_t bits, max_len;
    int32_t unk_id;
    int32_t* ids;                   // [capacity_in]
    uint32_t* status;
};
hipError_t launch_token_ids(const VocabParams& P, hipStream_t stream);
// The vocabulary counter (kernels_vocab_count.hip; vocab_count.hpp): an accumulating table token surface -> 64-bit count in ONE device allocation.
//   ctrl     kVc* words below
//   slots    [n_slots], n_slots a power of two: 0 empty; bit 63 set: a committed key, the low bits its index in `keys`; else token index + 1 of
//            the representative of the count call that is running
//   counts   [n_slots]: the count of the slot's key
//   keys     [max_keys] {first code point in arena, chars, fingerprint (high 32 bits of the surface's hash), 0}
//   arena    [arena_chars]: the keys' code points
//   out      [max_keys] {count low, count high, first code point in arena, chars}: what finish leaves for the host
constexpr uint32_t kVcKeys = 0, kVcArena = 1, kVcCounted = 2, kVcSkipped = 3, kVcFull = 4, kVcOut = 5, kVcCtrlWords = 32;
constexpr uint32_t kVcNoSlot = 0xFFFFFFFFu;
constexpr uint64_t kVcCommitted = 1ull << 63;
struct VocabCounterView {
    uint64_t* ctrl;
    uint64_t* slots;
    uint64_t* counts;
    uint4* keys;
    uint32_t* arena;
    uint4* out;
    uint64_t arena_chars;
    uint32_t n_slots, max_keys, max_chars;
};
// A count call over a finished span CSR (the id pass's conventions): three launches over the batch's tokens, a lane per token in tiles of
// kVocabTile.  rec: two uint4 per token, [2 * capacity_in], scratch of the batch: {hash low, hash high, first byte in the text low, high},
// {bytes, chars (0: skipped), the slot this token won or kVcNoSlot, 0}.
struct VocabCountParams {
    const uint8_t* text;
    const uint64_t* boff;           // [n_docs + 1]
    uint64_t n_docs;
    const uint64_t* token_offsets;  // [n_docs + 1]
    const uint32_t* token_starts;   // [capacity_in] or nullptr
    const uint32_t* token_ends;     // [capacity_in]
    uint64_t capacity_in;
    const uint32_t* cinfo;
    VocabCounterView C;
    uint4* rec;
    uint32_t* status;
};
hipError_t launch_vocab_count(const VocabCountParams& P, hipStream_t stream);
// one launch, a lane per slot: out[0 .. ctrl[kVcOut]) for every committed key of count >= min_count (ctrl[kVcOut] zero before)
hipError_t launch_vocab_count_finish(const VocabCounterView& C, uint64_t min_count, hipStream_t stream);
// Postings of a finished span CSR's ids (kernels_postings.hip): term -> (document, tf), term-major, by one stable sort of the capacity_in places
// by key (the id, or the sentinel n_terms for a dropped token and for a place behind the tokens) and a run-length pass.  Scratch of the batch,
// 28 bytes a place and the sort's histograms (16 bytes per 16 places): keydoc [2 * capacity_in] {key, document}; order, skey, flags
// [capacity_in]; scan [capacity_in + 1].  The caller runs train_radix_sort (keydoc, stride 2 -> order; skey is its second index array) between
// keys and heads, and train_scan (flags -> scan) between heads and emit.
constexpr uint32_t kPostingsSortTile = 4096;   // the tile of train_radix_sort and train_scan (vpt_postings_tile checks it against them)
constexpr uint32_t kPostingsMaxTerms = 1u << 24;
struct PostingsParams {
    const uint64_t* token_offsets;  // [n_docs + 1]
    uint64_t n_docs;
    const int32_t* ids;             // [capacity_in]
    uint64_t capacity_in;
    uint32_t n_terms;
    uint64_t doc_base;
    uint32_t* keydoc;
    uint32_t* order;
    uint32_t* skey;
    uint32_t* flags;
    uint64_t* scan;
    uint64_t* term_offsets;         // [n_terms + 1]
    uint32_t* post_docs;            // [capacity_out]
    uint32_t* post_tfs;             // [capacity_out]
    uint64_t capacity_out;
    uint64_t* post_first;           // [capacity_out + 1] or nullptr
    uint32_t* token_order;          // [capacity_in] or nullptr
    uint64_t* counts;               // [2]: postings (written), dropped tokens (added to: zero before the launches)
    uint32_t* status;
};
hipError_t launch_postings_keys(const PostingsParams& P, hipStream_t stream);
hipError_t launch_postings_heads(const PostingsParams& P, hipStream_t stream);
hipError_t launch_postings_emit(const PostingsParams& P, hipStream_t stream);   // emit, then the terms
// Merge of K postings segments that share a term id space (kernels_postings_merge.hip).  The segments' descriptors live in the batch's scratch
// (segs [n_segs], loaded by launch_postings_merge_load from kernel arguments, kPostingsMergeLoad a launch); every launch is over the n_places =
// the sum of the capacities, over the n_terms + 1 term bounds, or over the segments.  A place p belongs to the segment s with
// place_base[s] <= p < place_base[s + 1]; it holds a posting when p - place_base[s] < min(term_offsets_s[n_terms_s], capacity_s).
// Ordered route: table [n_segs * (n_terms + 1)], table[s * (n_terms + 1) + k] = where segment s's list of term k starts in the output; range
// [2 * n_segs] the segments' smallest and largest document.  General route: rec [3 * n_places] {term or the sentinel n_terms, document, tf};
// order, skey, flags [n_places]; scan [n_places + 1]; the caller runs train_radix_sort (rec, stride 3: the document word, then the term word)
// between records and heads, and train_scan (flags -> scan) between heads and emit.
constexpr uint32_t kPostingsMergeMaxSegments = 1024;
constexpr uint32_t kPostingsMergeLoad = 64;   // descriptors a load launch carries in its arguments
struct PostingsMergeSegment {
    const uint64_t* term_offsets;   // [n_terms + 1]
    const uint32_t* docs;           // [capacity]
    const uint32_t* tfs;            // [capacity]
    uint64_t capacity;
    uint64_t place_base;            // the capacities in front
    uint32_t n_terms;
    uint32_t pad;
};
struct PostingsMergeLoadArgs {
    PostingsMergeSegment seg[kPostingsMergeLoad];
};
struct PostingsMergeParams {
    PostingsMergeSegment* segs;     // [n_segs], scratch
    uint32_t n_segs;
    uint32_t n_terms;               // n_terms_out
    uint64_t n_places;              // the sum of the capacities, < 2^32
    uint64_t* table;                // ordered
    uint32_t* range;                // ordered
    uint32_t* rec;                  // general
    uint32_t* order;
    uint32_t* skey;
    uint32_t* flags;
    uint64_t* scan;
    uint64_t* term_offsets;         // [n_terms + 1]
    uint32_t* post_docs;            // [capacity_out]
    uint32_t* post_tfs;             // [capacity_out]
    uint64_t capacity_out;
    uint64_t* counts;               // [2]: merged postings, input postings combined into another
    uint32_t* status;
};
hipError_t launch_postings_merge_load(const PostingsMergeParams& P, const PostingsMergeSegment* host_segs, hipStream_t stream);
hipError_t launch_postings_merge_ordered(const PostingsMergeParams& P, hipStream_t stream);   // table, copy, check
hipError_t launch_postings_merge_records(const PostingsMergeParams& P, hipStream_t stream);   // the offsets' check, then the records
hipError_t launch_postings_merge_heads(const PostingsMergeParams& P, hipStream_t stream);
hipError_t launch_postings_merge_emit(const PostingsMergeParams& P, hipStream_t stream);      // emit, then the terms
// The merge of POSITIONAL segments: the launches above write the three arrays as they do without positions, the launches below add post_first
// and post_positions.  psegs [n_segs] lies beside segs (loaded by launch_postings_merge_positions_load); a POSITION PLACE pp belongs to the
// segment s with pplace_base[s] <= pp < pplace_base[s + 1] (the capacity_positions laid end to end, n_pplaces their sum) and holds a position
// when pp - pplace_base[s] < min(post_first_s[postings_s], capacity_positions_s).
// Ordered route: ptable [n_segs * (n_terms + 1)], ptable[s * (n_terms + 1) + k] = where segment s's positions of term k start in the output =
// the sum over the segments of post_first_t[term_offsets_t[k]] plus the positions of term k in the segments in front of s.  launch_..._ordered
// runs offsets (M's table and ptable), copy (M's copy and post_first), check and pcopy in place of launch_postings_merge_ordered.
// General route, behind launch_postings_merge_heads: ptf [n_places] = the tf of the input posting at sorted place j, inv [n_places] = the sorted
// place of input place p (launch_..._ranks); the caller runs train_scan (flags -> scan), launch_postings_merge_emit and train_scan (ptf ->
// pscan [n_places + 1]); then launch_..._general: first (post_first of a head = pscan at it) and pcopy (a position's rank inside its merged
// posting = its rank in its own posting + the positions below it in the other members of its run, at most n_segs - 1 bisections).
struct PostingsMergePosSegment {
    const uint64_t* first;          // [capacity + 1]
    const uint32_t* positions;      // [capacity_positions]
    uint64_t capacity_positions;
    uint64_t pplace_base;           // the capacity_positions in front
};
struct PostingsMergePosLoadArgs {
    PostingsMergePosSegment seg[kPostingsMergeLoad];
};
struct PostingsMergePosParams {
    PostingsMergeParams M;          // M.counts: [3], the third the merged positions
    PostingsMergePosSegment* psegs; // [n_segs], scratch
    uint64_t n_pplaces;             // the sum of the capacity_positions, < 2^32
    uint64_t* ptable;               // ordered
    uint32_t* ptf;                  // general
    uint32_t* inv;
    uint64_t* pscan;
    uint64_t* post_first;           // [capacity_out + 1]
    uint32_t* post_positions;       // [capacity_positions_out]
    uint64_t capacity_positions_out;
};
hipError_t launch_postings_merge_positions_load(const PostingsMergePosParams& Q, const PostingsMergePosSegment* host_psegs, hipStream_t stream);
hipError_t launch_postings_merge_positions_ordered(const PostingsMergePosParams& Q, hipStream_t stream);
hipError_t launch_postings_merge_positions_ranks(const PostingsMergePosParams& Q, hipStream_t stream);
hipError_t launch_postings_merge_positions_general(const PostingsMergePosParams& Q, hipStream_t stream);   // first, then pcopy
// BM25 top-k search of a batch of queries over one postings segment (kernels_postings_search.hip).  A CANDIDATE is a (slot, posting of the slot's
// term) pair; the slots' dfs are scanned into candidate bases, and every launch is over the capacity_slots slots, the capacity_candidates PLACES,
// the n_queries + 1 query bounds or the n_queries * k outputs.  Scratch of the batch: per slot slot_df (u64), base (u64, [capacity_slots + 1]) and
// slot_query (u32); per place rec [3] {document - doc_base, query or the sentinel n_queries, bits of c}, hit [3] {query or the sentinel,
// document - doc_base, ~bits of the score}, order, skey, flags (u32) and scan (u64, [places + 1]); qstart [n_queries + 1] (u64).  The caller runs
// train_scan (slot_df -> base) between slots and expand, train_radix_sort (rec, stride 3: the document word, then the query word) between expand
// and heads, train_scan (flags -> scan) between heads and sum, train_radix_sort (hit, stride 3: the score word, then the query word) between
// sum and take.  A launch behind expand that finds one of error_mask in the status leaves the four outputs alone: kSearchErrors, and for the
// clause search, which is enqueued behind a lists call without a sync between them, that call's bits too (kClauseErrors).
constexpr uint32_t kSearchMaxQuerySlots = 1024;
constexpr uint32_t kSearchMaxQueries = 1u << 24;
constexpr uint32_t kSearchErrors = kErrBadSegment | kErrBadQueryCsr | kErrBadWeights | kErrQueryTooLong | kErrCandidatesTooSmall | kErrBadOccur;
struct PostingsSearchParams {
    const uint64_t* term_offsets;   // [n_terms + 1]
    const uint32_t* post_docs;      // [capacity_postings]
    const uint32_t* post_tfs;       // [capacity_postings]
    uint64_t capacity_postings;
    uint32_t n_terms;
    uint64_t doc_base;
    uint64_t n_docs;
    const uint32_t* doc_lens;       // [n_docs]
    const uint64_t* query_offsets;  // [n_queries + 1]
    const int32_t* query_terms;     // [capacity_slots]
    const float* query_weights;     // [capacity_slots]
    uint32_t n_queries;
    uint64_t capacity_slots;        // < 2^32
    uint64_t n_places;              // capacity_candidates, < 2^32
    float k1, b, avgdl;
    uint32_t k;
    uint64_t* slot_df;
    uint64_t* base;
    uint32_t* slot_query;
    uint32_t* rec;
    uint32_t* hit;
    uint32_t* order;
    uint32_t* skey;
    uint32_t* flags;
    uint64_t* scan;
    uint64_t* qstart;
    uint32_t* hit_docs;             // [n_queries * k]
    float* hit_scores;              // [n_queries * k]
    uint32_t* hit_counts;           // [n_queries]
    uint64_t* match_counts;         // [n_queries]
    uint64_t* counts;               // [3]: candidates, matches (written), skipped slots (added to: zero before the launches)
    uint32_t* status;
    uint32_t error_mask;            // the status bits with which ranges and take write nothing
};
hipError_t launch_postings_search_slots(const PostingsSearchParams& P, hipStream_t stream);
hipError_t launch_postings_search_expand(const PostingsSearchParams& P, hipStream_t stream);
hipError_t launch_postings_search_heads(const PostingsSearchParams& P, hipStream_t stream);
hipError_t launch_postings_search_sum(const PostingsSearchParams& P, hipStream_t stream);    // sum, then the queries' ranges
hipError_t launch_postings_search_take(const PostingsSearchParams& P, hipStream_t stream);
// BM25 top-k search with MUST / SHOULD / MUST_NOT slots (kernels_postings_boolean.hip).  S is the OR search's block: the same inputs, scratch and
// outputs, and heads, sum, ranges and take are the OR search's launches over S as they stand.  A query's ANCHOR is its first MUST slot of the
// smallest df.  A PLACE is a posting of the anchor, or, in a query without a MUST slot, a posting of a SHOULD slot (a candidate of the OR
// search); S.slot_df holds a slot's places, S.n_places bounds their sum.  Scratch beside S's: q_anchor (u64) and q_flags (u32) per query.  The
// caller runs queries, slots, train_scan (S.slot_df -> S.base), expand, then the OR search's launches from the first sort on.
// The CLAUSE search (vpt_postings_clause_search_device) is the same three kernels over TWO segments: a term t in [S.n_terms, S.n_terms +
// n_lists) names list t - S.n_terms of the derived segment {list_offsets, list_docs, list_tfs, capacity_lists} -- the phrase lists call's
// output -- and is, for the rest of the rule, a term whose list is that one.  n_lists 0: one segment, the boolean search as it was.
constexpr uint32_t kOccurShould = 0, kOccurMust = 1, kOccurMustNot = 2;
constexpr uint64_t kBoolNoAnchor = ~uint64_t(0);      // q_anchor: the query has no MUST slot
constexpr uint64_t kBoolDead = ~uint64_t(0) - 1;      // q_anchor: no document can match (a MUST slot of df 0 or out of range, a query that is none)
constexpr uint32_t kBoolHasNot = 1u;                  // q_flags: the query has a MUST_NOT slot
struct PostingsBooleanParams {
    PostingsSearchParams S;
    const uint8_t* occurs;          // [capacity_slots]
    uint64_t* q_anchor;             // [n_queries]
    uint32_t* q_flags;              // [n_queries]
    const uint64_t* list_offsets;   // [n_lists + 1]          (the clause search; n_lists 0: none of the four is looked at)
    const uint32_t* list_docs;      // [capacity_lists]
    const uint32_t* list_tfs;       // [capacity_lists]
    uint64_t capacity_lists;
    uint32_t n_lists;               // S.n_terms + n_lists <= kPostingsMaxTerms
};
hipError_t launch_postings_boolean_queries(const PostingsBooleanParams& P, hipStream_t stream);
hipError_t launch_postings_boolean_slots(const PostingsBooleanParams& P, hipStream_t stream);
hipError_t launch_postings_boolean_expand(const PostingsBooleanParams& P, hipStream_t stream);
// The position lists of a segment (kernels_postings_phrase.hip): one launch, a lane per place of capacity_in, behind the postings pass that wrote
// post_first / token_order.  post_positions[i] = the position of token token_order[i] for every i below the indexed tokens.
struct PostingsPositionsParams {
    const uint64_t* token_offsets;  // [n_docs + 1]
    uint64_t n_docs;                // >= 1
    uint64_t capacity_in;
    const uint32_t* positions;      // [capacity_in] or nullptr: the token's index inside its document
    const uint64_t* term_offsets;   // [n_terms + 1]
    uint32_t n_terms;
    const uint64_t* post_first;     // [capacity_postings + 1]
    uint64_t capacity_postings;
    const uint32_t* token_order;    // [capacity_in]
    uint32_t* post_positions;       // [capacity_in]
    uint32_t* status;
};
hipError_t launch_postings_positions(const PostingsPositionsParams& P, hipStream_t stream);
// Exact-phrase BM25 top-k search over a POSITIONAL segment (kernels_postings_phrase.hip).  A query is one phrase; its ANCHOR is the slot whose
// term has the fewest indexed tokens (the first such slot), and its PROBES are the anchor term's positions, one contiguous run of
// post_positions.  The probe counts are scanned into probe bases, and every launch is over the n_queries + 1 query bounds, the capacity_probes
// PLACES or the n_queries * k outputs.  Scratch of the batch: per query q_anchor (u32), q_run, q_probes, base [n_queries + 1] and qstart
// [n_queries + 1] (u64): 36 bytes; per slot nothing; per place flags, plen, pdoc, pq, hpf, order, skey (u32), hit [3] {query or the sentinel
// n_queries, document - doc_base, ~bits of the score} and scan (u64, [places + 1]): 48 bytes.  The caller runs train_scan (q_probes -> base)
// between queries and probe, train_scan (flags -> scan) between probe and heads and again between heads and emit, and train_radix_sort (hit,
// stride 3: the score word, then the query word) between emit and take.  A launch behind probe that finds one of kPhraseErrors in the status
// leaves the five outputs alone.
// The phrase LISTS (vpt_postings_phrase_lists_device) are the same launches up to the second heads scan, with query_weights NULL (no weight is
// looked at), and one launch of their own behind it: a head with scan value h writes list entry h {doc_base + document, pf}, a lane per query
// bound writes list_offsets by ranges' rule; with one of kPhraseErrors in the status, or more entries than capacity_lists (kErrListsTooSmall),
// it writes the counts only.  No sort, no take; doc_lens, k1, b, avgdl, k and the hit arrays are not looked at.
// The SLOPPY calls (vpt_postings_sloppy_phrase_search_device, .._lists_device) are the launches above with query_slops set and the sloppy probe
// in probe's place: flags[p] = the occurrences the place owns, 0 .. 32 (2 * kPhraseMaxSlop + 1 = 63 bits of a 64-bit mask per slot), and pf
// is clamped to 2^32 - 1 in heads.  Everything behind probe is the exact search's.
constexpr uint32_t kPhraseMaxTerms = 64;
constexpr uint32_t kPhraseMaxSlop = 31;
constexpr uint32_t kPhraseErrors = kErrBadSegment | kErrBadQueryCsr | kErrBadWeights | kErrPhraseTooLong | kErrProbesTooSmall | kErrBadSlop;
constexpr uint32_t kClauseErrors = kSearchErrors | kPhraseErrors | kErrListsTooSmall;
constexpr uint32_t kListsVoid = kErrPhraseTooLong | kErrProbesTooSmall | kErrListsTooSmall | kErrBadSlop;   // set by the lists calls alone: no list was written
struct PostingsPhraseParams {
    const uint64_t* term_offsets;   // [n_terms + 1]
    const uint32_t* post_docs;      // [capacity_postings]
    const uint32_t* post_tfs;       // [capacity_postings]
    const uint64_t* post_first;     // [capacity_postings + 1]
    const uint32_t* post_positions; // [capacity_positions]
    uint64_t capacity_postings;
    uint64_t capacity_positions;
    uint32_t n_terms;
    uint64_t doc_base;
    uint64_t n_docs;
    const uint32_t* doc_lens;       // [n_docs]
    const uint64_t* query_offsets;  // [n_queries + 1]
    const int32_t* query_terms;     // [capacity_slots]
    const float* query_weights;     // [n_queries]; nullptr: the lists call
    uint32_t n_queries;
    uint64_t capacity_slots;        // < 2^32
    uint64_t n_places;              // capacity_probes, < 2^32
    float k1, b, avgdl;
    uint32_t k;
    uint32_t* q_anchor;             // [n_queries]: the anchor's slot inside the query
    uint64_t* q_run;                // [n_queries]: the anchor run's first place in post_positions
    uint64_t* q_probes;             // [n_queries]: the run's length, 0 when the query cannot match
    uint64_t* base;                 // [n_queries + 1]
    uint64_t* qstart;               // [n_queries + 1]
    uint32_t* flags;                // probe: 1 at an occurrence; heads: 1 at a head
    uint64_t* scan;                 // of the occurrences, then of the heads
    uint32_t* plen;                 // probe: the posting's tf at its first place, else 0; heads: pf at a head
    uint32_t* pdoc;                 // document - doc_base
    uint32_t* pq;                   // the place's query, or n_queries
    uint32_t* hit;
    uint32_t* hpf;
    uint32_t* order;
    uint32_t* skey;
    uint32_t* hit_docs;             // [n_queries * k]
    float* hit_scores;              // [n_queries * k]
    uint32_t* hit_freqs;            // [n_queries * k] or nullptr
    uint32_t* hit_counts;           // [n_queries]
    uint64_t* match_counts;         // [n_queries]
    uint64_t* counts;               // [3]: probes, matches (written), skipped queries (added to: zero before the launches)
    uint32_t* status;
    uint64_t* list_offsets;         // [n_queries + 1]        (the lists call)
    uint32_t* list_docs;            // [capacity_lists]
    uint32_t* list_tfs;             // [capacity_lists]
    uint64_t capacity_lists;
    const uint32_t* query_slops;    // [n_queries]; nullptr: every slop 0 (and the exact calls).  The last member: no other argument moves
};
hipError_t launch_postings_phrase_queries(const PostingsPhraseParams& P, hipStream_t stream);
hipError_t launch_postings_phrase_probe(const PostingsPhraseParams& P, hipStream_t stream);
hipError_t launch_postings_phrase_sloppy_probe(const PostingsPhraseParams& P, hipStream_t stream);   // in probe's place: the sloppy calls
hipError_t launch_postings_phrase_heads(const PostingsPhraseParams& P, hipStream_t stream);
hipError_t launch_postings_phrase_emit(const PostingsPhraseParams& P, hipStream_t stream);    // emit, then the queries' ranges
hipError_t launch_postings_phrase_take(const PostingsPhraseParams& P, hipStream_t stream);
hipError_t launch_postings_phrase_lists(const PostingsPhraseParams& P, hipStream_t stream);   // behind the second heads scan
// ConcatGraphemeClustersFilter on the labels (kernels_graphemes.hip): labels[ooff[i] + b] = 0 for every boundary b of sentence i inside an extended
// grapheme cluster of the text as it was scored.  Two launches over tiles of kGraphemeTile chars, cut by flat position.
constexpr uint32_t kGraphemeTile = 1024;
struct GraphemeParams {
    const uint32_t* cps;        // decode_chars' words of the batch (or the scoring kernel's ScoreParams::cps_out): the chars as they were scored
    const uint64_t* boff;       // [S+1]
    const uint64_t* ooff;       // [S+1]
    uint64_t n_sent;
    uint64_t total_chars;       // what cps holds: total boundaries + S, or an upper bound of it (the offsets say how many there are)
    uint64_t total_boundaries;  // what labels holds (or an upper bound)
    const uint8_t* table;       // tables.hpp, grapheme_class
    uint8_t* cls;               // workspace [n_tiles * kGraphemeTile]: class byte | 0x80 at a sentence's first char
    uint32_t* summ;             // workspace [n_tiles]: the tiles' summaries
    uint32_t* first;            // workspace [n_tiles]: sentences that start in front of the tile
    uint8_t* labels;            // [total boundaries], edited in place
    uint32_t* status;
    uint32_t n_tiles;           // ceil(total_chars / kGraphemeTile)
};
hipError_t launch_concat_graphemes(const GraphemeParams& P, hipStream_t stream);

// PatternMatchTagger behind fill_tags (kernels_pattern.hip; the table: pattern_tagger.hpp): every token whose whole surface is a rule's key gets the
// rule's tags in the slots fill_tags left None.  A rule tag is -(2 + id) in rec_tags and in the dense array (-1 stays None, >= 0 a candidate of the
// tag model); a record the rules made for a token without a tag model carries kTokModelMask where a model's records carry model + 1.
// The merged records go to arrays of their own, sorted by position like fill_tags' -- a count per run, a scan, a scatter; no sort, no atomics.
constexpr uint32_t kPatternStep = 256;   // chars a workgroup takes at a time (vpt_pattern_tagger_tile)
struct PatternParams {
    const uint4* slots; const uint32_t* surf; const int32_t* rule_tags; const uint2* id_str;   // the table; id_str: a tag's escaped bytes {start, length} in the writer's arena
    uint32_t bits, max_len, n_tags;
    const uint32_t* cps;        // decode_chars' words of the batch
    const uint64_t* ooff;       // [S+1]
    const uint8_t* labels;      // [total boundaries]
    uint64_t n_sent, total_chars;
    TagRecordsView in;          // what fill_tags left (capacity = total_chars, n_tags = n_tags)
    uint2* hits;                // workspace [total_chars]: {rule + 1 | a new record << 31, new records of the run in front of the char}
    uint4* out_records; int32_t* out_rec_tags; uint2* out_rec_str;
    uint64_t* out_run_pref;     // [in.n_runs + 1], zero in front of the launches
    uint64_t* scan_state;       // scan_part_entries(in.n_runs) zero words
    int32_t* tags;              // the dense array of the C ABI, or nullptr
    uint32_t n_cus;
    uint32_t* status;           // the batch's control word: with kErrBadOffsets in it no run is looked at (TagParams::status)
};
hipError_t launch_pattern_tagger(const PatternParams& P, hipStream_t stream);

// the predict CLI's listings (kernels_listing.hip): per line T, the scores block and the tag block in one arena (predict/src/main.rs:66-93, 122-176)
constexpr uint32_t kListingScores = 1u, kListingTagScores = 2u, kListingTagged = 4u, kListingNoNormOrder = 8u;   // VPT_LISTING_*
struct ListingParams {
    const uint32_t* cps;        // decode_chars' words of the batch: the chars as they were scored
    const uint64_t* ooff;       // [S+1]
    const int32_t* scores;      // [total boundaries] (kListingScores)
    const uint8_t* labels;      // [total boundaries] 0 / 1 (kListingTagScores: the writer has checked them)
    uint64_t n_sent, total_boundaries;
    uint64_t n_elem;            // 2 * (total boundaries + S) + S: the elements (kernels_listing.hip)
    const uint8_t* t_text;      // the writer's text for the same batch and labels, t_cap bytes, and its offsets [S+1]
    const uint64_t* t_off;
    uint64_t t_cap;
    const int32_t* tag_models;  // fill_tags' dense arrays (TagParams::model_out / scores_out); nullptr: no token has a tag model
    const int32_t* tag_scores;
    uint32_t score_stride, n_models, n_strings, flags;
    const uint32_t *models, *slots, *slot_str, *str_off;   // HostTagTables
    const uint8_t* str_bytes;
    uint64_t* pos;              // [n_elem + 1] workspace: the elements' sizes, then their positions
    uint8_t* out;               // [capacity]
    uint64_t* out_offsets;      // [S+1] the lines' ranges in out
    uint64_t capacity;
    uint32_t* status;
};
// scan_part: scan_part_entries(n_elem) zero words
hipError_t launch_listing(const ListingParams& P, uint64_t* scan_part, hipStream_t stream);
// copy[n_sent + 1] = ooff when it is non-decreasing and ends inside total_boundaries, else zeros and kErrBadOffsets; flag: a zero word
hipError_t launch_listing_offsets(const uint64_t* ooff, uint64_t n_sent, uint64_t total_boundaries, uint64_t* copy, uint32_t* flag, uint32_t* status,
                                  hipStream_t stream);
// vpt_count_boundaries on the device: ooff_out[S+1]; *max_chars (atomicMax) = the longest sentence in chars; text_bytes_hint: the batch's text
// bytes when the host knows them (0: not), which sizes the workgroups' shares
hipError_t launch_count_boundaries(const uint8_t* text, const uint64_t* boff, uint64_t n_sent, uint64_t* ooff_out, uint64_t* scan_part, uint32_t* status,
                                   uint32_t* max_chars, uint64_t text_bytes_hint, hipStream_t stream);

// annotated text -> raw text + labels + tags (kernels_parse.hip), one frame for two syntaxes:
//   kTokenized  Sentence::from_tokenized (sentence.rs:285-400): labels 0 / 1, tags on a token's last char;
//   kPartial    Sentence::from_partial_annotation (sentence.rs:516-631): labels 0 / 1 / 2, tags on any char.
// Count pass: raw_off / ooff / tag_off / tb_off [line + 1] = the line's surface bytes / boundaries / tags / tag bytes, n_tags[line]; four
// chained scans turn them into offsets; the write pass fills raw, labels, tag_index (first tag of every char, [chars + 1]), span_off
// (first byte of every tag in tag_bytes, [tags + 1]) and tag_bytes (escapes removed).  *_cap: what the caller's buffers hold.
enum class ParseKind { kTokenized, kPartial };
struct ParseParams {
    const uint8_t* text;
    const uint64_t* boff;       // [S+1]
    uint64_t n_sent;
    uint8_t* raw; uint64_t raw_cap;
    uint64_t* raw_off;          // [S+1]
    uint64_t* ooff;             // [S+1], as vpt_count_boundaries lays it out
    uint8_t* labels; uint64_t label_cap;
    uint32_t* n_tags;           // [S]
    uint64_t* tag_index; uint64_t index_cap;
    uint64_t* span_off; uint64_t span_cap;
    uint8_t* tag_bytes; uint64_t tb_cap;
    uint64_t* tag_off;          // [S+1] workspace: tags in front of every line
    uint64_t* tb_off;           // [S+1] workspace: tag bytes in front of every line
    uint32_t* status;           // the workspace's status words (kErrParse / kErrParsePartial + the syntax's reason words)
};
hipError_t launch_parse(ParseKind kind, const ParseParams& P, uint64_t* scan_part, hipStream_t stream);
// Sentence::write_partial_annotation_text for a batch (sentence.rs:907-944) from what the parsers write: a count pass (out_off[line + 1] = the
// line's bytes), the chained scan, a write pass.  tag_index == nullptr: no tags.
struct WritePartialParams {
    const uint8_t* text;        // raw text
    const uint64_t* boff;       // [S+1]
    const uint64_t* ooff;       // [S+1]
    uint64_t n_sent;
    const uint8_t* labels;      // 0 / 1 / 2 per boundary
    const uint64_t* tag_index;  // the parsers' tag CSR, or nullptr
    const uint64_t* span_off;
    const uint8_t* tag_bytes;
    uint8_t* out; uint64_t capacity;
    uint64_t* out_off;          // [S+1]
    uint32_t* status;
};
hipError_t launch_write_partial(const WritePartialParams& P, uint64_t* scan_part, hipStream_t stream);
// the counters of evaluate/src/main.rs:124-191, ADDED to counts[kEvalCounts]: tp, tn, fp, fn, n_sys, n_ref, n_cor, n_sentences
constexpr uint32_t kEvalCounts = 8;
constexpr uint32_t kEvalTagsNone = 0, kEvalTagsGold = 1, kEvalTagsPredicted = 2;
constexpr uint32_t kWordBoundary = 1;
struct EvalParams {
    const uint8_t* gold;        // [total boundaries]
    const uint8_t* sys;         // [total boundaries]
    const uint64_t* ooff;       // [S+1]
    uint64_t n_sent;
    const uint32_t* gold_n_tags;   // [S]
    const uint64_t* tag_index;  // gold tags (ParseParams)
    const uint64_t* span_off;
    const uint8_t* tag_bytes;
    uint32_t mode;              // kEvalTags*: the system's tag vectors are empty / the gold ones / fill_tags' records
    TagRecordsView sys_tags;    // kEvalTagsPredicted: the records fill_tags left on the workspace (n_tags: the predictor's)
    uint64_t* counts;
};
hipError_t launch_evaluate(const EvalParams& P, hipStream_t stream);

size_t score_tiles_lds_bytes();
hipError_t launch_assign_tiles(const uint64_t* ooff, uint64_t n_sent, int pad, uint32_t tile_flat, uint32_t n_tiles,
                               uint32_t* tile_first, uint32_t* ctrl, hipStream_t stream);
// specialised kernel (kernels_fast.hip): packed tables (windows up to 8, BMP, i16), type rows, the type window table (row window 3) or none
bool fast_path_supported(const ScoreParams& P);
int fast_path_cap(const ScoreParams& P);   // flat positions per tile / workgroups per CU of the instance that scores P
int fast_path_wg(const ScoreParams& P);
size_t score_tiles_fast_lds_bytes(const ScoreParams& P);
hipError_t launch_score_tiles_fast(const ScoreParams& P, uint32_t n_tiles, hipStream_t stream);
// its tiles: whole sentences (launch_assign_tiles, as for the general kernel; ScoreParams::tiles stays nullptr) or cut anywhere: lead-byte counts per 256-byte block of the text (cut_local: exclusive inside a superblock of 256 blocks,
// cut_super: exclusive over the superblocks; sized from cut_index_entries), then the tiles
struct CutGeometry { uint32_t tile_flat, halo_left, halo_right, cap_eff, mis /* text pointer & 15 */, pad /* separator slots */, cap /* the kernel's tile */; };
void cut_index_entries(uint64_t total_chars_bound, size_t* n_local, size_t* n_super);
hipError_t launch_assign_tiles_cut(const ScoreParams& P, const CutGeometry& G, uint32_t n_tiles, uint64_t total_chars_bound, uint32_t* cut_local,
                                   uint64_t* cut_super, TileDesc* tiles, uint32_t* ctrl, hipStream_t stream);
hipError_t launch_score_tiles(const ScoreParams& P, int chunks, uint32_t n_tiles, hipStream_t stream);
hipError_t launch_score_slow(const ScoreParams& P, int chunks, uint32_t n_blocks, hipStream_t stream);

// boundary-model training (kernels_train.hip)
constexpr uint32_t kCharMaskTrain = 0x1FFFFFu;   // the scalar value of a decode_chars cps word (scored | CharacterType << 24)
// TrainKey: kind << 120 | c0 << 99 | c1 << 78 | c2 << 57 | c3 << 36 | c4 << 15 | len << 5 | (rel_position + 16), as two words (low, high)
// (kind 0 char n-gram, 1 type n-gram, 2 dictionary word: c0 = min(len, dictn), c1 = 0 Left / 1 Inside / 2 Right, len = 0, rel = -16;
// the tag trainer's keys hold the context alone: left of the token, then right, rel = chars to the right)
struct TrainKey {
    uint32_t kind, c[5], len;
    int32_t rel;
};
VPT_HD uint32_t train_key_shift(uint32_t k) {
    const uint32_t sh[5] = {99, 78, 57, 36, 15};
    return sh[k];
}
// the key of fields c[0 .. n) into keys[2 * at], keys[2 * at + 1]
VPT_HD void put_train_key(uint64_t* keys, uint64_t at, uint32_t kind, const uint32_t* c, uint32_t n, uint32_t len, int32_t rel) {
    unsigned __int128 v = ((unsigned __int128)kind << 120) | ((len << 5) | uint32_t(rel + 16));
    for (uint32_t k = 0; k < n; ++k) v |= (unsigned __int128)(c[k] & kCharMaskTrain) << train_key_shift(k);
    keys[2 * at] = uint64_t(v);
    keys[2 * at + 1] = uint64_t(v >> 64);
}
inline TrainKey train_key(uint64_t lo, uint64_t hi) {
    const unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
    TrainKey k{uint32_t(v >> 120) & 3u, {}, uint32_t(v >> 5) & 7u, int32_t(uint32_t(v) & 31u) - 16};
    for (uint32_t q = 0; q < 5; ++q) k.c[q] = uint32_t(v >> train_key_shift(q)) & kCharMaskTrain;
    return k;
}
// The hash of a string of code points, char by char (the dictionary's table, compiled on the host and probed on the device, and the
// surfaces' table): FNV-1a over the chars, finished with the length through mix64 (which also spreads the words of a key).
constexpr uint64_t kCpsHashSeed = 0xCBF29CE484222325ull;
VPT_HD uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    return x ^ (x >> 33);
}
VPT_HD uint64_t cps_hash_step(uint64_t h, uint32_t cps_word) { return (h ^ (cps_word & kCharMaskTrain)) * 0x100000001B3ull; }
VPT_HD uint64_t cps_hash_finish(uint64_t h, uint64_t len) { return mix64(h ^ len); }
struct TrainFeatParams {
    const uint32_t* cps;        // decode_chars' words: sentence i's char c at ooff[i] + i + c
    const uint64_t* ooff;       // [n_sent + 1] vpt_count_boundaries' layout
    uint64_t n_sent, total_b;
    uint32_t charw, charn, typew, typen, dictn, dict_maxlen;
    const uint32_t* dict_slots; // open addressing by the hash of (code points, length): word index + 1, 0 empty
    uint64_t dict_mask;         // slots - 1; 0: no dictionary
    const uint32_t* dict_cps;   // the words' code points, word w at dict_off[w] .. dict_off[w + 1]
    const uint64_t* dict_off;
    uint32_t* counts;           // count pass: features per boundary
    const uint64_t* row_off;    // emit pass: where boundary b's keys start
    uint64_t* keys;             // emit pass: two words per key (low, high)
};
hipError_t train_features(const TrainFeatParams& P, bool emit, hipStream_t st);
hipError_t train_check_labels(const uint8_t* labels, uint64_t n, uint32_t* status, hipStream_t st);   // ORs kErrBadLabel for a label above 2
uint64_t train_scan_scratch(uint64_t n);
hipError_t train_scan(const uint32_t* in, uint64_t n, uint64_t* out, uint64_t* scratch, hipStream_t st);   // out[n + 1], exclusive
hipError_t train_scan(const uint64_t* in, uint64_t n, uint64_t* out, uint64_t* scratch, hipStream_t st);
// Distinct items and their ranks: every item finds (or becomes) the representative of its equals through an open-addressing table
// (rep[i]; flag[i] = 1 at a representative), the representatives are compacted in order of first occurrence (slot[i] = where, at a
// representative) and sorted by the caller, and train_ids maps every item to its representative's rank.  Keys here, surfaces below.
hipError_t train_insert(const uint64_t* keys, uint64_t nnz, uint64_t* table, uint64_t mask, uint32_t* rep, uint32_t* flag, hipStream_t st);
hipError_t train_compact(const uint64_t* keys, const uint32_t* rep, const uint64_t* pos, uint64_t nnz, uint64_t* dkeys, uint32_t* slot, hipStream_t st);
uint64_t train_radix_scratch(uint64_t n);
// word_shifts[p] = u32 word << 8 | bit shift of pass p (least significant digit first)
hipError_t train_radix_sort(const uint32_t* base, uint32_t stride, const uint32_t* word_shifts, uint32_t n_passes, uint64_t n, uint32_t* idx,
                            uint32_t* idx_tmp, uint64_t* hist, uint64_t* hist_scan, uint64_t* scan_scratch, hipStream_t st);
// the nd distinct items ranked by their place in `order`, then ids[i] = rank[slot[rep[i]]] for the n items
hipError_t train_ids(const uint32_t* order, uint64_t nd, uint32_t* rank, const uint32_t* rep, const uint32_t* slot, uint64_t n, uint32_t* ids, hipStream_t st);
hipError_t train_sorted_keys(const uint64_t* dkeys, const uint32_t* order, uint64_t nd, uint64_t* sorted_keys, hipStream_t st);
hipError_t train_row_sort(uint32_t* ids, const uint64_t* row_off, uint64_t nrows, uint32_t* merged, hipStream_t st);
hipError_t train_row_merge(const uint32_t* ids, const uint64_t* row_off, const uint64_t* csr_ptr, uint64_t nrows, uint32_t* cols, uint16_t* vals,
                           uint32_t* rows, uint32_t* status, hipStream_t st);
hipError_t train_csc_fill(const uint32_t* order, const uint32_t* cols, const uint16_t* vals, const uint32_t* rows, uint64_t nnz, uint32_t* crow,
                          uint16_t* cval, uint64_t* cptr, hipStream_t st);
hipError_t train_seg_count(const uint64_t* ptr, uint64_t nd, uint64_t* cnt, hipStream_t st);
hipError_t train_seg_col(const uint64_t* nptr, uint64_t nd, uint32_t* seg_col, hipStream_t st);
hipError_t train_xv(const uint64_t* csr_ptr, const uint32_t* cols, const uint16_t* vals, uint64_t nrows, const double* v, uint64_t bias_col, double* out,
                    hipStream_t st);
hipError_t train_xtv_level(const uint64_t* ptr, const uint64_t* nptr, const uint32_t* seg_col, uint64_t nseg, const double* in, const uint32_t* crow,
                           const uint16_t* cval, const double* u, double* out, hipStream_t st);
uint64_t train_dot_partials(uint64_t n);
hipError_t train_dot(const double* a, const double* b, uint64_t n, double* partial, hipStream_t st);
hipError_t train_axpy(uint64_t n, double alpha, const double* x, double* y, hipStream_t st);
hipError_t train_xpby(uint64_t n, const double* x, double beta, double* y, hipStream_t st);
hipError_t train_add(uint64_t n, const double* a, const double* b, const double* bias_sum, double* y, hipStream_t st);
hipError_t train_scale_rows(uint64_t n, const double* d, double* t, hipStream_t st);
hipError_t train_loss(uint64_t n, const double* z, const double* y, double c, int solver, double* loss, hipStream_t st);
hipError_t train_grad_rows(uint64_t n, const double* z, const double* y, double c, int solver, double* gz, double* D, hipStream_t st);

// solver 5 (kernels_train_l1.hip): coordinate descent over a group of columns that share no row, one launch a group
constexpr uint32_t kL1rLaneMax = 64;     // nonzeros of a column a lane takes; a wave takes one of at most kL1rWaveMax, a workgroup a longer one
constexpr uint32_t kL1rWaveMax = 1024;   // (picked, not measured)
struct L1rPair;
struct L1rParams {
    const uint64_t* cptr;       // the CSC copy of the design matrix; column nd is the bias: every row, value 1
    const uint32_t* crow;
    const uint16_t* cval;
    uint64_t nd, nr, nnz;
    const double* y;            // [nr] +1 / -1
    double* b;                  // [nr] 1 - y w.x
    double* w;                  // [nd + 1]
    double* xj_sq;              // [nd + 1] C sum x^2 (written by the init launch)
    double* viol;               // [nd + 1] the columns' violations of this sweep
    uint32_t* halvings;         // one counter over the training
    L1rPair *tile0, *tile1;     // the workgroups' level sums: train_l1r_scratch(.., 0) and (.., 1) elements
    double c;
};
uint64_t train_l1r_scratch(uint64_t nnz, uint64_t nr, uint64_t nd, int level);
// cols[0 .. n_lane + n_wave + n_block): the group's columns in that order of length class; init: xj_sq alone
hipError_t train_l1r_group(const L1rParams& P, bool init, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block, hipStream_t st);

// solver 6 (kernels_train_l1lr.hip): the device backend of l1r_lr.h; columns by length class as train_l1r_group takes them, the
// workgroups' level sums in tile0 / tile1 of train_l1r_scratch's sizes
struct L1lrParams {
    const uint64_t* cptr;       // the CSC copy of the design matrix; column nd is the bias: every row, value 1
    const uint32_t* crow;
    const uint16_t* cval;
    uint64_t nd, nr, nnz;
    const double* y;            // [nr] +1 / -1
    double *e, *tau, *D, *xTd;  // [nr] exp(w.x), C / (1 + e), C e / (1 + e)^2, x.(wpd - w)
    double *w, *wpd;            // [nd + 1]
    double *hdiag, *grad;       // [nd + 1] of this Newton iteration
    double* xjneg;              // [nd + 1] C sum_{y = -1} x
    double* viol;               // [nd + 1] the columns' violations of the last grad launch or sweep
    L1rPair *tile0, *tile1;
    double c;
};
// all columns in one launch: xjneg (neg_sum) or hdiag, grad and viol at w
hipError_t train_l1lr_grad(const L1lrParams& P, bool neg_sum, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block, hipStream_t st);
// a group's columns of an inner sweep: wpd, xTd and viol
hipError_t train_l1lr_cd_group(const L1lrParams& P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block, hipStream_t st);
hipError_t train_l1lr_start(const L1lrParams& P, bool setup, hipStream_t st);   // xTd = 0; setup: e = 1 too
hipError_t train_l1lr_accept(const L1lrParams& P, hipStream_t st);              // e *= exp(xTd), tau and D from it
hipError_t train_l1lr_ls_terms(const L1lrParams& P, double* out, hipStream_t st);    // [nr] the line search's row terms
hipError_t train_l1lr_neg_terms(const L1lrParams& P, double* out, hipStream_t st);   // [nr] C xTd where y = -1
hipError_t train_l1lr_exp(uint64_t n, double* z, hipStream_t st);               // z = exp(z)
// [nd + 1] Grad_j (wpd_j - w_j) (delta NULL: skipped) and |wpd_j|
hipError_t train_l1lr_feat_terms(const L1lrParams& P, double* delta, double* norm1, hipStream_t st);
hipError_t train_l1lr_halve(const L1lrParams& P, hipStream_t st);               // wpd = (w + wpd) / 2, xTd /= 2

// tag-model training (kernels_train_tags.hip)
struct TagFeatParams {
    const uint32_t* cps;        // decode_chars' words: sentence i's char c at ooff[i] + i + c
    const uint64_t* ooff;       // [n_sent + 1]
    const uint8_t* labels;      // sentence i's boundary b at ooff[i] + b
    const uint32_t* n_tags;     // [n_sent] Sentence::n_tags
    uint64_t n_sent, total_chars;
    uint32_t charn, typen;
    uint32_t* is_ex;            // count pass: 1 where a token with tag slots ends at the char
    uint32_t* counts;           // count pass: that token's features
    const uint64_t* ex_off;     // emit pass: the scans of the two
    const uint64_t* key_off;
    uint32_t* recs;             // emit pass: per example (sentence, start, end, features)
    uint64_t* keys;             // emit pass: two words per key (low, high)
};
hipError_t train_tag_features(const TagFeatParams& P, bool emit, hipStream_t st);
hipError_t train_tag_validate(const uint32_t* n_tags, const uint64_t* ooff, uint64_t n_sent, uint64_t total_chars, const uint64_t* tag_index,
                              const uint64_t* span_off, uint64_t n_spans, uint64_t n_tag_bytes, uint32_t* status, hipStream_t st);
// the trainer's example records: (first char in its char pool, chars, first key, keys)
hipError_t train_tag_rec_finish(const uint32_t* recs, uint64_t n_ex, const uint64_t* ooff, const uint64_t* key_off, uint32_t cps_base, uint32_t key_base,
                                uint32_t* out, hipStream_t st);
// surface ids: representatives by a hash table, the distinct surfaces as a padded matrix (radix-sorted by the caller), ids by train_ids
hipError_t train_surf_insert(const uint32_t* ex, uint64_t n_ex, const uint32_t* cps, uint64_t* table, uint64_t mask, uint32_t* rep, uint32_t* flag,
                             uint32_t* maxlen, hipStream_t st);
hipError_t train_surf_matrix(const uint32_t* ex, uint64_t n_ex, const uint32_t* flag, const uint64_t* pos, const uint32_t* cps, uint32_t maxlen,
                             uint32_t* mat, uint32_t* slot, hipStream_t st);
// all problems' matrices over concatenated arrays: occ_off NULL counts a row's keys into nk_or_occ, else writes the (key, problem) records
hipError_t train_tag_expand(const uint32_t* row_ex, const uint32_t* row_prob, uint64_t n_rows, const uint32_t* ex, const uint64_t* occ_off,
                            const uint64_t* keys, uint32_t* nk_or_occ, uint32_t* occ_row, hipStream_t st);
hipError_t train_tag_flags(const uint32_t* occ, const uint32_t* order, uint64_t n, uint32_t* flag, hipStream_t st);
struct TagBuildParams {
    uint64_t n_prob, n_rows, n_occ;
    const uint64_t* prob_row_ptr;   // [n_prob + 1] the problems' rows
    const uint32_t* row_prob;       // [n_rows]
    const uint64_t* occ_off;        // [n_rows + 1] the rows' occurrences
    const uint32_t* occ;            // [5 * n_occ] (key, problem)
    const uint32_t* occ_row;        // [n_occ]
    const uint32_t* order;          // [n_occ] sorted by (problem, key), stable
    const uint32_t* flag;           // [n_occ] first of its key
    const uint64_t* dpos;           // [n_occ + 1] exclusive scan of flag
    uint64_t *prob_occ0, *key_ptr;  // out [n_prob + 1]
    uint32_t* occ_col;              // out [n_occ] the CSR's columns (rows sorted)
    uint64_t* dkeys;                // out [2 * distinct] the problems' sorted keys, back to back
    uint32_t *rp, *cp, *crow;       // out: row pointers [n_rows + n_prob], column pointers [distinct + n_prob], CSC rows [n_occ]
};
hipError_t train_tag_assemble(const TagBuildParams& B, hipStream_t st);
// the in-kernel solver keeps 7 vectors of features + 1 and 3 of rows in LDS
constexpr uint32_t kTagLdsDoubles = 7424;
struct TagSolveDesc {
    uint64_t rp, cols, cp, y, w, stats;   // where the problem's row pointers, nonzeros (CSR and CSC alike), column pointers, labels, weights and stats start
    uint32_t nf, l, k, pad;               // features (the bias is one more), rows, classes
};
bool train_tag_fits(uint64_t rows, uint64_t features);
hipError_t train_tag_solve(const TagSolveDesc* descs, uint32_t n_prob, const uint32_t* rp, const uint32_t* cols, const uint32_t* cp, const uint32_t* crow,
                           const uint32_t* y, double eps, double cost, int solver, double* w, vpt_train_stats* stats, hipStream_t st);

// solver 5 for tag problems (kernels_train_tags_l1.hip): the in-kernel solver keeps w (features + 1) and b (rows) in LDS and nothing
// else of the problem's size, so a problem fits iff (features + 1) + rows <= kTagL1LdsDoubles; the rest of tag_solve_kernel's 61568
// bytes holds the level sums of the summation rule, the groups' order and the halvings
constexpr uint32_t kTagL1LdsDoubles = 7256;
constexpr uint32_t kTagL1MaxGroups = 64;   // templates of a kind: 20 with n-grams of up to 5 symbols; two kinds and the bias: 41
struct TagL1Group {
    uint32_t at, n_lane, n_wave, n;        // the group's columns gcols[at .. at + n): those a lane takes, then a wave's, then the workgroup's
};
struct TagL1Desc {                         // beside a problem's TagSolveDesc
    uint64_t gcols, groups, viol;          // where its columns by group, its groups and its features + 1 violations start
    uint32_t n_groups, pad;
};
bool train_tag_l1_fits(uint64_t rows, uint64_t features);
hipError_t train_tag_l1_solve(const TagSolveDesc* descs, const TagL1Desc* l1descs, uint32_t n_prob, const uint32_t* rp, const uint32_t* cols,
                              const uint32_t* cp, const uint32_t* crow, const uint32_t* y, const uint32_t* gcols, const TagL1Group* groups, double eps,
                              double cost, double* viol, double* w, vpt_train_stats* stats, hipStream_t st);

// solver 6 for tag problems (kernels_train_tags_l1lr.hip): the in-kernel newGLMNET keeps in LDS what a sweep gathers or scatters per
// nonzero and the feature vector it writes -- tau, D and xTd (rows each) and wpd (features + 1) -- so a problem fits iff
// 3 rows + (features + 1) <= kTagL1LdsDoubles; w is the output itself, and Grad, Hdiag, xjneg_sum, the violations (features + 1 each)
// and e (rows) are train_tag_l1lr_scratch doubles of global memory per problem, which start at its TagL1Desc's `viol`.  Groups and
// descriptors are solver 5's.
bool train_tag_l1lr_fits(uint64_t rows, uint64_t features);
uint64_t train_tag_l1lr_scratch(uint64_t rows, uint64_t features);
hipError_t train_tag_l1lr_solve(const TagSolveDesc* descs, const TagL1Desc* l1descs, uint32_t n_prob, const uint32_t* rp, const uint32_t* cols,
                                const uint32_t* cp, const uint32_t* crow, const uint32_t* y, const uint32_t* gcols, const TagL1Group* groups, double eps,
                                double cost, double* scratch, double* w, vpt_train_stats* stats, hipStream_t st);

}  // namespace vpt
