/*
 * vaporetto_hip.h -- C ABI of the MI355X-native Vaporetto boundary scorer (libvaporetto_hip.so).
 *
 * The reference (daac-tools/vaporetto) has no FFI: its boundary is the public Rust API of the `vaporetto`
 * crate (/root/reference/vaporetto/src/lib.rs:82-91).  Each entry point below names the reference item it
 * stands in for; INTEGRATION.md shows the Rust `extern "C"` block and the `Predictor`/`Sentence` shim a
 * maintainer would add on top.  Plain pointers and sizes only; no torch, no C++ types.
 *
 * Conventions
 *   - every function returns a vpt_status; vpt_last_error() gives the message of the calling thread's last
 *     failure (VaporettoError's Display text where the reference defines one, errors.rs:15-38);
 *   - a vpt_predictor is immutable after creation and may be shared by any number of host threads
 *     (mirrors `&self` in Predictor::predict, predictor.rs:518); all mutable state lives in the caller's
 *     buffers or in a per-caller vpt_batch workspace (mirrors the caller-owned `Sentence`);
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails with
 *     VPT_RUNTIME_ERROR.
 */
#ifndef VAPORETTO_HIP_H
#define VAPORETTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vpt_status {
    VPT_OK = 0,
    VPT_INVALID_MODEL = 1,    /* VaporettoError::InvalidModel / DecodeError   (errors.rs:15-38) */
    VPT_INVALID_ARGUMENT = 2, /* VaporettoError::InvalidArgument              (errors.rs:15-38) */
    VPT_RUNTIME_ERROR = 3     /* HIP / device failure, or no device */
} vpt_status;

/* CharacterBoundary discriminants written to `labels` (sentence.rs:70-82) */
enum { VPT_NOT_WORD_BOUNDARY = 0, VPT_WORD_BOUNDARY = 1, VPT_BOUNDARY_UNKNOWN = 2 };

/* Flags of the *_flags entry points and of vpt_batch_set_flags.
 * VPT_FLAG_KYTEA_FULLWIDTH: score the text as KyteaFullwidthFilter would rewrite it
 *   (vaporetto_rules/src/string_filters/kytea_fullwidth.rs:13-117: a 1:1 char map, so boundaries keep their places);
 *   this is what the reference's CLI does before update_raw unless --no-norm is given (predict/src/main.rs:126-129),
 *   folded into the kernel's char classification table at no extra cost. */
enum { VPT_FLAG_KYTEA_FULLWIDTH = 1 };
/* Post-filters on the LABELS (scores are never touched), applied in this order after the sign threshold:
 * VPT_FLAG_WSCONST(t), t = CharacterType 1..6: KyteaWsConstFilter::new(t) -- a boundary between two chars of type t
 *   becomes NotWordBoundary (vaporetto_rules/src/sentence_filters/kytea_wsconst.rs:26-43; the CLI's --wsconst);
 * VPT_FLAG_SPLIT_LINEBREAKS: SplitLinebreaksFilter -- a boundary next to '\r' or '\n' becomes WordBoundary
 *   (vaporetto_rules/src/sentence_filters/split_linebreaks.rs:9-36).
 * Types are those of the scored text (after VPT_FLAG_KYTEA_FULLWIDTH, as in the CLI). */
#define VPT_FLAG_WSCONST(char_type) (1u << (char_type))
enum { VPT_FLAG_SPLIT_LINEBREAKS = 1 << 7, VPT_FLAG_ALL = 0xFF };
/* VPT_FLAG_LINEBREAKS_FIRST (with VPT_FLAG_SPLIT_LINEBREAKS; vpt_predict_batch_flags and vpt_batch_set_flags take it): SplitLinebreaksFilter runs BEFORE
 * the VPT_FLAG_WSCONST filters instead of after them -- the order of vaporetto_tantivy's post-filters (vaporetto_tantivy/src/lib.rs:69-86).  It
 * shows where a linebreak stands next to a char of its own type under its wsconst flag ('\n', '\r' and ' ' are Other): "a\n\nb" with
 * VPT_FLAG_WSCONST(6) gives a | \n\n | b with this bit, a | \n | \n | b without.  Not part of VPT_FLAG_ALL. */
enum { VPT_FLAG_LINEBREAKS_FIRST = 1 << 8 };
/* VPT_FLAG_CONCAT_GRAPHEMES: ConcatGraphemeClustersFilter (vaporetto_rules/src/sentence_filters/concat_grapheme_clusters.rs:10-36; the `G` of
 * --wsconst and of the tantivy adapter) -- every label inside an extended grapheme cluster (UAX #29) of the text as it was scored (the
 * KyteaFullwidthFilter image under VPT_FLAG_KYTEA_FULLWIDTH) becomes NotWordBoundary, Unknown labels included.  A launch of its own behind the
 * scoring launch, position-parallel (vaporetto_amd/csrc/kernels_graphemes.hip).  It and the VPT_FLAG_WSCONST filters only clear labels and
 * commute; SplitLinebreaksFilter sets them, so the order matters there, and on the device this filter always runs LAST:
 *   with VPT_FLAG_LINEBREAKS_FIRST   split, wsconst, graphemes -- the tantivy adapter's result for any place of `G` in its string
 *                                    (vaporetto_tantivy/src/lib.rs:69-86): "\r\n" stays joined;
 *   without it                       wsconst, split, graphemes.
 * A caller that wants another order runs vpt_concat_graphemes_batch[_device] (below) between calls of its own.  Accepted wherever the label
 * post-filter flags are (vpt_predict_batch_flags, vpt_batch_set_flags, vpt_tokenize_batch, vpt_predict_listing_batch, vpt_evaluate_batch,
 * vpt_predict_batch_sharded, and as a bit of vpt_token_stream_batch's wsconst_flags).  Not part of VPT_FLAG_ALL.  The classes are those of
 * include/vaporetto_grapheme_tables.inc. */
enum { VPT_FLAG_CONCAT_GRAPHEMES = 1 << 9 };

typedef struct vpt_predictor vpt_predictor;
typedef struct vpt_batch vpt_batch;

/* Message of the calling thread's most recent failed call ("" if none). Never NULL. */
const char *vpt_last_error(void);

/* Library version string. */
const char *vpt_version(void);

/* ---------------------------------------------------------------------------------------------------------
 * Model::read_slice + Predictor::new            (model.rs:127-135, predictor.rs:450-508)
 *
 * model_bytes : an un-compressed model file: "VaporettoTokenizer 0.5.0\n" + bincode (zstd is outside the
 *               API in the reference too, README.md:50-63).  The bytes are copied; the caller may free them.
 * predict_tags: as Predictor::new's flag.  Tag models are parsed and validated; boundary scores are
 *               identical either way; tag scoring itself is vpt_fill_tags_batch below.
 * device_id   : HIP device ordinal.
 * Errors      : VPT_INVALID_MODEL  "model version mismatch" | decode error | "failed to build the automaton"
 *               (empty pattern) | "invalid character type n-grams" (empty/duplicate type n-gram, cache
 *               variant, boundary_scorer_cache.rs:23-24) | "words must be shorter than or equal to 32767
 *               characters" | weight vector longer than its pattern allows | a tag n-gram whose rel_position exceeds
 *               the window (model contract);
 *               VPT_RUNTIME_ERROR when the device cannot be used.
 */
vpt_status vpt_predictor_create(const uint8_t *model_bytes, size_t len, int predict_tags, int device_id,
                                vpt_predictor **out);
void vpt_predictor_destroy(vpt_predictor *p);

/* ---------------------------------------------------------------------------------------------------------
 * The compiled predictor: Predictor::serialize_to_vec / deserialize_from_slice_unchecked   (predictor.rs:640-664)
 *
 * Compiling a bccwj-suw+unidic-sized model takes seconds; the result -- every device table plus a fixed-size
 * description -- can be saved and loaded back without the model (a format of this library: not the reference's
 * daachorse-internal one, and only valid for the library version that wrote it; like the reference's *_unchecked
 * loader it trusts the bytes beyond a version check and a checksum), and copied from one GPU to another device to
 * device (xGMI between the GPUs of a node), which is how the ranks of a multi-GPU job get their predictor.
 *
 * vpt_predictor_save : *needed = the size of the compiled form; with out == NULL only that; else capacity must cover it.
 * vpt_predictor_load : VPT_INVALID_MODEL "not a compiled predictor" | "... version mismatch" | "... truncated" |
 *                      "... corrupt (checksum)".
 * vpt_predictor_clone_to_device: a predictor on device_id with the same tables (hipMemcpyPeer; same device: a copy). */
vpt_status vpt_predictor_save(const vpt_predictor *p, uint8_t *out, size_t capacity, size_t *needed);
vpt_status vpt_predictor_load(const uint8_t *blob, size_t len, int device_id, vpt_predictor **out);
vpt_status vpt_predictor_clone_to_device(const vpt_predictor *src, int device_id, vpt_predictor **out);
/* For one process per GPU: vpt_predictor_describe gives the fixed-size description (meta_out may be NULL to ask for its size)
 * and the device address and size of the table arena; the caller moves those bytes to the other ranks' GPUs itself -- one
 * RCCL broadcast over xGMI -- and every rank turns what it received into a predictor with vpt_predictor_adopt_device
 * (device-to-device copy into an allocation the predictor owns; d_arena stays the caller's). */
vpt_status vpt_predictor_describe(const vpt_predictor *p, uint8_t *meta_out, size_t capacity, size_t *meta_bytes,
                                  const void **d_arena, size_t *arena_bytes);
vpt_status vpt_predictor_adopt_device(const uint8_t *meta, size_t meta_len, const void *d_arena, size_t arena_bytes,
                                      int device_id, vpt_predictor **out);

/* ---------------------------------------------------------------------------------------------------------
 * Sentence::from_raw's bookkeeping for a batch     (sentence.rs:160-196)
 *
 * Sentence i is utf8[byte_offsets[i] .. byte_offsets[i+1]) (valid UTF-8, as a Rust &str always is).
 * Writes out_offsets[0..S]: out_offsets[i] = sum_{j<i} (chars(j) - 1), i.e. where sentence i's n-1 boundary
 * scores start in the flat output arrays.  Host-only, no device needed.
 * Errors: VPT_INVALID_ARGUMENT "text: must contain at least one character" | "text: must not contain NULL".
 */
vpt_status vpt_count_boundaries(const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences,
                                uint64_t *out_offsets);

/* ---------------------------------------------------------------------------------------------------------
 * Predictor::predict over a batch of sentences, host buffers     (predictor.rs:518-543)
 *
 * scores_out[out_offsets[i] + b] = boundary score b of sentence i (what Sentence::boundary_scores() returns,
 * sentence.rs:1040-1046); labels_out likewise (Sentence::boundaries(), sentence.rs:993).  Either output
 * pointer may be NULL.  out_offsets must come from vpt_count_boundaries.  Copies H2D, launches, copies D2H,
 * synchronises.  Thread-safe on a shared predictor.
 */
vpt_status vpt_predict_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                             size_t n_sentences, int32_t *scores_out, uint8_t *labels_out,
                             const uint64_t *out_offsets);

/* The same with VPT_FLAG_* (0 = exactly vpt_predict_batch). */
vpt_status vpt_predict_batch_flags(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                                   size_t n_sentences, int32_t *scores_out, uint8_t *labels_out,
                                   const uint64_t *out_offsets, unsigned flags);

/* Host buffers and the PCIe link.  vpt_predict_batch cuts a large batch into chunks and runs the copy in of one chunk, the
 * kernels of another and the copy out of a third at the same time: up to 16 M chars as 512 K-char chunks alternating over four
 * streams (a chunk's copy in, kernels and copy out in order on one of them), larger batches as 4 M-char chunks on a copy-in, a
 * compute and a copy-out stream.  Either output pointer may be NULL: a caller that only needs the labels saves four of the
 * five bytes per boundary that cross the link back.  With PINNED caller buffers -- vpt_host_alloc, or memory the caller registered with HIP
 * itself -- the copies are DMA transfers in both directions at once; with pageable buffers they go through the runtime's
 * staging.  vpt_host_alloc / vpt_host_free = hipHostMalloc / hipHostFree, exported so that callers need no HIP headers. */
vpt_status vpt_host_alloc(size_t bytes, void **out);
void vpt_host_free(void *ptr);

/* Predictor::predict over ONE batch on SEVERAL GPUs of a node: the batch is cut into n_preds contiguous sentence ranges of
 * about equal CHARACTER count (vpt_shard_bounds), range r is scored by preds[r] (normally vpt_predictor_clone_to_device
 * copies of one predictor) on a host thread of its own and written straight into its slice of scores_out / labels_out.
 * Sentences are independent (predictor.rs:518-543 keeps no state between calls), so there is no exchange step.
 * Arguments as for vpt_predict_batch_flags.  Mirrors how vaporetto_tantivy shares one Arc<Predictor> between indexing
 * threads (vaporetto_tantivy/src/lib.rs:62-67), with one device per thread. */
vpt_status vpt_predict_batch_sharded(const vpt_predictor *const *preds, size_t n_preds, const uint8_t *utf8,
                                     const uint64_t *byte_offsets, size_t n_sentences, int32_t *scores_out,
                                     uint8_t *labels_out, const uint64_t *out_offsets, unsigned flags);
/* bounds[0 .. n_shards]: shard r = sentences bounds[r] .. bounds[r+1], balanced by chars (host only). */
vpt_status vpt_shard_bounds(const uint64_t *out_offsets, size_t n_sentences, size_t n_shards, uint64_t *bounds);

/* Sentence::char_types for a batch (sentence.rs:1016; CharacterType::get_type, sentence.rs:50-67), computed on the device:
 * types_out[out_offsets[i] + i + c] = CharacterType (1..6) of char c of sentence i; flags: VPT_FLAG_KYTEA_FULLWIDTH gives the
 * types of the normalised text.  The *_device variant: device pointers, asynchronous, flags from vpt_batch_set_flags. */
vpt_status vpt_char_types_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                                size_t n_sentences, const uint64_t *out_offsets, unsigned flags, uint8_t *types_out);
vpt_status vpt_char_types_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8,
                                       const uint64_t *d_byte_offsets, const uint64_t *d_out_offsets,
                                       size_t n_sentences, uint64_t total_boundaries, uint8_t *d_types_out,
                                       void *hip_stream);

/* Sentence::from_raw + Predictor::predict for one sentence (same path, batch of one).
 * scores/labels need room for chars-1 entries (<= len-1). */
vpt_status vpt_predict_one(const vpt_predictor *p, const uint8_t *utf8, size_t len, int32_t *scores,
                           uint8_t *labels, size_t *n_boundaries);

/* ---------------------------------------------------------------------------------------------------------
 * Device-resident variant: inputs and outputs already in HBM, asynchronous on a HIP stream.
 *
 * A vpt_batch is the per-caller mutable workspace (what a reused `Sentence` is to the reference's callers,
 * predict/src/main.rs:122,129): tile tables, the device error word, timing events.  One per host thread /
 * stream; not shareable between concurrent calls.
 */
vpt_status vpt_batch_create(const vpt_predictor *p, vpt_batch **out);
void vpt_batch_destroy(vpt_batch *b);

/* d_utf8, d_byte_offsets[S+1], d_out_offsets[S+1], d_scores, d_labels are device pointers (d_scores or
 * d_labels may be NULL).  total_boundaries = out_offsets[S] (the caller sized the outputs with it), or any upper bound of it
 * when the offsets were made on the device and the caller will not wait for them (text bytes - S always is one; the same bound
 * must then be passed to the fill_tags / write calls that follow on this batch).
 * max_sentence_bytes: an upper bound on the byte length of any sentence (sizes the long-sentence scratch).
 * hip_stream: a hipStream_t (NULL = default stream).  Returns after enqueueing; errors found on the device
 * (empty sentence, NUL char, offsets inconsistent with the text) are reported by vpt_batch_sync. */
vpt_status vpt_predict_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8,
                                    const uint64_t *d_byte_offsets, const uint64_t *d_out_offsets,
                                    size_t n_sentences, uint64_t total_boundaries, uint64_t max_sentence_bytes,
                                    int32_t *d_scores, uint8_t *d_labels, void *hip_stream);

/* Optional hint for the following vpt_predict_batch_device calls on this workspace: an upper bound on the number of
 * CHARACTERS of any sentence (0 = unknown: max_sentence_bytes is used, which is 3x pessimistic for Japanese text
 * and leaves the kernel's tiles about 10 % emptier).  An understated bound is reported by vpt_batch_sync like an
 * understated max_sentence_bytes. */
vpt_status vpt_batch_set_max_sentence_chars(vpt_batch *b, uint64_t max_sentence_chars);

/* VPT_FLAG_* for the following vpt_predict_batch_device calls on this workspace (default 0). */
vpt_status vpt_batch_set_flags(vpt_batch *b, unsigned flags);

/* Waits for the batch's last enqueued work and returns its device-side verdict. */
vpt_status vpt_batch_sync(vpt_batch *b);

/* Optional kernel timing: when enabled, vpt_predict_batch_device brackets the scoring kernel with HIP events
 * on the launch stream; after vpt_batch_sync, vpt_batch_kernel_ms returns that kernel's AVERAGE duration (ms)
 * over the calls made since the previous vpt_batch_kernel_ms (at most the 256 most recent) and the number of
 * workgroups (tiles) of the last call. */
/* How the last vpt_predict_batch_device call on this workspace cut its batch (diagnostics): the number of tiles, the flat
 * positions (chars + separators) a tile covers, and the kind -- 1 whole-sentence tiles, 2 tiles cut at any position with a halo
 * (batches with sentences too long for a tile), 0 the general kernels (models outside the packed shape). */
vpt_status vpt_batch_last_plan(const vpt_batch *b, uint32_t *n_tiles, uint32_t *tile_flat, uint32_t *kind);
/* The cache policy under which the last vpt_predict_batch_device call on this workspace loaded its text (diagnostics): 0 plain, 1 non-temporal.
 * The library chooses per launch from the bytes the launch streams (vpt_text_policy_for); the general kernels always load it plain. */
vpt_status vpt_batch_last_text_policy(const vpt_batch *b, uint32_t *policy);
/* The rule itself (a pure function of the host; diagnostics and tests): the policy of a launch that scores `text_bytes` of text with
 * `total_boundaries` boundaries and writes scores (4 bytes each) and / or labels (1 byte each), and the threshold the rule compares their
 * sum with.  Either pointer may be NULL. */
vpt_status vpt_text_policy_for(uint64_t text_bytes, uint64_t total_boundaries, int want_scores, int want_labels, uint32_t *policy,
                               uint64_t *threshold_bytes);
/* How the last vpt_fill_tags_batch_device call on this workspace cut its batch (diagnostics): the number of front-end runs and the
 * sentences of a run (the last run may hold fewer); both 0 before the first call.  Either pointer may be NULL. */
vpt_status vpt_batch_tag_plan(const vpt_batch *b, uint64_t *n_runs, uint32_t *run_sentences);
vpt_status vpt_batch_set_timing(vpt_batch *b, int enabled);
vpt_status vpt_batch_kernel_ms(vpt_batch *b, float *score_kernel_ms, uint32_t *n_tiles);
/* The individual durations (ms, oldest first) of the timed calls since the previous vpt_batch_kernel_ms, at most `capacity`
 * of the 256 most recent; *n_out = how many were written (with ms_out == NULL: how many there are).  Does not reset. */
vpt_status vpt_batch_kernel_times(vpt_batch *b, float *ms_out, size_t capacity, size_t *n_out);

/* ---------------------------------------------------------------------------------------------------------
 * Sentence::fill_tags -> Predictor::predict_tags over a batch     (sentence.rs:1144-1148, predictor.rs:546-637)
 *
 * The predictor must have been created with predict_tags != 0 (the reference panics otherwise, predictor.rs:548-551:
 * here VPT_INVALID_ARGUMENT "this predictor is created with predict_tags = false").
 * n_tags  = the largest number of tag slots of any tag model (predictor.rs:466); 0 when the model has no tag models.
 * labels  : CharacterBoundary per boundary, laid out like labels_out of vpt_predict_batch -- normally its output,
 *           possibly edited by the caller's post-filters (as predict/src/main.rs:130-134 does between predict and
 *           fill_tags); VPT_BOUNDARY_UNKNOWN is honoured (tokens touching it get no tags).
 * tags_out: int32 [(total boundaries + n_sentences) * n_tags]: for char c (0-based) of sentence i, slot j:
 *           tags_out[(out_offsets[i] + i + c) * n_tags + j] = index of the chosen candidate in the matching tag
 *           model's j-th candidate list (model.rs:41-47), or -1 (None).  Only the LAST char of a token carries tags
 *           (predictor.rs:595-598), like Sentence::tags(). */
vpt_status vpt_predictor_n_tags(const vpt_predictor *p, uint32_t *n_tags);
vpt_status vpt_fill_tags_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                               size_t n_sentences, const uint64_t *out_offsets, const uint8_t *labels,
                               int32_t *tags_out);
/* The same with VPT_FLAG_*: with VPT_FLAG_KYTEA_FULLWIDTH tokens and tag n-grams are matched on the normalised text,
 * as the CLI fills tags on the normalised sentence (predict/src/main.rs:156-170). */
vpt_status vpt_fill_tags_batch_flags(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                                     size_t n_sentences, const uint64_t *out_offsets, const uint8_t *labels,
                                     int32_t *tags_out, unsigned flags);

/* Device-resident variant of vpt_fill_tags_batch: all pointers are device pointers, asynchronous on `hip_stream`
 * (NULL = default stream).  d_labels as written by vpt_predict_batch_device (possibly edited by the caller's own
 * kernels).  The reference stores None for every char that does not end a token with a tag model (predictor.rs:558-573);
 * what this call leaves IN THE WORKSPACE is one record per token that HAS one (last char, tag model, chosen candidates),
 * sorted by position -- what vpt_write_tagged_batch_device reads.  d_tags_out: NULL (a tokenizer needs no more than the
 * records), or (total_boundaries + n_sentences) * n_tags int32 that receive the dense array described above (None = -1
 * everywhere else: a memset + a scatter of the records); vpt_expand_tags_batch_device makes it from the records later.
 * At most 2^32 - 257 chars per call.  The workspace keeps the decoded scalar values (4 bytes per char) between the
 * kernels; flags as set by vpt_batch_set_flags (fullwidth only).
 * When the call BEFORE this one on this workspace was vpt_predict_batch_device for the SAME buffers, sizes, flags and stream
 * (as Sentence::fill_tags follows Predictor::predict on the same sentence, predictor.rs:542), the chars that call decoded are
 * taken over and the decode kernel is skipped: do not rewrite d_utf8 in place between those two calls.  The chars are good
 * for that one call only, and only while no vpt_batch_sync lies between the two (a caller that waited for the device may have
 * rewritten its buffers): any other fill_tags call decodes the text it is given.
 * d_out_offsets that do not describe the text (out of order, past total_boundaries, not the chars the text holds) are an error reported
 * by vpt_batch_sync and never a write outside d_tags_out, the other arrays of the call or the workspace; the records such a call leaves are empty. */
vpt_status vpt_fill_tags_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8,
                                      const uint64_t *d_byte_offsets, const uint64_t *d_out_offsets,
                                      size_t n_sentences, uint64_t total_boundaries, const uint8_t *d_labels,
                                      int32_t *d_tags_out, void *hip_stream);
/* Sentence::tags() of the batch of the last vpt_fill_tags_batch_device call on this workspace (same n_sentences and
 * total_boundaries): d_tags_out, (total_boundaries + n_sentences) * n_tags int32, receives the dense array -- None (-1)
 * for every char but the last one of a token that has a tag model (predictor.rs:556-598).  Whatever offsets the fill_tags call was given,
 * nothing outside those (total_boundaries + n_sentences) * n_tags entries is written. */
vpt_status vpt_expand_tags_batch_device(const vpt_predictor *p, vpt_batch *b, size_t n_sentences, uint64_t total_boundaries,
                                        int32_t *d_tags_out, void *hip_stream);

/* ---------------------------------------------------------------------------------------------------------
 * Predictor::store_tag_scores(true) + Token::tag_candidates       (predictor.rs:510-514,599-601,632-634; sentence.rs:1218-1250)
 *
 * vpt_fill_tags_batch_flags, and besides the chosen candidates the i32 tag SCORES of every token that has a tag model --
 * the vector the reference keeps in sentence.tag_scores[i] when store_tag_scores is on: bias + the weights of the tag
 * n-grams that match around the token, laid out slot after slot over the slots with >= 2 candidates (a slot with one
 * candidate takes no entries; Token::tag_candidates reports score 0 for it).
 * vpt_predictor_tag_score_stride: the longest such vector over the predictor's tag models (0: none has scores).
 * tag_scores_out: int32 [(total boundaries + n_sentences) * stride] or NULL; row of char c of sentence i = out_offsets[i] + i + c;
 *                 the row of a token's LAST char holds its scores in entries [0, bias.len()); other rows read 0 (host variant)
 *                 or are left untouched (device variant).
 * tag_models_out: int32 [total boundaries + n_sentences] or NULL: index, in Model::tag_models order, of the tag model whose
 *                 token the token ending at that char is (the LAST one of a repeated token, predictor.rs:466-478); -1 where
 *                 no such token ends.  It says which rows of tag_scores_out are meaningful and whose candidate lists they score. */
vpt_status vpt_predictor_tag_score_stride(const vpt_predictor *p, uint32_t *stride);
vpt_status vpt_fill_tags_scores_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                                      size_t n_sentences, const uint64_t *out_offsets, const uint8_t *labels, unsigned flags,
                                      int32_t *tags_out, int32_t *tag_scores_out, int32_t *tag_models_out);
vpt_status vpt_fill_tags_scores_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8,
                                             const uint64_t *d_byte_offsets, const uint64_t *d_out_offsets,
                                             size_t n_sentences, uint64_t total_boundaries, const uint8_t *d_labels,
                                             int32_t *d_tags_out, int32_t *d_tag_scores_out, int32_t *d_tag_models_out,
                                             void *hip_stream);

/* ---------------------------------------------------------------------------------------------------------
 * Sentence::write_tokenized_text over a batch, boundary part                            (sentence.rs:850-886)
 *
 * Every sentence's tokens (the runs between WordBoundary labels, sentence.rs:1270-1300) joined by ' ', with a '\\' in
 * front of every ' ', '\\' and '/' of a surface -- what `vaporetto` prints for a model without tag models.  ("/tag"
 * suffixes are host-side strings: append them from vpt_fill_tags_batch's indices, as vaporetto_amd/api.py does.)
 * labels          : 0 / 1 per boundary, laid out like labels_out of vpt_predict_batch; VPT_BOUNDARY_UNKNOWN (only
 *                   partially annotated corpora have it, never predict) is VPT_INVALID_ARGUMENT.
 * text_out        : the tokenized sentences back to back, text_capacity bytes; 2 * (text bytes) + (chars) always
 *                   suffices.  Too small a capacity is VPT_INVALID_ARGUMENT, nothing useful is written.
 * text_offsets_out: [n_sentences + 1] byte range of every sentence's tokenized text in text_out. */
vpt_status vpt_write_tokenized_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                                     size_t n_sentences, const uint64_t *out_offsets, const uint8_t *labels,
                                     uint8_t *text_out, uint64_t text_capacity, uint64_t *text_offsets_out);
/* The whole of write_tokenized_text for a predictor with tag models: Sentence::fill_tags on the given labels, then
 * every token followed by "/tag" for its slots up to the last Some -- an empty string for a None in between -- with
 * the same escaping (sentence.rs:866-881); what `vaporetto --predict-tags` prints.  flags: VPT_FLAG_KYTEA_FULLWIDTH
 * as for vpt_fill_tags_batch_flags (the tokens printed are the caller's text either way).  text_capacity: the bound
 * above + vpt_predictor_max_tag_suffix bytes per char.  A predictor without tag models writes what
 * vpt_write_tokenized_batch writes; one created with predict_tags == 0 is VPT_INVALID_ARGUMENT. */
vpt_status vpt_predictor_max_tag_suffix(const vpt_predictor *p, uint32_t *n_bytes);
vpt_status vpt_write_tagged_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                                  size_t n_sentences, const uint64_t *out_offsets, const uint8_t *labels, unsigned flags,
                                  uint8_t *text_out, uint64_t text_capacity, uint64_t *text_offsets_out);
/* Predictor::predict (predictor.rs:518-543) AND Sentence::write_tokenized_text without tags (sentence.rs:850-886) for a batch in ONE scoring
 * launch: every tile of the specialised kernel writes the tokenized text of the chars it owns straight from its LDS, placed by a look-back
 * over the tiles' sizes (no second pass over the text, no writer launch).  d_scores / d_labels may be NULL (a tokenizer needs neither);
 * d_text_out needs 3 bytes per text byte at most, d_text_offsets_out [n_sentences + 1].  Asynchronous on hip_stream; errors (an output
 * larger than text_capacity among them) at vpt_batch_sync.  A model outside the specialised kernel's reach runs predict and the writer
 * one after the other. */
vpt_status vpt_predict_write_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8, const uint64_t *d_byte_offsets,
                                          const uint64_t *d_out_offsets, size_t n_sentences, uint64_t total_boundaries,
                                          uint64_t max_sentence_bytes, int32_t *d_scores, uint8_t *d_labels, uint8_t *d_text_out,
                                          uint64_t text_capacity, uint64_t *d_text_offsets_out, void *hip_stream);

/* Device-resident variants: all pointers are device pointers, asynchronous on `hip_stream`; errors at vpt_batch_sync.
 * One kernel (kernels_emit.hip: a workgroup per run of sentences sizes, places and writes it).  The tagged one takes its
 * tags from the RECORDS a vpt_fill_tags_batch_device call left on the SAME workspace for the same batch AND THE SAME
 * LABELS (one per token that call found a tag model for: the model, the chosen candidates, the bytes they take; labels
 * changed in between are reported as offsets that do not match -- Sentence::fill_tags and write_tokenized_text see the
 * same boundaries too, sentence.rs:1144-1148, 850-886).  d_tags: not read (until round 6 the dense array of that
 * fill_tags call); NULL is fine.  Offsets that do not describe the text -- those of this call, or those the fill_tags call was given -- are
 * an error reported by vpt_batch_sync and never a write outside d_text_out[0, text_capacity) and d_text_offsets_out[0, n_sentences]. */
vpt_status vpt_write_tokenized_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8,
                                            const uint64_t *d_byte_offsets, const uint64_t *d_out_offsets,
                                            size_t n_sentences, uint64_t total_boundaries, const uint8_t *d_labels,
                                            uint8_t *d_text_out, uint64_t text_capacity,
                                            uint64_t *d_text_offsets_out, void *hip_stream);
vpt_status vpt_write_tagged_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8,
                                         const uint64_t *d_byte_offsets, const uint64_t *d_out_offsets,
                                         size_t n_sentences, uint64_t total_boundaries, const uint8_t *d_labels,
                                         const int32_t *d_tags, uint8_t *d_text_out, uint64_t text_capacity,
                                         uint64_t *d_text_offsets_out, void *hip_stream);

/* vpt_count_boundaries on the device (one wave per sentence + a prefix sum): d_out_offsets[n_sentences + 1]; the same
 * validation, reported at vpt_batch_sync. */
vpt_status vpt_count_boundaries_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8,
                                       const uint64_t *d_byte_offsets, size_t n_sentences, uint64_t *d_out_offsets,
                                       void *hip_stream);

/* Lines in, tokenized lines out -- the loop of predict/src/main.rs:122-176 for a whole batch: Sentence::from_raw,
 * [KyteaFullwidthFilter], Predictor::predict, [KyteaWsConstFilter / SplitLinebreaksFilter], [fill_tags],
 * write_tokenized_text.  Only the text crosses PCIe: char counting, scoring, tagging and the writer run on the
 * device.  flags: any VPT_FLAG_*; tagged != 0 needs a predictor created with predict_tags.  text_capacity:
 * 3 * (text bytes), plus (text bytes) * vpt_predictor_max_tag_suffix when tagged, always suffices. */
vpt_status vpt_tokenize_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                              size_t n_sentences, unsigned flags, int tagged, uint8_t *text_out,
                              uint64_t text_capacity, uint64_t *text_offsets_out);

/* ---------------------------------------------------------------------------------------------------------
 * The `predict` CLI's stdout for a batch of lines, with --scores and --tag-scores     (predict/src/main.rs:66-93, 122-176)
 *
 * Line i's bytes are out[listing_offsets[i] .. listing_offsets[i + 1]): with N the text as it was scored (KyteaFullwidthFilter's image under
 * VPT_FLAG_KYTEA_FULLWIDTH, main.rs:154; else the line itself),
 *   T             write_tokenized_text of the line with the labels (main.rs:135, 161-165), with "/tag" suffixes under VPT_LISTING_TAGGED;
 *   scores block  VPT_LISTING_SCORES, print_scores (main.rs:66-75): "{i}:{N[i]}{N[i+1]} {score}\n" per boundary, then "\n";
 *   tag block     VPT_LISTING_TAG_SCORES, print_tag_scores (main.rs:77-93): per token of N its surface, unescaped, then per slot of its tag model
 *                 "\t" and "tag:score" joined by "," (Token::tag_candidates, sentence.rs:1228-1250: score 0 for a slot with one candidate;
 *                 the LAST tag model of a repeated token, predictor.rs:466-478), "\n"; then "\n".  Tags are written raw.
 * in the order  T "\n" [scores block] [tag block]  (main.rs:154-176), or with VPT_LISTING_NO_NORM_ORDER  T [scores block] "\n" [tag block]  (the
 * --no-norm loop, main.rs:129-144: no newline between T and the first score line).
 * Formatting runs on the device (kernels_listing.hip: a count pass, a prefix sum, a write pass; the bytes depend on the input alone).
 * VPT_LISTING_TAG_SCORES or VPT_LISTING_TAGGED on a predictor created with predict_tags == 0 is VPT_INVALID_ARGUMENT (the reference panics).
 * capacity: with B text bytes, C chars, S lines and b = C - S boundaries,
 *     3 B + S                                                  T and its newline            (sentence.rs:850-886: every byte escaped, a space per char)
 *   + C * vpt_predictor_max_tag_suffix                         with VPT_LISTING_TAGGED
 *   + 32 b + S                                                 with VPT_LISTING_SCORES: a line is at most 10 + 1 + 4 + 4 + 1 + 11 + 1 = 32 bytes (main.rs:70)
 *   + 3 B + C + S + C * vpt_predictor_max_tag_listing          with VPT_LISTING_TAG_SCORES: the chars of N (a fullwidth char has 3 bytes), a "\n" per
 *                                                              token and block, the candidates of a token (main.rs:79-91)
 * always suffices.  Too small a capacity, offsets that do not match the text and VPT_BOUNDARY_UNKNOWN among the labels are VPT_INVALID_ARGUMENT;
 * nothing is written outside the caller's arrays.
 * vpt_predict_listing_batch: host buffers.  labels == NULL: Sentence::from_raw's checks, Predictor::predict and the post-filters of `flags` (any
 *   VPT_FLAG_*) run here.  labels != NULL: the caller's scores (needed with VPT_LISTING_SCORES) and labels, laid out as vpt_count_boundaries
 *   lays them out from 0, are listed -- the path of a host filter such as ConcatGraphemeClustersFilter between predict and the listing; of
 *   `flags` only VPT_FLAG_KYTEA_FULLWIDTH then matters.  One call holds its batch on the device: callers with streams cut them (the CLI does).
 * vpt_predict_listing_batch_device: device pointers, asynchronous on hip_stream, errors at vpt_batch_sync; d_scores / d_labels as
 *   vpt_predict_batch_device left them (possibly edited), VPT_FLAG_KYTEA_FULLWIDTH from vpt_batch_set_flags; text_bytes: the batch's text bytes or
 *   an upper bound (sizes the workspace's copy of T; understated: "text_capacity" at the sync).  At most 2^32 - 257 chars per call. */
enum { VPT_LISTING_SCORES = 1, VPT_LISTING_TAG_SCORES = 2, VPT_LISTING_TAGGED = 4, VPT_LISTING_NO_NORM_ORDER = 8, VPT_LISTING_ALL = 15 };
vpt_status vpt_predictor_max_tag_listing(const vpt_predictor *p, uint32_t *n_bytes);
vpt_status vpt_predict_listing_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences, unsigned flags,
                                     unsigned listing, const int32_t *scores, const uint8_t *labels, uint8_t *out, uint64_t capacity,
                                     uint64_t *listing_offsets_out);
vpt_status vpt_predict_listing_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8, const uint64_t *d_byte_offsets,
                                            const uint64_t *d_out_offsets, size_t n_sentences, uint64_t total_boundaries, uint64_t text_bytes,
                                            const int32_t *d_scores, const uint8_t *d_labels, unsigned listing, uint8_t *d_out, uint64_t capacity,
                                            uint64_t *d_listing_offsets_out, void *hip_stream);

/* ---------------------------------------------------------------------------------------------------------
 * VaporettoTokenizer::token_stream over a batch of documents                  (vaporetto_tantivy/src/lib.rs:157-229)
 *
 * What an indexer takes from the tokenizer: per document the byte span of every token IN THE CALLER'S TEXT, as CSR:
 *   token_offsets [n + 1]   document i owns the tokens token_offsets[i] .. token_offsets[i + 1]; their number is the adapter's position_length;
 *   token_ends [capacity]   the adapter's boundary_pos (lib.rs:183-192): the byte offset, from the document's first byte, behind every token.  A
 *                           token's offset_to; its offset_from is the entry before it in the same document, or 0; its position is its index
 *                           minus token_offsets[i].  One entry per char always suffices.
 * vpt_token_spans_batch_device: lib.rs:183-192 (the char_indices / boundaries zip) for labels that are on the device already -- laid out as
 *   vpt_predict_batch_device writes them, possibly edited by the caller's own filters; one launch (kernels_tokens.hip), asynchronous on hip_stream,
 *   no host wait between the scoring launch and this one.  Errors at vpt_batch_sync: VPT_BOUNDARY_UNKNOWN among the labels, offsets that do not
 *   match the text, a document of 2^32 bytes or more (all VPT_INVALID_ARGUMENT), and more tokens than `capacity`
 *   (VPT_INVALID_ARGUMENT "text_capacity: ..."): nothing is written past `capacity` entries.
 * vpt_token_spans_batch: the same from host buffers (the labels: the caller's -- what callers with filters of their own use, and the
 *   ConcatGraphemeClustersFilter path, whose filter runs on the host).  out_offsets from vpt_count_boundaries.
 * vpt_token_stream_batch: lib.rs:160-192 for a batch -- an empty document has no tokens (lib.rs:161-169; not an error here), KyteaFullwidthFilter always
 *   (lib.rs:172), Predictor::predict, SplitLinebreaksFilter, then the KyteaWsConstFilter of every VPT_FLAG_WSCONST bit of wsconst_flags (lib.rs:69-86;
 *   any other bit is VPT_INVALID_ARGUMENT "Could not parse a wsconst value"), the spans counted on the caller's bytes.  Only the text crosses
 *   PCIe on the way in and 8 (n + 1) + 4 x tokens bytes on the way out: char counting, scoring, filters and spans run on the device, large batches
 *   as chunks of whole documents through vpt_tokenize_batch's pipeline.  A NUL in a document (Sentence::from_raw(..).unwrap() panics there,
 *   lib.rs:173) is VPT_INVALID_ARGUMENT "text: must not contain NULL".  "G" is VPT_FLAG_CONCAT_GRAPHEMES in wsconst_flags: the filter runs last,
 *   which is the adapter's result wherever "G" stands in its string. */
vpt_status vpt_token_spans_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8, const uint64_t *d_byte_offsets,
                                        const uint64_t *d_out_offsets, size_t n_documents, uint64_t total_boundaries, const uint8_t *d_labels,
                                        uint64_t *d_token_offsets, uint32_t *d_token_ends, uint64_t capacity, void *hip_stream);
vpt_status vpt_token_spans_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_documents,
                                 const uint64_t *out_offsets, const uint8_t *labels, uint64_t *token_offsets_out, uint32_t *token_ends_out,
                                 uint64_t capacity);
vpt_status vpt_token_stream_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_documents,
                                  unsigned wsconst_flags, uint64_t *token_offsets_out, uint32_t *token_ends_out, uint64_t capacity);

/* ---------------------------------------------------------------------------------------------------------
 * The token spans with every token's tags                                     (an indexer's part-of-speech filter; no item of the adapter)
 *
 * The tag vocabulary: a predictor created with predict_tags != 0 holds the distinct RAW (unescaped) tag strings of its tag models, numbered in
 *   order of first appearance over Model::tag_models, then slots, then candidates.  vpt_predictor_n_tag_strings: their number (0 without tag
 *   models or without predict_tags); vpt_predictor_tag_string: the bytes of `id`, owned by the predictor (an id that is none: VPT_INVALID_ARGUMENT).
 *   Built from the compiled tables, so vpt_predictor_load / _adopt_device / _clone_to_device give the same vocabulary, id for id: with
 *   predict_tags and tag models every such call reads five small table sections back from the device once (synchronous copies).  A HIP
 *   error there does not fail the creation -- every other call is what it was --; the calls of this section then return it (VPT_RUNTIME_ERROR).
 * vpt_token_tags_batch_device: vpt_token_spans_batch_device plus
 *   token_tags [capacity * n_tags]   n_tags int32 per token at token_tags[token * n_tags + slot], `token` its index in token_ends:
 *                           >= 0 an id of the tag vocabulary; -1 None (a token without a tag model, an empty candidate list, a slot the model
 *                           left None); -(2 + id) a rule tag of the pattern tagger set on the workspace (vpt_pattern_tagger_tag).
 *   The tags are the RECORDS the vpt_fill_tags_batch_device call on THIS workspace left (the tagged writer's contract): call it first, for the same
 *   batch and the same labels (else VPT_INVALID_ARGUMENT "call vpt_fill_tags_batch_device ..."); labels changed in between are reported at
 *   vpt_batch_sync as offsets that do not match.  One launch (kernels_tokens.hip, the tagged instance), asynchronous; errors as for
 *   vpt_token_spans_batch_device, and nothing is written past `capacity` tokens or capacity * n_tags tags.  A predictor whose model has no tag
 *   models (n_tags == 0) writes what vpt_token_spans_batch_device writes and touches no tag entry; one created with predict_tags == 0 is
 *   VPT_INVALID_ARGUMENT "this predictor is created with predict_tags = false". */
vpt_status vpt_predictor_n_tag_strings(const vpt_predictor *p, uint32_t *n);
vpt_status vpt_predictor_tag_string(const vpt_predictor *p, uint32_t id, const uint8_t **bytes, size_t *len);
vpt_status vpt_token_tags_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8, const uint64_t *d_byte_offsets,
                                       const uint64_t *d_out_offsets, size_t n_documents, uint64_t total_boundaries, const uint8_t *d_labels,
                                       uint64_t *d_token_offsets, uint32_t *d_token_ends, int32_t *d_token_tags, uint64_t capacity,
                                       void *hip_stream);

/* The tag stop filter: the token stream without the tokens an indexer drops (particles, auxiliaries, symbols), positions kept.
 *
 * vpt_tag_stop_create: a stop set from n_entries (slot, tag string) pairs -- slots[e], tag_bytes[tag_offsets[e] .. tag_offsets[e + 1]).  A token
 *   is STOPPED when, for some pair, its slot's tag string equals the pair's string, whether a tag model or a rule of `tagger` (or NULL) gave the
 *   tag; None never matches; a string that neither the predictor's vocabulary nor the tagger's holds matches nothing and is no error.  The host
 *   resolves the strings once into one bitmap per slot over the vocabulary ids (and one over the tagger's ids).  VPT_INVALID_ARGUMENT
 *   "stop tags: ... (entry e)": a slot >= n_tags, a tag that contains NUL; "tagger: does not belong to this predictor".  The handle is immutable,
 *   tied to its predictor (and to the tagger's ids), shareable between workspaces and host threads; vpt_tag_stop_destroy frees it.
 * vpt_token_filter_batch_device: a pass of its own over a finished CSR (token_offsets [n + 1], token_ends, token_tags as
 *   vpt_token_tags_batch_device writes them; capacity_in: what the two arrays hold, the tokens are token_offsets[n] or fewer) -- a keep-flag count
 *   per block of vpt_token_filter_tile tokens, a prefix sum, a scatter; no sort, no atomics on what decides an order: two runs give identical
 *   bytes.  Out, for the kept tokens: offsets_out [n + 1]; starts_out / ends_out (u32: offset_from, offset_to); positions_out (u32: the token's
 *   index in its document BEFORE filtering -- what position increments need); tags_out.  A document may keep no token.  stop == NULL keeps
 *   every token (starts: the entry before or 0; positions: the index).  Asynchronous; more kept tokens than `capacity` is reported at
 *   vpt_batch_sync (VPT_INVALID_ARGUMENT "text_capacity: ...") and nothing is written past `capacity`, whatever the offsets say.
 * vpt_token_stream_tagged_batch: vpt_token_stream_batch's steps (empty documents, the 2^32 limit, the NUL message and the wsconst parsing are
 *   its) with, per chunk of whole documents, Sentence::fill_tags (on the normalised text, `tagger`'s rules behind it when not NULL) between the
 *   label filters and the spans, the tagged span instance, and the filter pass (`stop` or NULL) -- everything after the copy in on the device.
 *   The five arrays as above, `capacity` entries each (capacity * n_tags tags); one per text byte always suffices.  The result does not depend
 *   on how the batch is cut into chunks.  A predictor with predict_tags == 0: VPT_INVALID_ARGUMENT. */
vpt_status vpt_tag_stop_create(const vpt_predictor *p, const void *tagger, const uint32_t *slots, const uint8_t *tag_bytes,
                               const uint64_t *tag_offsets, size_t n_entries, void **out);
void vpt_tag_stop_destroy(void *stop);
vpt_status vpt_token_filter_tile(uint32_t *n_tokens);
vpt_status vpt_token_filter_batch_device(const vpt_predictor *p, vpt_batch *b, const void *stop, const uint64_t *d_token_offsets,
                                         const uint32_t *d_token_ends, const int32_t *d_token_tags, size_t n_documents, uint64_t capacity_in,
                                         uint64_t *d_offsets_out, uint32_t *d_starts_out, uint32_t *d_ends_out, uint32_t *d_positions_out,
                                         int32_t *d_tags_out, uint64_t capacity, void *hip_stream);
vpt_status vpt_token_stream_tagged_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_documents,
                                         unsigned wsconst_flags, const void *tagger, const void *stop, uint64_t *token_offsets_out,
                                         uint32_t *token_starts_out, uint32_t *token_ends_out, uint32_t *token_positions_out,
                                         int32_t *token_tags_out, uint64_t capacity);

/* ---------------------------------------------------------------------------------------------------------
 * Vocabulary ids in the token stream                  (no item of the adapter: what the consumer of its Token::text, vaporetto_tantivy/src/lib.rs:204-219,
 *                                                      does with a term dictionary or a model's vocabulary -- here without the strings leaving the device)
 *
 * vpt_vocab_create: a vocabulary of n_entries surfaces -- entry k is surfaces[offsets[k] .. offsets[k + 1]) and gets id k; unk_id (any int32) is
 *   the id of a token that is no entry.  The host builds a hashed table laid out like the pattern tagger's (open addressing, 16-byte slots {id + 1,
 *   chars, fingerprint, first code point}, load factor in (1/4, 1/2], the surfaces' code points back to back) and puts it on the predictor's device.
 *   Up to 2^24 entries.  VPT_INVALID_ARGUMENT "InvalidArgumentError: vocab: <reason> (entry k)" for the first failing entry: not valid UTF-8, an
 *   empty surface, a NUL, a surface an earlier entry has (an id names one string: no last-wins here).  The handle is immutable, tied to its
 *   predictor's device, shareable between workspaces and host threads; vpt_vocab_destroy frees it.
 * vpt_vocab_info: keys, slots and the longest surface in chars; vpt_vocab_surface: the bytes of `id`, owned by the handle (an id that is none:
 *   VPT_INVALID_ARGUMENT); vpt_vocab_tile: the tokens a workgroup of the id pass takes (the tests place tokens across its edges).
 * vpt_token_ids_batch_device: a pass of its own over a FINISHED span CSR (one launch, kernels_vocab.hip), asynchronous on hip_stream, errors at
 *   vpt_batch_sync.  d_token_offsets [n + 1] and d_token_ends as vpt_token_spans_batch_device / vpt_token_tags_batch_device write them with
 *   d_token_starts == NULL (a token starts where the one before it in its document ends, or at 0), or d_offsets_out / d_starts_out / d_ends_out of
 *   vpt_token_filter_batch_device (a document may own no token).  capacity_in: what the arrays hold; the tokens are token_offsets[n].
 *   d_token_ids [capacity_in]: per token the id of its surface, or unk_id.  The surface is the token's bytes IN THE CALLER'S TEXT; with
 *   flags == VPT_FLAG_KYTEA_FULLWIDTH it is the KyteaFullwidthFilter image of those chars -- the text as it was scored, the convention of the rule
 *   surfaces of vpt_pattern_tagger_create.  The vocabulary's surfaces are taken as they are.  Any other flag bit: VPT_INVALID_ARGUMENT.  A token of
 *   more bytes than 4 * max_surface_chars is unk_id and its surface is not read.  No atomics on anything that decides a value: two runs give
 *   identical bytes.  Whatever the device arrays hold, nothing is read outside [byte_offsets[0], byte_offsets[n]) of the text and nothing is written
 *   outside d_token_ids[0 .. capacity_in); token_offsets that decrease or exceed capacity_in, a span with start > end or end past its document, and
 *   a start or an end inside a char are VPT_INVALID_ARGUMENT at the sync (the ids of such tokens are unspecified).
 * vpt_token_stream_ids_batch: host buffers in, the stream with ids out.  With tagger == stop == token_tags_out == NULL: vpt_token_stream_batch's
 *   steps (starts and positions are written all the same); otherwise vpt_token_stream_tagged_batch's, which need predict_tags.  The id pass runs
 *   last, on every chunk's finished CSR, on the device; vocab_flags as `flags` above.  token_ids_out [capacity].  The result does not depend on how
 *   the batch is cut into chunks. */
vpt_status vpt_vocab_create(const vpt_predictor *p, const uint8_t *surfaces, const uint64_t *offsets, size_t n_entries, int32_t unk_id,
                            void **out);
void vpt_vocab_destroy(void *vocab);
vpt_status vpt_vocab_info(const void *vocab, uint32_t *n_keys, uint32_t *n_slots, uint32_t *max_surface_chars);
vpt_status vpt_vocab_surface(const void *vocab, uint32_t id, const uint8_t **bytes, size_t *len);
vpt_status vpt_vocab_tile(uint32_t *n_tokens);
vpt_status vpt_token_ids_batch_device(const vpt_predictor *p, vpt_batch *b, const void *vocab, const uint8_t *d_utf8,
                                      const uint64_t *d_byte_offsets, size_t n_documents, const uint64_t *d_token_offsets,
                                      const uint32_t *d_token_starts, const uint32_t *d_token_ends, uint64_t capacity_in, unsigned flags,
                                      int32_t *d_token_ids, void *hip_stream);
vpt_status vpt_token_stream_ids_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_documents,
                                      unsigned wsconst_flags, const void *tagger, const void *stop, const void *vocab, unsigned vocab_flags,
                                      uint64_t *token_offsets_out, uint32_t *token_starts_out, uint32_t *token_ends_out,
                                      uint32_t *token_positions_out, int32_t *token_tags_out, int32_t *token_ids_out, uint64_t capacity);

/* ---------------------------------------------------------------------------------------------------------
 * Build a vocabulary on the device: count token surfaces over a corpus          (no item of the adapter: the dict over Token::text that a caller
 *                                                      fills on the host before it can make the vocabulary above -- here the strings stay on the device)
 *
 * vpt_vocab_counter_create: an accumulating table token surface -> 64-bit count on the predictor's device, tied to that predictor.  max_keys
 *   (1 .. 2^24): the distinct surfaces it can hold; it has n_slots = the smallest power of two >= 2 * max_keys slots.  max_surface_chars (>= 1):
 *   a longer token is skipped.  arena_chars: the code points it can keep over all keys, 0 = 8 * max_keys.  One device allocation.
 *   THE HANDLE IS MUTABLE, unlike a vocabulary: only one call may be in flight on it at a time, in stream order -- a count call on another
 *   stream, or a host call below, while one is running is the caller's error.  vpt_vocab_counter_destroy frees it (after the stream of the last
 *   count call is through); vpt_vocab_counter_reset empties it.
 * vpt_vocab_counter_info: distinct keys, tokens counted, tokens skipped, slots, and whether it is full.  Synchronises the last count call's stream.
 * vpt_vocab_count_batch_device: counts the tokens of a FINISHED span CSR -- the arrays, conventions and flags of vpt_token_ids_batch_device
 *   (d_token_starts == NULL or the filter's starts, documents that own no token, capacity_in; flags 0 or VPT_FLAG_KYTEA_FULLWIDTH, any other bit
 *   VPT_INVALID_ARGUMENT) and its definition of a surface: a vocabulary built with a flag and looked up with the same flag agrees token for token.
 *   Three launches (kernels_vocab_count.hip), asynchronous on hip_stream, errors at vpt_batch_sync; two uint4 per token of the batch's workspace.
 *   Not counted, and one more in n_skipped: an empty token, a token that is not strict UTF-8 inside its span, a token of more than
 *   max_surface_chars chars (one of more than 4 * max_surface_chars bytes is not read).  Every other token adds 1 to its key's count and to
 *   n_counted.  Counts are integer atomics: the result does not depend on the order of the lanes.  Whatever the device arrays hold, nothing is read
 *   outside [byte_offsets[0], byte_offsets[n]) of the text and nothing is written outside the counter and the batch's scratch; the id pass's
 *   conditions are the same VPT_INVALID_ARGUMENT at the sync -- the counter's contents are then unspecified and reset makes it usable again.
 *   FULL: more than max_keys distinct keys, more than arena_chars code points, or a probe that has seen every slot: a sticky bit, and the sync
 *   returns VPT_INVALID_ARGUMENT "InvalidArgumentError: vocab counter: full (max_keys / arena_chars)"; later count calls (at the call or at
 *   their sync) and finish refuse with the same message until reset.  No kernel waits for another lane: every loop is bounded.
 * vpt_vocab_counter_finish: a snapshot (counting may go on): the keys of count >= min_count, by count descending, then by code points ascending
 *   -- a total order: two runs give identical bytes --, the first max_entries of them (0: all).  surfaces: UTF-8 (the KyteaFullwidthFilter
 *   image under that flag, else the caller's chars), entry k at surfaces[offsets[k] .. offsets[k + 1]); offsets [n + 1]; counts [n].  Owned by
 *   the handle until the next finish, reset or destroy.  Synchronises the last count call's stream.  surfaces, offsets and *n_entries are what
 *   vpt_vocab_create takes.
 * vpt_token_stream_count_batch: host buffers in, nothing out: vpt_token_stream_batch's steps when tagger == stop == NULL, else
 *   vpt_token_stream_tagged_batch's (which need predict_tags); the count call runs on every chunk's finished CSR, on the device, one chunk after
 *   the other; vocab_flags as `flags` above.  The result does not depend on how the batch is cut into chunks.  Returns when the device is through. */
vpt_status vpt_vocab_counter_create(const vpt_predictor *p, uint64_t max_keys, uint64_t max_surface_chars, uint64_t arena_chars, void **out);
void vpt_vocab_counter_destroy(void *counter);
vpt_status vpt_vocab_counter_reset(void *counter);
vpt_status vpt_vocab_counter_info(void *counter, uint64_t *n_keys, uint64_t *n_counted, uint64_t *n_skipped, uint32_t *n_slots, uint32_t *full);
vpt_status vpt_vocab_count_batch_device(const vpt_predictor *p, vpt_batch *b, void *counter, const uint8_t *d_utf8,
                                        const uint64_t *d_byte_offsets, size_t n_documents, const uint64_t *d_token_offsets,
                                        const uint32_t *d_token_starts, const uint32_t *d_token_ends, uint64_t capacity_in, unsigned flags,
                                        void *hip_stream);
vpt_status vpt_vocab_counter_finish(void *counter, uint64_t min_count, uint64_t max_entries, const uint8_t **surfaces, const uint64_t **offsets,
                                    const uint64_t **counts, size_t *n_entries);
vpt_status vpt_token_stream_count_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_documents,
                                        unsigned wsconst_flags, const void *tagger, const void *stop, void *counter, unsigned vocab_flags);

/* ---------------------------------------------------------------------------------------------------------
 * Postings on the device: term -> (document, tf) lists from token ids           (no item of the adapter: what the index writer behind its token
 *                                                      stream does first -- here one int32 per token never has to reach the host to be grouped)
 *
 * vpt_postings_batch_device: the postings of one batch (a SEGMENT: doc_base makes its document numbers global, vpt_postings_merge_device below
 *   merges segments) from a FINISHED span CSR -- d_token_offsets [n_documents + 1] and capacity_in as vpt_token_ids_batch_device takes them, a document may own
 *   no token, the tokens are min(token_offsets[n], capacity_in) -- and d_token_ids [capacity_in], what that call wrote.  It reads those two arrays
 *   and nothing else.  Token t of document d is INDEXED when 0 <= ids[t] < n_terms; every other token (negative, >= n_terms) adds 1 to
 *   d_counts[1] and appears nowhere else.  THE PASS SEES IDS ONLY: a vocabulary's unk_id chosen inside [0, n_terms) is a term like any other.
 *   A posting is a (term, document) pair with at least one indexed token; postings are ordered by term, then by document.  Posting q:
 *   d_post_docs[q] = doc_base + d, d_post_tfs[q] = the number of such tokens.  Term k's postings are [d_term_offsets[k], d_term_offsets[k + 1]),
 *   its document frequency their difference; d_term_offsets[0] = 0, d_term_offsets[n_terms] = d_counts[0] = the postings.
 *   The optional pair (both NULL or neither): d_token_order[0 .. sum of tfs) = the indexed tokens' indices sorted by (term, token index);
 *   d_post_first[q] = posting q's first place in it, d_post_first[d_counts[0]] = the indexed tokens: posting q's tokens are
 *   d_token_order[d_post_first[q] .. d_post_first[q + 1]), ascending -- with token_positions, a positional index by one gather.
 *   Four launches with the trainer's stable radix sort (ceil(bit_width(n_terms) / 8) passes) and scan in between (kernels_postings.hip);
 *   asynchronous on hip_stream, errors at vpt_batch_sync.  No atomic decides a value: two runs give identical bytes.  The workspace keeps
 *   28 bytes per token of capacity_in (key, document, two index words, a flag, a scan word) and 16 bytes per 16 tokens of histograms.
 *   At the call, VPT_INVALID_ARGUMENT: a NULL pointer other than the optional pair, only one of the pair, n_terms == 0 or > 2^24,
 *   capacity_in >= 2^32, doc_base + n_documents > 2^32, a workspace of another predictor.
 *   At the sync, VPT_INVALID_ARGUMENT: the id pass's message when token_offsets decrease, exceed capacity_in or leave a token below
 *   token_offsets[n] that no document owns (the outputs are then unspecified); "InvalidArgumentError: capacity: smaller than the number of
 *   postings" when there are more than capacity_out -- d_counts[0] then holds the number needed, the postings below capacity_out are written and
 *   nothing behind it.  capacity_out >= the tokens always suffices.  Whatever the arrays hold, nothing is read outside token_offsets[0 .. n] and
 *   token_ids[0 .. capacity_in), and nothing is written outside term_offsets [n_terms + 1], post_docs / post_tfs [capacity_out], post_first
 *   [capacity_out + 1], token_order [capacity_in], counts [2] and the workspace.
 * vpt_postings_tile: the tokens a workgroup of the sort takes (the tests' edges; the key pass's tile is vpt_vocab_tile).
 * vpt_token_stream_postings_batch: host buffers in, the segment's postings out: vpt_token_stream_ids_batch's steps into buffers of the call,
 *   then the whole batch's offsets and ids on the device and the pass once; n_terms = the vocabulary's keys, term_offsets_out [n_keys + 1].  A
 *   document's index is the caller's, empty documents included.  The result does not depend on how the stream is cut into chunks.  More than
 *   `capacity` postings: VPT_INVALID_ARGUMENT with the message above, *n_postings_out = the number needed, nothing else written but
 *   *n_dropped_out.  Returns when the device is through. */
vpt_status vpt_postings_batch_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_token_offsets, size_t n_documents,
                                     const int32_t *d_token_ids, uint64_t capacity_in, uint32_t n_terms, uint64_t doc_base,
                                     uint64_t *d_term_offsets, uint32_t *d_post_docs, uint32_t *d_post_tfs, uint64_t capacity_out,
                                     uint64_t *d_post_first, uint32_t *d_token_order, uint64_t *d_counts, void *hip_stream);
vpt_status vpt_postings_tile(uint32_t *n_tokens);
vpt_status vpt_token_stream_postings_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_documents,
                                           unsigned wsconst_flags, const void *tagger, const void *stop, const void *vocab, unsigned vocab_flags,
                                           uint64_t doc_base, uint64_t *term_offsets_out, uint32_t *post_docs_out, uint32_t *post_tfs_out,
                                           uint64_t capacity, uint64_t *n_postings_out, uint64_t *n_dropped_out);

/* ---------------------------------------------------------------------------------------------------------
 * Merging postings segments on the device                       (no item of the adapter: a corpus indexed in batches ends in ONE index that never
 *                                                                left the device -- the 28 bytes per token of the postings pass bound a batch)
 *
 * vpt_postings_segment: a segment as vpt_postings_batch_device (or this call) left it.  The number of its postings stays on the device --
 *   d_term_offsets[n_terms], read there -- so K postings calls and the merge behind them need no sync in between; `capacity` bounds it. */
typedef struct vpt_postings_segment {
    const uint64_t *d_term_offsets;   /* [n_terms + 1]                                                         */
    const uint32_t *d_post_docs;      /* [capacity], global document numbers                                   */
    const uint32_t *d_post_tfs;       /* [capacity]                                                            */
    uint32_t        n_terms;          /* <= n_terms_out; terms at or above it have no postings here            */
    uint64_t        capacity;         /* the size of the two arrays; the postings: d_term_offsets[n_terms]     */
} vpt_postings_segment;
/* VPT_POSTINGS_MERGE_ORDERED: the caller's promise that every document of segment s is below every document of the next segment that has
 *   postings (what ascending doc_bases give).  The device CHECKS it. */
enum { VPT_POSTINGS_MERGE_ORDERED = 1 };
/* vpt_postings_merge_device: `segments` is a HOST array of n_segments vpt_postings_segment structs -- 1 .. 1024, vpt_postings_merge_limits; read during the
 *   call, it may go afterwards -- whose pointers are device pointers; the segments share the term id space [0, n_terms_out).  One segment comes
 *   out, in the three arrays and with the guarantees of vpt_postings_batch_device: for every term k the merged list is the union of the
 *   segments' lists of k, ordered by document; a document that stands in several segments' lists of k is ONE posting whose tf is the sum.
 *   d_term_offsets_out[0] = 0, d_term_offsets_out[n_terms_out] = d_counts[0] = the merged postings; d_counts[1] = the input postings that were
 *   combined into another (input minus output postings; 0 when no document repeats).  So: however a batch's indexed tokens are dealt out to
 *   segments, the merge of the segments' postings is, byte for byte, what the one-pass call over the whole batch writes.  The optional token
 *   lists (post_first / token_order) are not merged: token indices are local to a segment.
 *   flags = VPT_POSTINGS_MERGE_ORDERED: no sort; the merged list of a term is the segments' lists one after another.  Three launches over the
 *   scratch: a lane per term bound sums the K term_offsets columns and leaves every segment's base inside the term (a K x (n_terms_out + 1)
 *   table of 8-byte words, read and written coalesced across terms); a lane per input place (the sum of the capacities) finds its segment and
 *   its term by bisection and copies its posting; the segments' smallest and largest documents (integer atomic min / max) are compared.  A
 *   broken promise: "InvalidArgumentError: segments: document ranges overlap or descend" at the sync, the outputs unspecified.
 *   flags = 0: any document numbers, repeats combined.  A {term, document, tf} record per input place, the trainer's stable radix sort over
 *   the document word (4 passes) and the term word (ceil(bit_width(n_terms_out) / 8) passes), heads, the trainer's scan, emit (the tf a sum
 *   over the run) and terms, as in the postings pass.
 *   Both: asynchronous on hip_stream, errors at vpt_batch_sync; launch sizes come from the capacities; no atomic decides a value and two runs
 *   give identical bytes.  THE OUTPUTS MUST NOT ALIAS THE INPUTS.  Scratch of the workspace: 48 bytes per segment, and ordered 8 bytes per
 *   segment and 8 bytes per (segment, term bound) -- 8 * n_segments * (n_terms_out + 1) --, general 32 bytes per input place (three record
 *   words, two index words, a flag, a scan word) and 16 bytes per 16 places of histograms.
 *   At the call, VPT_INVALID_ARGUMENT: a NULL pointer (a segment's three included, whatever its capacity), n_segments == 0 or > 1024,
 *   n_terms_out == 0 or > 2^24, a segment's n_terms > n_terms_out, a sum of capacities >= 2^32, an unknown flag bit, a workspace of another
 *   predictor.
 *   At the sync, VPT_INVALID_ARGUMENT: "InvalidArgumentError: segment: term_offsets or postings are not a segment's" -- a segment's
 *   term_offsets do not start at 0, decrease or end above its capacity, or inside one term's list documents do not strictly ascend or a tf
 *   is 0; "InvalidArgumentError: tf: sum exceeds 32 bits"; "InvalidArgumentError: capacity: smaller than the number of postings" when there are
 *   more than capacity_out merged postings -- d_counts[0] then holds the number needed, the postings below capacity_out are written and
 *   nothing behind them.  capacity_out >= the sum of the capacities always suffices.  Whatever the arrays hold, nothing is read outside
 *   term_offsets[0 .. n_terms] and [0, capacity) of each segment, and nothing is written outside d_term_offsets_out [n_terms_out + 1],
 *   d_post_docs_out / d_post_tfs_out [capacity_out], d_counts [2] and the workspace.
 * vpt_postings_merge_limits: the most segments a call takes.
 * vpt_postings_merge: the same over HOST arrays: `segments` with host pointers, each segment's postings term_offsets[n_terms] (at most its
 *   capacity) read here; host arrays out.  More than `capacity` merged postings: VPT_INVALID_ARGUMENT with the message above,
 *   *n_postings_out = the number needed, nothing else written.  Returns when the device is through.
 * (`segments` is declared const void * as the other struct arguments of this header are; pass a const vpt_postings_segment *.) */
vpt_status vpt_postings_merge_device(const vpt_predictor *p, vpt_batch *b, const void *segments, size_t n_segments, uint32_t n_terms_out,
                                     unsigned flags, uint64_t *d_term_offsets_out, uint32_t *d_post_docs_out, uint32_t *d_post_tfs_out,
                                     uint64_t capacity_out, uint64_t *d_counts, void *hip_stream);
vpt_status vpt_postings_merge_limits(uint32_t *max_segments);
vpt_status vpt_postings_merge(const vpt_predictor *p, const void *segments, size_t n_segments, uint32_t n_terms_out, unsigned flags,
                              uint64_t *term_offsets_out, uint32_t *post_docs_out, uint32_t *post_tfs_out, uint64_t capacity,
                              uint64_t *n_postings_out, uint64_t *n_combined_out);

/* ---------------------------------------------------------------------------------------------------------
 * BM25 top-k search over a postings segment on the device     (no item of the adapter: the ranking tantivy applies behind its token stream --
 *                                                                here the index that never left the device is also READ there)
 *
 * vpt_postings_search_device: a batch of queries against ONE segment, as vpt_postings_batch_device or vpt_postings_merge_device left it.
 *   Segment: d_term_offsets [n_terms + 1], d_post_docs / d_post_tfs [capacity_postings]; the postings are d_term_offsets[n_terms], read on the
 *   device, so indexing, merging and searching need no sync in between.
 *   Documents: doc_base, n_documents, d_doc_lens uint32 [n_documents] = the length of document doc_base + i (the wrappers pass its token count,
 *   token_offsets[i + 1] - token_offsets[i], dropped tokens included, as tantivy's field norm counts every token).
 *   Queries, a CSR: d_query_offsets [n_queries + 1], d_query_terms int32 / d_query_weights float [capacity_slots]; the slots are
 *   min(query_offsets[n_queries], capacity_slots).  A slot whose term is outside [0, n_terms) scores nothing and adds 1 to d_counts[2] (an unk_id
 *   of -1 is such a term).  A term repeated in a query is scored once per slot.  The weight is the caller's -- idf for BM25, vpt_okapi_idf; the
 *   device never takes a logarithm.
 *   Score, all in IEEE binary32, round to nearest, no contraction, in exactly this order: for a slot with weight w and a posting (d, tf) of its
 *   term
 *       r = float(dl[d - doc_base]) / avgdl;  K = k1 * ((1.0f - b) + b * r);  f = float(tf);  c = w * ((f * (k1 + 1.0f)) / (f + K))
 *   A document MATCHES a query when at least one slot has a posting for it; its score is the sum of its c values in slot order, left to right,
 *   starting from the first c.
 *   Output, per query q: d_match_counts[q] = the matching documents; d_hit_counts[q] = min(k, matches); d_hit_docs[q * k + j] /
 *   d_hit_scores[q * k + j] for j below the hit count = the matches by score descending, then document ascending; entries at or behind the hit
 *   count are not written.  d_counts[0] = the candidates (the sum over in-range slots of the term's df), d_counts[1] = the matches of all
 *   queries, d_counts[2] = the skipped slots.  Two runs, on one workspace or on two, give identical bytes.
 *   Launches (kernels_postings_search.hip), each sized from capacity_slots, capacity_candidates, n_queries or n_queries * k, none from a value
 *   read back: slots (df, checks), the trainer's scan (candidate bases), expand (a {document, query, c} record per candidate place), the
 *   trainer's stable radix sort over the document word (ceil(bit_width(n_documents) / 8) passes, at most 4) and the query word
 *   (ceil(bit_width(n_queries) / 8) passes), heads, the trainer's scan, sum (a head adds its run in slot order) and ranges, the trainer's sort
 *   over ~bits(score) (4 passes) and the query word, take.  Asynchronous on hip_stream, errors at vpt_batch_sync; no atomic decides a value.
 *   Scratch of the workspace: 20 bytes per slot of capacity_slots, 44 bytes per place of capacity_candidates (two records of three words, two
 *   index words, a flag, a scan word), 8 bytes per query and 16 bytes per 16 places of histograms.
 *   At the call, VPT_INVALID_ARGUMENT: a NULL pointer, n_terms == 0 or > 2^24, n_queries == 0 or > 2^24, k == 0 or n_queries * k >= 2^32,
 *   capacity_slots or capacity_candidates >= 2^32, doc_base + n_documents > 2^32, k1 outside [0, 65536], b outside [0, 1], avgdl outside
 *   [2^-32, 2^32] (with these and tf >= 1 every denominator is >= 1 and no NaN arises from finite non-negative weights; a sum may reach +inf,
 *   which sorts first, ties by document), a workspace of another predictor.
 *   At the sync, VPT_INVALID_ARGUMENT: "InvalidArgumentError: query_offsets: do not describe the queries' slots" (they decrease, exceed
 *   capacity_slots or leave a slot unowned); "InvalidArgumentError: segment: term_offsets or postings are not a segment's" (a scored term's two
 *   bounds descend or end above capacity_postings, a tf of 0, a document outside [doc_base, doc_base + n_documents) or not above the one before
 *   it in its list); "InvalidArgumentError: weights: negative or not finite" (bits above 0x7F7FFFFF); "InvalidArgumentError: query: more than
 *   1024 slots" (vpt_postings_search_limits); "InvalidArgumentError: capacity_candidates: smaller than the number of candidates" -- d_counts[0]
 *   then holds the number needed.  After any of these the four outputs are as they were before the call (so are they while an error of this
 *   list from an earlier call on the workspace waits for its sync).  Whatever the arrays hold, nothing is read outside
 *   term_offsets[0 .. n_terms], [0, capacity_postings), doc_lens[0 .. n_documents) and the query arrays' stated sizes, and nothing is written
 *   outside d_hit_docs / d_hit_scores [n_queries * k], d_hit_counts / d_match_counts [n_queries], d_counts [3] and the workspace.
 * vpt_postings_search_limits: the most slots a query may have.
 * vpt_postings_search: the same over HOST arrays: what the segment holds (term_offsets[n_terms] postings) is uploaded, the candidates are
 *   counted from the host's term_offsets, the device call runs once, the four outputs and counts_out [3] come back (hit entries at or behind a
 *   query's hit count come back 0).  Returns when the device is through.
 * vpt_okapi_idf: (float)log(1 + (N - df + 0.5) / (df + 0.5)) evaluated in double -- tantivy's idf; df > N is VPT_INVALID_ARGUMENT.  The one
 *   implementation every binding calls, so all agree on the weights' bits. */
vpt_status vpt_postings_search_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_term_offsets, const uint32_t *d_post_docs,
                                      const uint32_t *d_post_tfs, uint32_t n_terms, uint64_t capacity_postings, uint64_t doc_base,
                                      uint64_t n_documents, const uint32_t *d_doc_lens, const uint64_t *d_query_offsets,
                                      const int32_t *d_query_terms, const float *d_query_weights, uint32_t n_queries, uint64_t capacity_slots,
                                      float k1, float b_param, float avgdl, uint32_t k, uint64_t capacity_candidates, uint32_t *d_hit_docs,
                                      float *d_hit_scores, uint32_t *d_hit_counts, uint64_t *d_match_counts, uint64_t *d_counts, void *hip_stream);
vpt_status vpt_postings_search_limits(uint32_t *max_query_slots);
vpt_status vpt_postings_search(const vpt_predictor *p, const uint64_t *term_offsets, const uint32_t *post_docs, const uint32_t *post_tfs,
                               uint32_t n_terms, uint64_t doc_base, uint64_t n_documents, const uint32_t *doc_lens, const uint64_t *query_offsets,
                               const int32_t *query_terms, const float *query_weights, uint32_t n_queries, float k1, float b_param, float avgdl,
                               uint32_t k, uint32_t *hit_docs_out, float *hit_scores_out, uint32_t *hit_counts_out, uint64_t *match_counts_out,
                               uint64_t *counts_out);
vpt_status vpt_okapi_idf(uint64_t n_documents, uint64_t df, float *idf_out);

/* ---------------------------------------------------------------------------------------------------------
 * Boolean queries on the device: MUST / SHOULD / MUST_NOT slots in the BM25 search      (tantivy's BooleanQuery of Occur::{Must, Should, MustNot}
 *                                                                                          clauses over term queries: what `+a -b c` parses to)
 *
 * vpt_postings_boolean_search_device: every argument of vpt_postings_search_device with the same meaning, and d_query_occurs uint8
 *   [capacity_slots] behind d_query_weights: VPT_OCCUR_SHOULD, VPT_OCCUR_MUST or VPT_OCCUR_MUST_NOT per slot.
 *   A slot HAS a document when its term is inside [0, n_terms) and the term's list holds a posting for it.  A document MATCHES query q when
 *   every MUST slot of q has it, no MUST_NOT slot of q has it and, if q has no MUST slot, at least one SHOULD slot has it.  So: a query with
 *   no slots matches nothing; a query with only MUST_NOT slots matches nothing (as in tantivy); a MUST slot whose term is out of range or has
 *   df 0 leaves the query with no match; an out-of-range SHOULD or MUST_NOT slot is ignored; every out-of-range slot adds 1 to d_counts[2].  A
 *   repeated term is one slot per repetition: the same term as MUST and as MUST_NOT matches nothing, a term twice as MUST is scored twice.
 *   Score: c is vpt_postings_search_device's, computed for every MUST or SHOULD slot that has the document; the c values are added in slot
 *   order, left to right, starting from the first c, each add rounded to binary32.  MUST_NOT slots contribute nothing; their weights are
 *   checked like the rest.  A call whose slots are all SHOULD gives the documents, counts and score bits of vpt_postings_search_device.
 *   Outputs, their order (score descending, then document ascending), k, "entries at or behind the hit count are not written" and
 *   determinism: as in vpt_postings_search_device.  d_counts[1] = the matches of all queries, d_counts[2] = the skipped slots.
 *   PLACES: a query's ANCHOR is its first MUST slot of the smallest df.  A query with an anchor needs the anchor's df places; a query without a
 *   MUST slot needs the sum of the dfs of its in-range SHOULD slots; a query with a MUST slot out of range or of df 0 needs none.
 *   d_counts[0] = the places of all queries; capacity_candidates bounds them ("InvalidArgumentError: capacity_candidates: smaller than the
 *   number of candidates" at the sync, d_counts[0] then holds the number needed).  The sum of the dfs of all in-range slots always suffices.
 *   Launches (kernels_postings_boolean.hip), none sized from a value read back: queries (a lane per query: the occurs, the anchor, whether a
 *   MUST_NOT slot is there), slots (the OR search's checks; a slot's places), the trainer's scan, expand (a lane per place: its posting with
 *   the OR search's checks; in an anchored query every other in-range slot of the query is bisected in its list -- at most 64 steps inside
 *   the term's two bounds, which are clamped to capacity_postings -- for the anchor's document: a MUST slot without it or a MUST_NOT slot
 *   with it drops the place, the others add their c in slot order; in a query without an anchor only its MUST_NOT slots are bisected, and
 *   none when it has none); from the first sort on, the launches of vpt_postings_search_device as they stand.  No atomic decides a value;
 *   every loop is bounded by 1024 slots or 64 halvings.
 *   Scratch of the workspace: the OR search's (20 bytes per slot of capacity_slots, 44 bytes per place of capacity_candidates, 8 bytes per
 *   query, the histograms) and 12 bytes more per query (the anchor, a flag word).
 *   At the call, VPT_INVALID_ARGUMENT: vpt_postings_search_device's list, d_query_occurs NULL included.
 *   At the sync, VPT_INVALID_ARGUMENT: vpt_postings_search_device's list and "InvalidArgumentError: occurs: a value above 2"; after any of
 *   these the four outputs are as they were before the call.  Only a list that deals out places (the anchor's, or a SHOULD slot's in a query
 *   without an anchor) is checked for ascent, tf and document range posting by posting; of a bisected list the two bounds are checked
 *   (every in-range slot's, as in the OR search), and a posting found there with tf 0 is "segment: term_offsets or postings are not a
 *   segment's".  A bisected list that does not ascend is not reported: the bisection ends inside the list's bounds on some posting, and the
 *   answer is that posting's.  Whatever the arrays hold, nothing is read outside term_offsets[0 .. n_terms], [0, capacity_postings),
 *   doc_lens[0 .. n_documents) and the query arrays' stated sizes, and nothing is written outside the four outputs' stated sizes, d_counts [3]
 *   and the workspace.
 * vpt_postings_boolean_search: the same over HOST arrays, as vpt_postings_search is; the places are counted on the host by the rule above. */
enum { VPT_OCCUR_SHOULD = 0, VPT_OCCUR_MUST = 1, VPT_OCCUR_MUST_NOT = 2 };
vpt_status vpt_postings_boolean_search_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_term_offsets, const uint32_t *d_post_docs,
                                              const uint32_t *d_post_tfs, uint32_t n_terms, uint64_t capacity_postings, uint64_t doc_base,
                                              uint64_t n_documents, const uint32_t *d_doc_lens, const uint64_t *d_query_offsets,
                                              const int32_t *d_query_terms, const float *d_query_weights, const uint8_t *d_query_occurs,
                                              uint32_t n_queries, uint64_t capacity_slots, float k1, float b_param, float avgdl, uint32_t k,
                                              uint64_t capacity_candidates, uint32_t *d_hit_docs, float *d_hit_scores, uint32_t *d_hit_counts,
                                              uint64_t *d_match_counts, uint64_t *d_counts, void *hip_stream);
vpt_status vpt_postings_boolean_search(const vpt_predictor *p, const uint64_t *term_offsets, const uint32_t *post_docs, const uint32_t *post_tfs,
                                       uint32_t n_terms, uint64_t doc_base, uint64_t n_documents, const uint32_t *doc_lens,
                                       const uint64_t *query_offsets, const int32_t *query_terms, const float *query_weights,
                                       const uint8_t *query_occurs, uint32_t n_queries, float k1, float b_param, float avgdl, uint32_t k,
                                       uint32_t *hit_docs_out, float *hit_scores_out, uint32_t *hit_counts_out, uint64_t *match_counts_out,
                                       uint64_t *counts_out);

/* ---------------------------------------------------------------------------------------------------------
 * Phrase queries on the device: the positions of a segment, exact-phrase BM25 top-k      (the adapter indexes WithFreqsAndPositions, and positions
 *                                                 serve phrase queries: what tantivy's query parser makes of a query text of several tokens)
 *
 * vpt_postings_positions_device: the position lists of a segment, behind a vpt_postings_batch_device call that was given the optional pair.
 *   d_token_offsets [n_documents + 1], capacity_in: as that call took them.  d_token_positions uint32 [capacity_in] or NULL: NULL makes the
 *   position of token t of document d t - token_offsets[d]; else it is the array the stream calls write (a stop filter leaves gaps).
 *   d_term_offsets [n_terms + 1]: the postings are min(d_term_offsets[n_terms], capacity_postings), read on the device.  d_post_first
 *   [capacity_postings + 1], d_token_order [capacity_in]: what the postings call wrote.  Out: d_post_positions uint32 [capacity_in]; for every
 *   i below the indexed tokens post_first[postings], d_post_positions[i] = the position of token d_token_order[i]; nothing is written at or
 *   behind the indexed tokens.  One launch, a lane per place of capacity_in, the owner document by the id pass's bisection; asynchronous on
 *   hip_stream.  At the call, VPT_INVALID_ARGUMENT: a NULL pointer other than d_token_positions, n_terms == 0 or > 2^24, capacity_in >= 2^32,
 *   a workspace of another predictor.  At vpt_batch_sync, VPT_INVALID_ARGUMENT: the id pass's message when token_offsets decrease, exceed
 *   capacity_in or leave a token no document owns (a token_order entry at or above the tokens included); "InvalidArgumentError: positions: do
 *   not strictly ascend inside a document's list" when inside one posting a position is not above the one before it (checked against the
 *   neighbour in the same posting; the search's bisection relies on it).  Whatever the arrays hold, a token index is below
 *   min(token_offsets[n], capacity_in) before anything is read through it and a place below capacity_in before it is written.
 *
 * A POSITIONAL SEGMENT is a segment's three arrays plus post_first [postings + 1] and post_positions [indexed tokens]: posting q's positions are
 *   post_positions[post_first[q] .. post_first[q + 1]), strictly ascending, post_tfs[q] of them.
 *
 * vpt_postings_phrase_search_device: a batch of exact-phrase queries against ONE positional segment.
 *   Segment: d_term_offsets [n_terms + 1], d_post_docs / d_post_tfs [capacity_postings], d_post_first [capacity_postings + 1],
 *   d_post_positions [capacity_positions].  Documents: doc_base, n_documents, d_doc_lens as in vpt_postings_search_device.
 *   Queries, a CSR: d_query_offsets [n_queries + 1], d_query_terms int32 [capacity_slots]; query q is ONE phrase, its slots in order.
 *   d_query_weights float [n_queries]: one weight per query, the caller's (the wrappers pass tantivy's phrase weight: the binary32 sum, in slot
 *   order, of vpt_okapi_idf of every slot's term); the device never takes a logarithm.
 *   Occurrence: phrase q of L >= 1 slots occurs in document d at start s when for every j in [0, L) the positions of posting (term_j, d)
 *   contain s + j (64-bit arithmetic; a repeated term is two distinct places).  pf(q, d) = the number of distinct starts; d MATCHES q when
 *   pf >= 1.  A query with a slot outside [0, n_terms) matches nothing and adds 1 to d_counts[2]; an empty query and a query with a term of
 *   df 0 match nothing.  Slop is 0; nothing is reordered.
 *   Score, in IEEE binary32, round to nearest, no contraction, in exactly the order of vpt_postings_search_device's c, with the query's weight
 *   w and f = float(pf):
 *       r = float(dl[d - doc_base]) / avgdl;  K = k1 * ((1.0f - b) + b * r);  f = float(pf);  score = w * ((f * (k1 + 1.0f)) / (f + K))
 *   one c, no sum: a phrase of one slot has the bits vpt_postings_search_device gives a one-slot query of the same weight.
 *   Output, per query q: d_match_counts[q] = the matching documents; d_hit_counts[q] = min(k, matches); d_hit_docs[q * k + j] /
 *   d_hit_scores[q * k + j] / d_hit_freqs[q * k + j] (uint32, the hit's pf; d_hit_freqs may be NULL) for j below the hit count = the matches by
 *   score descending, then document ascending; entries at or behind the hit count are not written.  d_counts [3] = the probes (below), the
 *   matches of all queries, the skipped queries.  Two runs, on one workspace or on two, give identical bytes.
 *   Launches (kernels_postings_phrase.hip), each sized from n_queries, capacity_probes or n_queries * k, none from a value read back.  A
 *   query's ANCHOR is the slot whose term has the fewest indexed tokens, post_first[term_offsets[t + 1]] - post_first[term_offsets[t]], the
 *   first such slot; its PROBES are the anchor term's positions, one contiguous run of post_positions (0 when the query cannot match);
 *   capacity_probes bounds the sum over the queries.  queries (a lane per query: checks, anchor, probe count), the trainer's scan (probe
 *   bases), probe (a lane per probe place: its posting by bisection over post_first, start = position - anchor slot, every other slot's
 *   posting of that document by bisection over post_docs and start + j by bisection over its positions), the trainer's scan, heads (pf = the
 *   scan's difference over a posting), the trainer's scan, emit (hits are born in (query, document) order) and ranges, the trainer's stable
 *   radix sort over ~bits(score) (4 passes) and the query word, take.  Asynchronous on hip_stream, errors at vpt_batch_sync; no atomic decides a
 *   value.  Scratch of the workspace: 36 bytes per query, nothing per slot, 48 bytes per place of capacity_probes (a hit of three words, a scan
 *   word, seven index and flag words) and 16 bytes per 16 places of histograms.
 *   At the call, VPT_INVALID_ARGUMENT: vpt_postings_search_device's list, with d_post_first / d_post_positions among the pointers,
 *   capacity_probes for capacity_candidates and d_hit_freqs the one pointer that may be NULL.
 *   At the sync, VPT_INVALID_ARGUMENT: the query_offsets, segment and weights messages of vpt_postings_search_device (segment: a slot's term
 *   bounds descend or end above capacity_postings; post_first of a term's two bounds or of a probed posting descend or exceed
 *   capacity_positions, or their difference is not the posting's tf; a probed posting's document outside [doc_base, doc_base + n_documents) or
 *   not above the one before it -- all seen before doc_lens is touched); "InvalidArgumentError: query: a phrase of more than 64 terms"
 *   (vpt_postings_phrase_limits); "InvalidArgumentError: capacity_probes: smaller than the number of probes" -- d_counts[0] then holds the
 *   number needed.  After any of these the five outputs are as they were before the call; d_counts[0] is the probes (the need), d_counts[1] and
 *   d_counts[2] are written and unspecified.  Positions that do not ascend inside a posting are
 *   NOT seen here (vpt_postings_positions_device reports them): the result is then unspecified.  Whatever the arrays hold, nothing is read
 *   outside the stated sizes and nothing is written outside the five outputs' stated sizes, d_counts [3] and the workspace.
 * vpt_postings_phrase_limits: the most slots a phrase may have.
 * vpt_postings_phrase_search: the same over HOST arrays (post_first[term_offsets[n_terms]] positions); the probes are counted on the host as
 *   the device counts them, the device call runs once, the five outputs and counts_out [3] come back (hit entries at or behind a query's hit
 *   count come back 0).  Returns when the device is through.
 * vpt_token_stream_positional_postings_batch: vpt_token_stream_postings_batch's steps, also returning post_first_out [capacity + 1] and
 *   post_positions_out [capacity_positions], the latter from the stream's token_positions; *n_positions_out = the indexed tokens.  More than
 *   capacity_positions of them: VPT_INVALID_ARGUMENT "InvalidArgumentError: capacity_positions: smaller than the number of indexed tokens",
 *   *n_positions_out = the number needed. */
vpt_status vpt_postings_positions_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_token_offsets, size_t n_documents,
                                         uint64_t capacity_in, const uint32_t *d_token_positions, const uint64_t *d_term_offsets,
                                         uint32_t n_terms, const uint64_t *d_post_first, uint64_t capacity_postings,
                                         const uint32_t *d_token_order, uint32_t *d_post_positions, void *hip_stream);
vpt_status vpt_postings_phrase_search_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_term_offsets, const uint32_t *d_post_docs,
                                             const uint32_t *d_post_tfs, const uint64_t *d_post_first, const uint32_t *d_post_positions,
                                             uint32_t n_terms, uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base,
                                             uint64_t n_documents, const uint32_t *d_doc_lens, const uint64_t *d_query_offsets,
                                             const int32_t *d_query_terms, const float *d_query_weights, uint32_t n_queries,
                                             uint64_t capacity_slots, float k1, float b_param, float avgdl, uint32_t k, uint64_t capacity_probes,
                                             uint32_t *d_hit_docs, float *d_hit_scores, uint32_t *d_hit_freqs, uint32_t *d_hit_counts,
                                             uint64_t *d_match_counts, uint64_t *d_counts, void *hip_stream);
vpt_status vpt_postings_phrase_limits(uint32_t *max_phrase_terms);
vpt_status vpt_postings_phrase_search(const vpt_predictor *p, const uint64_t *term_offsets, const uint32_t *post_docs, const uint32_t *post_tfs,
                                      const uint64_t *post_first, const uint32_t *post_positions, uint32_t n_terms, uint64_t doc_base,
                                      uint64_t n_documents, const uint32_t *doc_lens, const uint64_t *query_offsets, const int32_t *query_terms,
                                      const float *query_weights, uint32_t n_queries, float k1, float b_param, float avgdl, uint32_t k,
                                      uint32_t *hit_docs_out, float *hit_scores_out, uint32_t *hit_freqs_out, uint32_t *hit_counts_out,
                                      uint64_t *match_counts_out, uint64_t *counts_out);
vpt_status vpt_token_stream_positional_postings_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets,
                                                      size_t n_documents, unsigned wsconst_flags, const void *tagger, const void *stop,
                                                      const void *vocab, unsigned vocab_flags, uint64_t doc_base, uint64_t *term_offsets_out,
                                                      uint32_t *post_docs_out, uint32_t *post_tfs_out, uint64_t *post_first_out,
                                                      uint64_t capacity, uint32_t *post_positions_out, uint64_t capacity_positions,
                                                      uint64_t *n_postings_out, uint64_t *n_dropped_out, uint64_t *n_positions_out);

/* ---------------------------------------------------------------------------------------------------------
 * Phrase clauses in boolean queries: phrases to posting lists, the boolean search over a segment and such lists      (tantivy's query parser
 *                                                            makes a clause of several tokens a PhraseQuery inside the BooleanQuery: `+東京都`)
 *
 * vpt_postings_phrase_lists_device: a batch of phrases against ONE positional segment, each phrase's matching documents out as a posting list.
 *   Segment: d_term_offsets, d_post_docs, d_post_tfs, d_post_first, d_post_positions, n_terms, capacity_postings, capacity_positions, doc_base
 *   and n_documents as vpt_postings_phrase_search_device takes them (doc_base and n_documents for the range checks; no doc_lens, weights, k1,
 *   b, avgdl or k).  Phrases, a CSR: d_phrase_offsets [n_phrases + 1], d_phrase_terms int32 [capacity_slots].  capacity_probes: as in the
 *   phrase search.
 *   Out: d_list_offsets uint64 [n_phrases + 1], d_list_docs / d_list_tfs uint32 [capacity_lists]: list q is the entries
 *   [d_list_offsets[q], d_list_offsets[q + 1]); d_list_docs holds the GLOBAL numbers of the documents that match phrase q, ascending, and
 *   d_list_tfs their pf >= 1; d_list_offsets[0] = 0, entries at or behind d_list_offsets[n_phrases] are not written.  d_counts [3] = the
 *   probes, the list entries of all phrases, the skipped phrases.
 *   pf and "matches" are vpt_postings_phrase_search_device's: slop 0, 64-bit starts, a repeated term is two distinct places.  A phrase matches
 *   nothing and its list is empty when it is empty, has a slot outside [0, n_terms) (it adds 1 to d_counts[2]) or has a term of df 0.  A phrase
 *   of one in-range term has that term's own list: its documents and its tfs.
 *   A phrase's list never has more entries than the smallest df among its terms: the sum of those over the phrases always suffices as
 *   capacity_lists.
 *   Launches: the phrase search's queries, scan, probe, scan, heads and scan as they stand (no weight is looked at), then lists
 *   (kernels_postings_phrase.hip): a lane per place, a head writes {doc_base + document, pf} at its scan index -- entries are born in (phrase,
 *   document) order; a lane per phrase bound writes d_list_offsets by the phrase search's ranges rule.  No sort, no take.  Nothing is sized
 *   from a value read back, no atomic decides a value, two runs give identical bytes.  Scratch of the workspace: the phrase search's.
 *   At the call, VPT_INVALID_ARGUMENT: a NULL pointer, n_terms == 0 or > 2^24, "n_phrases: must be between 1 and 2^24", capacity_slots or
 *   capacity_probes >= 2^32 (the phrase search's message), "capacity_lists: must be below 2^32", doc_base + n_documents above 2^32, a
 *   workspace of another predictor.
 *   At the sync, VPT_INVALID_ARGUMENT: the segment and query_offsets messages and the 64-term limit of vpt_postings_phrase_search_device;
 *   capacity_probes too small (d_counts[0] holds the need); "InvalidArgumentError: capacity_lists: smaller than the number of list entries"
 *   (d_counts[1] holds the need).  After any of these the three list arrays are as they were before the call.  Whatever the arrays hold,
 *   nothing is read outside the stated sizes and nothing is written outside d_list_offsets [n_phrases + 1], d_list_docs / d_list_tfs
 *   [capacity_lists], d_counts [3] and the workspace.
 *
 * vpt_postings_clause_search_device: vpt_postings_boolean_search_device over a segment PLUS derived lists.  Every argument of that call with
 *   the same meaning, and d_list_offsets uint64 [n_lists + 1], d_list_docs / d_list_tfs uint32 [capacity_lists], n_lists
 *   (n_terms + n_lists <= 2^24), capacity_lists (< 2^32): what the lists call wrote, or any arrays of that shape.  n_lists may be 0; the three
 *   pointers are then not looked at.
 *   A slot whose d_query_terms value t lies in [n_terms, n_terms + n_lists) names list t - n_terms, and is for the rest of the rule a term
 *   whose list is that list: has-document, df (d_list_offsets[i + 1] - d_list_offsets[i]), the anchor choice (the first MUST slot of the
 *   smallest df, read on the device), the veto, and c from the entry's tf -- for a list of the lists call c is bm25 of (w, pf, dl): the
 *   bits vpt_postings_phrase_search_device gives the phrase under the same weight.  A value at or above n_terms + n_lists or below 0 is out
 *   of range as in the boolean search.  Everything else of vpt_postings_boolean_search_device's definition, order, outputs, counts, places and
 *   determinism holds verbatim; with n_lists = 0 the four outputs and the counts are that call's, byte for byte.
 *   Launches: the boolean search's three kernels as one body over one or two segments (kernels_postings_boolean.hip), then the OR search's
 *   launches from the first sort on.  Scratch: the boolean search's.
 *   THE STATUS IS STICKY until vpt_batch_sync: a lists call and a clause search enqueued on one stream with no sync between them is the
 *   intended use, and an error of the lists call (or of anything else enqueued since the last sync that sets one of the search, phrase or lists
 *   bits) leaves the clause search's four outputs as they were before the call.
 *   At the call: the boolean search's list; a NULL list pointer with n_lists > 0; "InvalidArgumentError: n_lists: n_terms + n_lists must
 *   not exceed 2^24"; "InvalidArgumentError: capacity_lists: must be below 2^32".
 *   At the sync: the boolean search's list; a derived list is checked as a segment's list is (bounds that descend or end above
 *   capacity_lists, and in a list that deals out places a tf of 0, a document outside the range or not above the one before it, are
 *   "segment: term_offsets or postings are not a segment's").  Whatever the arrays hold, nothing is read outside the boolean search's sizes,
 *   d_list_offsets [n_lists + 1] and [0, capacity_lists) of the two list arrays, and nothing is written outside the four outputs, d_counts
 *   [3] and the workspace.
 *
 * vpt_postings_phrase_lists: the lists call over HOST arrays; the probes are counted on the host, capacity_lists is the size of the caller's
 *   list_docs_out / list_tfs_out.  counts_out [3] comes back after an error at the sync too (the need).
 * vpt_postings_clause_search: queries of CLAUSES over a host positional segment.  query_offsets [n_queries + 1] is a CSR over the clauses,
 *   clause_offsets [clauses + 1] a CSR over clause_terms; clause_weights / clause_occurs: one per clause.  A clause of exactly one term is a
 *   slot of that term; every other clause is a phrase (an empty one matches nothing) whose list the lists call makes and whose slot names
 *   that list.  One upload, the two device calls with no sync between them, one download; the probes, list entries and places are counted on
 *   the host by the bounds above.  counts_out [3] = the places, the matches, the skipped slots plus the phrases with a term out of range. */
vpt_status vpt_postings_phrase_lists_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_term_offsets, const uint32_t *d_post_docs,
                                            const uint32_t *d_post_tfs, const uint64_t *d_post_first, const uint32_t *d_post_positions,
                                            uint32_t n_terms, uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base,
                                            uint64_t n_documents, const uint64_t *d_phrase_offsets, const int32_t *d_phrase_terms,
                                            uint32_t n_phrases, uint64_t capacity_slots, uint64_t capacity_probes, uint64_t *d_list_offsets,
                                            uint32_t *d_list_docs, uint32_t *d_list_tfs, uint64_t capacity_lists, uint64_t *d_counts,
                                            void *hip_stream);
vpt_status vpt_postings_clause_search_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_term_offsets, const uint32_t *d_post_docs,
                                             const uint32_t *d_post_tfs, uint32_t n_terms, uint64_t capacity_postings,
                                             const uint64_t *d_list_offsets, const uint32_t *d_list_docs, const uint32_t *d_list_tfs,
                                             uint32_t n_lists, uint64_t capacity_lists, uint64_t doc_base, uint64_t n_documents,
                                             const uint32_t *d_doc_lens, const uint64_t *d_query_offsets, const int32_t *d_query_terms,
                                             const float *d_query_weights, const uint8_t *d_query_occurs, uint32_t n_queries,
                                             uint64_t capacity_slots, float k1, float b_param, float avgdl, uint32_t k,
                                             uint64_t capacity_candidates, uint32_t *d_hit_docs, float *d_hit_scores, uint32_t *d_hit_counts,
                                             uint64_t *d_match_counts, uint64_t *d_counts, void *hip_stream);
vpt_status vpt_postings_phrase_lists(const vpt_predictor *p, const uint64_t *term_offsets, const uint32_t *post_docs, const uint32_t *post_tfs,
                                     const uint64_t *post_first, const uint32_t *post_positions, uint32_t n_terms, uint64_t doc_base,
                                     uint64_t n_documents, const uint64_t *phrase_offsets, const int32_t *phrase_terms, uint32_t n_phrases,
                                     uint64_t *list_offsets_out, uint32_t *list_docs_out, uint32_t *list_tfs_out, uint64_t capacity_lists,
                                     uint64_t *counts_out);
vpt_status vpt_postings_clause_search(const vpt_predictor *p, const uint64_t *term_offsets, const uint32_t *post_docs, const uint32_t *post_tfs,
                                      const uint64_t *post_first, const uint32_t *post_positions, uint32_t n_terms, uint64_t doc_base,
                                      uint64_t n_documents, const uint32_t *doc_lens, const uint64_t *query_offsets,
                                      const uint64_t *clause_offsets, const int32_t *clause_terms, const float *clause_weights,
                                      const uint8_t *clause_occurs, uint32_t n_queries, float k1, float b_param, float avgdl, uint32_t k,
                                      uint32_t *hit_docs_out, float *hit_scores_out, uint32_t *hit_counts_out, uint64_t *match_counts_out,
                                      uint64_t *counts_out);

/* ---------------------------------------------------------------------------------------------------------
 * Sloppy phrase queries on the device: a slop budget per phrase                     (tantivy's PhraseQuery::set_slop, `"東京 特許"~2`: behind a
 *                                        morphological tokenizer a particle or another split between two query tokens makes an exact phrase miss)
 *
 * vpt_postings_sloppy_phrase_search_device: vpt_postings_phrase_search_device's arguments plus d_query_slops uint32 [n_queries] (NULL: every
 *   slop 0), one slop in [0, 31] per query (vpt_postings_sloppy_phrase_limits).
 *   THE DEFINITION.  A query is one phrase of L slots with one weight and one slop.  For slot j and document d the ADJUSTED POSITIONS are
 *   p - j over the positions p of posting (term_j, d): signed 64-bit values, which may be negative.  An integer s is an OCCURRENCE of the
 *   phrase in d when (1) every slot j has an adjusted position in [s, s + slop] and (2) some slot has the adjusted position s itself.
 *   pf(q, d) = the number of distinct occurrences, clamped to 2^32 - 1; d MATCHES q when pf >= 1; the score is the exact search's, with
 *   f = float(pf).  Put another way: one position is chosen per slot, the choice matches when max(p_j - j) - min(p_j - j) <= slop, and pf
 *   counts the distinct minima of the matching choices.
 *   So "A B C" with slop 1 matches `A X B C` and `A B X C` but not `A X B X C`, and "A B" matches `B A` with slop 2 and not with slop 1:
 *   the cases the documentation of tantivy's set_slop lists.  The integer pf is THIS PROJECT'S OWN count (no tantivy source was at hand to
 *   compare the phrase frequency of a sloppy match against); which documents match is what those cases fix.
 *   Slots choose independently: a token may serve two slots that name the same term, so "A A" with slop 1 matches a document with a single
 *   A (at position p: s = p - 1).  With slop 0 the definition is the exact search's: every adjusted position equals s, s >= 0 follows from slot 0, a
 *   repeated term needs two distinct places -- with every slop 0, or d_query_slops NULL, the five outputs and d_counts are
 *   vpt_postings_phrase_search_device's byte for byte.  The result is a function of the document: it does not depend on the anchor.
 *   Launches: the exact search's, with the sloppy probe in probe's place (kernels_postings_phrase.hip).  A lane per probe place makes
 *   probe's checks; with a = its anchor position - anchor slot it OWNS the occurrences s in [lo, a], lo = max(a - slop, a_prev + 1), a_prev
 *   the adjusted position of the place before it in the same posting -- every occurrence has an anchor position in [s, s + slop] and
 *   belongs to the lane of the first one at or after s.  Per slot (the anchor's included, a repeated term like any other): the document's
 *   posting by bisection, one bisection to the first position >= max(lo + j, 0), a walk of at most 2 * slop + 1 places (bounded by the
 *   count of steps, not by the values read) that sets bit p - j - lo of a 64-bit mask M_j (2 * 31 + 1 = 63 bits: the limit); C_j = M_j
 *   smeared down by 0 .. slop; the lane's count = popcount(AND C_j & OR M_j & bits [0, a - lo]), 0 .. 32.  heads sums the counts of a
 *   posting (the scan's difference) and clamps.  No LDS, no atomic other than the status OR.  Probes, capacity_probes, scratch, counts and
 *   determinism: the exact search's.
 *   At the call: the exact search's list.  At the sync: the exact search's list, and "InvalidArgumentError: query: a slop above 31"; after
 *   any of them the five outputs are as they were.  Positions that do not ascend inside a posting: the result is unspecified and bounded
 *   as in the exact search; nothing is read outside the stated sizes and d_query_slops [n_queries].
 * vpt_postings_sloppy_phrase_lists_device: vpt_postings_phrase_lists_device's arguments plus d_phrase_slops uint32 [n_phrases] (NULL: all
 *   0); the lists hold the sloppy pf and feed vpt_postings_clause_search_device unchanged.  A phrase of one in-range term has that term's
 *   own list at any slop.  A slop above 31: the message above at the sync, no list is written, and a clause search enqueued behind it
 *   leaves its outputs alone.
 * vpt_postings_sloppy_phrase_limits: the most slots a phrase may have and the largest slop.
 * vpt_postings_sloppy_phrase_search, vpt_postings_sloppy_phrase_lists: the same over HOST arrays, as vpt_postings_phrase_search and
 *   vpt_postings_phrase_lists are (query_slops / phrase_slops NULL: all 0).
 * vpt_postings_sloppy_clause_search: vpt_postings_clause_search with clause_slops uint32 [clauses] (NULL: all 0): the slop of every clause
 *   that is a phrase; a one-term clause's entry is not looked at. */
vpt_status vpt_postings_sloppy_phrase_search_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_term_offsets,
                                                    const uint32_t *d_post_docs, const uint32_t *d_post_tfs, const uint64_t *d_post_first,
                                                    const uint32_t *d_post_positions, uint32_t n_terms, uint64_t capacity_postings,
                                                    uint64_t capacity_positions, uint64_t doc_base, uint64_t n_documents,
                                                    const uint32_t *d_doc_lens, const uint64_t *d_query_offsets, const int32_t *d_query_terms,
                                                    const float *d_query_weights, const uint32_t *d_query_slops, uint32_t n_queries,
                                                    uint64_t capacity_slots, float k1, float b_param, float avgdl, uint32_t k,
                                                    uint64_t capacity_probes, uint32_t *d_hit_docs, float *d_hit_scores, uint32_t *d_hit_freqs,
                                                    uint32_t *d_hit_counts, uint64_t *d_match_counts, uint64_t *d_counts, void *hip_stream);
vpt_status vpt_postings_sloppy_phrase_lists_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_term_offsets,
                                                   const uint32_t *d_post_docs, const uint32_t *d_post_tfs, const uint64_t *d_post_first,
                                                   const uint32_t *d_post_positions, uint32_t n_terms, uint64_t capacity_postings,
                                                   uint64_t capacity_positions, uint64_t doc_base, uint64_t n_documents,
                                                   const uint64_t *d_phrase_offsets, const int32_t *d_phrase_terms,
                                                   const uint32_t *d_phrase_slops, uint32_t n_phrases, uint64_t capacity_slots,
                                                   uint64_t capacity_probes, uint64_t *d_list_offsets, uint32_t *d_list_docs,
                                                   uint32_t *d_list_tfs, uint64_t capacity_lists, uint64_t *d_counts, void *hip_stream);
vpt_status vpt_postings_sloppy_phrase_limits(uint32_t *max_phrase_terms, uint32_t *max_slop);
vpt_status vpt_postings_sloppy_phrase_search(const vpt_predictor *p, const uint64_t *term_offsets, const uint32_t *post_docs,
                                             const uint32_t *post_tfs, const uint64_t *post_first, const uint32_t *post_positions,
                                             uint32_t n_terms, uint64_t doc_base, uint64_t n_documents, const uint32_t *doc_lens,
                                             const uint64_t *query_offsets, const int32_t *query_terms, const float *query_weights,
                                             const uint32_t *query_slops, uint32_t n_queries, float k1, float b_param, float avgdl, uint32_t k,
                                             uint32_t *hit_docs_out, float *hit_scores_out, uint32_t *hit_freqs_out, uint32_t *hit_counts_out,
                                             uint64_t *match_counts_out, uint64_t *counts_out);
vpt_status vpt_postings_sloppy_phrase_lists(const vpt_predictor *p, const uint64_t *term_offsets, const uint32_t *post_docs,
                                            const uint32_t *post_tfs, const uint64_t *post_first, const uint32_t *post_positions,
                                            uint32_t n_terms, uint64_t doc_base, uint64_t n_documents, const uint64_t *phrase_offsets,
                                            const int32_t *phrase_terms, const uint32_t *phrase_slops, uint32_t n_phrases,
                                            uint64_t *list_offsets_out, uint32_t *list_docs_out, uint32_t *list_tfs_out,
                                            uint64_t capacity_lists, uint64_t *counts_out);
vpt_status vpt_postings_sloppy_clause_search(const vpt_predictor *p, const uint64_t *term_offsets, const uint32_t *post_docs,
                                             const uint32_t *post_tfs, const uint64_t *post_first, const uint32_t *post_positions,
                                             uint32_t n_terms, uint64_t doc_base, uint64_t n_documents, const uint32_t *doc_lens,
                                             const uint64_t *query_offsets, const uint64_t *clause_offsets, const int32_t *clause_terms,
                                             const float *clause_weights, const uint8_t *clause_occurs, const uint32_t *clause_slops,
                                             uint32_t n_queries, float k1, float b_param, float avgdl, uint32_t k, uint32_t *hit_docs_out,
                                             float *hit_scores_out, uint32_t *hit_counts_out, uint64_t *match_counts_out,
                                             uint64_t *counts_out);

/* ---------------------------------------------------------------------------------------------------------
 * Merging POSITIONAL segments on the device: phrase search over a corpus indexed in batches          (no item of the adapter: the merge above
 *                                                                         with the position lists carried along, so the merged index serves phrases)
 *
 * vpt_postings_positional_segment: a positional segment as vpt_postings_batch_device with the optional pair and vpt_postings_positions_device
 *   (or this call) left it.  Its postings are d_term_offsets[n_terms], its positions d_post_first[postings]; both are read on the device, so K
 *   postings calls, K positions calls and the merge behind them need no sync in between; the two capacities bound them. */
typedef struct vpt_postings_positional_segment {
    const uint64_t *d_term_offsets;   /* [n_terms + 1]                                                         */
    const uint32_t *d_post_docs;      /* [capacity], global document numbers                                   */
    const uint32_t *d_post_tfs;       /* [capacity]                                                            */
    const uint64_t *d_post_first;     /* [capacity + 1]                                                        */
    const uint32_t *d_post_positions; /* [capacity_positions]                                                  */
    uint32_t        n_terms;          /* <= n_terms_out; terms at or above it have no postings here            */
    uint64_t        capacity;         /* the postings: d_term_offsets[n_terms]                                 */
    uint64_t        capacity_positions; /* the positions: d_post_first[postings]                               */
} vpt_postings_positional_segment;
/* vpt_postings_merge_positional_device: `segments` is a HOST array of n_segments (1 .. 1024, vpt_postings_merge_limits)
 *   vpt_postings_positional_segment structs whose pointers are device pointers; flags as vpt_postings_merge_device takes them.  ONE positional
 *   segment comes out: d_term_offsets_out [n_terms_out + 1], d_post_docs_out / d_post_tfs_out [capacity_out] are exactly what
 *   vpt_postings_merge_device writes for the same segments and flags; d_post_first_out [capacity_out + 1]: post_first_out[0] = 0,
 *   post_first_out[q + 1] - post_first_out[q] = post_tfs_out[q], post_first_out[merged postings] = d_counts[2]; d_post_positions_out
 *   [capacity_positions_out]: the position list of the merged posting (term k, document d) is the ascending union of the position lists of every
 *   input posting (k, d).  d_counts [3] = the merged postings, the input postings combined into another, the merged positions.  Nothing is
 *   written at or behind the merged postings + 1 entries of post_first_out or behind d_counts[2] positions.  The result is what
 *   vpt_postings_phrase_search_device takes as it is.  So: however a batch's indexed tokens are dealt out to segments -- token_positions given to
 *   the positions call so that every token keeps its position in its document --, the merge with flags 0 is, array for array, the one-pass
 *   positional segment of the whole batch.  THE OUTPUTS MUST NOT ALIAS THE INPUTS.
 *   Launches (kernels_postings_merge.hip), sized from the places of the posting arrays (the sum of the capacities), the POSITION PLACES (the
 *   segments' capacity_positions laid end to end), the term bounds or the segments, none from a value read back.
 *   VPT_POSTINGS_MERGE_ORDERED: the table applied to post_first.  The positions of segment s in front of term k are
 *   post_first_s[term_offsets_s[k]], so a lane per term bound sums them over the segments -- the merged position offset of the term, no scan --
 *   and leaves where every segment's positions of the term start in the output (a SECOND K x (n_terms_out + 1) table of 8-byte words); the copy
 *   of a posting also writes its post_first; a lane per position place finds its segment, its posting (over post_first) and its term (over
 *   term_offsets) by bisection and copies its position.
 *   flags = 0: behind the merge's records, sort and heads, the tf of every sorted input posting is scanned (post_first of a merged posting is
 *   the scan at its head) and the inverse of the sort order is scattered; a lane per position place finds its segment and posting by
 *   bisection, the posting's run of at most n_segments input postings of one (term, document), and adds to its rank in its own posting the
 *   positions below its own in every other member of the run, one bisection each.  No second sort.
 *   Both: asynchronous on hip_stream, errors at vpt_batch_sync; no atomic decides a value, every loop is bounded by n_segments or 64 bisection
 *   steps, two runs give identical bytes.  Scratch of the workspace: what vpt_postings_merge_device keeps, and 32 bytes more per segment;
 *   ordered a second 8 * n_segments * (n_terms_out + 1) bytes; general 16 bytes more per input place (48 in all: a tf word, an inverse index
 *   word, a second scan word).
 *   At the call, VPT_INVALID_ARGUMENT: what vpt_postings_merge_device refuses, with d_post_first / d_post_positions of every segment and
 *   d_post_first_out / d_post_positions_out among the pointers that must not be NULL; a sum of capacity_positions >= 2^32;
 *   capacity_positions_out >= 2^32.
 *   At the sync, VPT_INVALID_ARGUMENT: the merge's messages -- the segment message also when a segment's post_first[0] != 0, post_first
 *   descends or ends above capacity_positions, or post_first[i + 1] - post_first[i] != post_tfs[i] --; "InvalidArgumentError: positions: do not
 *   strictly ascend inside a document's list" when positions do not strictly ascend inside an input posting or two input postings of one
 *   (term, document) hold an equal position (the outputs are then unspecified); "InvalidArgumentError: capacity_positions: smaller than the
 *   number of indexed tokens" when there are more than capacity_positions_out merged positions -- d_counts[2] then holds the number needed and
 *   what fits is written; the capacity message of the merge as there.  capacity_positions_out >= the sum of the capacity_positions always
 *   suffices.  Whatever the arrays hold, every index is clamped or bounded before use: nothing is read outside the segments' stated sizes and
 *   nothing is written outside the five outputs' stated sizes, d_counts [3] and the workspace.
 * vpt_postings_merge_positional: the same over HOST arrays: each segment's term_offsets[n_terms] postings and post_first[postings] positions
 *   are uploaded; five arrays come back with *n_postings_out, *n_combined_out and *n_positions_out.  Too small a `capacity` or
 *   `capacity_positions`: VPT_INVALID_ARGUMENT with the message above, the three numbers as needed, nothing else written.
 * (`segments` is declared const void *; pass a const vpt_postings_positional_segment *.) */
vpt_status vpt_postings_merge_positional_device(const vpt_predictor *p, vpt_batch *b, const void *segments, size_t n_segments,
                                                uint32_t n_terms_out, unsigned flags, uint64_t *d_term_offsets_out, uint32_t *d_post_docs_out,
                                                uint32_t *d_post_tfs_out, uint64_t *d_post_first_out, uint64_t capacity_out,
                                                uint32_t *d_post_positions_out, uint64_t capacity_positions_out, uint64_t *d_counts,
                                                void *hip_stream);
vpt_status vpt_postings_merge_positional(const vpt_predictor *p, const void *segments, size_t n_segments, uint32_t n_terms_out, unsigned flags,
                                         uint64_t *term_offsets_out, uint32_t *post_docs_out, uint32_t *post_tfs_out, uint64_t *post_first_out,
                                         uint64_t capacity, uint32_t *post_positions_out, uint64_t capacity_positions,
                                         uint64_t *n_postings_out, uint64_t *n_combined_out, uint64_t *n_positions_out);

/* ConcatGraphemeClustersFilter on the CALLER'S labels (for callers that want it at another place among their filters than
 * VPT_FLAG_CONCAT_GRAPHEMES puts it): labels[out_offsets[i] + b] = 0 for every boundary b of sentence i inside an extended grapheme cluster; no
 * other label is written.  out_offsets from vpt_count_boundaries.
 * vpt_concat_graphemes_batch: host buffers; flags: 0 or VPT_FLAG_KYTEA_FULLWIDTH (the clusters of the KyteaFullwidthFilter image -- what a
 *   predict call with that flag scored); anything else is VPT_INVALID_ARGUMENT "flags: unknown bit".
 * vpt_concat_graphemes_batch_device: device pointers, asynchronous on hip_stream, VPT_FLAG_KYTEA_FULLWIDTH from vpt_batch_set_flags, the verdict
 *   (empty sentences, NUL, offsets that do not match the text) at vpt_batch_sync.
 * vpt_concat_graphemes_tile: the chars of a tile of the kernel (the tests place clusters across its edges). */
vpt_status vpt_concat_graphemes_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences,
                                      const uint64_t *out_offsets, unsigned flags, uint8_t *labels);
vpt_status vpt_concat_graphemes_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8, const uint64_t *d_byte_offsets,
                                             const uint64_t *d_out_offsets, size_t n_sentences, uint64_t total_boundaries, uint8_t *d_labels,
                                             void *hip_stream);
vpt_status vpt_concat_graphemes_tile(uint32_t *n_chars);

/* ---------------------------------------------------------------------------------------------------------
 * Sentence::from_tokenized over a batch                                                  (sentence.rs:285-514)
 *
 * Line i is utf8[byte_offsets[i] .. byte_offsets[i+1]): tokens separated by ' ', "/tag" suffixes, '\\' escaping the next char.
 * Outputs (B = the input's bytes; each bound below holds for any input that parses):
 *   raw_out [B]              the raw text (Sentence::as_raw_text), lines back to back; raw_offsets_out [S+1] their byte ranges;
 *   out_offsets_out [S+1]    laid out as vpt_count_boundaries lays it out for the raw text;
 *   labels_out [B]           the gold CharacterBoundary per boundary (Sentence::boundaries), at out_offsets[i] + b;
 *   n_tags_out [S]           Sentence::n_tags: the largest tag count of any char of the line;
 *   tag_index_out [B+1]      per char (out_offsets[i] + i + c) its first tag: char g has tags tag_index[g] .. tag_index[g+1]
 *                            (slots past them, up to n_tags, are None), tag_index[total chars] = the number of tags;
 *   span_offsets_out [B+1]   per tag its bytes in tag_bytes_out: span_offsets[k] .. span_offsets[k+1]; an empty tag is None;
 *   tag_bytes_out [B]        the tags' bytes, escapes removed.
 * Errors: VPT_INVALID_ARGUMENT "InvalidArgumentError: tokenized_text: " + the reference's reason + " (line i)" for the smallest failing line:
 *   must contain at least one character (empty, or no char at all -- where the reference divides by zero, sentence.rs:450) |
 *   must not start with a whitespace | must not contain consecutive whitespaces | must not end with a whitespace |
 *   a slash must follow a character | must not contain NULL.
 * The host variant runs on the host (no device).  The *_device variant: device pointers, each output buffer sized for `capacity` >= B
 * elements (tag_index / span_offsets: capacity + 1), asynchronous on hip_stream; errors at vpt_batch_sync -- an output that would not
 * fit `capacity` is VPT_INVALID_ARGUMENT "... text_capacity: smaller than the tokenized text" (nothing is written past the buffers). */
vpt_status vpt_parse_tokenized_batch(const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences, uint8_t *raw_out,
                                     uint64_t *raw_offsets_out, uint64_t *out_offsets_out, uint8_t *labels_out, uint32_t *n_tags_out,
                                     uint64_t *tag_index_out, uint64_t *span_offsets_out, uint8_t *tag_bytes_out);
vpt_status vpt_parse_tokenized_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8, const uint64_t *d_byte_offsets,
                                            size_t n_sentences, uint64_t capacity, uint8_t *d_raw_out, uint64_t *d_raw_offsets_out,
                                            uint64_t *d_out_offsets_out, uint8_t *d_labels_out, uint32_t *d_n_tags_out, uint64_t *d_tag_index_out,
                                            uint64_t *d_span_offsets_out, uint8_t *d_tag_bytes_out, void *hip_stream);

/* ---------------------------------------------------------------------------------------------------------
 * Sentence::from_partial_annotation / write_partial_annotation_text over a batch          (sentence.rs:516-769, 907-944)
 *
 * Line i is utf8[byte_offsets[i] .. byte_offsets[i+1]): chars alternating with boundary marks -- '-' NotWordBoundary (0), '|' WordBoundary (1),
 * ' ' Unknown (2) -- and "/tag" suffixes behind any char, '\\' escaping the next code point of an annotation.  Signatures, output arrays,
 * bounds, the capacity rule and error delivery are those of vpt_parse_tokenized_batch[_device] above; what differs:
 *   labels_out       0 / 1 / 2;
 *   tag_index_out    EVERY char may carry tags, not only a token's last one; an empty tag is None but counts towards n_tags.
 * The reference's rules, quirks included.  A char is a lead byte and the continuation bytes behind it.
 *   - The code point behind a mark (or at the line's start) is a char WHATEVER it is: ' ', '-', '|', '/' and '\\' can all be chars
 *     ("a||-b" is the raw text "a|b" with labels 1, 0).
 *   - '\\' escapes only inside the annotation.  An escaped or ordinary code point outside a tag is the error
 *     "contains an invalid boundary character: 'c'" -- c is that code point, not the backslash.
 *   - A dangling escape at the line's end is accepted ("a\\" is the one char a; "a/x\\" has the tag x).
 *   - NUL is "must not contain NULL" only where a char is expected; inside a tag it is a tag byte.
 *   - A line that ends right behind a mark is "invalid annotation"; an empty line is "must contain at least one character".
 * Errors: VPT_INVALID_ARGUMENT "InvalidArgumentError: partial_annotation_text: <reason> (line i)" for the smallest failing line and that
 * line's first error in reading order.  (The message is a C string: a NUL named by the invalid-boundary-character reason ends it.)  The
 * device returns the line, the reason and the offending code point's bytes in its status words; the host formats them at vpt_batch_sync. */
vpt_status vpt_parse_partial_batch(const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences, uint8_t *raw_out,
                                   uint64_t *raw_offsets_out, uint64_t *out_offsets_out, uint8_t *labels_out, uint32_t *n_tags_out,
                                   uint64_t *tag_index_out, uint64_t *span_offsets_out, uint8_t *tag_bytes_out);
vpt_status vpt_parse_partial_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8, const uint64_t *d_byte_offsets,
                                          size_t n_sentences, uint64_t capacity, uint8_t *d_raw_out, uint64_t *d_raw_offsets_out,
                                          uint64_t *d_out_offsets_out, uint8_t *d_labels_out, uint32_t *d_n_tags_out, uint64_t *d_tag_index_out,
                                          uint64_t *d_span_offsets_out, uint8_t *d_tag_bytes_out, void *hip_stream);
/* The other direction, from what the two parsers write: the raw text and its byte offsets, out_offsets, labels 0 / 1 / 2 and the tag arrays
 * (n_tags == NULL: no tags, the three tag arrays are not read).  text_out: the lines back to back, byte for byte write_partial_annotation_text --
 * the first char as it is; before every later char its boundary's '-' / '|' / ' '; behind a char its tags up to the last non-empty one, each
 * preceded by '/', an empty one among them an empty field (a char whose tags are all empty prints no '/').  Tags are NOT escaped (the reference
 * does not escape them), so only tags without ' ', '-', '|', '/' and '\\' parse back to themselves.  text_offsets_out [S+1]: the lines' ranges.
 * Errors (VPT_INVALID_ARGUMENT): a label above 2, an empty line, out_offsets that do not match the text, and an output larger than
 * text_capacity (nothing is written past it; raw bytes + chars + tags + tag bytes always suffices).  The host variant runs on the host; the
 * *_device variant is asynchronous on hip_stream with its errors at vpt_batch_sync. */
vpt_status vpt_write_partial_batch(const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences, const uint64_t *out_offsets,
                                   const uint8_t *labels, const uint32_t *n_tags, const uint64_t *tag_index, const uint64_t *span_offsets,
                                   const uint8_t *tag_bytes, uint8_t *text_out, uint64_t text_capacity, uint64_t *text_offsets_out);
vpt_status vpt_write_partial_batch_device(const vpt_predictor *p, vpt_batch *b, const uint8_t *d_utf8, const uint64_t *d_byte_offsets,
                                          size_t n_sentences, const uint64_t *d_out_offsets, const uint8_t *d_labels, const uint32_t *d_n_tags,
                                          const uint64_t *d_tag_index, const uint64_t *d_span_offsets, const uint8_t *d_tag_bytes,
                                          uint8_t *d_text_out, uint64_t text_capacity, uint64_t *d_text_offsets_out, void *hip_stream);

/* ---------------------------------------------------------------------------------------------------------
 * The `evaluate` CLI's counters                                                          (evaluate/src/main.rs:91-193)
 *
 * counts: eight uint64_t, indexed by VPT_EVAL_*: the char metric's TP / TN / FP / FN over the boundaries, Nagata's word metric's
 * n_sys / n_ref / n_cor, and the number of sentences.  (The reference's counters are i32; these do not wrap.)
 * The word metric compares the tag vectors of a token's last char, length included; the system side's vector is
 *   VPT_EVAL_TAGS_NONE       empty (the CLI predicts a normalised Sentence::from_raw and fills no tags): a token is correct only where the
 *                            sentence's gold has no tags;
 *   VPT_EVAL_TAGS_GOLD       the gold one (--no-norm without tags: the parsed sentence keeps its tags);
 *   VPT_EVAL_TAGS_PREDICTED  fill_tags' (predictor.rs:553-562): the records vpt_fill_tags_batch_device left on this workspace for the
 *                            same batch and the same system labels; a predictor without tag models gives empty vectors.
 * vpt_evaluate_labels_batch_device: the compare alone (device pointers, asynchronous; the counts are ADDED to d_counts) for callers with
 *   post-filters of their own: the gold side as vpt_parse_tokenized_batch_device wrote it, d_sys_labels laid out the same way.
 * vpt_evaluate_batch: tokenized lines in, counts out -- Sentence::from_tokenized, [KyteaFullwidthFilter + from_raw when flags has
 *   VPT_FLAG_KYTEA_FULLWIDTH, i.e. without --no-norm], Predictor::predict, the VPT_FLAG_WSCONST filters, [fill_tags when predict_tags],
 *   compare.  The lines are copied in, parsed, scored and compared on the device; 64 bytes come back.  Batches above a budget
 *   (VPT_EVAL_CHUNK_BYTES, 64 MB) run as chunks of whole lines; the pooled workspace keeps about 22 bytes of device memory per
 *   byte of the largest chunk (the text, the raw text, two label arrays, the tag bytes, and 8-byte tag_index / span_offsets entries
 *   sized for one per input byte): about 1.4 GB at the default.  An empty line is an error here (the CLI skips them). */
enum { VPT_EVAL_TAGS_NONE = 0, VPT_EVAL_TAGS_GOLD = 1, VPT_EVAL_TAGS_PREDICTED = 2 };
enum { VPT_EVAL_TP = 0, VPT_EVAL_TN = 1, VPT_EVAL_FP = 2, VPT_EVAL_FN = 3, VPT_EVAL_N_SYS = 4, VPT_EVAL_N_REF = 5, VPT_EVAL_N_COR = 6,
       VPT_EVAL_N_SENTENCES = 7, VPT_EVAL_COUNTS = 8 };
vpt_status vpt_evaluate_labels_batch_device(const vpt_predictor *p, vpt_batch *b, const uint64_t *d_out_offsets, size_t n_sentences,
                                            const uint8_t *d_gold_labels, const uint32_t *d_n_tags, const uint64_t *d_tag_index,
                                            const uint64_t *d_span_offsets, const uint8_t *d_tag_bytes, const uint8_t *d_sys_labels,
                                            int sys_tags, uint64_t *d_counts, void *hip_stream);
vpt_status vpt_evaluate_batch(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences,
                              unsigned flags, int predict_tags, uint64_t *counts_out);

/* ---------------------------------------------------------------------------------------------------------
 * PatternMatchTagger: rule tags for the slots fill_tags leaves None      (vaporetto_rules/src/sentence_filters/pattern_match_tagger.rs:10-41)
 *
 * The filter callers put behind Sentence::fill_tags: a table surface -> tags (HashMap<String, Vec<Option<String>>>).  Per sentence, with
 * n_tags = vpt_predictor_n_tags: for every token and every slot j < n_tags that is None, if the token's WHOLE surface is a key of the table the
 * slot becomes rules[surface].get(j) -- possibly None itself (a None entry, or a list shorter than j + 1).  Slots that are Some are never
 * touched; rule entries at j >= n_tags are ignored; Some("") is not None (as a last slot it prints a trailing '/').  A predictor whose model has
 * no tag models has n_tags == 0 and the filter changes NOTHING, as in the reference (its loop runs over the token's n_tags slots): a tagged
 * writer then writes what the untagged one writes.  The surfaces are those of the text fill_tags sees (the KyteaFullwidthFilter image under
 * VPT_FLAG_KYTEA_FULLWIDTH, as predict/src/main.rs tags the normalised sentence; the bytes printed are the caller's); rule surfaces are taken as
 * they are.  A token that touches VPT_BOUNDARY_UNKNOWN gets no rule tags (the rule stated for fill_tags above).
 *
 * The handle is an opaque `void *` (a `const void *` where it is only read): immutable after creation, tied to the predictor it was created
 * for (its device, its n_tags, its tag strings), shareable by any number of that predictor's workspaces and host threads; destroy it after them.
 * vpt_pattern_tagger_create: surfaces / offsets [n_rules + 1]: the rules' surfaces as packed UTF-8; slot_counts [n_rules]: the length of each
 *   rule's list; present [sum of slot_counts] and tag_offsets [that + 1]: per (rule, slot), in order, present != 0: Some(tag_bytes[tag_offsets[k] ..
 *   tag_offsets[k + 1])), else None.  A duplicate surface keeps the LAST rule (HashMap::insert).  The table -- open addressing over (code
 *   points, length), at most half full, the whole surface kept for verification -- is built on the host and uploaded once.
 *   Errors, VPT_INVALID_ARGUMENT "InvalidArgumentError: rules: <reason> (rule i)" for the first failing rule: a surface is not valid UTF-8 | a
 *   surface must contain at least one character | a surface must not contain NULL | a tag must not contain NULL.
 * Encoding: a rule tag is -(2 + id) wherever a tag index is an int32 (the dense arrays of the fill_tags calls and of
 *   vpt_expand_tags_batch_device); -1 stays None and values >= 0 stay candidates of the token's tag model.  id < vpt_pattern_tagger_n_tags
 *   indexes the tagger's distinct tag strings in the order the rules name them first; vpt_pattern_tagger_tag gives the bytes of one (owned by the
 *   tagger).
 * vpt_batch_set_pattern_tagger(b, tagger or NULL): while one is set, vpt_fill_tags_batch_device, vpt_fill_tags_scores_batch_device and the
 *   fill_tags inside vpt_predict_listing_batch_device apply the rules behind fill_tags on the same stream (kernels_pattern.hip), and
 *   vpt_expand_tags_batch_device / vpt_write_tagged_batch_device / the listing's T read the result.  Order guarantee: the workspace's records
 *   stay sorted by position -- the rule tags are merged by a count, a prefix sum and a scatter, no sort and no atomics -- so two runs give the
 *   same bytes.  Setting or clearing a tagger drops the records on the workspace: call fill_tags again.  With none set every call makes
 *   exactly the launches it made before this section existed.  vpt_evaluate_labels_batch_device (VPT_EVAL_TAGS_PREDICTED) keeps reading what
 *   fill_tags itself left, never the rule tags: the evaluate CLI runs no PatternMatchTagger.  In the listing a token the rules tagged without a tag model has no line of
 *   candidates in the tag block (Token::tag_candidates knows model candidates only).
 * Capacity: wherever a bound above says vpt_predictor_max_tag_suffix, add vpt_pattern_tagger_max_tag_suffix (the most bytes one rule's tags
 *   take, escapes included) while a tagger is used.
 * vpt_fill_tags_batch_rules / vpt_write_tagged_batch_rules / vpt_tokenize_batch_rules: vpt_fill_tags_batch_flags / vpt_write_tagged_batch /
 *   vpt_tokenize_batch with the tagger applied behind their fill_tags (NULL: exactly those calls).
 * vpt_pattern_tagger_info: keys (distinct surfaces), slots of the table, the longest surface in chars (any pointer may be NULL).
 * vpt_pattern_tagger_tile: the chars a workgroup of the kernel takes at a time (the tests place tokens across its edges). */
vpt_status vpt_pattern_tagger_create(const vpt_predictor *p, const uint8_t *surfaces, const uint64_t *offsets, size_t n_rules,
                                     const uint32_t *slot_counts, const uint8_t *present, const uint8_t *tag_bytes, const uint64_t *tag_offsets,
                                     void **out);
void vpt_pattern_tagger_destroy(void *tagger);
vpt_status vpt_pattern_tagger_n_tags(const void *tagger, uint32_t *n_tags);
vpt_status vpt_pattern_tagger_tag(const void *tagger, uint32_t id, const uint8_t **bytes, size_t *len);
vpt_status vpt_pattern_tagger_max_tag_suffix(const void *tagger, uint32_t *n_bytes);
vpt_status vpt_pattern_tagger_info(const void *tagger, uint32_t *n_keys, uint32_t *n_slots, uint32_t *max_surface_chars);
vpt_status vpt_pattern_tagger_tile(uint32_t *n_chars);
vpt_status vpt_batch_set_pattern_tagger(vpt_batch *b, const void *tagger);
vpt_status vpt_fill_tags_batch_rules(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences,
                                     const uint64_t *out_offsets, const uint8_t *labels, int32_t *tags_out, unsigned flags, const void *tagger);
vpt_status vpt_write_tagged_batch_rules(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences,
                                        const uint64_t *out_offsets, const uint8_t *labels, unsigned flags, uint8_t *text_out,
                                        uint64_t text_capacity, uint64_t *text_offsets_out, const void *tagger);
vpt_status vpt_tokenize_batch_rules(const vpt_predictor *p, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences,
                                    unsigned flags, int tagged, uint8_t *text_out, uint64_t text_capacity, uint64_t *text_offsets_out,
                                    const void *tagger);

/* Diagnostics: when the environment variable VPT_PROFILE_PHASES is set at vpt_batch_create, the specialised
 * kernel accumulates, per workgroup (wave 0), the shader cycles spent in 0 text scan, 1 per-char decode,
 * 2 pattern lookups, 3 barrier wait, 4 boundary output.  Reads the sums (after a device sync) and resets them;
 * all zeros when profiling is off. */
vpt_status vpt_batch_phase_cycles(vpt_batch *b, uint64_t cycles[8]);
/* Diagnostics, same switch: the node reads the specialised kernel's lanes ISSUED since the last call, per level -- [0] unigram, [1] bigram,
 * [2] trigram nodes, [3] deep-trie entries, [4] deep-trie rows, [5] type rows in global memory (layout.h) -- i.e. the useful bytes of its
 * gathers (reads x node size) to set beside the 128-byte lines the L2 fetches for them; zeros without VPT_PROFILE_PHASES. */
vpt_status vpt_batch_node_reads(vpt_batch *b, uint64_t reads[8]);

/* ---------------------------------------------------------------------------------------------------------
 * Introspection (host-only; used by tests and the bench's roofline accounting)
 */
typedef struct vpt_model_info {
    uint32_t n_char_ngrams, n_type_ngrams, n_dict_words, n_tag_models;
    int32_t bias;
    uint32_t char_window, type_window;
    uint32_t max_pattern_chars;    /* longest char n-gram / dict word */
    uint32_t n_short_entries;      /* distinct strings of <= 3 chars (plus 3-char prefixes of longer ones) */
    uint32_t n_long_nodes;         /* trie nodes for strings of > 3 chars */
    uint32_t type_kind;            /* 0 none, 1 window table (cache variant), 2 pattern tables */
    uint64_t device_table_bytes;   /* bytes all tables occupy in HBM */
    uint64_t hot_table_bytes;      /* bytes of the tables the scoring kernel chosen for this model reads */
    uint32_t packed;               /* 1: the specialised kernel's packed tables (double-array trie, layout.h) are in use */
    uint32_t n_displaced;          /* hash-table keys that do not sit in their home slot */
    uint32_t type_rows;            /* type scores as rows added with a position's unigram row: 1 = the 294 rows in LDS (type n-grams of <= 3
                                      symbols), 2 = rows in global memory (up to 6 symbols); 0: window table / pattern tables */
    uint32_t n_overflow_children;  /* 0 (kept for layout compatibility: the double-array tables have no overflow) */
    uint32_t predict_tags;         /* the predict_tags flag the predictor was created with (0 from vpt_model_inspect without it) */
} vpt_model_info;

/* Model::read_slice's decoding (model.rs:127-135) without keeping the model: validates the bytes ("VaporettoTokenizer 0.5.0\n"
 * + bincode) and reports how many of them the model takes -- read_slice returns the rest to the caller.  Host only.
 * Errors: VPT_INVALID_MODEL "model version mismatch" | a decode error. */
vpt_status vpt_model_read_len(const uint8_t *model_bytes, size_t len, size_t *consumed);

/* Parses + validates + compiles the tables on the host only (no device).  Same errors as create. */
vpt_status vpt_model_inspect(const uint8_t *model_bytes, size_t len, int predict_tags, vpt_model_info *info);
vpt_status vpt_predictor_info(const vpt_predictor *p, vpt_model_info *info);

/* ---------------------------------------------------------------------------------------------------------
 * Trainer: boundary-model training                                 (trainer.rs:201-490, train/src/main.rs:73-190)
 *
 * Features are exactly Trainer::gen_features' (trainer.rs:260-318): char n-grams and CharacterType n-grams of the windows with their
 * rel_position, dictionary words by min(length, dictn) and Left / Inside / Right for every occurrence of every word; a feature's value
 * is its count at the boundary (trainer.rs:321-350).  Every boundary is an example, Unknown ones too; the trained problem is "y = +1 iff
 * WordBoundary", whose coefficients the reference keeps (trainer.rs:365-374), with a bias feature 1.0 regularised as liblinear does.
 * Solvers: 0 (L2R_LR) and 2 (L2R_L2LOSS_SVC), the primal TRON solvers of liblinear as scikit-learn bundles it (CG without a
 * preconditioner): the reference's newer liblinear preconditions its CG, so weights agree with it to the stopping tolerance, not bit
 * for bit.  Sums run in a fixed order: the same examples and arguments give byte-identical models on every run.
 * Solver 5 (L1R_L2LOSS_SVC, the one the reference's README trains with) is opt-in: a trainer created with VPT_TRAIN_L1R in
 * params->flags also accepts solver == 5 and then runs liblinear's coordinate descent (solve_l1r_l2_svc) on the device, a launch per
 * group of columns that share no row (the columns of one template (kind, n-gram length, rel_position); every dictionary column and the
 * bias alone), the groups in a new seeded order every sweep, without shrinking, stopping by liblinear's rule (the sweep's violation sum
 * <= eps * max(min(pos, neg), 1) / rows * the first sweep's) or after 1000 sweeps.  Weights that end at exactly 0 are not written, so
 * the model is sparse.  Without the flag solver 5 is refused as below; with it solvers 0 and 2 train exactly as without it, solvers 1,
 * 3, 4, 6, 7 are VPT_INVALID_ARGUMENT "solver: only 0, 2 and 5 are implemented", and solver 5 together with VPT_TRAIN_TAGS is
 * VPT_INVALID_ARGUMENT "solver 5: tag models are trained with solvers 0 and 2 only".  That last sentence holds for a trainer without
 * VPT_TRAIN_TAGS_L1R.  A trainer created with all three of VPT_TRAIN_TAGS | VPT_TRAIN_L1R | VPT_TRAIN_TAGS_L1R (the third without
 * both others is VPT_INVALID_ARGUMENT "flags: ...") trains, under solver 5, the boundary model as above and every tag problem by the
 * same coordinate descent, one-vs-rest over the problem's 0/1 matrix (one mirrored solve for two candidates), every class from w = 0
 * and the same seed; the groups are the templates (kind, number of context symbols, rel_position) of the problem's features -- a tag
 * example has at most one feature of a template -- and the bias alone.  A problem with (features + 1) + rows <= 7256 doubles is solved
 * by one workgroup of one launch with w and b in LDS (path 1), a larger one, or every one after vpt_trainer_set_tag_path(1), by the
 * group launches of the boundary solver, a class at a time (path 2); both use one summation rule.  vpt_trainer_tag_weights' stats then
 * have solver 5's meanings (below).  With the third flag solvers 0 and 2 give the bytes they give without it.
 * Solver 6 (L1R_LR, L1-regularised logistic regression) is opt-in too: a trainer created with VPT_TRAIN_L1R_LR in params->flags -- alone
 * or beside any accepted combination of the flags above -- also accepts solver == 6 and then runs liblinear's newGLMNET (solve_l1r_lr)
 * on the device for  |w|_1 + C sum log(1 + exp(-y w.x)),  the bias inside the norm: per Newton iteration one launch over all columns
 * for the model's diagonal, the gradient and the violations at w; coordinate descent over the quadratic model by the same column
 * groups, a launch per group, the groups in a new seeded order every inner sweep, until a sweep's violation sum is <= inner_eps * the
 * first outer one (inner_eps 1, times 0.25 after an iteration of one sweep; at most 1000 sweeps); then a line search over all rows
 * that halves the step at most 20 times.  It stops by liblinear's rule (the violation sum at w <= eps * max(min(pos, neg), 1) / rows *
 * the first one) or after 100 Newton iterations.  Divergences from liblinear: no shrinking at either level; after 20 refused trials
 * the trial weights are put back to w; sums run in the fixed order of solver 5's kernels, so the same examples and arguments give
 * byte-identical models on every run.  Without the flag every message and every byte of every model is as above.  With it solvers 0
 * and 2 (and 5, with VPT_TRAIN_L1R) train exactly as without it; the other solvers are VPT_INVALID_ARGUMENT "solver: only 0, 2 and 6
 * are implemented" ("only 0, 2, 5 and 6" with VPT_TRAIN_L1R); solver 6 on a trainer with VPT_TRAIN_TAGS is VPT_INVALID_ARGUMENT
 * "solver 6: tag models are trained with solvers 0, 2 and 5 only".  That last sentence holds for a trainer without
 * VPT_TRAIN_TAGS_L1R_LR.  A trainer created with VPT_TRAIN_TAGS | VPT_TRAIN_L1R_LR | VPT_TRAIN_TAGS_L1R_LR (the third without both
 * others is VPT_INVALID_ARGUMENT "flags: ..."; VPT_TRAIN_L1R and VPT_TRAIN_TAGS_L1R may stand beside them) trains, under solver 6, the
 * boundary model as above and every tag problem by the same newGLMNET, one-vs-rest over the problem's 0/1 matrix (one mirrored solve
 * for two candidates), every class from w = 0 and the same seed, over solver 5's groups of a tag problem.  A problem with
 * 3 * rows + (features + 1) <= 7256 doubles is solved by one workgroup of one launch (path 1): tau, D and xTd per row and the trial
 * weights per feature in LDS, the weights, Grad, Hdiag, the negative-row sums and the violations per feature and exp(w.x) per row in
 * global memory (5 * (features + 1) + rows doubles a problem); a larger one, or every one after vpt_trainer_set_tag_path(1), by the
 * launches of the boundary solver, a class at a time (path 2); both use one summation rule.  In the kernel a sum that is not finite
 * ends the solve.  vpt_trainer_tag_weights' stats then have solver 6's meanings (below).  With the flag solvers 0 and 2 (and 5, where
 * the trainer accepts it) give the bytes they give without it.
 * Divergences: tag models are trained only by a trainer created with VPT_TRAIN_TAGS (below), without it the caller rejects or drops tags
 * (the train CLI's --ignore-tags); solvers 1, 3-7 are
 * VPT_INVALID_ARGUMENT "solver: only 0 and 2 are implemented"; a corpus without WordBoundary, or with nothing else, is
 * VPT_INVALID_ARGUMENT (the reference unwraps or fails in liblinear); typew > charw is VPT_INVALID_ARGUMENT (the reference panics).
 * Limits: 1 <= charn, typen <= 5; charw, typew <= 16; dictn >= 1 with a non-empty dictionary; fewer than 2^32 boundaries and feature
 * occurrences; a feature at most 65535 times at one boundary.
 *
 * Device memory: per boundary 5 bytes while examples are added (the label and a feature count) and 16 bytes of key per feature
 * occurrence, kept until the trainer is destroyed.  The design matrix adds 8 bytes per boundary (CSR row pointer), 12 bytes per
 * nonzero (CSR and CSC copies: 4-byte index + 2-byte count each), 16 bytes (sorted key) + 8 bytes (CSC column pointer) per feature,
 * and the column segments of Xᵀv: per level 8 bytes per feature (pointers) and 12 bytes per segment (column + partial sum), with at
 * least one segment per feature per level and ceil(log64(longest column)) levels -- about 100 bytes per feature when one column
 * holds tens of millions of nonzeros.  Training adds 48 bytes per boundary and 56 per feature for the fp64 vectors: solver 6's five
 * vectors per boundary (exp(w.x), tau, D, xTd, the terms of a sum) and six per feature (trial weights, diagonal, gradient, negative-row
 * sums, violations, the terms of a sum) are TRON's own, so it adds none; like solver 5 it adds 16 bytes per 64 nonzeros and per
 * feature for the long columns' partial sums, and 4 bytes per feature twice for the column lists.  While the ids
 * are assigned, about 52 bytes per feature occurrence are in use for the table, the sort and the per-occurrence ids.
 *
 * vpt_trainer_create: dictionary words utf8[offsets[i] .. offsets[i+1]), distinct and non-empty, in the order the model lists them
 *   (the CLI passes the BTreeSet's, main.rs:132-161); params->flags must be 0, VPT_TRAIN_TAGS, VPT_TRAIN_L1R, both, or both with
 *   VPT_TRAIN_TAGS_L1R, each with or without VPT_TRAIN_L1R_LR (any other bit or combination is VPT_INVALID_ARGUMENT "flags: ..."),
 *   or a combination with VPT_TRAIN_TAGS and VPT_TRAIN_L1R_LR in it beside VPT_TRAIN_TAGS_L1R_LR.
 * vpt_trainer_add_batch: sentences as vpt_count_boundaries takes them, labels (0 / 1 / 2) laid out as it lays them out; flags:
 *   VPT_FLAG_KYTEA_FULLWIDTH extracts the features from the KyteaFullwidthFilter image of the text (the CLI without --no-norm).
 * vpt_trainer_add_batch_device: the same from device buffers (vpt_parse_tokenized_batch_device's or vpt_parse_partial_batch_device's raw
 *   text, offsets and labels): the examples are appended after hip_stream's work so far; returns when they are.  The text may start
 *   anywhere in a larger buffer, at any alignment.  total_boundaries is EXACT here, not an upper bound as in the predictor's device
 *   calls.  Checked once hip_stream's work is done and before a kernel follows an offset, each VPT_INVALID_ARGUMENT with nothing added:
 *   d_out_offsets[0] != 0 "out_offsets: must start at 0"; d_out_offsets[n_sentences] != total_boundaries "total_boundaries: must
 *   equal out_offsets[n_sentences]"; a label above 2 "labels: must be 0, 1 or 2" (vpt_trainer_add_batch's message).
 * vpt_trainer_n_features: the distinct features of the examples so far (Trainer::n_features).
 * vpt_trainer_csr: the design matrix: row_ptr[n_rows + 1], per nonzero its column (features in key order) and count; NULL outputs ask
 *   for the sizes only.
 * vpt_trainer_train: Trainer::train (trainer.rs:352-487): 16-bit quantisation, the model's layout, Model::to_vec without tag models.
 *   *needed = the model's size; model_out may be NULL, else capacity must cover it.  vpt_trainer_model returns it again.
 *   Errors: VPT_INVALID_ARGUMENT (solver, eps / cost, one class); VPT_INVALID_MODEL "all weights are zero".
 * vpt_trainer_weights: after train, the fp64 weights of the features in key order, the bias, and the keys (two words each, low first:
 *   kind << 120 | c0 << 99 | c1 << 78 | c2 << 57 | c3 << 36 | c4 << 15 | length << 5 | (rel_position + 16), kind 0 char, 1 type
 *   (c = CharacterType values), 2 dictionary (c0 = min(length, dictn), c1 = 0 Left / 1 Inside / 2 Right, no length or position)).
 * vpt_trainer_last_stats: TRON iterations, CG steps, the gradient norms at w = 0 and at the result, and the objective.  After solver 5
 *   the same layout holds: iterations = sweeps, cg_steps = line-search halvings (each follows a pass over the column's data; a step
 *   that the data-free test accepts costs none), gnorm0 / gnorm = the first and the last sweep's violation sums, objective =
 *   |w|_1 + C sum max(0, 1 - y w.x)^2, the bias inside the norm as liblinear has it.  After solver 6: iterations = Newton iterations,
 *   cg_steps = inner sweeps over all of them, gnorm0 / gnorm = the first and the last violation sum at w, objective =
 *   |w|_1 + C sum log(1 + exp(-y w.x)) recomputed from the returned weights. */
typedef struct vpt_train_params {
    uint32_t charw, charn, typew, typen, dictn;
    uint32_t flags; /* 0 or VPT_TRAIN_TAGS | VPT_TRAIN_L1R | VPT_TRAIN_TAGS_L1R | VPT_TRAIN_L1R_LR | VPT_TRAIN_TAGS_L1R_LR */
} vpt_train_params;
enum {
    VPT_TRAIN_TAGS = 1,
    VPT_TRAIN_L1R = 4,
    VPT_TRAIN_TAGS_L1R = 8, /* needs both others; bit 1 stays an unknown flag */
    VPT_TRAIN_L1R_LR = 16,  /* solver 6; alone or beside any accepted combination of the others */
    VPT_TRAIN_TAGS_L1R_LR = 32 /* solver 6 for the tag models; needs both VPT_TRAIN_TAGS and VPT_TRAIN_L1R_LR */
};
typedef struct vpt_train_stats {
    uint32_t iterations;
    uint32_t cg_steps;
    double gnorm0;
    double gnorm;
    double objective;
} vpt_train_stats;
/* The prototypes below use only the ABI's plain types: a trainer is a `void *` handle, `params` is six uint32_t (charw, charn,
 * typew, typen, dictn, flags) laid out as vpt_train_params, `eps_cost` two doubles (eps, cost), the weights and bias doubles, the
 * counts uint16_t, and `stats` a vpt_train_stats. */
vpt_status vpt_trainer_create(const uint32_t *params, const uint8_t *dict_utf8, const uint64_t *dict_offsets, size_t n_dict_words,
                              int device_id, void **out);
void vpt_trainer_destroy(void *t);
vpt_status vpt_trainer_add_batch(void *t, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences, const uint8_t *labels,
                                 unsigned flags);
vpt_status vpt_trainer_add_batch_device(void *t, const uint8_t *d_utf8, const uint64_t *d_byte_offsets, const uint64_t *d_out_offsets,
                                        size_t n_sentences, uint64_t total_boundaries, const uint8_t *d_labels, unsigned flags, void *hip_stream);
vpt_status vpt_trainer_n_features(void *t, size_t *out);
vpt_status vpt_trainer_csr(void *t, uint64_t *row_ptr_out, uint32_t *cols_out, void *counts_out, size_t capacity, size_t *n_rows,
                           size_t *nnz);
vpt_status vpt_trainer_train(void *t, const void *eps_cost, int solver, uint8_t *model_out, size_t capacity, size_t *needed);
vpt_status vpt_trainer_model(const void *t, uint8_t *model_out, size_t capacity, size_t *needed);
vpt_status vpt_trainer_weights(void *t, void *weights_out, void *bias_out, uint64_t *keys_out, size_t capacity, size_t *n_features);
vpt_status vpt_trainer_last_stats(const void *t, void *stats);

/* ---------------------------------------------------------------------------------------------------------
 * Tag models: TagTrainer                                            (tag_trainer.rs, trainer.rs:231-238, 338, 449)
 *
 * Opt-in: a trainer created with VPT_TRAIN_TAGS in params->flags.  Without it every call below is VPT_INVALID_ARGUMENT "tags: the trainer
 * was created without VPT_TRAIN_TAGS", and the trainer behaves and writes models exactly as before.
 * Examples: every token of Sentence::iter_tokens (tokens with an Unknown boundary inside are skipped) of a sentence with n_tags > 0, its tags
 * those of its last char; features: the char and CharacterType n-grams that cover the token and n + 1 <= charn (typen) more chars,
 * rel_position of them to its right (tag_trainer.rs:79-100).  Per surface (byte order) and slot with at least two candidate tags (ids in
 * order of first appearance) a 0/1 problem with a bias feature is trained: one binary problem for two candidates (class 0 positive, class 1 its
 * negation), one-vs-rest for more, each with liblinear's tolerance eps * max(min(pos, neg), 1) / rows.  Quantisation per slot:
 * trunc(w / (max(1e-6, max |w|) / 32767)); an n-gram entry exists where a class's quantised weight is not zero.
 * Where it runs: the examples, their chars and their feature keys are extracted on the device and stay there; surfaces get their ids (byte
 * order) from a device hash table and radix sort, the examples are sorted by (surface, corpus order), and the keys of all problems are
 * deduplicated, numbered and written as CSR and CSC in a few launches over concatenated arrays.  The host interns the tag strings and, from
 * 8 bytes of ids an example, picks each problem's candidates, rows and y.  Every problem with 7 * (features + 1) + 3 * rows <= 7424 doubles is solved by one workgroup of one kernel
 * launch (TRON with its vectors in LDS), a larger one by the global-memory TRON of the boundary model, a class at a time.  (Solver 5 on a
 * trainer with VPT_TRAIN_TAGS_L1R: see the Trainer section; its in-kernel rule is (features + 1) + rows <= 7256.  Solver 6 on a trainer
 * with VPT_TRAIN_TAGS_L1R_LR: see there too; its in-kernel rule is 3 * rows + (features + 1) <= 7256.)
 * Divergences: the in-kernel CG loop stops after 16 * (features + 1) + 64 steps (exact CG needs at most features + 1; liblinear's loop and the
 * global-memory solver have no cap), so that a non-finite problem cannot spin on the device.  A HIP error (not an argument error) after the
 * boundary examples of a batch were added leaves them added without the batch's tag examples: destroy the trainer then.
 * Limits: fewer than 2^32 chars per batch; fewer than 2^24 - 1 distinct surfaces (the predictor's limit: more is VPT_INVALID_ARGUMENT at train);
 * a tag must be UTF-8 without NUL (VPT_INVALID_ARGUMENT naming the sentence); fewer than 2^32 chars, tagged tokens, feature occurrences and
 * nonzeros over all problems in a trainer.  Memory, on the device until the trainer is destroyed: 4 bytes per char, 16 per tagged token and 16
 * per feature occurrence; 20 more per char while a batch is added; while the problems are built about 45 bytes per nonzero (the (key,
 * problem) records and the sort), of which 8 per nonzero and 4 per row stay.  The host keeps about 16 bytes per tagged token and slot.
 * No buffer is read past its stated size.
 *
 * vpt_trainer_add_tagged_batch[_device]: vpt_trainer_add_batch[_device]'s arguments plus the gold tags as vpt_parse_tokenized_batch[_device]
 *   writes them: n_tags[S], tag_index[chars + 1], span_offsets[n_spans + 1], tag_bytes[n_tag_bytes] (an empty span is None).  The CSR is
 *   checked on the device before an offset is followed: VPT_INVALID_ARGUMENT "tag_index: ..." / "span_offsets: ...", nothing added.  The
 *   boundary examples are added exactly as the untagged call adds them, behind the call's last refusal.
 *   vpt_trainer_add_tagged_batch_device holds its batch to vpt_trainer_add_batch_device's three rules first, with the same messages and
 *   nothing added: d_out_offsets[0] == 0, total_boundaries == d_out_offsets[n_sentences] exactly (no upper bound, unlike the predictor's
 *   device calls), and no label above 2.
 * vpt_trainer_set_tag_dictionary: replaces the tag dictionary: surface i is surfaces_utf8[surface_offsets[i] .. [i+1]) with n_tags[i] slots,
 *   whose tags are the next n_tags[i] spans of span_offsets into tag_bytes (empty: None); the first occurrence of a surface wins.  A surface
 *   with a tag and no example gets a model of fixed tags.  Host only.
 * vpt_trainer_train: with VPT_TRAIN_TAGS also trains the tag models and writes them into the model.
 * vpt_trainer_set_tag_path: 0 (default) picks the solver by size, 1 sends every problem through the global-memory solver (tests, benchmarks).
 * vpt_trainer_n_tag_problems: the trained problems (and the tag models, fixed ones included).
 * vpt_trainer_tag_problem: problem i as a vpt_tag_problem_info, and into any non-NULL output: the surface, the candidates in id order
 *   (cand_offsets[n_classes + 1] into cand_bytes), the sorted feature keys (two words each, low first: the boundary trainer's layout, the
 *   chars being the left context then the right context, length = their number, rel_position = those to the right), the 0/1 CSR
 *   (row_ptr[n_rows + 1], cols[nnz]) and the tag id per row.  info.path: 0 before training, 1 in-kernel, 2 global-memory.
 * vpt_trainer_tag_weights: after train, problem i's fp64 weights [n_classes][n_features + 1] (the bias last) and n_classes vpt_train_stats.
 * vpt_trainer_tag_summary: the last training's problems and seconds per path. */
typedef struct vpt_tag_problem_info {
    uint32_t slot, n_classes, path, model;
    uint64_t n_rows, n_features, nnz, surface_bytes, cand_bytes;
    double seconds_setup, seconds_solve; /* path 2 after train: the matrix upload and its CSC; the TRON runs of the classes */
} vpt_tag_problem_info;
typedef struct vpt_tag_train_summary {
    uint64_t problems_in_kernel, problems_large;
    double seconds_in_kernel;     /* upload, the one launch, and the weights back */
    double seconds_large;         /* the large path, setup included */
    double seconds_large_solve;   /* of which the TRON runs */
    double seconds_construction;  /* the last build: surface ids, grouping and the problems' matrices */
    double seconds_add_host;      /* the host's tag interning inside the add calls so far */
    double seconds_construction_host; /* of seconds_construction, the host's grouping by tag (candidates, rows, y) */
} vpt_tag_train_summary;
vpt_status vpt_trainer_add_tagged_batch(void *t, const uint8_t *utf8, const uint64_t *byte_offsets, size_t n_sentences, const uint8_t *labels,
                                        const uint32_t *n_tags, const uint64_t *tag_index, const uint64_t *span_offsets, const uint8_t *tag_bytes,
                                        uint64_t n_spans, uint64_t n_tag_bytes, unsigned flags);
vpt_status vpt_trainer_add_tagged_batch_device(void *t, const uint8_t *d_utf8, const uint64_t *d_byte_offsets, const uint64_t *d_out_offsets,
                                               size_t n_sentences, uint64_t total_boundaries, const uint8_t *d_labels, const uint32_t *d_n_tags,
                                               const uint64_t *d_tag_index, const uint64_t *d_span_offsets, const uint8_t *d_tag_bytes,
                                               uint64_t n_spans, uint64_t n_tag_bytes, unsigned flags, void *hip_stream);
vpt_status vpt_trainer_set_tag_dictionary(void *t, const uint8_t *surfaces_utf8, const uint64_t *surface_offsets, size_t n_surfaces,
                                          const uint32_t *n_tags, const uint64_t *span_offsets, const uint8_t *tag_bytes);
vpt_status vpt_trainer_set_tag_path(void *t, int mode);
vpt_status vpt_trainer_n_tag_problems(void *t, size_t *n_problems, size_t *n_models);
vpt_status vpt_trainer_tag_problem(void *t, size_t i, void *info, uint8_t *surface_out, uint8_t *cand_bytes_out, uint64_t *cand_offsets_out,
                                   uint64_t *keys_out, uint64_t *row_ptr_out, uint32_t *cols_out, uint32_t *y_out);
vpt_status vpt_trainer_tag_weights(void *t, size_t i, void *weights_out, size_t capacity, void *stats_out);
vpt_status vpt_trainer_tag_summary(const void *t, void *summary);

#ifdef __cplusplus
}
#endif
#endif /* VAPORETTO_HIP_H */
