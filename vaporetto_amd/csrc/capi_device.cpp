// C ABI of libvaporetto_hip.so, the device-resident entry points: Predictor::predict (tile planning + the scoring launch), Sentence::fill_tags (the tag
// records), write_tokenized_text (the flat writer), the char count, Sentence::char_types -- all on device buffers, asynchronous on the caller's stream.
#include "capi_internal.hpp"
#include "vocab_count.hpp"
#include "vocab_table.hpp"

// (the entry points have C linkage from their declarations in include/vaporetto_hip.h)

namespace vptc {

vpt_status predict_device_impl(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                               const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries,
                               uint64_t max_sentence_bytes, int32_t* d_scores, uint8_t* d_labels, void* hip_stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (n_sentences == 0) { b->last_tiles = 0; return VPT_OK; }   // nothing enqueued; earlier work stays pending
    if (!d_utf8 || !d_byte_offsets || !d_out_offsets) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    if (n_sentences >= 0xFFFFFFFFull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: n_sentences: at most 2^32-2 per call");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    VPT_HIP(hipSetDevice(p->device));
    vpt::ScoreParams P{};
    P.ct = p->ct; P.tt = p->tt; P.pk = p->pk; P.type_table = p->d_type_table;
    P.ctype = p->d_ctype;
    P.cinfo = (b->flags & VPT_FLAG_KYTEA_FULLWIDTH) ? p->d_cinfo + 65536 : nullptr;
    P.cid = p->d_cid ? p->d_cid + ((b->flags & VPT_FLAG_KYTEA_FULLWIDTH) ? 65536 : 0) : nullptr;
    P.post = b->flags & 0x1FEu;   // (bit 8: VPT_FLAG_LINEBREAKS_FIRST)
    P.type_window = p->type_window; P.type_kind = p->type_kind; P.bias = p->bias; P.pad = p->pad;
    P.force_window_table = p->knobs.force_window_table ? 1u : 0u;
    // flat positions of the longest sentence: its chars, bounded by the caller's hint or else by its bytes
    const uint64_t max_chars = (b->max_chars && b->max_chars < max_sentence_bytes) ? b->max_chars : max_sentence_bytes;
    const uint64_t total_flat = total_boundaries + uint64_t(n_sentences) * uint64_t(1 + p->pad);
    const uint64_t total_chars = total_boundaries + n_sentences;
    // The specialised kernel takes whole-sentence tiles while every sentence is short, and tiles cut at any flat position (with a
    // halo of the longest pattern on either side) otherwise -- a sentence of any length is scored there.  Only a model whose longest
    // pattern leaves no room for a tile between its halos sends long sentences to the general kernels.
    bool fast = vpt::fast_path_supported(P) && !b->knobs.force_generic;
    const uint64_t fast_cap = fast ? uint64_t(vpt::fast_path_cap(P)) : 0;   // flat positions per tile of the instance that scores this predictor
    vpt::CutGeometry cut{};
    bool cut_tiles = false;
    if (fast) {
        const uint32_t lmax = std::max<uint32_t>(p->info.max_pattern_chars, 3);
        // A pattern of m chars that starts at s touches the boundaries s - wl .. s + max(wl, m) - 1 (layout.h, row_lo / row_hi): a
        // boundary needs the start positions within max(lmax, wl) - 1 to its left and within wl to its right, and those need their
        // chars -- lmax - 1 further on -- and the types their row is indexed by.
        const uint32_t wl = p->pk.wl;
        const uint32_t levels = p->pk.trow_mode == vpt::kTypeRowsGlobal ? p->pk.trow_levels : 3u;
        cut.halo_left = std::max<uint32_t>(lmax - 1, wl); cut.halo_right = wl + std::max<uint32_t>(std::max<uint32_t>(lmax - 1, wl), levels);
        cut.pad = uint32_t(p->pad); cut.cap = uint32_t(fast_cap);
        cut.cap_eff = uint32_t(fast_cap - vpt::kFastStageSlack);
        const int64_t room = int64_t(cut.cap_eff) - int64_t(p->pad) - int64_t(cut.halo_left) - int64_t(cut.halo_right);
        const bool can_cut = room >= 256;
        cut.tile_flat = can_cut ? uint32_t(room) : 0u;
        cut.mis = uint32_t(reinterpret_cast<uintptr_t>(d_utf8) & 15u);
        const bool fits_whole = max_chars + 2 * uint64_t(p->pad) <= fast_cap / 2;
        const bool whole_possible = max_chars + 2 * uint64_t(p->pad) + fast_cap / 2 <= fast_cap;
        // Whole-sentence tiles are cut every (capacity - longest sentence) positions: the longer the longest sentence, the emptier
        // they run, while a tile cut anywhere is always full -- at the price of the index of the text (a pass over it).  Measured on
        // configs[4] (8 .. 512 chars, profiles/r03_u_cut_vs_whole.txt): kernel 2.14 -> 1.99 ms, step 3.80 -> 3.76; on configs[1] (64
        // chars) the kernel is the same and the index costs 19 us of 117.  So: cut above a quarter of the capacity.
        const bool prefer_cut = max_chars > fast_cap / 4;
        cut_tiles = can_cut && (b->knobs.force_cut > 0 || (b->knobs.force_cut == 0 ? (prefer_cut || !fits_whole) : !whole_possible));
        if (!cut_tiles && max_chars + 2 * uint64_t(p->pad) + fast_cap / 2 > fast_cap) fast = false;   // neither kind of tile holds the batch
    }
    const uint64_t cap = fast ? fast_cap : vpt::kCap;
    // Whole-sentence tiles are cut every `tile_flat` flat positions (chars + separators) and end with the sentence that crosses
    // the cut, so a tile holds < tile_flat + longest sentence: pick tile_flat to fill the kernel's LDS capacity.
    uint64_t tile_flat = cap / 2;
    if (cut_tiles) tile_flat = cut.tile_flat;
    else if (max_chars + 2 * uint64_t(p->pad) + cap / 2 <= cap) tile_flat = cap - 2 * uint64_t(p->pad) - max_chars;
    // Whole rounds: the chip runs `slots` tiles at a time; cutting the batch into a multiple of that many tiles (by
    // shrinking the tiles a little) avoids a last round that leaves most CUs idle.
    if (p->tile_slots > 0) {
        const uint64_t n_min = (total_flat + tile_flat - 1) / tile_flat;
        const uint64_t rounds = (n_min + p->tile_slots - 1) / p->tile_slots;
        const uint64_t even = (total_flat + rounds * p->tile_slots - 1) / (rounds * p->tile_slots);
        if (even < tile_flat) tile_flat = std::max<uint64_t>(even, 256);
    }
    if (b->knobs.tile_flat && b->knobs.tile_flat < tile_flat) tile_flat = std::max<uint64_t>(b->knobs.tile_flat, 16);
    if (cut_tiles) {   // the window a cut tile decodes and walks: its own positions and the two halos
        cut.tile_flat = uint32_t(tile_flat);
        cut.cap_eff = uint32_t(p->pad) + cut.halo_left + cut.tile_flat + cut.halo_right;
        // what the tile planner promises the scoring kernel (kernels_fast.hip: a tile of n positions stages at most 4 n + 2 * 256 bytes,
        // the staging area holds 4 * cap + 15): an internal inconsistency, not the caller's offsets
        if (uint64_t(cut.cap_eff) * 4 + 2 * 256 > cap * 4 + 15 || cut.cap_eff > cap)
            return fail(VPT_RUNTIME_ERROR, "internal error: the tile planner produced a cut tile that does not fit the kernel's staging area");
    }
    const uint64_t n_tiles64 = (total_flat + tile_flat - 1) / tile_flat;
    if (n_tiles64 >= 0x7FFFFFFFull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch too large for one call");
    const uint32_t n_tiles = uint32_t(n_tiles64);
    vpt_status st;
    bool need_slow = false;
    uint32_t slow_blocks = 0, scratch_cap = 0;
    uint64_t slab = 0;
    if (fast && cut_tiles) {
        if ((st = b->d_tiles.grow(size_t(n_tiles) + 1)) != VPT_OK) return st;
        size_t n_local = 0, n_super = 0;
        vpt::cut_index_entries(total_chars, &n_local, &n_super);
        if ((st = b->d_cut_local.grow(n_local + 16)) != VPT_OK) return st;
        if ((st = b->d_cut_super.grow(n_super + 16)) != VPT_OK) return st;
    } else {
        if ((st = grow_pair(b->d_tile_first, b->d_slow_list, size_t(n_tiles) + 1)) != VPT_OK) return st;
        // long-sentence scratch of the general kernels (only when a sentence might not fit the LDS tile)
        need_slow = !fast && max_chars + 2 * uint64_t(p->pad) + tile_flat > cap;
        if (need_slow) {
            const uint64_t cap64 = max_chars + 2 * uint64_t(p->pad) + vpt::kMargin + 8;
            if (cap64 >= 0x7FFFFFF0ull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: max_sentence_bytes: too large");
            scratch_cap = uint32_t((cap64 + 15) & ~15ull);
            slab = (uint64_t(scratch_cap) * 9 + 255) & ~255ull;
            slow_blocks = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(64, (8ull << 30) / slab)));
            const size_t need = size_t(slab) * slow_blocks;
            if (need > b->d_scratch.cap && (st = b->d_scratch.alloc(need)) != VPT_OK) return st;
        }
    }
    P.text = d_utf8; P.boff = d_byte_offsets; P.ooff = d_out_offsets; P.tile_first = b->d_tile_first; P.tiles = (fast && cut_tiles) ? b->d_tiles.p : nullptr;
    P.scores = d_scores; P.labels = d_labels; P.status = b->d_ctrl; P.slow_list = b->d_slow_list; P.slow_count = b->d_ctrl + 1;
    P.scratch = b->d_scratch; P.scratch_stride = slab; P.scratch_cap = scratch_cap;
    P.prof = b->d_prof;
    P.total_chars = total_chars;
    // A predictor with tag models: the specialised kernel also leaves the decoded chars behind, and a vpt_fill_tags_batch_device
    // call for the same buffers on this workspace (Sentence::fill_tags follows Predictor::predict on the same sentence,
    // predictor.rs:542) skips its own decode pass.
    b->cps_text = nullptr;
    if (p->has_tags && p->predict_tags && fast) {
        vpt_status st2 = b->d_cps.grow(size_t(total_chars) + 16);
        if (st2 != VPT_OK) return st2;
        P.cps_out = b->d_cps;
        b->cps_text = d_utf8; b->cps_ooff = d_out_offsets; b->cps_sentences = n_sentences; b->cps_boundaries = total_boundaries;
        b->cps_flags = b->flags & VPT_FLAG_KYTEA_FULLWIDTH;
    }
    if (b->knobs.debug_ablate) { P.debug = b->knobs.debug_ablate; P.ct.debug = P.debug; P.tt.debug = P.debug; }

    P.n_sent = n_sentences; P.tile_flat = uint32_t(tile_flat); P.n_tiles = n_tiles;
    // The text's cache policy (capi_internal.hpp, text_policy_for).  The offsets are on the device: the text's bytes are bounded from what
    // the caller says of the batch -- at most 4 a char and max_sentence_bytes a sentence (exact for sentences of one length).
    if (fast) {
        const uint64_t text_bytes = std::min<uint64_t>(total_chars * 4, uint64_t(n_sentences) * max_sentence_bytes);
        P.text_nt = b->knobs.text_policy >= 0 ? uint32_t(b->knobs.text_policy)
                                              : text_policy_for(text_bytes, launch_output_bytes(total_boundaries, d_scores != nullptr, d_labels != nullptr));
    }
    // the tiles (a kernel of its own: finding them at the head of every workgroup measured slower, profiles/r02_c1_ab.jsonl); for
    // cut tiles preceded by the lead-byte index of the text
    if (fast && cut_tiles) VPT_HIP(vpt::launch_assign_tiles_cut(P, cut, n_tiles, total_chars, b->d_cut_local, b->d_cut_super, b->d_tiles, b->d_ctrl, stream));
    else VPT_HIP(vpt::launch_assign_tiles(d_out_offsets, n_sentences, p->pad, uint32_t(tile_flat), n_tiles, b->d_tile_first, b->d_ctrl, stream));
    if (b->split_stream) {
        VPT_HIP(hipEventRecord(b->split_event, stream));
        VPT_HIP(hipStreamWaitEvent(b->split_stream, b->split_event, 0));
        stream = b->split_stream;
    }
    const size_t slot = b->ev_calls % kTimingRing;
    if (b->timing) VPT_HIP(hipEventRecord(b->ev[2 * slot], stream));
    if (fast) VPT_HIP(vpt::launch_score_tiles_fast(P, n_tiles, stream));
    else VPT_HIP(vpt::launch_score_tiles(P, p->chunks, n_tiles, stream));
    if (need_slow) VPT_HIP(vpt::launch_score_slow(P, p->chunks, slow_blocks, stream));   // inside the timed events: it is part of the scoring
    if (b->timing) { VPT_HIP(hipEventRecord(b->ev[2 * slot + 1], stream)); ++b->ev_calls; }
    b->last_tiles = n_tiles; b->last_stream = stream; b->pending = true;
    b->last_tile_flat = uint32_t(tile_flat); b->last_plan = !fast ? 0u : cut_tiles ? 2u : 1u;
    b->last_text_policy = P.text_nt;
    // ConcatGraphemeClustersFilter: behind the scoring launch (whose epilogue applied the other label filters) on its stream, in front of
    // whatever the caller enqueues on the labels
    if ((b->flags & VPT_FLAG_CONCAT_GRAPHEMES) && d_labels)
        return concat_graphemes_impl(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, d_labels, P.cps_out != nullptr, stream);
    return VPT_OK;
}

namespace {
// the class table on `device`: uploaded by the first call that asks for it there (model-independent: no predictor owns it, none frees it)
vpt_status grapheme_table_on(int device, const uint8_t** out) {
    constexpr int kMaxDevices = 64;
    static std::mutex mu;
    static const uint8_t* tables[kMaxDevices] = {};
    if (device < 0 || device >= kMaxDevices) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: device_id: no such HIP device");
    std::lock_guard<std::mutex> g(mu);
    if (!tables[device]) {
        const std::vector<uint8_t>& h = vpt::grapheme_table_host();
        uint8_t* d = nullptr;
        VPT_HIP(hipMalloc(reinterpret_cast<void**>(&d), h.size() + kTablePadBytes));
        const hipError_t e = hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); return fail(VPT_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e)); }
        tables[device] = d;
    }
    *out = tables[device];
    return VPT_OK;
}
}  // namespace

vpt_status concat_graphemes_impl(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                 const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries, uint8_t* d_labels, bool have_cps,
                                 hipStream_t stream) {
    if (n_sentences == 0 || total_boundaries == 0) return VPT_OK;   // no boundary, no label
    const uint64_t total_c = total_boundaries + n_sentences;
    const uint64_t n_tiles = (total_c + vpt::kGraphemeTile - 1) / vpt::kGraphemeTile;
    if (n_tiles >= 0x7FFFFFFFull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch too large for one call");
    vpt::GraphemeParams G{};
    vpt_status st;
    if ((st = grapheme_table_on(p->device, &G.table)) != VPT_OK) return st;
    if ((st = b->d_gcls.grow(size_t(n_tiles) * vpt::kGraphemeTile)) != VPT_OK) return st;
    if ((st = b->d_gsum.grow(2 * size_t(n_tiles))) != VPT_OK) return st;
    if (!have_cps) {
        const bool fw = (b->flags & VPT_FLAG_KYTEA_FULLWIDTH) != 0;
        if ((st = b->d_cps.grow(size_t(total_c) + 16)) != VPT_OK) return st;
        b->cps_text = nullptr;
        VPT_HIP(vpt::launch_decode_chars(d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_c, p->d_cinfo + (fw ? 65536 : 0), b->d_cps, nullptr, b->d_ctrl, stream, fw));
    }
    G.cps = b->d_cps; G.boff = d_byte_offsets; G.ooff = d_out_offsets; G.n_sent = n_sentences; G.total_chars = total_c; G.total_boundaries = total_boundaries;
    G.cls = b->d_gcls; G.summ = b->d_gsum; G.first = b->d_gsum + n_tiles; G.labels = d_labels; G.status = b->d_ctrl; G.n_tiles = uint32_t(n_tiles);
    VPT_HIP(vpt::launch_concat_graphemes(G, stream));
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}
}  // namespace vptc

vpt_status vpt_concat_graphemes_tile(uint32_t* n_chars) {
    if (!n_chars) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *n_chars = vpt::kGraphemeTile;
    return VPT_OK;
}

// ConcatGraphemeClustersFilter on the caller's labels, device buffers: the classes are those of the text under the workspace's VPT_FLAG_KYTEA_FULLWIDTH
vpt_status vpt_concat_graphemes_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                             const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries, uint8_t* d_labels,
                                             void* hip_stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (n_sentences == 0) return VPT_OK;
    if (!d_utf8 || !d_byte_offsets || !d_out_offsets || (total_boundaries && !d_labels)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    if (n_sentences >= 0xFFFFFFFFull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: n_sentences: at most 2^32-2 per call");
    VPT_HIP(hipSetDevice(p->device));
    return concat_graphemes_impl(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, d_labels, false, static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_predict_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                    const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries,
                                    uint64_t max_sentence_bytes, int32_t* d_scores, uint8_t* d_labels, void* hip_stream) {
    return predict_device_impl(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, max_sentence_bytes, d_scores, d_labels, hip_stream);
}

// Predictor::predict + Sentence::write_tokenized_text (no tags) for a batch as ONE call: the scoring launch and the writer's, back to back on the
// stream; scores and labels are optional outputs (no d_labels: the labels stay in the workspace).  (Rounds 4 - 5 fused the writer into the scoring
// kernel as a fourth phase: slower than the two launches on every batch size and, chunk by chunk, in vpt_tokenize_batch too -- HISTORY.md.)
vpt_status vpt_predict_write_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                          const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries,
                                          uint64_t max_sentence_bytes, int32_t* d_scores, uint8_t* d_labels, uint8_t* d_text_out,
                                          uint64_t text_capacity, uint64_t* d_text_offsets_out, void* hip_stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (!d_text_offsets_out || (text_capacity && !d_text_out)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    if (n_sentences == 0) {
        VPT_HIP(hipSetDevice(p->device));
        VPT_HIP(hipMemsetAsync(d_text_offsets_out, 0, sizeof(uint64_t), static_cast<hipStream_t>(hip_stream)));
        b->last_stream = static_cast<hipStream_t>(hip_stream); b->pending = true; b->cps_text = nullptr;
        return VPT_OK;
    }
    if (!d_utf8 || !d_byte_offsets || !d_out_offsets) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    uint8_t* labels = d_labels;
    if (!labels) {
        const vpt_status st = b->d_tlab.grow(size_t(total_boundaries) + 16);
        if (st != VPT_OK) return st;
        labels = b->d_tlab;
    }
    const vpt_status st = predict_device_impl(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, max_sentence_bytes, d_scores, labels, hip_stream);
    if (st != VPT_OK) return st;
    return emit_device(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, labels, false, d_text_out, text_capacity, d_text_offsets_out,
                       static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_batch_last_plan(const vpt_batch* b, uint32_t* n_tiles, uint32_t* tile_flat, uint32_t* kind) {
    if (!b) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (n_tiles) *n_tiles = b->last_tiles;
    if (tile_flat) *tile_flat = b->last_tile_flat;
    if (kind) *kind = b->last_plan;
    return VPT_OK;
}

vpt_status vpt_batch_last_text_policy(const vpt_batch* b, uint32_t* policy) {
    if (!b || !policy) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *policy = b->last_text_policy;
    return VPT_OK;
}

vpt_status vpt_text_policy_for(uint64_t text_bytes, uint64_t total_boundaries, int want_scores, int want_labels, uint32_t* policy, uint64_t* threshold_bytes) {
    if (policy) *policy = text_policy_for(text_bytes, launch_output_bytes(total_boundaries, want_scores != 0, want_labels != 0));
    if (threshold_bytes) *threshold_bytes = kTextNtMinStreamBytes;
    return VPT_OK;
}

vpt_status vpt_batch_tag_plan(const vpt_batch* b, uint64_t* n_runs, uint32_t* run_sentences) {
    if (!b) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (n_runs) *n_runs = b->tag_out.own.n_runs;
    if (run_sentences) *run_sentences = b->tag_out.own.run_sent;
    return VPT_OK;
}

vpt_status vpt_batch_sync(vpt_batch* b) {
    if (!b) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    // A caller that waits for the device may rewrite its buffers afterwards: the chars a predict call left decoded for the fill_tags
    // call behind it (matched by buffer address and shape only) are good for a fill_tags enqueued BEFORE the next sync, no longer.
    b->cps_text = nullptr;
    if (!b->pending) return VPT_OK;
    VPT_HIP(hipSetDevice(b->device));
    uint32_t ctrl[16] = {};
    VPT_HIP(hipMemcpyAsync(ctrl, b->d_ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, b->last_stream));
    VPT_HIP(hipStreamSynchronize(b->last_stream));
    b->pending = false;
    if (ctrl[0]) VPT_HIP(hipMemset(b->d_ctrl, 0, sizeof(uint32_t)));   // reported once; accumulates over every call enqueued since the last sync
    if (ctrl[0] & vpt::kErrParse) {   // tokenized text (vpt_parse_tokenized_batch_device): the reason words too
        VPT_HIP(hipMemset(b->d_ctrl + vpt::kParseErrWord, 0, 8 * sizeof(uint32_t)));
        return parse_status(ctrl, 0);
    }
    if (ctrl[0] & vpt::kErrParsePartial) {   // partially annotated text (vpt_parse_partial_batch_device): its reason words and the offender's bytes
        VPT_HIP(hipMemset(b->d_ctrl + vpt::kPartialErrWord + 1, 0, 6 * sizeof(uint32_t)));
        return partial_status(ctrl, 0);
    }
    return status_from_bits(ctrl[0]);
}

vpt_status vpt_fill_tags_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                      const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries,
                                      const uint8_t* d_labels, int32_t* d_tags_out, void* hip_stream) {
    return vpt_fill_tags_scores_batch_device(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, d_labels, d_tags_out,
                                             nullptr, nullptr, hip_stream);
}

vpt_status vpt_fill_tags_scores_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                             const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries,
                                             const uint8_t* d_labels, int32_t* d_tags_out, int32_t* d_tag_scores_out,
                                             int32_t* d_tag_models_out, void* hip_stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (!p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    if (n_sentences == 0 || p->n_tags == 0) return VPT_OK;
    if (!d_utf8 || !d_byte_offsets || !d_out_offsets || (total_boundaries && !d_labels))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    VPT_HIP(hipSetDevice(p->device));
    const uint64_t total_c = total_boundaries + n_sentences;
    // record numbers and queue places are 32-bit (one per char at most)
    if (total_c >= 0xFFFFFF00ull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: fill_tags takes fewer than 2^32 - 256 chars per call");
    vpt_status st = b->d_cps.grow(size_t(total_c) + 16);
    if (st != VPT_OK) return st;
    b->tag_out.chars = 0;   // (until the launches are enqueued: a failure below leaves no records behind)
    // What the call leaves is ONE RECORD PER TOKEN THAT HAS A TAG MODEL (kernels.hpp, TagParams): the reference holds None for every other
    // char (predictor.rs:558-573).  Everything is sized for the worst case -- a tagged token per char, which a real tag model comes close
    // to (most tokens of real text have one; the synthetic M3's one token in thirty-five is the other end) -- so nothing can overflow and
    // there is no second path: records 16 + 12 n_tags bytes, the candidates between the launches 16.
    const uint32_t run_sent = vpt::tag_run_sentences(n_sentences, total_c);
    const uint64_t n_runs = (uint64_t(n_sentences) + run_sent - 1) / run_sent;
    const size_t n_state = vpt::scan_part_entries(n_runs), ctl_words = n_state + size_t(n_runs) + 2;
    if ((st = b->d_tag_records.grow(size_t(total_c) + 16)) != VPT_OK) return st;
    if ((st = b->d_rec_tags.grow(size_t(total_c) * p->n_tags + 16)) != VPT_OK) return st;
    if ((st = b->d_rec_str.grow(size_t(total_c) * p->n_tags + 16)) != VPT_OK) return st;
    if ((st = b->d_tag_cands.grow(size_t(total_c) + 16)) != VPT_OK) return st;
    if ((st = b->d_tag_ctl.grow(ctl_words)) != VPT_OK) return st;
    if (!b->d_tag_summary && (st = b->d_tag_summary.alloc(vpt::tag_summary_words() * sizeof(uint32_t))) != VPT_OK) return st;
    VPT_HIP(hipMemsetAsync(b->d_tag_ctl, 0, ctl_words * sizeof(uint64_t), stream));   // the scan's state, the runs' counts
    // the dense arrays of the C ABI, for the callers that want them: None everywhere (what `resize(n_tags * len, None)` leaves, predictor.rs:556-557);
    // the passes write the entries of the tokens that have a model
    if (d_tags_out) VPT_HIP(hipMemsetAsync(d_tags_out, 0xFF, size_t(total_c) * p->n_tags * sizeof(int32_t), stream));
    if (d_tag_models_out) VPT_HIP(hipMemsetAsync(d_tag_models_out, 0xFF, size_t(total_c) * sizeof(int32_t), stream));
    const uint32_t* cinfo = p->d_cinfo + ((b->flags & VPT_FLAG_KYTEA_FULLWIDTH) ? 65536 : 0);
    const bool have_cps = b->cps_text == d_utf8 && b->cps_ooff == d_out_offsets && b->cps_sentences == n_sentences &&
                          b->cps_boundaries == total_boundaries && b->cps_flags == (b->flags & VPT_FLAG_KYTEA_FULLWIDTH) && b->last_stream == stream;
    b->cps_text = nullptr;   // one shot: only the fill_tags call that FOLLOWS the predict call takes its chars (predictor.rs:542)
    if (!have_cps) {
        VPT_HIP(vpt::launch_decode_chars(d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_c, cinfo, b->d_cps, nullptr, b->d_ctrl, stream, (b->flags & VPT_FLAG_KYTEA_FULLWIDTH) != 0));
    }
    vpt::TagParams T{};
    T.tok_tab = p->dtag.tok_tab; T.models = p->dtag.models; T.mfilt = p->dtag.mfilt; T.ngrams = p->dtag.ngrams; T.nrec = p->dtag.nrec; T.syms = p->dtag.syms; T.slots = p->dtag.slots;
    T.weights = p->dtag.weights; T.cinfo = cinfo; T.tok_bits = p->tok_bits; T.n_tags = p->n_tags;
    T.use_char = p->tag_use_char ? 1u : 0u; T.use_type = p->tag_use_type ? 1u : 0u;
    T.cps = b->d_cps; T.ooff = d_out_offsets; T.labels = d_labels; T.n_sent = n_sentences; T.total_chars = total_c; T.tags = d_tags_out;
    T.slot_str = p->dtag.slot_str; T.str_off = p->dtag.str_off; T.n_strings = p->dtag.n_strings;
    T.scores_out = p->max_tag_scores ? d_tag_scores_out : nullptr; T.model_out = d_tag_models_out; T.score_stride = p->max_tag_scores;
    T.n_cus = p->n_cus;
    T.records = b->d_tag_records; T.rec_tags = b->d_rec_tags; T.rec_str = b->d_rec_str; T.cands = b->d_tag_cands;
    T.scan_state = b->d_tag_ctl; T.run_pref = b->d_tag_ctl + n_state;
    T.n_runs = n_runs; T.run_sent = run_sent;
    T.summary = b->d_tag_summary; T.status = b->d_ctrl;
    VPT_HIP(vpt::launch_tag_tokens(T, stream));
    vpt::TagRecordsView own = vpt::records_view(T, p->dtag.str_bytes), merged = own;
    b->tag_out.own = own;
    if (const vpt_pattern_tagger* t = b->tagger) {   // PatternMatchTagger: the rules' tags merged into records of their own (kernels_pattern.hip)
        if ((st = b->d_pm_records.grow(size_t(total_c) + 16)) != VPT_OK) return st;
        if ((st = b->d_pm_rec_tags.grow(size_t(total_c) * p->n_tags + 16)) != VPT_OK) return st;
        if ((st = b->d_pm_rec_str.grow(size_t(total_c) * p->n_tags + 16)) != VPT_OK) return st;
        if ((st = b->d_pm_hits.grow(size_t(total_c) + 16)) != VPT_OK) return st;
        if ((st = b->d_pm_ctl.grow(ctl_words)) != VPT_OK) return st;   // (its own scan state and run_pref)
        VPT_HIP(hipMemsetAsync(b->d_pm_ctl, 0, ctl_words * sizeof(uint64_t), stream));
        vpt::PatternParams R{};
        R.slots = t->slots; R.surf = t->surf; R.rule_tags = t->rule_tags; R.id_str = t->id_str; R.bits = t->bits; R.max_len = t->max_len; R.n_tags = p->n_tags;
        R.cps = b->d_cps; R.ooff = d_out_offsets; R.labels = d_labels; R.n_sent = n_sentences; R.total_chars = total_c;
        R.in = own;
        R.hits = b->d_pm_hits; R.out_records = b->d_pm_records; R.out_rec_tags = b->d_pm_rec_tags; R.out_rec_str = b->d_pm_rec_str;
        R.scan_state = b->d_pm_ctl; R.out_run_pref = b->d_pm_ctl + n_state; R.tags = d_tags_out; R.n_cus = p->n_cus; R.status = b->d_ctrl;
        VPT_HIP(vpt::launch_pattern_tagger(R, stream));
        merged.records = R.out_records; merged.rec_tags = R.out_rec_tags; merged.rec_str = R.out_rec_str; merged.run_pref = R.out_run_pref; merged.str_bytes = t->arena;
    }
    b->tag_out.merged = merged; b->tag_out.chars = total_c; b->tag_out.sentences = n_sentences;
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}

vpt_status vpt_expand_tags_batch_device(const vpt_predictor* p, vpt_batch* b, size_t n_sentences, uint64_t total_boundaries, int32_t* d_tags_out, void* hip_stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (!p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    if (n_sentences == 0 || p->n_tags == 0) return VPT_OK;
    if (!d_tags_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    vpt::TagRecordsView V;
    if (const vpt_status st = tag_records_for(b, n_sentences, total_boundaries, true, &V); st != VPT_OK) return st;
    VPT_HIP(hipSetDevice(p->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    VPT_HIP(vpt::launch_expand_tags(V, d_tags_out, p->n_cus, stream));
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}

namespace {
// The runs of a flat kernel over sentences (the writer, the token spans) and the state words of their chain: fills F.
vpt_status plan_runs(const vpt_predictor* p, vpt_batch* b, size_t n_sentences, uint64_t total_boundaries, bool records, uint32_t run_sent,
                     uint64_t* total_out, const uint64_t* chain_in, uint64_t* chain_out, hipStream_t stream, vpt::EmitFuse* F_out) {
    // A WORKGROUP per run of sentences (emit_flat_kernel, round 5; a wave per block of 2 K chars before): 5 K chars when the batch is small (the
    // chip wants a thousand workgroups and more), up to 20 K on a big one -- fewer look-backs and size passes per byte (measured,
    // profiles/r05_h_*, r05_k_*, r06_t_*: configs[2] 2.03 ms at 128 sentences, 1.80 at 256; tagged configs[4] 2.39 / 2.10 / 2.04 at 5 K / 10 K / 20 K
    // chars; without tags up to 32 K chars: 512 sentences of 64, `r06_zv_*`); at most 512 sentences (two a thread).  With tags: a whole multiple of fill_tags' runs, so that a workgroup's records are run_pref[a] .. run_pref[b].
    vpt::EmitFuse F{};
    {
        const uint64_t chars = total_boundaries + n_sentences;
        const uint64_t auto_run = std::min<uint64_t>(std::max<uint64_t>(chars / (uint64_t(16) * std::max<uint32_t>(p->n_cus, 64)), 5120), records ? 20480 : 32768);
        const uint64_t target = auto_run;
        uint64_t per = std::min<uint64_t>(std::max<uint64_t>((target * n_sentences + chars / 2) / chars, 1), vpt::kEmitFlatMaxBlock);   // round(target / mean chars per sentence)
        if (records && run_sent <= vpt::kEmitFlatMaxBlock)
            per = std::min<uint64_t>(std::max<uint64_t>((per + run_sent / 2) / run_sent, 1) * run_sent, (vpt::kEmitFlatMaxBlock / run_sent) * run_sent);
        F.per_block = uint32_t(per);
        if (b->knobs.emit_per_block) F.per_block = std::min<uint32_t>(b->knobs.emit_per_block, vpt::kEmitFlatMaxBlock);
        F.n_blocks = (n_sentences + F.per_block - 1) / F.per_block;
    }
    const size_t words = size_t(F.n_blocks) + 1;
    if (words > b->emit_state_cap) {
        const size_t cap = std::max(words + words / 2, size_t(4096));
        b->emit_state_cap = 0;
        if (const vpt_status st = b->d_emit_state.alloc(2 * cap * sizeof(uint64_t)); st != VPT_OK) return st;   // (freeing the old one waits for the device)
        VPT_HIP(hipMemsetAsync(b->d_emit_state, 0, 2 * cap * sizeof(uint64_t), stream));   // (in front of the kernel on ITS stream: a plain hipMemset is not ordered with a non-blocking stream)
        b->emit_state_cap = cap; b->emit_dirty[0] = b->emit_dirty[1] = 0; b->emit_flip = 0;
    }
    F.state = b->d_emit_state + size_t(b->emit_flip) * b->emit_state_cap;
    F.clear = b->d_emit_state + size_t(b->emit_flip ^ 1) * b->emit_state_cap;
    F.clear_n = b->emit_dirty[b->emit_flip ^ 1];
    F.total_out = total_out; F.chain_in = chain_in; F.chain_out = chain_out;
    b->emit_dirty[b->emit_flip ^ 1] = 0; b->emit_dirty[b->emit_flip] = words;
    b->emit_flip ^= 1;
    *F_out = F;
    return VPT_OK;
}
}  // namespace

namespace vptc {
vpt_status emit_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                       const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries, const uint8_t* d_labels,
                       bool tagged, uint8_t* d_text_out, uint64_t text_capacity, uint64_t* d_text_offsets_out,
                       hipStream_t stream, uint64_t* total_out, const uint64_t* chain_in, uint64_t* chain_out) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (!d_text_offsets_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    VPT_HIP(hipSetDevice(p->device));
    if (n_sentences == 0) {
        VPT_HIP(hipMemsetAsync(d_text_offsets_out, 0, sizeof(uint64_t), stream));
        b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
        return VPT_OK;
    }
    if (!d_utf8 || !d_byte_offsets || !d_out_offsets || (total_boundaries && !d_labels) || (text_capacity && !d_text_out))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    vpt::EmitParams E{};
    E.text = d_utf8; E.boff = d_byte_offsets; E.ooff = d_out_offsets; E.labels = d_labels; E.n_sent = n_sentences;
    E.total_boundaries = total_boundaries; E.out_text = d_text_out; E.out_offsets = d_text_offsets_out; E.capacity = text_capacity;
    E.status = b->d_ctrl;
    if (tagged && p->n_tags > 0) {   // "/tag" suffixes: from the records the fill_tags call on this workspace left for this batch
        if (!p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
        if (const vpt_status st = tag_records_for(b, n_sentences, total_boundaries, true, &E.tag); st != VPT_OK) return st;
    }
    vpt::EmitFuse F{};
    {
        const vpt_status st = plan_runs(p, b, n_sentences, total_boundaries, E.tag.records != nullptr, E.tag.run_sent, total_out, chain_in, chain_out, stream, &F);
        if (st != VPT_OK) return st;
    }
    VPT_HIP(vpt::launch_emit_tokenized(E, F, stream));
    b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
    return VPT_OK;
}
// The token spans of a batch whose labels are on the device (kernels_tokens.hip), on the writer's runs; total_out / chain_in / chain_out as for
// the writer (vpt_token_stream_batch's chunks write ONE array of end-points).
vpt_status spans_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                        const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries, const uint8_t* d_labels,
                        uint64_t* d_token_offsets, uint32_t* d_token_ends, uint64_t capacity, hipStream_t stream, uint64_t* total_out,
                        const uint64_t* chain_in, uint64_t* chain_out) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (!d_token_offsets) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    VPT_HIP(hipSetDevice(p->device));
    if (n_sentences == 0) {
        VPT_HIP(hipMemsetAsync(d_token_offsets, 0, sizeof(uint64_t), stream));
        b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
        return VPT_OK;
    }
    if (!d_utf8 || !d_byte_offsets || !d_out_offsets || (total_boundaries && !d_labels) || (capacity && !d_token_ends))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    vpt::SpanParams S{};
    S.text = d_utf8; S.boff = d_byte_offsets; S.ooff = d_out_offsets; S.labels = d_labels; S.n_sent = n_sentences;
    S.total_boundaries = total_boundaries; S.token_ends = d_token_ends; S.token_offsets = d_token_offsets; S.capacity = capacity;
    S.status = b->d_ctrl;
    vpt::EmitFuse F{};
    const vpt_status st = plan_runs(p, b, n_sentences, total_boundaries, false, 0, total_out, chain_in, chain_out, stream, &F);
    if (st != VPT_OK) return st;
    VPT_HIP(vpt::launch_token_spans(S, F, stream));
    b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
    return VPT_OK;
}
}  // namespace vptc

// vaporetto_tantivy/src/lib.rs:183-192 for a batch whose labels are on the device
vpt_status vpt_token_spans_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                        const uint64_t* d_out_offsets, size_t n_documents, uint64_t total_boundaries, const uint8_t* d_labels,
                                        uint64_t* d_token_offsets, uint32_t* d_token_ends, uint64_t capacity, void* hip_stream) {
    return spans_device(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_documents, total_boundaries, d_labels, d_token_offsets, d_token_ends, capacity,
                        static_cast<hipStream_t>(hip_stream), nullptr, nullptr, nullptr);
}

// ... with every token's tags beside its end-point (token_spans_kernel<true>), from the records the fill_tags call on this workspace left for this
// batch and these labels -- the tagged writer's contract; on the tagged writer's runs (whole multiples of fill_tags')
namespace vptc {
vpt_status token_tags_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                             const uint64_t* d_out_offsets, size_t n_documents, uint64_t total_boundaries, const uint8_t* d_labels,
                             uint64_t* d_token_offsets, uint32_t* d_token_ends, int32_t* d_token_tags, uint64_t capacity, hipStream_t stream,
                             uint64_t* total_out) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (!p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    if (p->n_tags == 0 || n_documents == 0)   // no tag models: what the untagged call writes, and no tag entry is touched
        return spans_device(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_documents, total_boundaries, d_labels, d_token_offsets, d_token_ends, capacity,
                            stream, total_out, nullptr, nullptr);
    if (!p->vocab_error.empty()) return fail(VPT_RUNTIME_ERROR, p->vocab_error);
    if (!d_token_offsets || !d_utf8 || !d_byte_offsets || !d_out_offsets || (total_boundaries && !d_labels) || (capacity && (!d_token_ends || !d_token_tags)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    vpt::SpanTags T{};
    if (const vpt_status st = tag_records_for(b, n_documents, total_boundaries, true, &T.tag); st != VPT_OK) return st;
    VPT_HIP(hipSetDevice(p->device));
    T.token_tags = d_token_tags; T.vocab_slot = p->d_vocab_slot; T.vocab_ids = p->d_vocab_ids;
    T.n_models = uint32_t(p->vocab.slot.size() / (2 * size_t(p->n_tags))); T.n_strings = uint32_t(p->vocab.ids.size());
    vpt::SpanParams S{};
    S.text = d_utf8; S.boff = d_byte_offsets; S.ooff = d_out_offsets; S.labels = d_labels; S.n_sent = n_documents;
    S.total_boundaries = total_boundaries; S.token_ends = d_token_ends; S.token_offsets = d_token_offsets; S.capacity = capacity;
    S.status = b->d_ctrl;
    vpt::EmitFuse F{};
    if (const vpt_status st = plan_runs(p, b, n_documents, total_boundaries, true, T.tag.run_sent, total_out, nullptr, nullptr, stream, &F); st != VPT_OK) return st;
    VPT_HIP(vpt::launch_token_tags(S, T, F, stream));
    b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
    return VPT_OK;
}

// The stop filter over a finished CSR (kernels_token_filter.hip): count, scan, scatter.  The number of tokens is on the device; capacity_in bounds it.
vpt_status token_filter_device(const vpt_predictor* p, vpt_batch* b, const vpt_tag_stop* stop, const uint64_t* d_token_offsets,
                               const uint32_t* d_token_ends, const int32_t* d_token_tags, size_t n_documents, uint64_t capacity_in,
                               uint64_t* d_offsets_out, uint32_t* d_starts_out, uint32_t* d_ends_out, uint32_t* d_positions_out, int32_t* d_tags_out,
                               uint64_t capacity, hipStream_t stream, uint64_t* total_out, bool with_tags) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (stop && stop->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: stop: does not belong to this predictor");
    if (!d_token_offsets || !d_offsets_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    const uint32_t nt = (with_tags && p->predict_tags) ? p->n_tags : 0u;   // (without tags: the untagged stream's starts and positions)
    if ((capacity_in && (!d_token_ends || (nt && !d_token_tags))) || (capacity && (!d_starts_out || !d_ends_out || !d_positions_out || (nt && !d_tags_out))))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    VPT_HIP(hipSetDevice(p->device));
    vpt::TokenFilterParams P{};
    P.token_offsets = d_token_offsets; P.token_ends = d_token_ends; P.token_tags = d_token_tags; P.n_docs = n_documents; P.capacity_in = capacity_in;
    P.n_tags = nt;
    if (stop && nt) {
        P.model_bits = stop->model_bits; P.rule_bits = stop->rule_bits; P.model_words = stop->model_words; P.rule_words = stop->rule_words;
        P.n_vocab = stop->n_vocab; P.n_rule = stop->n_rule;
    }
    P.out_offsets = d_offsets_out; P.out_starts = d_starts_out; P.out_ends = d_ends_out; P.out_positions = d_positions_out; P.out_tags = d_tags_out;
    P.capacity_out = capacity;
    P.n_blocks = std::max<uint64_t>((capacity_in + vpt::kTokenFilterBlock - 1) / vpt::kTokenFilterBlock, 1);
    if (P.n_blocks > 0x7FFFFFFFull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: capacity: the filter takes fewer than 2^39 tokens per call");
    const size_t n_counts = size_t(P.n_blocks) + 1, n_part = vpt::scan_part_entries(P.n_blocks);
    if (const vpt_status st = b->d_filt.grow(n_counts + n_part); st != VPT_OK) return st;
    VPT_HIP(hipMemsetAsync(b->d_filt, 0, (n_counts + n_part) * sizeof(uint64_t), stream));
    P.counts = b->d_filt; P.total_out = total_out; P.status = b->d_ctrl;
    VPT_HIP(vpt::launch_token_filter(P, b->d_filt + n_counts, stream));
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}
}  // namespace vptc

vpt_status vpt_token_tags_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                       const uint64_t* d_out_offsets, size_t n_documents, uint64_t total_boundaries, const uint8_t* d_labels,
                                       uint64_t* d_token_offsets, uint32_t* d_token_ends, int32_t* d_token_tags, uint64_t capacity, void* hip_stream) {
    return token_tags_device(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_documents, total_boundaries, d_labels, d_token_offsets, d_token_ends,
                             d_token_tags, capacity, static_cast<hipStream_t>(hip_stream), nullptr);
}

vpt_status vpt_token_filter_batch_device(const vpt_predictor* p, vpt_batch* b, const void* stop, const uint64_t* d_token_offsets,
                                         const uint32_t* d_token_ends, const int32_t* d_token_tags, size_t n_documents, uint64_t capacity_in,
                                         uint64_t* d_offsets_out, uint32_t* d_starts_out, uint32_t* d_ends_out, uint32_t* d_positions_out,
                                         int32_t* d_tags_out, uint64_t capacity, void* hip_stream) {
    return token_filter_device(p, b, static_cast<const vpt_tag_stop*>(stop), d_token_offsets, d_token_ends, d_token_tags, n_documents, capacity_in,
                               d_offsets_out, d_starts_out, d_ends_out, d_positions_out, d_tags_out, capacity, static_cast<hipStream_t>(hip_stream), nullptr);
}

vpt_status vpt_token_filter_tile(uint32_t* n_tokens) {
    if (!n_tokens) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *n_tokens = vpt::kTokenFilterBlock;
    return VPT_OK;
}

// ---- the tag stop set (tag_stop.hpp): (slot, tag string) pairs resolved into bitmaps over the predictor's vocabulary and the tagger's
vpt_status vpt_tag_stop_create(const vpt_predictor* p, const void* tagger, const uint32_t* slots, const uint8_t* tag_bytes, const uint64_t* tag_offsets,
                               size_t n_entries, void** out) {
    if (out) *out = nullptr;
    if (!p || !out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (n_entries && (!slots || !tag_offsets)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    const vpt_pattern_tagger* t = static_cast<const vpt_pattern_tagger*>(tagger);
    if (t && t->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: tagger: does not belong to this predictor");
    if (!p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    if (!p->vocab_error.empty()) return fail(VPT_RUNTIME_ERROR, p->vocab_error);
    vpt::StopBitmap M, R;
    static const uint8_t none = 0;
    static const uint32_t zero_off = 0;
    try {
        M = vpt::build_stop_bitmap(slots, tag_bytes ? tag_bytes : &none, tag_offsets, n_entries, p->n_tags, p->vocab.raw_off.data(),
                                   p->vocab.raw_bytes.empty() ? &none : p->vocab.raw_bytes.data(), p->vocab.size());
        if (t) R = vpt::build_stop_bitmap(slots, tag_bytes ? tag_bytes : &none, tag_offsets, n_entries, p->n_tags, t->n_ids ? t->raw_off.data() : &zero_off,
                                          t->raw_bytes.empty() ? &none : t->raw_bytes.data(), t->n_ids);
    } catch (const vpt::StopError& e) {
        return fail(VPT_INVALID_ARGUMENT, e.what());
    } catch (const std::bad_alloc&) {
        return fail(VPT_RUNTIME_ERROR, "out of host memory while building the stop set");
    }
    VPT_HIP(hipSetDevice(p->device));
    vpt_tag_stop* s = new (std::nothrow) vpt_tag_stop();
    if (!s) return fail(VPT_RUNTIME_ERROR, "out of host memory");
    s->pred = p; s->tagger = t; s->device = p->device;
    s->model_words = M.words; s->rule_words = R.words; s->n_vocab = p->vocab.size(); s->n_rule = t ? t->n_ids : 0u;
    const size_t mb = (M.bits.size() * 4 + 255) & ~size_t(255), rb = R.bits.size() * 4, total = mb + rb + 256;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->mem), total);
    if (e == hipSuccess) e = hipMemset(s->mem, 0, total);
    if (e == hipSuccess && !M.bits.empty()) e = hipMemcpy(s->mem, M.bits.data(), M.bits.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && rb) e = hipMemcpy(s->mem + mb, R.bits.data(), rb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(s->mem);
        delete s;
        return fail(VPT_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
    }
    s->model_bits = M.bits.empty() ? nullptr : reinterpret_cast<const uint32_t*>(s->mem);
    s->rule_bits = rb ? reinterpret_cast<const uint32_t*>(s->mem + mb) : nullptr;
    *out = s;
    return VPT_OK;
}

void vpt_tag_stop_destroy(void* stop) {
    vpt_tag_stop* s = static_cast<vpt_tag_stop*>(stop);
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipFree(s->mem);
    delete s;
}

vpt_status vpt_write_tokenized_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                            const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries,
                                            const uint8_t* d_labels, uint8_t* d_text_out, uint64_t text_capacity,
                                            uint64_t* d_text_offsets_out, void* hip_stream) {
    return emit_device(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, d_labels, false, d_text_out, text_capacity,
                       d_text_offsets_out, static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_write_tagged_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                         const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries,
                                         const uint8_t* d_labels, const int32_t* d_tags, uint8_t* d_text_out, uint64_t text_capacity,
                                         uint64_t* d_text_offsets_out, void* hip_stream) {
    (void)d_tags;   // (until round 6: the dense array of fill_tags; the tags are the workspace's records of that call now -- NULL is fine)
    return emit_device(p, b, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, d_labels, true, d_text_out, text_capacity,
                       d_text_offsets_out, static_cast<hipStream_t>(hip_stream));
}

// The predict CLI's stdout for a batch whose scores and labels are on the device (predict/src/main.rs:66-93, 122-176): fill_tags (with its scores
// and tag models when the tag block is wanted), the writer's T into the workspace, then the listing's count / scan / write (kernels_listing.hip).
vpt_status vpt_predict_listing_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                            const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries, uint64_t text_bytes,
                                            const int32_t* d_scores, const uint8_t* d_labels, unsigned listing, uint8_t* d_out, uint64_t capacity,
                                            uint64_t* d_listing_offsets_out, void* hip_stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (listing & ~unsigned(VPT_LISTING_ALL)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: listing: unknown bit");
    if ((listing & (VPT_LISTING_TAG_SCORES | VPT_LISTING_TAGGED)) && !p->predict_tags)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    if (!d_listing_offsets_out || (capacity && !d_out)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    VPT_HIP(hipSetDevice(p->device));
    if (n_sentences == 0) {
        VPT_HIP(hipMemsetAsync(d_listing_offsets_out, 0, sizeof(uint64_t), stream));
        b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
        return VPT_OK;
    }
    if (!d_utf8 || !d_byte_offsets || !d_out_offsets || (total_boundaries && (!d_labels || ((listing & VPT_LISTING_SCORES) && !d_scores))))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    const uint64_t total_c = total_boundaries + n_sentences;
    if (total_c >= 0xFFFFFF00ull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: a listing takes fewer than 2^32 - 256 chars per call");
    const bool with_tags = (listing & (VPT_LISTING_TAG_SCORES | VPT_LISTING_TAGGED)) && p->n_tags > 0;
    const bool tag_block = (listing & VPT_LISTING_TAG_SCORES) && p->n_tags > 0;
    vpt_status st;
    // the workspace of the listing: the elements' sizes / positions, the scan's state, a flag word, and the checked copy of the offsets that every
    // launch below takes (kernels_listing.hip: offsets that decrease never reach fill_tags' runs)
    vpt::ListingParams L{};
    L.n_elem = 2 * total_c + n_sentences;
    const size_t n_part = vpt::scan_part_entries(L.n_elem), n_pos = size_t(L.n_elem) + 2;
    if ((st = b->d_lst_pos.grow(n_pos + n_part + 2 + n_sentences + 1)) != VPT_OK) return st;
    VPT_HIP(hipMemsetAsync(b->d_lst_pos + n_pos, 0, (n_part + 2) * sizeof(uint64_t), stream));
    uint64_t* const ooff = b->d_lst_pos + n_pos + n_part + 2;
    VPT_HIP(vpt::launch_listing_offsets(d_out_offsets, n_sentences, total_boundaries, ooff, reinterpret_cast<uint32_t*>(b->d_lst_pos + n_pos + n_part), b->d_ctrl, stream));
    if (with_tags) {   // Sentence::fill_tags with store_tag_scores (main.rs:113-115, 132-134): leaves the chars in d_cps, the records for the writer
        if (tag_block) {
            if ((st = b->d_tag_scores.grow(size_t(total_c) * p->max_tag_scores + 16)) != VPT_OK) return st;
            if ((st = b->d_tag_models.grow(size_t(total_c) + 16)) != VPT_OK) return st;
        }
        st = vpt_fill_tags_scores_batch_device(p, b, d_utf8, d_byte_offsets, ooff, n_sentences, total_boundaries, d_labels, nullptr,
                                               tag_block ? b->d_tag_scores.p : nullptr, tag_block ? b->d_tag_models.p : nullptr, hip_stream);
        if (st != VPT_OK) return st;
    } else if (listing & (VPT_LISTING_SCORES | VPT_LISTING_TAG_SCORES)) {
        if ((st = b->d_cps.grow(size_t(total_c) + 16)) != VPT_OK) return st;
        const bool fw = (b->flags & VPT_FLAG_KYTEA_FULLWIDTH) != 0;
        VPT_HIP(vpt::launch_decode_chars(d_utf8, d_byte_offsets, ooff, n_sentences, total_c, p->d_cinfo + (fw ? 65536 : 0), b->d_cps, nullptr, b->d_ctrl, stream, fw));
    }
    const bool tagged = (listing & VPT_LISTING_TAGGED) && p->n_tags > 0;
    const uint64_t t_cap = 3 * text_bytes + (tagged ? total_c * (uint64_t(p->max_tag_suffix) + (b->tagger ? b->tagger->max_suffix : 0u)) : 0) + 16;
    if ((st = b->d_tok.grow(size_t(t_cap) + 16)) != VPT_OK) return st;
    if ((st = b->d_toff.grow(n_sentences + 1)) != VPT_OK) return st;
    st = emit_device(p, b, d_utf8, d_byte_offsets, ooff, n_sentences, total_boundaries, d_labels, tagged, b->d_tok, t_cap, b->d_toff, stream);
    if (st != VPT_OK) return st;
    L.cps = b->d_cps; L.ooff = ooff; L.scores = d_scores; L.labels = d_labels; L.n_sent = n_sentences; L.total_boundaries = total_boundaries;
    L.t_text = b->d_tok; L.t_off = b->d_toff; L.t_cap = t_cap;
    if (tag_block) {
        L.tag_models = b->d_tag_models; L.tag_scores = p->max_tag_scores ? b->d_tag_scores.p : nullptr; L.score_stride = p->max_tag_scores;
        L.n_models = p->dtag.n_models; L.n_strings = p->dtag.n_strings;
        L.models = p->dtag.models; L.slots = p->dtag.slots; L.slot_str = p->dtag.slot_str; L.str_off = p->dtag.str_off; L.str_bytes = p->dtag.str_bytes;
    }
    L.flags = listing; L.pos = b->d_lst_pos; L.out = d_out; L.out_offsets = d_listing_offsets_out; L.capacity = capacity; L.status = b->d_ctrl;
    VPT_HIP(vpt::launch_listing(L, b->d_lst_pos + n_pos, stream));
    b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
    return VPT_OK;
}

// The most bytes the candidates of one token take in the tag block: per slot "\t", per candidate its string, ":", up to 11 chars of score and ","
vpt_status vpt_predictor_max_tag_listing(const vpt_predictor* p, uint32_t* n_bytes) {
    if (!p || !n_bytes) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *n_bytes = 0;
    if (!p->has_tags || p->dtag.n_models == 0) return VPT_OK;
    const int64_t known = p->max_tag_listing.load(std::memory_order_acquire);
    if (known >= 0) { *n_bytes = uint32_t(known); return VPT_OK; }
    VPT_HIP(hipSetDevice(p->device));
    const PredictorMeta& m = p->meta;
    std::vector<uint32_t> models(size_t(m.sec_bytes[kSecTagModels] / 4)), slots(size_t(m.sec_bytes[kSecTagSlots] / 4)), slot_str(size_t(m.sec_bytes[kSecTagSlotStr] / 4)),
        str_off(size_t(m.sec_bytes[kSecTagStrOff] / 4));
    VPT_HIP(hipMemcpy(models.data(), p->dtag.models, models.size() * 4, hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(slots.data(), p->dtag.slots, slots.size() * 4, hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(slot_str.data(), p->dtag.slot_str, slot_str.size() * 4, hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(str_off.data(), p->dtag.str_off, str_off.size() * 4, hipMemcpyDeviceToHost));
    uint64_t best = 0;
    for (uint32_t k = 0; k < p->dtag.n_models && 12ull * k + 9 < models.size(); ++k) {
        uint64_t n = 0;
        for (uint32_t s = models[12 * k + 8], e = s + models[12 * k + 9]; s < e && 2ull * s + 1 < slots.size() && s < slot_str.size(); ++s) {
            n += 1;
            for (uint32_t c = 0; c < slots[2 * s] && size_t(slot_str[s]) + c + 1 < str_off.size(); ++c)
                n += uint64_t(str_off[slot_str[s] + c + 1] - str_off[slot_str[s] + c]) + 13;
        }
        best = std::max(best, n);
    }
    *n_bytes = uint32_t(std::min<uint64_t>(best, 0xFFFFFFFFull));
    p->max_tag_listing.store(int64_t(*n_bytes), std::memory_order_release);
    return VPT_OK;
}

namespace vptc {
vpt_status count_boundaries_impl(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                 size_t n_sentences, uint64_t* d_out_offsets, void* hip_stream, uint64_t text_bytes_hint) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (!d_out_offsets || (n_sentences && (!d_utf8 || !d_byte_offsets))) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    VPT_HIP(hipSetDevice(p->device));
    if (n_sentences == 0) VPT_HIP(hipMemsetAsync(d_out_offsets, 0, sizeof(uint64_t), stream));
    else {
        const vpt_status st = b->d_scan_part.grow(vpt::scan_part_entries(n_sentences));
        if (st != VPT_OK) return st;
        VPT_HIP(vpt::launch_count_boundaries(d_utf8, d_byte_offsets, n_sentences, d_out_offsets, b->d_scan_part, b->d_ctrl, nullptr /* nobody reads the longest sentence: no launch to clear it */, text_bytes_hint, stream));
    }
    b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
    return VPT_OK;
}
}  // namespace vptc

vpt_status vpt_count_boundaries_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                       size_t n_sentences, uint64_t* d_out_offsets, void* hip_stream) {
    return count_boundaries_impl(p, b, d_utf8, d_byte_offsets, n_sentences, d_out_offsets, hip_stream, 0);
}

// Sentence::char_types for a batch (sentence.rs:1016; CharacterType::get_type, sentence.rs:50-67): one u8 per char,
// char c of sentence i at types_out[out_offsets[i] + i + c]; with VPT_FLAG_KYTEA_FULLWIDTH the types of the normalised text
// (what the CLI's Sentence holds, predict/src/main.rs:126-129).
vpt_status vpt_char_types_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                       const uint64_t* d_out_offsets, size_t n_sentences, uint64_t total_boundaries, uint8_t* d_types_out,
                                       void* hip_stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (n_sentences == 0) return VPT_OK;
    if (!d_utf8 || !d_byte_offsets || !d_out_offsets || !d_types_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    VPT_HIP(hipSetDevice(p->device));
    const uint32_t* cinfo = p->d_cinfo + ((b->flags & VPT_FLAG_KYTEA_FULLWIDTH) ? 65536 : 0);
    VPT_HIP(vpt::launch_decode_chars(d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries + n_sentences, cinfo, nullptr, d_types_out,
                                     b->d_ctrl, stream, (b->flags & VPT_FLAG_KYTEA_FULLWIDTH) != 0));
    b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
    return VPT_OK;
}

// ---- PatternMatchTagger (vaporetto_rules/src/sentence_filters/pattern_match_tagger.rs): the rule table on the predictor's device
vpt_status vpt_pattern_tagger_create(const vpt_predictor* p, const uint8_t* surfaces, const uint64_t* offsets, size_t n_rules, const uint32_t* slot_counts,
                                     const uint8_t* present, const uint8_t* tag_bytes, const uint64_t* tag_offsets, void** out) {
    if (out) *out = nullptr;
    if (!p || !out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (n_rules && (!surfaces || !offsets || !slot_counts)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    size_t n_entries = 0;
    for (size_t r = 0; r < n_rules; ++r) n_entries += slot_counts[r];
    if (n_entries && (!present || !tag_offsets)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    vpt::HostRuleTable H;
    try {
        static const uint8_t none = 0;
        H = vpt::build_rule_table(surfaces, offsets, n_rules, slot_counts, present, tag_bytes ? tag_bytes : &none, tag_offsets, p->n_tags);
    } catch (const vpt::RuleError& e) {
        return fail(VPT_INVALID_ARGUMENT, e.what());
    } catch (const std::bad_alloc&) {
        return fail(VPT_RUNTIME_ERROR, "out of host memory while building the rule table");
    }
    VPT_HIP(hipSetDevice(p->device));
    vpt_pattern_tagger* t = new (std::nothrow) vpt_pattern_tagger();
    if (!t) return fail(VPT_RUNTIME_ERROR, "out of host memory");
    t->pred = p; t->device = p->device;
    t->bits = H.bits; t->max_len = H.max_len; t->n_tags = p->n_tags; t->n_ids = H.n_ids; t->max_suffix = H.max_suffix; t->n_keys = H.n_keys;
    t->raw_off = std::move(H.raw_off); t->raw_bytes = std::move(H.raw_bytes);
    // one allocation, 256-byte sections: slots | surfaces' code points | rule_tags | id_str | the arena (the predictor's tag strings, then the rules')
    const size_t pred_bytes = p->has_tags ? size_t(p->meta.sec_bytes[kSecTagStrBytes]) : 0;
    if (uint64_t(pred_bytes) + H.str_bytes.size() >= 0xFFFFFFFFull) { delete t; return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: rules: the tags take 4 GB or more"); }
    std::vector<uint32_t> id_str(2 * size_t(H.n_ids));
    for (uint32_t k = 0; k < H.n_ids; ++k) { id_str[2 * k] = uint32_t(pred_bytes) + H.str_off[k]; id_str[2 * k + 1] = H.str_off[k + 1] - H.str_off[k]; }
    auto pad = [](size_t n) { return (n + kTablePadBytes + 255) & ~size_t(255); };
    const size_t o_slots = 0, o_surf = o_slots + pad(4 * H.slots.size()), o_rt = o_surf + pad(4 * H.cps.size()), o_ids = o_rt + pad(4 * H.rule_tags.size()),
                 o_arena = o_ids + pad(4 * id_str.size()), total = o_arena + pad(pred_bytes + H.str_bytes.size());
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&t->mem), total);
    if (e == hipSuccess) e = hipMemset(t->mem, 0, total);
    auto up = [&](size_t at, const void* src, size_t n) { if (e == hipSuccess && n) e = hipMemcpy(t->mem + at, src, n, hipMemcpyHostToDevice); };
    up(o_slots, H.slots.data(), 4 * H.slots.size());
    up(o_surf, H.cps.data(), 4 * H.cps.size());
    up(o_rt, H.rule_tags.data(), 4 * H.rule_tags.size());
    up(o_ids, id_str.data(), 4 * id_str.size());
    if (e == hipSuccess && pred_bytes) e = hipMemcpy(t->mem + o_arena, p->dtag.str_bytes, pred_bytes, hipMemcpyDeviceToDevice);
    up(o_arena + pred_bytes, H.str_bytes.data(), H.str_bytes.size());
    if (e != hipSuccess) {
        (void)hipFree(t->mem);
        delete t;
        return fail(VPT_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
    }
    t->slots = reinterpret_cast<const uint4*>(t->mem + o_slots); t->surf = reinterpret_cast<const uint32_t*>(t->mem + o_surf);
    t->rule_tags = reinterpret_cast<const int32_t*>(t->mem + o_rt); t->id_str = reinterpret_cast<const uint2*>(t->mem + o_ids);
    t->arena = t->mem + o_arena;
    *out = t;
    return VPT_OK;
}

void vpt_pattern_tagger_destroy(void* tagger) {
    vpt_pattern_tagger* t = static_cast<vpt_pattern_tagger*>(tagger);
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipFree(t->mem);
    delete t;
}

vpt_status vpt_pattern_tagger_n_tags(const void* tagger, uint32_t* n_tags) {
    const vpt_pattern_tagger* t = static_cast<const vpt_pattern_tagger*>(tagger);
    if (!t || !n_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *n_tags = t->n_ids;
    return VPT_OK;
}

vpt_status vpt_pattern_tagger_tag(const void* tagger, uint32_t id, const uint8_t** bytes, size_t* len) {
    const vpt_pattern_tagger* t = static_cast<const vpt_pattern_tagger*>(tagger);
    if (!t || !bytes || !len) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (id >= t->n_ids) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: id: no such rule tag");
    *bytes = t->raw_bytes.data() + t->raw_off[id];
    *len = size_t(t->raw_off[id + 1] - t->raw_off[id]);
    return VPT_OK;
}

vpt_status vpt_pattern_tagger_max_tag_suffix(const void* tagger, uint32_t* n_bytes) {
    const vpt_pattern_tagger* t = static_cast<const vpt_pattern_tagger*>(tagger);
    if (!t || !n_bytes) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *n_bytes = t->max_suffix;
    return VPT_OK;
}

vpt_status vpt_pattern_tagger_info(const void* tagger, uint32_t* n_keys, uint32_t* n_slots, uint32_t* max_surface_chars) {
    const vpt_pattern_tagger* t = static_cast<const vpt_pattern_tagger*>(tagger);
    if (!t) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (n_keys) *n_keys = t->n_keys;
    if (n_slots) *n_slots = 1u << t->bits;
    if (max_surface_chars) *max_surface_chars = t->max_len;
    return VPT_OK;
}

vpt_status vpt_pattern_tagger_tile(uint32_t* n_chars) {
    if (!n_chars) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *n_chars = vpt::kPatternStep;
    return VPT_OK;
}

vpt_status vpt_batch_set_pattern_tagger(vpt_batch* b, const void* tagger) {
    const vpt_pattern_tagger* t = static_cast<const vpt_pattern_tagger*>(tagger);
    if (!b) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (t && t->pred != b->pred) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: tagger: does not belong to this workspace's predictor");
    b->tagger = t;
    b->tag_out.chars = 0;   // the records on the workspace were made under the other setting
    return VPT_OK;
}

// ---- the vocabulary of the id pass (vocab_table.hpp): the hashed surface table on the predictor's device
vpt_status vpt_vocab_create(const vpt_predictor* p, const uint8_t* surfaces, const uint64_t* offsets, size_t n_entries, int32_t unk_id, void** out) {
    if (out) *out = nullptr;
    if (!p || !out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (n_entries && (!surfaces || !offsets)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    vpt::HostVocabTable H;
    try {
        H = vpt::build_vocab_table(surfaces, offsets, n_entries);
    } catch (const vpt::VocabError& e) {
        return fail(VPT_INVALID_ARGUMENT, e.what());
    } catch (const std::bad_alloc&) {
        return fail(VPT_RUNTIME_ERROR, "out of host memory while building the vocabulary");
    }
    VPT_HIP(hipSetDevice(p->device));
    vpt_vocab* v = new (std::nothrow) vpt_vocab();
    if (!v) return fail(VPT_RUNTIME_ERROR, "out of host memory");
    v->pred = p; v->device = p->device; v->bits = H.bits; v->max_len = H.max_len; v->n_keys = H.n_keys; v->unk_id = unk_id;
    v->off = std::move(H.off); v->bytes = std::move(H.bytes);
    // one allocation, 256-byte sections: slots | the surfaces' code points
    auto pad = [](size_t n) { return (n + kTablePadBytes + 255) & ~size_t(255); };
    const size_t o_slots = 0, o_surf = o_slots + pad(4 * H.slots.size()), total = o_surf + pad(4 * H.cps.size());
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&v->mem), total);
    if (e == hipSuccess) e = hipMemset(v->mem, 0, total);
    if (e == hipSuccess) e = hipMemcpy(v->mem + o_slots, H.slots.data(), 4 * H.slots.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !H.cps.empty()) e = hipMemcpy(v->mem + o_surf, H.cps.data(), 4 * H.cps.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(v->mem);
        delete v;
        return fail(VPT_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
    }
    v->slots = reinterpret_cast<const uint4*>(v->mem + o_slots); v->surf = reinterpret_cast<const uint32_t*>(v->mem + o_surf);
    *out = v;
    return VPT_OK;
}

void vpt_vocab_destroy(void* vocab) {
    vpt_vocab* v = static_cast<vpt_vocab*>(vocab);
    if (!v) return;
    (void)hipSetDevice(v->device);
    (void)hipFree(v->mem);
    delete v;
}

vpt_status vpt_vocab_info(const void* vocab, uint32_t* n_keys, uint32_t* n_slots, uint32_t* max_surface_chars) {
    const vpt_vocab* v = static_cast<const vpt_vocab*>(vocab);
    if (!v) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (n_keys) *n_keys = v->n_keys;
    if (n_slots) *n_slots = 1u << v->bits;
    if (max_surface_chars) *max_surface_chars = v->max_len;
    return VPT_OK;
}

vpt_status vpt_vocab_surface(const void* vocab, uint32_t id, const uint8_t** bytes, size_t* len) {
    const vpt_vocab* v = static_cast<const vpt_vocab*>(vocab);
    if (!v || !bytes || !len) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (id >= v->n_keys) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: id: no such vocabulary entry");
    *bytes = v->bytes.data() + v->off[id];
    *len = size_t(v->off[id + 1] - v->off[id]);
    return VPT_OK;
}

vpt_status vpt_vocab_tile(uint32_t* n_tokens) {
    if (!n_tokens) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *n_tokens = vpt::kVocabTile;
    return VPT_OK;
}

// The id pass over a finished CSR (kernels_vocab.hip): one launch.  The number of tokens is on the device; capacity_in bounds it and sizes the grid.
namespace vptc {
vpt_status token_ids_device(const vpt_predictor* p, vpt_batch* b, const vpt_vocab* vocab, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                            size_t n_documents, const uint64_t* d_token_offsets, const uint32_t* d_token_starts, const uint32_t* d_token_ends,
                            uint64_t capacity_in, unsigned flags, int32_t* d_token_ids, hipStream_t stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (!vocab) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: vocab: must not be NULL");
    if (vocab->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: vocab: does not belong to this predictor");
    if (flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (n_documents == 0) return VPT_OK;   // no document owns a token: nothing is enqueued
    if (!d_utf8 || !d_byte_offsets || !d_token_offsets || (capacity_in && (!d_token_ends || !d_token_ids)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    if ((capacity_in + vpt::kVocabTile - 1) / vpt::kVocabTile > 0x7FFFFFFFull)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: capacity: the id pass takes fewer than 2^39 tokens per call");
    VPT_HIP(hipSetDevice(p->device));
    vpt::VocabParams P{};
    P.text = d_utf8; P.boff = d_byte_offsets; P.n_docs = n_documents; P.token_offsets = d_token_offsets; P.token_starts = d_token_starts;
    P.token_ends = d_token_ends; P.capacity_in = capacity_in; P.slots = vocab->slots; P.surf = vocab->surf;
    P.cinfo = (flags & VPT_FLAG_KYTEA_FULLWIDTH) ? p->d_cinfo + 65536 : nullptr;
    P.bits = vocab->bits; P.max_len = vocab->max_len; P.unk_id = vocab->unk_id; P.ids = d_token_ids; P.status = b->d_ctrl;
    VPT_HIP(vpt::launch_token_ids(P, stream));
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}
}  // namespace vptc

vpt_status vpt_token_ids_batch_device(const vpt_predictor* p, vpt_batch* b, const void* vocab, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                      size_t n_documents, const uint64_t* d_token_offsets, const uint32_t* d_token_starts, const uint32_t* d_token_ends,
                                      uint64_t capacity_in, unsigned flags, int32_t* d_token_ids, void* hip_stream) {
    return token_ids_device(p, b, static_cast<const vpt_vocab*>(vocab), d_utf8, d_byte_offsets, n_documents, d_token_offsets, d_token_starts,
                            d_token_ends, capacity_in, flags, d_token_ids, static_cast<hipStream_t>(hip_stream));
}

// ---- the vocabulary counter (vocab_count.hpp; kernels_vocab_count.hip): an accumulating table of token surfaces on the predictor's device
namespace {
// everything enqueued on the counter is through: the host may read and rewrite it
vpt_status vocab_counter_quiesce(vpt_vocab_counter* c) {
    VPT_HIP(hipSetDevice(c->device));
    if (c->in_flight) VPT_HIP(hipStreamSynchronize(c->last_stream));
    c->in_flight = false;
    c->last_stream = nullptr;
    return VPT_OK;
}
vpt_status vocab_counter_ctrl(vpt_vocab_counter* c, uint64_t* ctrl) {
    if (const vpt_status st = vocab_counter_quiesce(c); st != VPT_OK) return st;
    VPT_HIP(hipMemcpy(ctrl, c->view.ctrl, 8 * vpt::kVcCtrlWords, hipMemcpyDeviceToHost));
    if (uint32_t(ctrl[vpt::kVcFull])) c->known_full = true;
    return VPT_OK;
}
}  // namespace

vpt_status vpt_vocab_counter_create(const vpt_predictor* p, uint64_t max_keys, uint64_t max_surface_chars, uint64_t arena_chars, void** out) {
    if (out) *out = nullptr;
    if (!p || !out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (max_keys < 1 || max_keys > vpt::kVocabCounterMaxKeys) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: max_keys: must be between 1 and 2^24");
    if (max_surface_chars < 1 || max_surface_chars > vpt::kVocabCounterMaxSurfaceChars)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: max_surface_chars: must be between 1 and 2^24");
    const uint64_t arena = vpt::vocab_counter_arena_chars(max_keys, arena_chars);
    if (arena > vpt::kVocabCounterMaxArenaChars) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: arena_chars: must be below 2^32");
    VPT_HIP(hipSetDevice(p->device));
    vpt_vocab_counter* c = new (std::nothrow) vpt_vocab_counter();
    if (!c) return fail(VPT_RUNTIME_ERROR, "out of host memory");
    c->pred = p; c->device = p->device;
    const uint32_t n_slots = vpt::vocab_counter_slots(max_keys);
    // one allocation, 256-byte sections: control words | slots | counts | key records | arena | finish's entries
    auto pad = [](size_t n) { return (n + 255) & ~size_t(255); };
    const size_t o_ctrl = 0, o_slots = o_ctrl + pad(8 * vpt::kVcCtrlWords), o_counts = o_slots + pad(8 * size_t(n_slots)),
                 o_keys = o_counts + pad(8 * size_t(n_slots)), o_arena = o_keys + pad(16 * size_t(max_keys)), o_out = o_arena + pad(4 * size_t(arena)),
                 total = o_out + pad(16 * size_t(max_keys));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->mem), total);
    if (e == hipSuccess) e = hipMemset(c->mem, 0, total);
    if (e != hipSuccess) {
        (void)hipFree(c->mem);
        delete c;
        return fail(VPT_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
    }
    c->state_bytes = o_keys;
    vpt::VocabCounterView& V = c->view;
    V.ctrl = reinterpret_cast<uint64_t*>(c->mem + o_ctrl); V.slots = reinterpret_cast<uint64_t*>(c->mem + o_slots);
    V.counts = reinterpret_cast<uint64_t*>(c->mem + o_counts); V.keys = reinterpret_cast<uint4*>(c->mem + o_keys);
    V.arena = reinterpret_cast<uint32_t*>(c->mem + o_arena); V.out = reinterpret_cast<uint4*>(c->mem + o_out);
    V.arena_chars = arena; V.n_slots = n_slots; V.max_keys = uint32_t(max_keys); V.max_chars = uint32_t(max_surface_chars);
    c->offsets.assign(1, 0);
    *out = c;
    return VPT_OK;
}

void vpt_vocab_counter_destroy(void* counter) {
    vpt_vocab_counter* c = static_cast<vpt_vocab_counter*>(counter);
    if (!c) return;
    (void)vocab_counter_quiesce(c);
    (void)hipFree(c->mem);
    delete c;
}

vpt_status vpt_vocab_counter_reset(void* counter) {
    vpt_vocab_counter* c = static_cast<vpt_vocab_counter*>(counter);
    if (!c) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: counter: must not be NULL");
    if (const vpt_status st = vocab_counter_quiesce(c); st != VPT_OK) return st;
    VPT_HIP(hipMemset(c->mem, 0, c->state_bytes));
    c->known_full = false;
    c->surfaces.clear(); c->counts.clear(); c->offsets.assign(1, 0);
    return VPT_OK;
}

vpt_status vpt_vocab_counter_info(void* counter, uint64_t* n_keys, uint64_t* n_counted, uint64_t* n_skipped, uint32_t* n_slots, uint32_t* full) {
    vpt_vocab_counter* c = static_cast<vpt_vocab_counter*>(counter);
    if (!c) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: counter: must not be NULL");
    uint64_t ctrl[vpt::kVcCtrlWords] = {};
    if (const vpt_status st = vocab_counter_ctrl(c, ctrl); st != VPT_OK) return st;
    if (n_keys) *n_keys = std::min<uint64_t>(ctrl[vpt::kVcKeys], c->view.max_keys);
    if (n_counted) *n_counted = ctrl[vpt::kVcCounted];
    if (n_skipped) *n_skipped = ctrl[vpt::kVcSkipped];
    if (n_slots) *n_slots = c->view.n_slots;
    if (full) *full = uint32_t(ctrl[vpt::kVcFull]) ? 1u : 0u;
    return VPT_OK;
}

namespace vptc {
vpt_status vocab_count_device(const vpt_predictor* p, vpt_batch* b, vpt_vocab_counter* c, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                              size_t n_documents, const uint64_t* d_token_offsets, const uint32_t* d_token_starts, const uint32_t* d_token_ends,
                              uint64_t capacity_in, unsigned flags, hipStream_t stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (!c) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: counter: must not be NULL");
    if (c->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: counter: does not belong to this predictor");
    if (flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (c->known_full) return fail(VPT_INVALID_ARGUMENT, kVocabCounterFull);
    if (n_documents == 0) return VPT_OK;   // no document owns a token: nothing is enqueued
    if (!d_utf8 || !d_byte_offsets || !d_token_offsets || (capacity_in && !d_token_ends))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    if ((capacity_in + vpt::kVocabTile - 1) / vpt::kVocabTile > 0x7FFFFFFFull)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: capacity: a count call takes fewer than 2^39 tokens");
    VPT_HIP(hipSetDevice(p->device));
    if (const vpt_status st = b->d_vrec.grow(2 * size_t(capacity_in) + 2); st != VPT_OK) return st;
    vpt::VocabCountParams P{};
    P.text = d_utf8; P.boff = d_byte_offsets; P.n_docs = n_documents; P.token_offsets = d_token_offsets; P.token_starts = d_token_starts;
    P.token_ends = d_token_ends; P.capacity_in = capacity_in;
    P.cinfo = (flags & VPT_FLAG_KYTEA_FULLWIDTH) ? p->d_cinfo + 65536 : nullptr;
    P.C = c->view; P.rec = b->d_vrec; P.status = b->d_ctrl;
    VPT_HIP(vpt::launch_vocab_count(P, stream));
    c->last_stream = stream; c->in_flight = true;
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}
}  // namespace vptc

vpt_status vpt_vocab_count_batch_device(const vpt_predictor* p, vpt_batch* b, void* counter, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                        size_t n_documents, const uint64_t* d_token_offsets, const uint32_t* d_token_starts,
                                        const uint32_t* d_token_ends, uint64_t capacity_in, unsigned flags, void* hip_stream) {
    return vocab_count_device(p, b, static_cast<vpt_vocab_counter*>(counter), d_utf8, d_byte_offsets, n_documents, d_token_offsets, d_token_starts,
                              d_token_ends, capacity_in, flags, static_cast<hipStream_t>(hip_stream));
}

// ---- postings of a finished CSR's ids (kernels_postings.hip): keys, the trainer's sort, heads, the trainer's scan, emit and terms
vpt_status vpt_postings_tile(uint32_t* n_tokens) {
    if (!n_tokens) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    // (the constant is the sort's tile: one tile of histograms up to it, two behind it)
    if (vpt::train_radix_scratch(vpt::kPostingsSortTile) != 256 || vpt::train_radix_scratch(uint64_t(vpt::kPostingsSortTile) + 1) != 512)
        return fail(VPT_RUNTIME_ERROR, "vpt_postings_tile: kPostingsSortTile is not the sort's tile");
    *n_tokens = vpt::kPostingsSortTile;
    return VPT_OK;
}

// (every driver below lays its scratch out in b->d_post through a struct of scratch_carve.hpp: S.x.at(m) is section x of the layout)
namespace vptc {
vpt_status postings_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_token_offsets, size_t n_documents, const int32_t* d_token_ids,
                           uint64_t capacity_in, uint32_t n_terms, uint64_t doc_base, uint64_t* d_term_offsets, uint32_t* d_post_docs, uint32_t* d_post_tfs,
                           uint64_t capacity_out, uint64_t* d_post_first, uint32_t* d_token_order, uint64_t* d_counts, hipStream_t stream) {
    VPT_TRY(check_batch(p, b));
    if (!d_token_offsets || !d_token_ids || !d_term_offsets || !d_post_docs || !d_post_tfs || !d_counts)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    if ((d_post_first == nullptr) != (d_token_order == nullptr))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: post_first / token_order: both or neither");
    VPT_TRY(check_n_terms(n_terms));
    VPT_TRY(check_pass_tokens(capacity_in));
    VPT_TRY(check_doc_range(doc_base, n_documents));
    VPT_HIP(hipSetDevice(p->device));
    VPT_HIP(hipMemsetAsync(d_counts, 0, 16, stream));
    if (n_documents == 0) {   // no document owns a token: no posting
        VPT_HIP(hipMemsetAsync(d_term_offsets, 0, 8 * (size_t(n_terms) + 1), stream));
        if (d_post_first) VPT_HIP(hipMemsetAsync(d_post_first, 0, 8, stream));
        b->last_stream = stream; b->pending = true;
        return VPT_OK;
    }
    const uint64_t n = capacity_in;
    const vptcarve::PostingsScratch S(n);
    VPT_TRY(b->d_post.grow(S.bytes()));
    unsigned char* m = b->d_post;
    vpt::PostingsParams P{};
    P.token_offsets = d_token_offsets; P.n_docs = n_documents; P.ids = d_token_ids; P.capacity_in = capacity_in; P.n_terms = n_terms; P.doc_base = doc_base;
    P.keydoc = S.keydoc.at(m); P.order = S.order.at(m); P.skey = S.skey.at(m); P.flags = S.flags.at(m); P.scan = S.scan.at(m);
    P.term_offsets = d_term_offsets; P.post_docs = d_post_docs; P.post_tfs = d_post_tfs; P.capacity_out = capacity_out; P.post_first = d_post_first;
    P.token_order = d_token_order; P.counts = d_counts; P.status = b->d_ctrl;
    uint64_t* part = S.tail.partials.at(m);
    vptcarve::PassList passes;
    passes.add(0, n_terms);
    VPT_HIP(vpt::launch_postings_keys(P, stream));
    VPT_HIP(vpt::train_radix_sort(P.keydoc, 2, passes.v, passes.n, n, P.order, P.skey, S.tail.hist.at(m), S.tail.hist_scan.at(m), part, stream));
    VPT_HIP(vpt::launch_postings_heads(P, stream));
    VPT_HIP(vpt::train_scan(P.flags, n, P.scan, part, stream));
    VPT_HIP(vpt::launch_postings_emit(P, stream));
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}
}  // namespace vptc

vpt_status vpt_postings_batch_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_token_offsets, size_t n_documents,
                                     const int32_t* d_token_ids, uint64_t capacity_in, uint32_t n_terms, uint64_t doc_base, uint64_t* d_term_offsets,
                                     uint32_t* d_post_docs, uint32_t* d_post_tfs, uint64_t capacity_out, uint64_t* d_post_first, uint32_t* d_token_order,
                                     uint64_t* d_counts, void* hip_stream) {
    return postings_device(p, b, d_token_offsets, n_documents, d_token_ids, capacity_in, n_terms, doc_base, d_term_offsets, d_post_docs, d_post_tfs,
                           capacity_out, d_post_first, d_token_order, d_counts, static_cast<hipStream_t>(hip_stream));
}

// ---- merge of postings segments (kernels_postings_merge.hip).  Ordered: load, offsets (the table), copy, check.  General: load, offsets,
// records, the trainer's sort over the document and the term word, heads, the trainer's scan, emit and terms.
// Of positional segments.  Ordered: load, offsets and the position offsets (the two tables), copy with post_first, check, pcopy.  General:
// load, offsets, records, the sort, heads, ranks (the tfs in sorted order, the inverse of the order), the scan of the heads, emit and terms,
// the scan of the tfs, first, pcopy.
vpt_status vpt_postings_merge_limits(uint32_t* max_segments) {
    if (!max_segments) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *max_segments = vpt::kPostingsMergeMaxSegments;
    return VPT_OK;
}

namespace {
// The plain merge (segments: vpt_postings_segment; the position arguments are not looked at) and the positional merge (segments:
// vpt_postings_positional_segment) over one block of arguments, checks and scratch: the plain one is the positional one without position
// arrays -- what only those need is a section of count 0 and a launch that is left out.
vpt_status merge_device_impl(const vpt_predictor* p, vpt_batch* b, const void* segments, bool positional, size_t n_segments, uint32_t n_terms_out,
                             unsigned flags, uint64_t* d_term_offsets_out, uint32_t* d_post_docs_out, uint32_t* d_post_tfs_out, uint64_t* d_post_first_out,
                             uint64_t capacity_out, uint32_t* d_post_positions_out, uint64_t capacity_positions_out, uint64_t* d_counts,
                             hipStream_t stream) {
    VPT_TRY(check_batch(p, b));
    if (!segments || !d_term_offsets_out || !d_post_docs_out || !d_post_tfs_out || !d_counts || (positional && (!d_post_first_out || !d_post_positions_out)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    VPT_TRY(check_n_segments(n_segments));
    VPT_TRY(check_n_terms(n_terms_out));
    if (flags & ~unsigned(VPT_POSTINGS_MERGE_ORDERED)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (positional) VPT_TRY(check_merge_positions(0, capacity_positions_out));
    const uint32_t K = uint32_t(n_segments);
    std::vector<vpt::PostingsMergeSegment> segs(K);
    std::vector<vpt::PostingsMergePosSegment> psegs(positional ? K : 0);
    uint64_t n = 0, np = 0;
    for (uint32_t s = 0; s < K; ++s) {
        const vpt_postings_positional_segment in = merge_segment(segments, positional, s);
        if (!in.d_term_offsets || !in.d_post_docs || !in.d_post_tfs || (positional && (!in.d_post_first || !in.d_post_positions)))
            return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
        if (in.n_terms > n_terms_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: segment: n_terms above n_terms_out");
        VPT_TRY(check_merge_places(n, in.capacity));
        VPT_TRY(check_merge_positions(np, in.capacity_positions));
        segs[s] = vpt::PostingsMergeSegment{in.d_term_offsets, in.d_post_docs, in.d_post_tfs, in.capacity, n, in.n_terms, 0u};
        if (positional) psegs[s] = vpt::PostingsMergePosSegment{in.d_post_first, in.d_post_positions, in.capacity_positions, np};
        n += in.capacity;
        np += in.capacity_positions;
    }
    VPT_HIP(hipSetDevice(p->device));
    const bool ordered = (flags & VPT_POSTINGS_MERGE_ORDERED) != 0;
    const uint64_t row = uint64_t(n_terms_out) + 1;
    const vptcarve::MergeScratch<vpt::PostingsMergeSegment, vpt::PostingsMergePosSegment> S(K, n, row, positional);
    VPT_TRY(b->d_post.grow(S.bytes(ordered)));
    unsigned char* m = b->d_post;
    vpt::PostingsMergePosParams Q{};
    vpt::PostingsMergeParams& P = Q.M;
    P.segs = S.segs.at(m); P.n_segs = K; P.n_terms = n_terms_out; P.n_places = n;
    P.term_offsets = d_term_offsets_out; P.post_docs = d_post_docs_out; P.post_tfs = d_post_tfs_out; P.capacity_out = capacity_out;
    P.counts = d_counts; P.status = b->d_ctrl;
    if (positional) {
        Q.psegs = S.psegs.at(m); Q.n_pplaces = np;
        Q.post_first = d_post_first_out; Q.post_positions = d_post_positions_out; Q.capacity_positions_out = capacity_positions_out;
    }
    if (ordered) {
        P.range = S.range.at(m); P.table = S.table.at(m);
        if (positional) Q.ptable = S.ptable.at(m);
    } else {
        P.rec = S.rec.at(m); P.order = S.order.at(m); P.skey = S.skey.at(m); P.flags = S.flags.at(m); P.scan = S.scan.at(m);
        if (positional) { Q.ptf = S.ptf.at(m); Q.inv = S.inv.at(m); Q.pscan = S.pscan.at(m); }
    }
    VPT_HIP(vpt::launch_postings_merge_load(P, segs.data(), stream));
    if (positional) VPT_HIP(vpt::launch_postings_merge_positions_load(Q, psegs.data(), stream));
    if (ordered) {
        VPT_HIP(positional ? vpt::launch_postings_merge_positions_ordered(Q, stream) : vpt::launch_postings_merge_ordered(P, stream));
    } else {
        uint64_t* part = S.tail.partials.at(m);
        VPT_HIP(vpt::launch_postings_merge_records(P, stream));
        if (n == 0) {   // no place: no posting, no position (the offsets were still checked)
            VPT_HIP(hipMemsetAsync(d_term_offsets_out, 0, 8 * size_t(row), stream));
            if (positional) VPT_HIP(hipMemsetAsync(d_post_first_out, 0, 8, stream));
            VPT_HIP(hipMemsetAsync(d_counts, 0, positional ? 24 : 16, stream));
        } else {
            vptcarve::PassList passes;   // the document word's four bytes, then the term word's for the values 0 .. n_terms_out
            passes.add(1, 0xFFFFFFFFu);
            passes.add(0, n_terms_out);
            VPT_HIP(vpt::train_radix_sort(P.rec, 3, passes.v, passes.n, n, P.order, P.skey, S.tail.hist.at(m), S.tail.hist_scan.at(m), part, stream));
            VPT_HIP(vpt::launch_postings_merge_heads(P, stream));
            if (positional) VPT_HIP(vpt::launch_postings_merge_positions_ranks(Q, stream));
            VPT_HIP(vpt::train_scan(P.flags, n, P.scan, part, stream));
            VPT_HIP(vpt::launch_postings_merge_emit(P, stream));
            if (positional) {
                VPT_HIP(vpt::train_scan(Q.ptf, n, Q.pscan, part, stream));
                VPT_HIP(vpt::launch_postings_merge_positions_general(Q, stream));
            }
        }
    }
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}
}  // namespace

namespace vptc {
vpt_status postings_merge_device(const vpt_predictor* p, vpt_batch* b, const vpt_postings_segment* segments, size_t n_segments, uint32_t n_terms_out,
                                 unsigned flags, uint64_t* d_term_offsets_out, uint32_t* d_post_docs_out, uint32_t* d_post_tfs_out, uint64_t capacity_out,
                                 uint64_t* d_counts, hipStream_t stream) {
    return merge_device_impl(p, b, segments, false, n_segments, n_terms_out, flags, d_term_offsets_out, d_post_docs_out, d_post_tfs_out, nullptr,
                             capacity_out, nullptr, 0, d_counts, stream);
}

vpt_status postings_merge_positional_device(const vpt_predictor* p, vpt_batch* b, const vpt_postings_positional_segment* segments, size_t n_segments,
                                            uint32_t n_terms_out, unsigned flags, uint64_t* d_term_offsets_out, uint32_t* d_post_docs_out,
                                            uint32_t* d_post_tfs_out, uint64_t* d_post_first_out, uint64_t capacity_out, uint32_t* d_post_positions_out,
                                            uint64_t capacity_positions_out, uint64_t* d_counts, hipStream_t stream) {
    return merge_device_impl(p, b, segments, true, n_segments, n_terms_out, flags, d_term_offsets_out, d_post_docs_out, d_post_tfs_out, d_post_first_out,
                             capacity_out, d_post_positions_out, capacity_positions_out, d_counts, stream);
}
}  // namespace vptc

vpt_status vpt_postings_merge_positional_device(const vpt_predictor* p, vpt_batch* b, const void* segments, size_t n_segments, uint32_t n_terms_out,
                                                unsigned flags, uint64_t* d_term_offsets_out, uint32_t* d_post_docs_out, uint32_t* d_post_tfs_out,
                                                uint64_t* d_post_first_out, uint64_t capacity_out, uint32_t* d_post_positions_out,
                                                uint64_t capacity_positions_out, uint64_t* d_counts, void* hip_stream) {
    return postings_merge_positional_device(p, b, static_cast<const vpt_postings_positional_segment*>(segments), n_segments, n_terms_out, flags,
                                            d_term_offsets_out, d_post_docs_out, d_post_tfs_out, d_post_first_out, capacity_out, d_post_positions_out,
                                            capacity_positions_out, d_counts, static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_postings_merge_device(const vpt_predictor* p, vpt_batch* b, const void* segments, size_t n_segments, uint32_t n_terms_out, unsigned flags,
                                     uint64_t* d_term_offsets_out, uint32_t* d_post_docs_out, uint32_t* d_post_tfs_out, uint64_t capacity_out,
                                     uint64_t* d_counts, void* hip_stream) {
    return postings_merge_device(p, b, static_cast<const vpt_postings_segment*>(segments), n_segments, n_terms_out, flags, d_term_offsets_out,
                                 d_post_docs_out, d_post_tfs_out, capacity_out, d_counts, static_cast<hipStream_t>(hip_stream));
}

// ---- BM25 top-k search over a segment (kernels_postings_search.hip): slots, the trainer's scan, expand, the trainer's sort over the document
// and the query word, heads, the trainer's scan, sum and ranges, the trainer's sort over the score and the query word, take.  The boolean search
// (kernels_postings_boolean.hip) puts queries, slots and expand of its own in front of the same sort.
vpt_status vpt_postings_search_limits(uint32_t* max_query_slots) {
    if (!max_query_slots) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *max_query_slots = vpt::kSearchMaxQuerySlots;
    return VPT_OK;
}

namespace {
// What the three searches check behind their pointers, in this order.  phrase: the phrase search's words for its sizes.
vpt_status check_search_arguments(bool phrase, uint32_t n_terms, uint32_t n_queries, uint32_t k, uint64_t capacity_slots, uint64_t capacity_places,
                                  uint64_t doc_base, uint64_t n_documents, float k1, float bm_b, float avgdl) {
    VPT_TRY(check_n_terms(n_terms));
    VPT_TRY(check_n_queries(n_queries));
    VPT_TRY(check_top_k(n_queries, k));
    VPT_TRY(check_search_sizes(phrase, capacity_slots, capacity_places));
    VPT_TRY(check_doc_range(doc_base, n_documents));
    if (!(k1 >= 0.0f && k1 <= 65536.0f)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: k1: must be between 0 and 65536");
    if (!(bm_b >= 0.0f && bm_b <= 1.0f)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: b: must be between 0 and 1");
    if (!(avgdl >= 0x1p-32f && avgdl <= 0x1p32f)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: avgdl: must be between 2^-32 and 2^32");
    return VPT_OK;
}

// The OR search (boolean false: d_query_occurs is not looked at) and the boolean search (kernels_postings_boolean.hip: queries, slots and expand
// of its own, then the OR search's launches as they stand) over one block of arguments, checks and scratch.  lists: the clause search's derived
// segment, or nullptr; with it the launches behind expand leave the outputs alone on the lists call's status bits too (kClauseErrors).
struct ClauseLists {
    const uint64_t* d_offsets;
    const uint32_t* d_docs;
    const uint32_t* d_tfs;
    uint32_t n_lists;
    uint64_t capacity;
};
vpt_status search_device_impl(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs, const uint32_t* d_post_tfs,
                              uint32_t n_terms, uint64_t capacity_postings, uint64_t doc_base, uint64_t n_documents, const uint32_t* d_doc_lens,
                              const uint64_t* d_query_offsets, const int32_t* d_query_terms, const float* d_query_weights, bool boolean,
                              const uint8_t* d_query_occurs, uint32_t n_queries, uint64_t capacity_slots, float k1, float bm_b, float avgdl, uint32_t k,
                              uint64_t capacity_candidates, uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_counts, uint64_t* d_match_counts,
                              uint64_t* d_counts, hipStream_t stream, const ClauseLists* lists = nullptr) {
    VPT_TRY(check_batch(p, b));
    if (!d_term_offsets || !d_post_docs || !d_post_tfs || !d_doc_lens || !d_query_offsets || !d_query_terms || !d_query_weights || !d_hit_docs ||
        !d_hit_scores || !d_hit_counts || !d_match_counts || !d_counts || (boolean && !d_query_occurs) ||
        (lists && lists->n_lists && (!lists->d_offsets || !lists->d_docs || !lists->d_tfs)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    VPT_TRY(check_search_arguments(false, n_terms, n_queries, k, capacity_slots, capacity_candidates, doc_base, n_documents, k1, bm_b, avgdl));
    if (lists) VPT_TRY(check_clause_lists(n_terms, lists->n_lists, lists->capacity));
    VPT_HIP(hipSetDevice(p->device));
    VPT_HIP(hipMemsetAsync(d_counts, 0, 24, stream));
    const uint64_t n = capacity_candidates, ns = capacity_slots;
    const vptcarve::SearchScratch S(n, ns, n_queries, boolean);
    VPT_TRY(b->d_post.grow(S.bytes()));
    unsigned char* m = b->d_post;
    vpt::PostingsSearchParams P{};
    P.term_offsets = d_term_offsets; P.post_docs = d_post_docs; P.post_tfs = d_post_tfs; P.capacity_postings = capacity_postings; P.n_terms = n_terms;
    P.doc_base = doc_base; P.n_docs = n_documents; P.doc_lens = d_doc_lens;
    P.query_offsets = d_query_offsets; P.query_terms = d_query_terms; P.query_weights = d_query_weights; P.n_queries = n_queries; P.capacity_slots = ns;
    P.n_places = n; P.k1 = k1; P.b = bm_b; P.avgdl = avgdl; P.k = k;
    P.slot_df = S.slot_df.at(m); P.base = S.base.at(m); P.slot_query = S.slot_query.at(m); P.rec = S.rec.at(m); P.hit = S.hit.at(m);
    P.order = S.order.at(m); P.skey = S.skey.at(m); P.flags = S.flags.at(m); P.scan = S.scan.at(m); P.qstart = S.qstart.at(m);
    P.hit_docs = d_hit_docs; P.hit_scores = d_hit_scores; P.hit_counts = d_hit_counts; P.match_counts = d_match_counts; P.counts = d_counts;
    P.status = b->d_ctrl; P.error_mask = lists ? vpt::kClauseErrors : vpt::kSearchErrors;
    uint64_t *hist = S.tail.hist.at(m), *hscan = S.tail.hist_scan.at(m), *part = S.tail.partials.at(m);
    vptcarve::PassList group, rank;
    group.add(0, n_documents);   // (at most four bytes: the key is relative to doc_base)
    group.add(1, n_queries);
    rank.add(2, 0xFFFFFFFFu);    // the four bytes of ~bits(score)
    rank.add(0, n_queries);
    if (boolean) {
        vpt::PostingsBooleanParams B{};
        B.S = P; B.occurs = d_query_occurs; B.q_anchor = S.q_anchor.at(m); B.q_flags = S.q_flags.at(m);
        if (lists && lists->n_lists) {   // (none: the kernels of one segment)
            B.list_offsets = lists->d_offsets; B.list_docs = lists->d_docs; B.list_tfs = lists->d_tfs;
            B.n_lists = lists->n_lists; B.capacity_lists = lists->capacity;
        }
        VPT_HIP(vpt::launch_postings_boolean_queries(B, stream));
        VPT_HIP(vpt::launch_postings_boolean_slots(B, stream));
        VPT_HIP(vpt::train_scan(P.slot_df, ns, P.base, part, stream));
        VPT_HIP(vpt::launch_postings_boolean_expand(B, stream));
    } else {
        VPT_HIP(vpt::launch_postings_search_slots(P, stream));
        VPT_HIP(vpt::train_scan(P.slot_df, ns, P.base, part, stream));
        VPT_HIP(vpt::launch_postings_search_expand(P, stream));
    }
    VPT_HIP(vpt::train_radix_sort(P.rec, 3, group.v, group.n, n, P.order, P.skey, hist, hscan, part, stream));
    VPT_HIP(vpt::launch_postings_search_heads(P, stream));
    VPT_HIP(vpt::train_scan(P.flags, n, P.scan, part, stream));
    VPT_HIP(vpt::launch_postings_search_sum(P, stream));
    VPT_HIP(vpt::train_radix_sort(P.hit, 3, rank.v, rank.n, n, P.order, P.skey, hist, hscan, part, stream));
    VPT_HIP(vpt::launch_postings_search_take(P, stream));
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}
}  // namespace

namespace vptc {
vpt_status postings_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs, const uint32_t* d_post_tfs,
                                  uint32_t n_terms, uint64_t capacity_postings, uint64_t doc_base, uint64_t n_documents, const uint32_t* d_doc_lens,
                                  const uint64_t* d_query_offsets, const int32_t* d_query_terms, const float* d_query_weights, uint32_t n_queries,
                                  uint64_t capacity_slots, float k1, float bm_b, float avgdl, uint32_t k, uint64_t capacity_candidates,
                                  uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_counts, uint64_t* d_match_counts, uint64_t* d_counts,
                                  hipStream_t stream) {
    return search_device_impl(p, b, d_term_offsets, d_post_docs, d_post_tfs, n_terms, capacity_postings, doc_base, n_documents, d_doc_lens, d_query_offsets,
                              d_query_terms, d_query_weights, false, nullptr, n_queries, capacity_slots, k1, bm_b, avgdl, k, capacity_candidates, d_hit_docs,
                              d_hit_scores, d_hit_counts, d_match_counts, d_counts, stream);
}

vpt_status postings_boolean_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                          const uint32_t* d_post_tfs, uint32_t n_terms, uint64_t capacity_postings, uint64_t doc_base, uint64_t n_documents,
                                          const uint32_t* d_doc_lens, const uint64_t* d_query_offsets, const int32_t* d_query_terms,
                                          const float* d_query_weights, const uint8_t* d_query_occurs, uint32_t n_queries, uint64_t capacity_slots, float k1,
                                          float bm_b, float avgdl, uint32_t k, uint64_t capacity_candidates, uint32_t* d_hit_docs, float* d_hit_scores,
                                          uint32_t* d_hit_counts, uint64_t* d_match_counts, uint64_t* d_counts, hipStream_t stream) {
    return search_device_impl(p, b, d_term_offsets, d_post_docs, d_post_tfs, n_terms, capacity_postings, doc_base, n_documents, d_doc_lens, d_query_offsets,
                              d_query_terms, d_query_weights, true, d_query_occurs, n_queries, capacity_slots, k1, bm_b, avgdl, k, capacity_candidates,
                              d_hit_docs, d_hit_scores, d_hit_counts, d_match_counts, d_counts, stream);
}

// The boolean search over the segment and a derived segment of lists (the phrase lists call's output): its scratch is the boolean search's.
vpt_status postings_clause_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                         const uint32_t* d_post_tfs, uint32_t n_terms, uint64_t capacity_postings, const uint64_t* d_list_offsets,
                                         const uint32_t* d_list_docs, const uint32_t* d_list_tfs, uint32_t n_lists, uint64_t capacity_lists,
                                         uint64_t doc_base, uint64_t n_documents, const uint32_t* d_doc_lens, const uint64_t* d_query_offsets,
                                         const int32_t* d_query_terms, const float* d_query_weights, const uint8_t* d_query_occurs, uint32_t n_queries,
                                         uint64_t capacity_slots, float k1, float bm_b, float avgdl, uint32_t k, uint64_t capacity_candidates,
                                         uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_counts, uint64_t* d_match_counts, uint64_t* d_counts,
                                         hipStream_t stream) {
    const ClauseLists lists{d_list_offsets, d_list_docs, d_list_tfs, n_lists, capacity_lists};
    return search_device_impl(p, b, d_term_offsets, d_post_docs, d_post_tfs, n_terms, capacity_postings, doc_base, n_documents, d_doc_lens, d_query_offsets,
                              d_query_terms, d_query_weights, true, d_query_occurs, n_queries, capacity_slots, k1, bm_b, avgdl, k, capacity_candidates,
                              d_hit_docs, d_hit_scores, d_hit_counts, d_match_counts, d_counts, stream, &lists);
}
}  // namespace vptc

vpt_status vpt_postings_clause_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                             const uint32_t* d_post_tfs, uint32_t n_terms, uint64_t capacity_postings, const uint64_t* d_list_offsets,
                                             const uint32_t* d_list_docs, const uint32_t* d_list_tfs, uint32_t n_lists, uint64_t capacity_lists,
                                             uint64_t doc_base, uint64_t n_documents, const uint32_t* d_doc_lens, const uint64_t* d_query_offsets,
                                             const int32_t* d_query_terms, const float* d_query_weights, const uint8_t* d_query_occurs,
                                             uint32_t n_queries, uint64_t capacity_slots, float k1, float b_param, float avgdl, uint32_t k,
                                             uint64_t capacity_candidates, uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_counts,
                                             uint64_t* d_match_counts, uint64_t* d_counts, void* hip_stream) {
    return postings_clause_search_device(p, b, d_term_offsets, d_post_docs, d_post_tfs, n_terms, capacity_postings, d_list_offsets, d_list_docs, d_list_tfs,
                                         n_lists, capacity_lists, doc_base, n_documents, d_doc_lens, d_query_offsets, d_query_terms, d_query_weights,
                                         d_query_occurs, n_queries, capacity_slots, k1, b_param, avgdl, k, capacity_candidates, d_hit_docs, d_hit_scores,
                                         d_hit_counts, d_match_counts, d_counts, static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_postings_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                      const uint32_t* d_post_tfs, uint32_t n_terms, uint64_t capacity_postings, uint64_t doc_base, uint64_t n_documents,
                                      const uint32_t* d_doc_lens, const uint64_t* d_query_offsets, const int32_t* d_query_terms,
                                      const float* d_query_weights, uint32_t n_queries, uint64_t capacity_slots, float k1, float b_param, float avgdl,
                                      uint32_t k, uint64_t capacity_candidates, uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_counts,
                                      uint64_t* d_match_counts, uint64_t* d_counts, void* hip_stream) {
    return postings_search_device(p, b, d_term_offsets, d_post_docs, d_post_tfs, n_terms, capacity_postings, doc_base, n_documents, d_doc_lens,
                                  d_query_offsets, d_query_terms, d_query_weights, n_queries, capacity_slots, k1, b_param, avgdl, k, capacity_candidates,
                                  d_hit_docs, d_hit_scores, d_hit_counts, d_match_counts, d_counts, static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_postings_boolean_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                              const uint32_t* d_post_tfs, uint32_t n_terms, uint64_t capacity_postings, uint64_t doc_base,
                                              uint64_t n_documents, const uint32_t* d_doc_lens, const uint64_t* d_query_offsets,
                                              const int32_t* d_query_terms, const float* d_query_weights, const uint8_t* d_query_occurs,
                                              uint32_t n_queries, uint64_t capacity_slots, float k1, float b_param, float avgdl, uint32_t k,
                                              uint64_t capacity_candidates, uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_counts,
                                              uint64_t* d_match_counts, uint64_t* d_counts, void* hip_stream) {
    return postings_boolean_search_device(p, b, d_term_offsets, d_post_docs, d_post_tfs, n_terms, capacity_postings, doc_base, n_documents, d_doc_lens,
                                          d_query_offsets, d_query_terms, d_query_weights, d_query_occurs, n_queries, capacity_slots, k1, b_param, avgdl, k,
                                          capacity_candidates, d_hit_docs, d_hit_scores, d_hit_counts, d_match_counts, d_counts,
                                          static_cast<hipStream_t>(hip_stream));
}

// ---- the position lists of a segment and the exact-phrase search over them (kernels_postings_phrase.hip).  Positions: one launch.  Search:
// queries, the trainer's scan (probe bases), probe, the trainer's scan, heads, the trainer's scan, emit and ranges, the trainer's sort over the
// score and the query word, take.
vpt_status vpt_postings_phrase_limits(uint32_t* max_phrase_terms) {
    if (!max_phrase_terms) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *max_phrase_terms = vpt::kPhraseMaxTerms;
    return VPT_OK;
}

vpt_status vpt_postings_sloppy_phrase_limits(uint32_t* max_phrase_terms, uint32_t* max_slop) {
    if (!max_phrase_terms || !max_slop) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    *max_phrase_terms = vpt::kPhraseMaxTerms;
    *max_slop = vpt::kPhraseMaxSlop;
    return VPT_OK;
}

namespace vptc {
vpt_status postings_positions_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_token_offsets, size_t n_documents, uint64_t capacity_in,
                                     const uint32_t* d_token_positions, const uint64_t* d_term_offsets, uint32_t n_terms, const uint64_t* d_post_first,
                                     uint64_t capacity_postings, const uint32_t* d_token_order, uint32_t* d_post_positions, hipStream_t stream) {
    VPT_TRY(check_batch(p, b));
    if (!d_token_offsets || !d_term_offsets || !d_post_first || !d_token_order || !d_post_positions)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    VPT_TRY(check_n_terms(n_terms));
    VPT_TRY(check_pass_tokens(capacity_in));
    VPT_HIP(hipSetDevice(p->device));
    vpt::PostingsPositionsParams P{};
    P.token_offsets = d_token_offsets; P.n_docs = n_documents; P.capacity_in = capacity_in; P.positions = d_token_positions;
    P.term_offsets = d_term_offsets; P.n_terms = n_terms; P.post_first = d_post_first; P.capacity_postings = capacity_postings;
    P.token_order = d_token_order; P.post_positions = d_post_positions; P.status = b->d_ctrl;
    VPT_HIP(vpt::launch_postings_positions(P, stream));   // (no document or no place: no token is indexed, nothing to write)
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}

vpt_status postings_phrase_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                         const uint32_t* d_post_tfs, const uint64_t* d_post_first, const uint32_t* d_post_positions, uint32_t n_terms,
                                         uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base, uint64_t n_documents,
                                         const uint32_t* d_doc_lens, const uint64_t* d_query_offsets, const int32_t* d_query_terms,
                                         const float* d_query_weights, uint32_t n_queries, uint64_t capacity_slots, float k1, float bm_b, float avgdl,
                                         uint32_t k, uint64_t capacity_probes, uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_freqs,
                                         uint32_t* d_hit_counts, uint64_t* d_match_counts, uint64_t* d_counts, bool sloppy,
                                         const uint32_t* d_query_slops, hipStream_t stream) {
    VPT_TRY(check_batch(p, b));
    if (!d_term_offsets || !d_post_docs || !d_post_tfs || !d_post_first || !d_post_positions || !d_doc_lens || !d_query_offsets || !d_query_terms ||
        !d_query_weights || !d_hit_docs || !d_hit_scores || !d_hit_counts || !d_match_counts || !d_counts)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    VPT_TRY(check_search_arguments(true, n_terms, n_queries, k, capacity_slots, capacity_probes, doc_base, n_documents, k1, bm_b, avgdl));
    VPT_HIP(hipSetDevice(p->device));
    VPT_HIP(hipMemsetAsync(d_counts, 0, 24, stream));
    const uint64_t n = capacity_probes, nq = n_queries;
    const vptcarve::PhraseScratch S(n, n_queries);
    VPT_TRY(b->d_post.grow(S.bytes()));
    unsigned char* m = b->d_post;
    vpt::PostingsPhraseParams P{};
    P.term_offsets = d_term_offsets; P.post_docs = d_post_docs; P.post_tfs = d_post_tfs; P.post_first = d_post_first; P.post_positions = d_post_positions;
    P.capacity_postings = capacity_postings; P.capacity_positions = capacity_positions; P.n_terms = n_terms;
    P.doc_base = doc_base; P.n_docs = n_documents; P.doc_lens = d_doc_lens;
    P.query_offsets = d_query_offsets; P.query_terms = d_query_terms; P.query_weights = d_query_weights; P.n_queries = n_queries;
    P.query_slops = sloppy ? d_query_slops : nullptr;
    P.capacity_slots = capacity_slots; P.n_places = n; P.k1 = k1; P.b = bm_b; P.avgdl = avgdl; P.k = k;
    P.q_anchor = S.q_anchor.at(m); P.q_run = S.q_run.at(m); P.q_probes = S.q_probes.at(m); P.base = S.base.at(m); P.qstart = S.qstart.at(m);
    P.flags = S.flags.at(m); P.plen = S.plen.at(m); P.pdoc = S.pdoc.at(m); P.pq = S.pq.at(m); P.hpf = S.hpf.at(m); P.order = S.order.at(m);
    P.skey = S.skey.at(m); P.hit = S.hit.at(m); P.scan = S.scan.at(m);
    P.hit_docs = d_hit_docs; P.hit_scores = d_hit_scores; P.hit_freqs = d_hit_freqs; P.hit_counts = d_hit_counts; P.match_counts = d_match_counts;
    P.counts = d_counts; P.status = b->d_ctrl;
    uint64_t* part = S.tail.partials.at(m);
    vptcarve::PassList rank;
    rank.add(2, 0xFFFFFFFFu);   // the four bytes of ~bits(score)
    rank.add(0, n_queries);
    VPT_HIP(vpt::launch_postings_phrase_queries(P, stream));
    VPT_HIP(vpt::train_scan(P.q_probes, nq, P.base, part, stream));
    VPT_HIP(sloppy ? vpt::launch_postings_phrase_sloppy_probe(P, stream) : vpt::launch_postings_phrase_probe(P, stream));
    VPT_HIP(vpt::train_scan(P.flags, n, P.scan, part, stream));
    VPT_HIP(vpt::launch_postings_phrase_heads(P, stream));
    VPT_HIP(vpt::train_scan(P.flags, n, P.scan, part, stream));
    VPT_HIP(vpt::launch_postings_phrase_emit(P, stream));
    VPT_HIP(vpt::train_radix_sort(P.hit, 3, rank.v, rank.n, n, P.order, P.skey, S.tail.hist.at(m), S.tail.hist_scan.at(m), part, stream));
    VPT_HIP(vpt::launch_postings_phrase_take(P, stream));
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}

// The phrase search's launches up to the second heads scan over the phrase search's scratch (what the sort and the take work in lies idle), no
// weights, then the lists launch: nothing is sized from a value read back.
vpt_status postings_phrase_lists_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                        const uint32_t* d_post_tfs, const uint64_t* d_post_first, const uint32_t* d_post_positions, uint32_t n_terms,
                                        uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base, uint64_t n_documents,
                                        const uint64_t* d_phrase_offsets, const int32_t* d_phrase_terms, uint32_t n_phrases, uint64_t capacity_slots,
                                        uint64_t capacity_probes, uint64_t* d_list_offsets, uint32_t* d_list_docs, uint32_t* d_list_tfs,
                                        uint64_t capacity_lists, uint64_t* d_counts, bool sloppy, const uint32_t* d_phrase_slops,
                                        hipStream_t stream) {
    VPT_TRY(check_batch(p, b));
    if (!d_term_offsets || !d_post_docs || !d_post_tfs || !d_post_first || !d_post_positions || !d_phrase_offsets || !d_phrase_terms || !d_list_offsets ||
        !d_list_docs || !d_list_tfs || !d_counts)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    VPT_TRY(check_n_terms(n_terms));
    VPT_TRY(bad_argument(n_phrases == 0 || n_phrases > vpt::kSearchMaxQueries, "InvalidArgumentError: n_phrases: must be between 1 and 2^24"));
    VPT_TRY(check_search_sizes(true, capacity_slots, capacity_probes));
    VPT_TRY(check_clause_lists(n_terms, 0, capacity_lists));
    VPT_TRY(check_doc_range(doc_base, n_documents));
    VPT_HIP(hipSetDevice(p->device));
    VPT_HIP(hipMemsetAsync(d_counts, 0, 24, stream));
    const uint64_t n = capacity_probes, nq = n_phrases;
    const vptcarve::PhraseScratch S(n, n_phrases);
    VPT_TRY(b->d_post.grow(S.bytes()));
    unsigned char* m = b->d_post;
    vpt::PostingsPhraseParams P{};
    P.term_offsets = d_term_offsets; P.post_docs = d_post_docs; P.post_tfs = d_post_tfs; P.post_first = d_post_first; P.post_positions = d_post_positions;
    P.capacity_postings = capacity_postings; P.capacity_positions = capacity_positions; P.n_terms = n_terms;
    P.doc_base = doc_base; P.n_docs = n_documents;
    P.query_offsets = d_phrase_offsets; P.query_terms = d_phrase_terms; P.n_queries = n_phrases; P.capacity_slots = capacity_slots; P.n_places = n;
    P.query_slops = sloppy ? d_phrase_slops : nullptr;
    P.q_anchor = S.q_anchor.at(m); P.q_run = S.q_run.at(m); P.q_probes = S.q_probes.at(m); P.base = S.base.at(m); P.qstart = S.qstart.at(m);
    P.flags = S.flags.at(m); P.plen = S.plen.at(m); P.pdoc = S.pdoc.at(m); P.pq = S.pq.at(m); P.scan = S.scan.at(m);
    P.counts = d_counts; P.status = b->d_ctrl;
    P.list_offsets = d_list_offsets; P.list_docs = d_list_docs; P.list_tfs = d_list_tfs; P.capacity_lists = capacity_lists;
    uint64_t* part = S.tail.partials.at(m);
    VPT_HIP(vpt::launch_postings_phrase_queries(P, stream));
    VPT_HIP(vpt::train_scan(P.q_probes, nq, P.base, part, stream));
    VPT_HIP(sloppy ? vpt::launch_postings_phrase_sloppy_probe(P, stream) : vpt::launch_postings_phrase_probe(P, stream));
    VPT_HIP(vpt::train_scan(P.flags, n, P.scan, part, stream));
    VPT_HIP(vpt::launch_postings_phrase_heads(P, stream));
    VPT_HIP(vpt::train_scan(P.flags, n, P.scan, part, stream));
    VPT_HIP(vpt::launch_postings_phrase_lists(P, stream));
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}
}  // namespace vptc

vpt_status vpt_postings_phrase_lists_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                            const uint32_t* d_post_tfs, const uint64_t* d_post_first, const uint32_t* d_post_positions,
                                            uint32_t n_terms, uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base,
                                            uint64_t n_documents, const uint64_t* d_phrase_offsets, const int32_t* d_phrase_terms, uint32_t n_phrases,
                                            uint64_t capacity_slots, uint64_t capacity_probes, uint64_t* d_list_offsets, uint32_t* d_list_docs,
                                            uint32_t* d_list_tfs, uint64_t capacity_lists, uint64_t* d_counts, void* hip_stream) {
    return postings_phrase_lists_device(p, b, d_term_offsets, d_post_docs, d_post_tfs, d_post_first, d_post_positions, n_terms, capacity_postings,
                                        capacity_positions, doc_base, n_documents, d_phrase_offsets, d_phrase_terms, n_phrases, capacity_slots,
                                        capacity_probes, d_list_offsets, d_list_docs, d_list_tfs, capacity_lists, d_counts, false, nullptr,
                                        static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_postings_sloppy_phrase_lists_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                                   const uint32_t* d_post_tfs, const uint64_t* d_post_first, const uint32_t* d_post_positions,
                                                   uint32_t n_terms, uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base,
                                                   uint64_t n_documents, const uint64_t* d_phrase_offsets, const int32_t* d_phrase_terms,
                                                   const uint32_t* d_phrase_slops, uint32_t n_phrases, uint64_t capacity_slots,
                                                   uint64_t capacity_probes, uint64_t* d_list_offsets, uint32_t* d_list_docs, uint32_t* d_list_tfs,
                                                   uint64_t capacity_lists, uint64_t* d_counts, void* hip_stream) {
    return postings_phrase_lists_device(p, b, d_term_offsets, d_post_docs, d_post_tfs, d_post_first, d_post_positions, n_terms, capacity_postings,
                                        capacity_positions, doc_base, n_documents, d_phrase_offsets, d_phrase_terms, n_phrases, capacity_slots,
                                        capacity_probes, d_list_offsets, d_list_docs, d_list_tfs, capacity_lists, d_counts, true, d_phrase_slops,
                                        static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_postings_positions_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_token_offsets, size_t n_documents, uint64_t capacity_in,
                                         const uint32_t* d_token_positions, const uint64_t* d_term_offsets, uint32_t n_terms,
                                         const uint64_t* d_post_first, uint64_t capacity_postings, const uint32_t* d_token_order,
                                         uint32_t* d_post_positions, void* hip_stream) {
    return postings_positions_device(p, b, d_token_offsets, n_documents, capacity_in, d_token_positions, d_term_offsets, n_terms, d_post_first,
                                     capacity_postings, d_token_order, d_post_positions, static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_postings_phrase_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                             const uint32_t* d_post_tfs, const uint64_t* d_post_first, const uint32_t* d_post_positions,
                                             uint32_t n_terms, uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base,
                                             uint64_t n_documents, const uint32_t* d_doc_lens, const uint64_t* d_query_offsets,
                                             const int32_t* d_query_terms, const float* d_query_weights, uint32_t n_queries, uint64_t capacity_slots,
                                             float k1, float b_param, float avgdl, uint32_t k, uint64_t capacity_probes, uint32_t* d_hit_docs,
                                             float* d_hit_scores, uint32_t* d_hit_freqs, uint32_t* d_hit_counts, uint64_t* d_match_counts,
                                             uint64_t* d_counts, void* hip_stream) {
    return postings_phrase_search_device(p, b, d_term_offsets, d_post_docs, d_post_tfs, d_post_first, d_post_positions, n_terms, capacity_postings,
                                         capacity_positions, doc_base, n_documents, d_doc_lens, d_query_offsets, d_query_terms, d_query_weights,
                                         n_queries, capacity_slots, k1, b_param, avgdl, k, capacity_probes, d_hit_docs, d_hit_scores, d_hit_freqs,
                                         d_hit_counts, d_match_counts, d_counts, false, nullptr, static_cast<hipStream_t>(hip_stream));
}

// The sloppy calls: the exact calls' arguments, checks, scratch and launches with the slops beside the queries and the sloppy probe in probe's
// place (d_query_slops NULL: every slop 0).
vpt_status vpt_postings_sloppy_phrase_search_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_term_offsets, const uint32_t* d_post_docs,
                                                    const uint32_t* d_post_tfs, const uint64_t* d_post_first, const uint32_t* d_post_positions,
                                                    uint32_t n_terms, uint64_t capacity_postings, uint64_t capacity_positions, uint64_t doc_base,
                                                    uint64_t n_documents, const uint32_t* d_doc_lens, const uint64_t* d_query_offsets,
                                                    const int32_t* d_query_terms, const float* d_query_weights, const uint32_t* d_query_slops,
                                                    uint32_t n_queries, uint64_t capacity_slots, float k1, float b_param, float avgdl, uint32_t k,
                                                    uint64_t capacity_probes, uint32_t* d_hit_docs, float* d_hit_scores, uint32_t* d_hit_freqs,
                                                    uint32_t* d_hit_counts, uint64_t* d_match_counts, uint64_t* d_counts, void* hip_stream) {
    return postings_phrase_search_device(p, b, d_term_offsets, d_post_docs, d_post_tfs, d_post_first, d_post_positions, n_terms, capacity_postings,
                                         capacity_positions, doc_base, n_documents, d_doc_lens, d_query_offsets, d_query_terms, d_query_weights,
                                         n_queries, capacity_slots, k1, b_param, avgdl, k, capacity_probes, d_hit_docs, d_hit_scores, d_hit_freqs,
                                         d_hit_counts, d_match_counts, d_counts, true, d_query_slops, static_cast<hipStream_t>(hip_stream));
}

// A snapshot: one launch over the slots leaves an entry per key of count >= min_count; those and the arena come to the host, which orders them
// (vocab_count.hpp).  Counting may go on afterwards.
vpt_status vpt_vocab_counter_finish(void* counter, uint64_t min_count, uint64_t max_entries, const uint8_t** surfaces, const uint64_t** offsets,
                                    const uint64_t** counts, size_t* n_entries) {
    vpt_vocab_counter* c = static_cast<vpt_vocab_counter*>(counter);
    if (!c) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: counter: must not be NULL");
    if (!surfaces || !offsets || !counts || !n_entries) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    uint64_t ctrl[vpt::kVcCtrlWords] = {};
    if (const vpt_status st = vocab_counter_ctrl(c, ctrl); st != VPT_OK) return st;
    if (c->known_full) return fail(VPT_INVALID_ARGUMENT, kVocabCounterFull);
    VPT_HIP(hipMemset(c->view.ctrl + vpt::kVcOut, 0, 8));
    VPT_HIP(vpt::launch_vocab_count_finish(c->view, min_count, nullptr));
    uint64_t n_out = 0;
    VPT_HIP(hipMemcpy(&n_out, c->view.ctrl + vpt::kVcOut, 8, hipMemcpyDeviceToHost));
    n_out = std::min<uint64_t>(n_out, c->view.max_keys);
    const uint64_t n_arena = std::min<uint64_t>(ctrl[vpt::kVcArena], c->view.arena_chars);
    try {
        std::vector<uint4> raw(size_t(n_out) + 1);
        std::vector<uint32_t> arena(size_t(n_arena) + 1);
        if (n_out) VPT_HIP(hipMemcpy(raw.data(), c->view.out, 16 * size_t(n_out), hipMemcpyDeviceToHost));
        if (n_arena) VPT_HIP(hipMemcpy(arena.data(), c->view.arena, 4 * size_t(n_arena), hipMemcpyDeviceToHost));
        std::vector<vpt::VocabCountEntry> entries(size_t(n_out) + 1);
        for (size_t k = 0; k < n_out; ++k) entries[k] = {uint64_t(raw[k].x) | (uint64_t(raw[k].y) << 32), raw[k].z, raw[k].w};
        vpt::VocabCountResult R = vpt::finish_vocab_count(entries.data(), size_t(n_out), arena.data(), size_t(n_arena), min_count, max_entries);
        c->surfaces = std::move(R.surfaces); c->offsets = std::move(R.offsets); c->counts = std::move(R.counts);
    } catch (const std::bad_alloc&) {
        return fail(VPT_RUNTIME_ERROR, "out of host memory while ordering the counted surfaces");
    }
    c->surfaces.reserve(1); c->counts.reserve(1);   // (data() of an empty result is still a pointer)
    *surfaces = c->surfaces.data(); *offsets = c->offsets.data(); *counts = c->counts.data();
    *n_entries = c->counts.size();
    return VPT_OK;
}
