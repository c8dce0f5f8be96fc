// C ABI of libvaporetto_hip.so, the host-buffer entry points: the pipelines that move a caller's batch over PCIe around the device-resident calls
// (vpt_predict_batch: chunks over lanes or three streams; vpt_tokenize_batch: lines in, tokenized lines out), the sharded call, single sentences.
#include "capi_internal.hpp"

#include <cmath>

// (the entry points have C linkage from their declarations in include/vaporetto_hip.h)

namespace {

// How vpt_predict_batch takes a host batch of `total_chars` (measured on MI355X behind PCIe 5 x16, profiles/r02_g_e2e.txt):
//   up to 1.5 M chars            one copy in, the kernels, one copy out
//   up to 16 M chars             predict_lanes: 4 lanes, 512 K-char chunks.  The batch is over in about a millisecond, so what counts is
//                                how soon the first copy out starts and that nothing waits on the host: 0.85 ms per 6.4 M chars against
//                                0.98 through the events (3 or 5 lanes, or 256 K / 1 M-char chunks: 0.93 .. 1.05)
//   more                         predict_pipelined: three streams and events, 4 M-char chunks: 6.9 .. 8.1 ms per 64 M chars, steadier over
//                                many chunks than the lanes, whose copies contend (7.3 .. 10 ms)
// VPT_CHUNK_CHARS / VPT_PIPE_LANES (0 = the event pipeline) override; the tests use them to cut small batches into many chunks.
struct PipePlan { int lanes; uint64_t chunk; bool pipelined; };
PipePlan pipeline_plan(const PredictorKnobs& knobs, uint64_t total_chars) {
    PipePlan plan = total_chars <= (uint64_t(16) << 20) ? PipePlan{4, uint64_t(512) << 10, false} : PipePlan{0, uint64_t(4) << 20, false};
    if (knobs.pipe_lanes >= 0) plan.lanes = knobs.pipe_lanes;
    if (knobs.chunk_chars) plan.chunk = knobs.chunk_chars;
    plan.pipelined = total_chars > (plan.lanes > 0 ? 3 * plan.chunk : plan.chunk + plan.chunk / 2);
    return plan;
}

// A few workspaces that take a call's chunks in turn, each on its own stream: lane 0 is the call's, the others are taken from the pool here and
// go back to it when the guard dies -- declared behind lane 0's Workspace, so before it does.
struct Lanes {
    static constexpr int kMax = 8;
    Workspace extra[kMax - 1];
    vpt_batch* lane[kMax] = {};
    int n = 1;
    vpt_status init(const vpt_predictor* p, vpt_batch* b, int n_lanes) {
        n = std::max(1, std::min(n_lanes, kMax));
        lane[0] = b;
        for (int l = 1; l < n; ++l) {
            const vpt_status st = acquire(p, &extra[l - 1]);
            if (st != VPT_OK) return st;
            lane[l] = extra[l - 1].b;
            lane[l]->flags = b->flags;
        }
        return VPT_OK;
    }
    vpt_batch* operator[](size_t k) const { return lane[k % size_t(n)]; }
    // The device's verdict over every chunk (a lane's status word accumulates), folded into `st`: the lanes' words are fetched together, one
    // round trip for all of them instead of one each.
    vpt_status verdict(vpt_status st = VPT_OK) {
        uint32_t ctrl[kMax][2] = {};
        for (int l = 0; l < n; ++l)
            if (lane[l]->pending) VPT_HIP(hipMemcpyAsync(ctrl[l], lane[l]->d_ctrl, sizeof(ctrl[l]), hipMemcpyDeviceToHost, lane[l]->last_stream));
        for (int l = 0; l < n; ++l) {
            if (!lane[l]->pending) continue;
            VPT_HIP(hipStreamSynchronize(lane[l]->last_stream));
            lane[l]->pending = false;
            if (ctrl[l][0]) {
                VPT_HIP(hipMemset(lane[l]->d_ctrl, 0, sizeof(uint32_t)));
                if (st == VPT_OK) st = status_from_bits(ctrl[l][0]);
            }
        }
        return st;
    }
};

// b->chunk_ev holds n events
vpt_status chunk_events(vpt_batch* b, size_t n) {
    while (b->chunk_ev.size() < n) {
        hipEvent_t e;
        VPT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        b->chunk_ev.push_back(e);
    }
    return VPT_OK;
}

// What a call left on the device for the caller, after its sync: the n + 1 offsets, then as many elements as the last of them says -- or none of
// them, and `too_small`, where the caller's buffer holds fewer.
template <typename T>
vpt_status download_sized(uint64_t* offsets_out, const uint64_t* d_offsets, size_t n, T* out, const T* d_out, uint64_t capacity, const char* too_small) {
    VPT_HIP(hipMemcpy(offsets_out, d_offsets, 8 * (n + 1), hipMemcpyDeviceToHost));
    const uint64_t total = offsets_out[n];
    if (total > capacity) return fail(VPT_INVALID_ARGUMENT, too_small);
    if (total) VPT_HIP(hipMemcpy(out, d_out, sizeof(T) * size_t(total), hipMemcpyDeviceToHost));
    return VPT_OK;
}
const char* const kTextTooSmall = "InvalidArgumentError: text_capacity: smaller than the tokenized text";
const char* const kTokensTooSmall = "InvalidArgumentError: capacity: smaller than the number of tokens";

// The cutter of a vpt_predict_batch call over b's pinned staging (both schedules).
vpt_status predict_cutter(vpt_batch* b, const uint64_t* byte_offsets, const uint64_t* out_offsets, size_t n_sentences, uint64_t chunk_chars, vptcut::PredictCutter* out) {
    const uint64_t total_chars = out_offsets[n_sentences] - out_offsets[0] + n_sentences;
    const size_t max_chunks = vptcut::predict_max_chunks(n_sentences, total_chars, chunk_chars);
    const vpt_status st = pinned_words(b, vptcut::predict_pinned_words(n_sentences, max_chunks));
    *out = vptcut::PredictCutter{byte_offsets, out_offsets, n_sentences, chunk_chars, max_chunks, b->h_off};
    return st;
}

// vpt_predict_batch for a LARGE batch: the copy in of chunk k + 1, the kernels of chunk k and the copy out of chunk k - 1 run at
// the same time on three streams over two sets of device buffers, so that a caller with PINNED buffers (vpt_host_alloc) gets
// both directions of the PCIe link busy at once instead of a copy-launch-copy sequence; pageable buffers go through the
// runtime's staging and still overlap with the kernels.  The host walks the sentences ONCE, chunk by chunk -- validating them,
// rebasing their offsets into pinned staging, finding the cut -- while the chunks before are in flight; a chunk costs eleven
// runtime calls (two copies in, two launches, two copies out, events) and a wait of the host for the chunk two before it.  The
// runtime performs this stream's copies out as blit kernels, which the next chunk's kernels queue behind (timeline in
// profiles/r02_g_e2e.txt): copy out and kernels take turns, 0.24 ms per 2 M chars -- 15 % above what the link does both ways.
vpt_status predict_pipelined(const vpt_predictor* p, vpt_batch* b, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                             int32_t* scores_out, uint8_t* labels_out, const uint64_t* out_offsets, uint64_t chunk_chars) {
    if (!b->s_in) {
        VPT_HIP(hipStreamCreateWithFlags(&b->s_in, hipStreamNonBlocking));
        VPT_HIP(hipStreamCreateWithFlags(&b->s_out, hipStreamNonBlocking));
        for (auto& ps : b->pipe) {
            VPT_HIP(hipEventCreateWithFlags(&ps.ev_in, hipEventDisableTiming));
            VPT_HIP(hipEventCreateWithFlags(&ps.ev_k, hipEventDisableTiming));
            VPT_HIP(hipEventCreateWithFlags(&ps.ev_out, hipEventDisableTiming));
        }
    }
    vptcut::PredictCutter cutter{};
    vpt_status st;
    if ((st = predict_cutter(b, byte_offsets, out_offsets, n_sentences, chunk_chars, &cutter)) != VPT_OK) return st;
    for (size_t k = 0; !cutter.done(); ++k) {
        vpt_batch::PipeSet& ps = b->pipe[k & 1];
        // ---- walk the chunk's sentences: validate, rebase, cut
        const vptcut::PredictChunk c = cutter.next();
        if (c.error != vptcut::CutError::kNone) return cut_fail(c.error);
        const size_t n = c.n;
        const uint64_t t0 = byte_offsets[c.a], o0 = out_offsets[c.a], nbytes = c.off[n], nb = c.off[2 * n + 1];
        // ---- this set's buffers are free once chunk k - 2 has been scored (inputs) and copied out (outputs)
        if (k >= 2) { VPT_HIP(hipEventSynchronize(ps.ev_out)); }   // also bounds how far the host runs ahead; growing a buffer below is then safe
        if ((st = ps.text.grow(size_t(nbytes) + 32)) != VPT_OK) return st;
        if ((st = ps.off.grow(2 * (n + 1))) != VPT_OK) return st;
        if (scores_out && (st = ps.scores.grow(size_t(nb) + 1)) != VPT_OK) return st;
        if (labels_out && (st = ps.labels.grow(size_t(nb) + 1)) != VPT_OK) return st;
        VPT_HIP(hipMemcpyAsync(ps.text, utf8 + t0, size_t(nbytes), hipMemcpyHostToDevice, b->s_in));
        VPT_HIP(hipMemcpyAsync(ps.off, c.off, 16 * (n + 1), hipMemcpyHostToDevice, b->s_in));
        VPT_HIP(hipEventRecord(ps.ev_in, b->s_in));
        VPT_HIP(hipStreamWaitEvent(b->own_stream, ps.ev_in, 0));
        b->max_chars = c.max_chars;
        st = vpt_predict_batch_device(p, b, ps.text, ps.off, ps.off + (n + 1), n, nb, c.max_bytes, scores_out ? ps.scores.p : nullptr,
                                      labels_out ? ps.labels.p : nullptr, b->own_stream);
        if (st != VPT_OK) return st;
        VPT_HIP(hipEventRecord(ps.ev_k, b->own_stream));
        VPT_HIP(hipStreamWaitEvent(b->s_out, ps.ev_k, 0));
        if (scores_out && nb) VPT_HIP(hipMemcpyAsync(scores_out + o0, ps.scores, 4 * size_t(nb), hipMemcpyDeviceToHost, b->s_out));
        if (labels_out && nb) VPT_HIP(hipMemcpyAsync(labels_out + o0, ps.labels, size_t(nb), hipMemcpyDeviceToHost, b->s_out));
        VPT_HIP(hipEventRecord(ps.ev_out, b->s_out));
    }
    VPT_HIP(hipStreamSynchronize(b->s_in));
    VPT_HIP(hipStreamSynchronize(b->s_out));
    return vpt_batch_sync(b);   // the device's verdict over every chunk (the status word accumulates)
}

// vpt_predict_batch for a batch of a few chunks: every chunk's copy in, kernels and copy out are enqueued IN ORDER on one stream,
// and the chunks alternate over `n_lanes` streams (each with a workspace and one set of device buffers of its own).  The
// overlap is between the lanes -- one copies out while the next copies in and scores -- and nothing crosses streams: no events,
// no host synchronisation before the end (a set's reuse is ordered by its own stream), and the copies out go through SDMA.
vpt_status predict_lanes(const vpt_predictor* p, vpt_batch* b, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                         int32_t* scores_out, uint8_t* labels_out, const uint64_t* out_offsets, uint64_t chunk_chars, int n_lanes) {
    Lanes lanes;
    vpt_status st;
    if ((st = lanes.init(p, b, n_lanes)) != VPT_OK) return st;
    vptcut::PredictCutter cutter{};
    if ((st = predict_cutter(b, byte_offsets, out_offsets, n_sentences, chunk_chars, &cutter)) != VPT_OK) return st;
    for (size_t k = 0; !cutter.done(); ++k) {
        vpt_batch* bb = lanes[k];
        vpt_batch::PipeSet& ps = bb->pipe[0];
        hipStream_t s = bb->own_stream;
        const vptcut::PredictChunk c = cutter.next();
        if (c.error != vptcut::CutError::kNone) return cut_fail(c.error);
        const size_t n = c.n;
        const uint64_t t0 = byte_offsets[c.a], o0 = out_offsets[c.a], nbytes = c.off[n], nb = c.off[2 * n + 1];
        // a buffer that has to grow may still be read or written by the lane's earlier chunk
        if (size_t(nbytes) + 32 > ps.text.cap || 2 * (n + 1) > ps.off.cap || (scores_out && size_t(nb) + 1 > ps.scores.cap) ||
            (labels_out && size_t(nb) + 1 > ps.labels.cap))
            VPT_HIP(hipStreamSynchronize(s));
        if ((st = ps.text.grow(size_t(nbytes) + 32)) != VPT_OK) return st;
        if ((st = ps.off.grow(2 * (n + 1))) != VPT_OK) return st;
        if (scores_out && (st = ps.scores.grow(size_t(nb) + 1)) != VPT_OK) return st;
        if (labels_out && (st = ps.labels.grow(size_t(nb) + 1)) != VPT_OK) return st;
        VPT_HIP(hipMemcpyAsync(ps.text, utf8 + t0, size_t(nbytes), hipMemcpyHostToDevice, s));
        VPT_HIP(hipMemcpyAsync(ps.off, c.off, 16 * (n + 1), hipMemcpyHostToDevice, s));
        bb->max_chars = c.max_chars;
        st = vpt_predict_batch_device(p, bb, ps.text, ps.off, ps.off + (n + 1), n, nb, c.max_bytes, scores_out ? ps.scores.p : nullptr,
                                      labels_out ? ps.labels.p : nullptr, s);
        if (st != VPT_OK) return st;
        if (scores_out && nb) VPT_HIP(hipMemcpyAsync(scores_out + o0, ps.scores, 4 * size_t(nb), hipMemcpyDeviceToHost, s));
        if (labels_out && nb) VPT_HIP(hipMemcpyAsync(labels_out + o0, ps.labels, size_t(nb), hipMemcpyDeviceToHost, s));
    }
    return lanes.verdict();
}

}  // namespace

vpt_status vpt_predict_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                             int32_t* scores_out, uint8_t* labels_out, const uint64_t* out_offsets) {
    return vpt_predict_batch_flags(p, utf8, byte_offsets, n_sentences, scores_out, labels_out, out_offsets, 0u);
}

vpt_status vpt_predict_batch_flags(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                   int32_t* scores_out, uint8_t* labels_out, const uint64_t* out_offsets, unsigned flags) {
    if (flags & ~unsigned(VPT_FLAG_ALL | VPT_FLAG_LINEBREAKS_FIRST | VPT_FLAG_CONCAT_GRAPHEMES)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (n_sentences == 0) return VPT_OK;
    if (!utf8 || !byte_offsets || !out_offsets) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    vpt_batch* b = w.b;
    b->flags = flags;
    if (byte_offsets[n_sentences] >= byte_offsets[0] && out_offsets[n_sentences] >= out_offsets[0]) {   // a batch of several chunks goes through a copy/compute pipeline
        const PipePlan plan = pipeline_plan(p->knobs, out_offsets[n_sentences] - out_offsets[0] + n_sentences);
        if (plan.pipelined && plan.lanes > 0) return predict_lanes(p, b, utf8, byte_offsets, n_sentences, scores_out, labels_out, out_offsets, plan.chunk, plan.lanes);
        if (plan.pipelined) return predict_pipelined(p, b, utf8, byte_offsets, n_sentences, scores_out, labels_out, out_offsets, plan.chunk);
    }
    uint64_t total_b = 0, max_bytes = 0, max_chars = 0;
    if ((st = stage(b, utf8, byte_offsets, out_offsets, n_sentences, nullptr, &total_b, &max_bytes, &max_chars)) != VPT_OK) return st;
    b->max_chars = max_chars;
    hipStream_t s = b->own_stream;
    st = vpt_predict_batch_device(p, b, b->d_text, b->d_boff, b->d_ooff, n_sentences, total_b, max_bytes,
                                  scores_out ? b->d_scores.p : nullptr, labels_out ? b->d_labels.p : nullptr, s);
    if (st != VPT_OK) return st;
    if (scores_out && total_b) VPT_HIP(hipMemcpyAsync(scores_out + out_offsets[0], b->d_scores, 4 * total_b, hipMemcpyDeviceToHost, s));
    if (labels_out && total_b) VPT_HIP(hipMemcpyAsync(labels_out + out_offsets[0], b->d_labels, total_b, hipMemcpyDeviceToHost, s));
    return vpt_batch_sync(b);
}

vpt_status vpt_fill_tags_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                               const uint64_t* out_offsets, const uint8_t* labels, int32_t* tags_out) {
    return vpt_fill_tags_batch_flags(p, utf8, byte_offsets, n_sentences, out_offsets, labels, tags_out, 0u);
}

vpt_status vpt_fill_tags_batch_flags(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                     const uint64_t* out_offsets, const uint8_t* labels, int32_t* tags_out, unsigned flags) {
    return vpt_fill_tags_scores_batch(p, utf8, byte_offsets, n_sentences, out_offsets, labels, flags, tags_out, nullptr, nullptr);
}

// (t: the PatternMatchTagger whose rules fill the slots left None, or nullptr)
static vpt_status fill_tags_host(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                 const uint64_t* out_offsets, const uint8_t* labels, unsigned flags, int32_t* tags_out,
                                 int32_t* tag_scores_out, int32_t* tag_models_out, const vpt_pattern_tagger* t) {
    if (flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    if (t && t->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: tagger: does not belong to this predictor");
    if (n_sentences == 0 || p->n_tags == 0) return VPT_OK;   // predictor.rs:553-555
    if (!utf8 || !byte_offsets || !out_offsets || !tags_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (out_offsets[n_sentences] != out_offsets[0] && !labels) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: labels: must not be NULL");
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    vpt_batch* b = w.b;
    uint64_t total_b = 0;
    if ((st = stage(b, utf8, byte_offsets, out_offsets, n_sentences, labels, &total_b, nullptr, nullptr)) != VPT_OK) return st;
    const size_t n_rows = size_t(total_b + n_sentences), n_tag_words = n_rows * p->n_tags, n_score_words = n_rows * p->max_tag_scores;
    if ((st = b->d_tags.grow(n_tag_words + 16)) != VPT_OK) return st;
    if (tag_scores_out && (st = b->d_tag_scores.grow(n_score_words + 16)) != VPT_OK) return st;
    if (tag_models_out && (st = b->d_tag_models.grow(n_rows + 16)) != VPT_OK) return st;
    // rows that end no token with a tag model are not written by the kernel: they read 0 (the reference holds None there)
    if (tag_scores_out && n_score_words) VPT_HIP(hipMemsetAsync(b->d_tag_scores, 0, n_score_words * sizeof(int32_t), b->own_stream));
    b->flags = flags;
    b->tagger = t;
    st = vpt_fill_tags_scores_batch_device(p, b, b->d_text, b->d_boff, b->d_ooff, n_sentences, total_b, b->d_labels, b->d_tags,
                                           tag_scores_out ? b->d_tag_scores.p : nullptr, tag_models_out ? b->d_tag_models.p : nullptr, b->own_stream);
    if (st != VPT_OK) return st;
    if ((st = vpt_batch_sync(b)) != VPT_OK) return st;
    const size_t row0 = size_t(out_offsets[0]);   // (the caller's rows start at out_offsets[0] + 0)
    VPT_HIP(hipMemcpy(tags_out + row0 * p->n_tags, b->d_tags, n_tag_words * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (tag_scores_out && n_score_words) VPT_HIP(hipMemcpy(tag_scores_out + row0 * p->max_tag_scores, b->d_tag_scores, n_score_words * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (tag_models_out) VPT_HIP(hipMemcpy(tag_models_out + row0, b->d_tag_models, n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VPT_OK;
}

vpt_status vpt_fill_tags_scores_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                      const uint64_t* out_offsets, const uint8_t* labels, unsigned flags, int32_t* tags_out,
                                      int32_t* tag_scores_out, int32_t* tag_models_out) {
    return fill_tags_host(p, utf8, byte_offsets, n_sentences, out_offsets, labels, flags, tags_out, tag_scores_out, tag_models_out, nullptr);
}

vpt_status vpt_fill_tags_batch_rules(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                     const uint64_t* out_offsets, const uint8_t* labels, int32_t* tags_out, unsigned flags,
                                     const void* tagger) {
    return fill_tags_host(p, utf8, byte_offsets, n_sentences, out_offsets, labels, flags, tags_out, nullptr, nullptr, static_cast<const vpt_pattern_tagger*>(tagger));
}

static vpt_status emit_host(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                            const uint64_t* out_offsets, const uint8_t* labels, bool tagged, unsigned flags, uint8_t* text_out,
                            uint64_t text_capacity, uint64_t* text_offsets_out, const vpt_pattern_tagger* t = nullptr) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!text_offsets_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (tagged && !p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    if (t && t->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: tagger: does not belong to this predictor");
    text_offsets_out[0] = 0;
    if (n_sentences == 0) return VPT_OK;
    if (!utf8 || !byte_offsets || !out_offsets || (text_capacity && !text_out)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (out_offsets[n_sentences] != out_offsets[0] && !labels) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: labels: must not be NULL");
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    vpt_batch* b = w.b;
    uint64_t total_b = 0;
    if ((st = stage(b, utf8, byte_offsets, out_offsets, n_sentences, labels, &total_b, nullptr, nullptr)) != VPT_OK) return st;
    if ((st = b->d_tok.grow(size_t(text_capacity) + 16)) != VPT_OK) return st;
    if ((st = b->d_toff.grow(n_sentences + 1)) != VPT_OK) return st;
    const bool with_tags = tagged && p->n_tags > 0;
    if (with_tags) {   // Sentence::fill_tags, then the writer, as the CLI does (predict/src/main.rs:156-176); no dense array: the records are the tags
        b->flags = flags;
        b->tagger = t;
        st = vpt_fill_tags_batch_device(p, b, b->d_text, b->d_boff, b->d_ooff, n_sentences, total_b, b->d_labels, nullptr, b->own_stream);
        if (st != VPT_OK) return st;
    }
    st = emit_device(p, b, b->d_text, b->d_boff, b->d_ooff, n_sentences, total_b, b->d_labels, with_tags, b->d_tok,
                     text_capacity, b->d_toff, b->own_stream);
    if (st != VPT_OK) return st;
    if ((st = vpt_batch_sync(b)) != VPT_OK) return st;
    return download_sized<uint8_t>(text_offsets_out, b->d_toff, n_sentences, text_out, b->d_tok, text_capacity, kTextTooSmall);
}

vpt_status vpt_write_tokenized_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                     const uint64_t* out_offsets, const uint8_t* labels, uint8_t* text_out, uint64_t text_capacity,
                                     uint64_t* text_offsets_out) {
    return emit_host(p, utf8, byte_offsets, n_sentences, out_offsets, labels, false, 0u, text_out, text_capacity, text_offsets_out);
}

vpt_status vpt_write_tagged_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                  const uint64_t* out_offsets, const uint8_t* labels, unsigned flags, uint8_t* text_out,
                                  uint64_t text_capacity, uint64_t* text_offsets_out) {
    return emit_host(p, utf8, byte_offsets, n_sentences, out_offsets, labels, true, flags, text_out, text_capacity, text_offsets_out);
}

vpt_status vpt_write_tagged_batch_rules(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                        const uint64_t* out_offsets, const uint8_t* labels, unsigned flags, uint8_t* text_out,
                                        uint64_t text_capacity, uint64_t* text_offsets_out, const void* tagger) {
    return emit_host(p, utf8, byte_offsets, n_sentences, out_offsets, labels, true, flags, text_out, text_capacity, text_offsets_out, static_cast<const vpt_pattern_tagger*>(tagger));
}

namespace {
// vpt_tokenize_batch without tags, in chunks: a chunk of lines is a copy in (text, offsets), the char count, the tile search, the scoring
// launch (labels into the workspace) and the writer's launch.  Every chunk's text follows the one before it -- the writers hand the output
// position on through a chain of device words (EmitFuse::chain_in / chain_out) -- so the batch's output is one piece however it is cut.
// Four stages overlap:
//   copy in of chunk k + 2            its own stream
//   char count + tile search of k + 1 the PREPARING stream, with the scratch of one of two workspaces (k + 1 & 1)
//   scoring + writer of chunk k       the SCORING stream: the launches follow each other with an event wait that has long fired in between
//                                     (profiles/r04_e_tokenize_timeline.txt: 33 us of small launches in front of every scoring launch before)
//   copy out of chunk k - 1           issued by the host as soon as the chunk's event has fired; a pinned word says where its text ends
// and the host is a fifth: a chunk is some fifteen runtime calls, and with everything enqueued before the first wait the copies out only
// started when the LAST chunk was enqueued (r04_i_tokenize_timeline.txt).  So the loop cuts and rebases a chunk's offsets when its copy in
// is due, keeps the copies in two chunks ahead of the kernels, and after every chunk looks whether an earlier one can leave.
// Round 6: rounds 4 - 5 scored a chunk with the writer FUSED into the scoring kernel (one launch, 88 us of device time per 3.2 MB chunk); with
// the flat writer (round 5) the two launches take 28 + 12 us and the whole call 0.83 ms per 100 K lines against 0.88, 5.75 against 5.83 per
// million (profiles/r06_k_tokenize.jsonl) -- the fused phase, a second instance of every scoring kernel, is gone.
// Measured and dropped earlier (profiles/r04_{e,g,k,m,n}_tokenize*): a small first and last chunk (0.96 ms against 0.88); two independent lanes,
// each chunk's text placed by an upper bound and closed up by the copies out (1.07); kernels storing STRAIGHT into a pinned caller buffer
// (their stores cross PCIe at 27 .. 34 GB/s against the copy engine's 56: 1.15 - 1.29); every kernel of every chunk on one stream (0.97).
// `text` = the batch's first byte; byte_offsets are the caller's (relative to byte_offsets[0]).
// ends_out (vpt_token_stream_batch): the same pipeline with the span kernel in the writer's place -- the chunks write ONE array of token end-points
// (four bytes each; text_capacity counts them) and the documents' ranges in it instead of text and text offsets.
vpt_status tokenize_chunked(const vpt_predictor* p, vpt_batch* b, const uint8_t* text, const uint64_t* byte_offsets, size_t n_sentences, unsigned flags,
                          uint8_t* text_out, uint64_t text_capacity, uint64_t* text_offsets_out, uint32_t* ends_out = nullptr) {
    const size_t nbytes = size_t(byte_offsets[n_sentences] - byte_offsets[0]);
    // 1/6 of the batch, at least 2 MB (a scoring launch costs 50 us + 1.3 us per 1000 lines) and at most 8 (1 M lines: 5.8 ms in 8 MB chunks, 6.4 in 32)
    const uint64_t chunk_bytes = p->knobs.tokenize_chunk_bytes_set ? std::max<uint64_t>(p->knobs.tokenize_chunk_bytes, 1)
                                                                   : std::min<uint64_t>(uint64_t(8) << 20, std::max<uint64_t>(uint64_t(2) << 20, (uint64_t(nbytes) + 5) / 6));
    const size_t max_chunks = vptcut::stream_max_chunks(n_sentences, nbytes, chunk_bytes);
    vpt_status st;
    Workspace second;   // the scratch (tiles, partial sums, the writer's words, labels, status) of every other chunk
    if ((st = acquire(p, &second)) != VPT_OK) return st;
    // Kernels enqueued on THIS workspace's streams look back over the second one's scratch (its writer words, its status): on any return --
    // an error one in the middle of the chunks included -- those streams are drained BEFORE `second` goes back to the pool (a guard declared
    // behind it is destroyed in front of it), or another host thread could take and clear what a chunk in flight still reads
    struct DrainFirst {
        vpt_batch* b;
        ~DrainFirst() { drain(b); }
    } drain_first{b};
    vpt_batch* const ws[2] = {b, second.b};
    if (!b->s_tok_in) VPT_HIP(hipStreamCreateWithFlags(&b->s_tok_in, hipStreamNonBlocking));
    if (!b->s_tok_out) VPT_HIP(hipStreamCreateWithFlags(&b->s_tok_out, hipStreamNonBlocking));
    if ((st = chunk_events(b, 3 * max_chunks)) != VPT_OK) return st;   // per chunk: copied in, tiles found, scored
    if ((st = b->d_text.grow(nbytes + 32)) != VPT_OK) return st;
    if ((st = grow_pair(b->d_boff, b->d_ooff, vptcut::offset_slots(n_sentences, max_chunks))) != VPT_OK) return st;
    if ((st = b->d_chain.grow(max_chunks + 2)) != VPT_OK) return st;
    const uint64_t out_cap = ends_out ? uint64_t(nbytes) : uint64_t(nbytes) * 3 + 16;   // (an end-point per char at most, a char per byte at most)
    if (ends_out) { if ((st = b->d_tends.grow(size_t(out_cap) + 16)) != VPT_OK) return st; }
    else if ((st = b->d_tok.grow(size_t(out_cap) + 16)) != VPT_OK) return st;
    if ((st = b->d_toff.grow(n_sentences + 2)) != VPT_OK) return st;
    uint8_t* const d_out = b->d_tok;
    uint64_t* const d_off_out = b->d_toff;
    if ((st = pinned_words(b, vptcut::stream_pinned_words(n_sentences, max_chunks))) != VPT_OK) return st;
    uint64_t* const h_boff = b->h_off;
    uint64_t* const h_end = b->h_off + n_sentences + 1;
    uint64_t* const h_ctrl = h_end + max_chunks + 1;
    hipStream_t s = b->own_stream, s_in = b->s_tok_in, s_out = b->s_tok_out;
    hipStream_t s_prep = second.b->own_stream;
    for (vpt_batch* w : ws) {
        w->flags = flags;
        w->max_chars = 0;   // unknown on the host (no round trip for it): the scoring kernel takes the geometry that fits any sentence
    }
    VPT_HIP(hipMemsetAsync(b->d_chain, 0, sizeof(uint64_t), s));
    using Chunk = vptcut::TokenizeChunk;
    std::vector<Chunk> chunks;
    chunks.reserve(max_chunks);
    vptcut::StreamCutter cutter(byte_offsets, n_sentences, chunk_bytes, h_boff);
    auto copy_in_next = [&]() -> vpt_status {   // the next chunk of lines: offsets rebased into pinned memory, text and offsets on their way
        if (cutter.done()) return VPT_OK;
        const size_t k = chunks.size();
        const Chunk c = cutter.next();
        VPT_HIP(hipMemcpyAsync(b->d_text + c.tb, text + c.tb, size_t(c.nby), hipMemcpyHostToDevice, s_in));
        VPT_HIP(hipMemcpyAsync(b->d_boff + c.a + k, h_boff + c.a, 8 * (c.n + 1), hipMemcpyHostToDevice, s_in));   // n + 1 entries per chunk; offsets into the WHOLE text: no rebasing
        VPT_HIP(hipEventRecord(b->chunk_ev[3 * k], s_in));
        chunks.push_back(c);
        return VPT_OK;
    };
    uint64_t at = 0;
    size_t next_out = 0;
    bool out_of_range = false, too_small = false;
    auto copy_out = [&](size_t k) -> vpt_status {   // chunk k has been scored: its text and offsets leave
        const uint64_t end = h_end[k];
        if (end > out_cap || end < at) { out_of_range = true; return VPT_OK; }   // the device found the inputs inconsistent and says so below
        if (end > text_capacity) { too_small = true; return VPT_OK; }
        if (end > at && ends_out) VPT_HIP(hipMemcpyAsync(ends_out + at, b->d_tends + at, 4 * size_t(end - at), hipMemcpyDeviceToHost, s_out));
        else if (end > at) VPT_HIP(hipMemcpyAsync(text_out + at, d_out + at, size_t(end - at), hipMemcpyDeviceToHost, s_out));
        VPT_HIP(hipMemcpyAsync(text_offsets_out + chunks[k].a, d_off_out + chunks[k].a, 8 * (chunks[k].n + 1), hipMemcpyDeviceToHost, s_out));
        at = end;
        return VPT_OK;
    };
    if ((st = copy_in_next()) != VPT_OK || (st = copy_in_next()) != VPT_OK) return st;
    for (size_t k = 0; k < chunks.size(); ++k) {
        const Chunk c = chunks[k];
        vpt_batch* const w = ws[k & 1];
        uint64_t* d_boff_k = b->d_boff + c.a + k;
        uint64_t* d_ooff_k = b->d_ooff + c.a + k;   // n + 1 entries per chunk, chunk-relative
        VPT_HIP(hipStreamWaitEvent(s_prep, b->chunk_ev[3 * k], 0));
        if (k >= 2) VPT_HIP(hipStreamWaitEvent(s_prep, b->chunk_ev[3 * (k - 2) + 2], 0));   // this workspace's scratch: the chunk before the last is through with it
        if ((st = count_boundaries_impl(p, w, b->d_text, d_boff_k, c.n, d_ooff_k, s_prep, c.nby)) != VPT_OK) return st;
        h_end[k] = ~uint64_t(0);
        if ((st = w->d_tlab.grow(size_t(c.nby) + 16)) != VPT_OK) return st;
        w->split_stream = s; w->split_event = b->chunk_ev[3 * k + 1];   // the scoring launch: on the scoring stream, behind the tile search
        st = predict_device_impl(p, w, b->d_text, d_boff_k, d_ooff_k, c.n, c.nby - c.n /* boundaries of the chunk, at most */, c.mb, nullptr, w->d_tlab, s_prep);
        w->split_stream = nullptr; w->split_event = nullptr;
        if (st != VPT_OK) return st;
        if (ends_out) st = spans_device(p, w, b->d_text, d_boff_k, d_ooff_k, c.n, c.nby - c.n, w->d_tlab, d_off_out + c.a, b->d_tends, out_cap, s, h_end + k, b->d_chain + k, b->d_chain + k + 1);
        else st = emit_device(p, w, b->d_text, d_boff_k, d_ooff_k, c.n, c.nby - c.n, w->d_tlab, false, d_out, out_cap, d_off_out + c.a, s, h_end + k, b->d_chain + k, b->d_chain + k + 1);
        if (st != VPT_OK) return st;
        VPT_HIP(hipEventRecord(b->chunk_ev[3 * k + 2], s));
        if ((st = copy_in_next()) != VPT_OK) return st;
        while (!out_of_range && !too_small && next_out < k && hipEventQuery(b->chunk_ev[3 * next_out + 2]) == hipSuccess)
            if ((st = copy_out(next_out++)) != VPT_OK) return st;
    }
    // ---- collect what is still on the device
    for (; next_out < chunks.size() && !out_of_range && !too_small; ++next_out) {
        VPT_HIP(hipEventSynchronize(b->chunk_ev[3 * next_out + 2]));
        if ((st = copy_out(next_out)) != VPT_OK) return st;
    }
    // ---- the device's verdict over every chunk (into pinned words: a copy to the stack is staged and waited for, 25 us each)
    h_ctrl[0] = h_ctrl[1] = 0;
    VPT_HIP(hipStreamSynchronize(s_prep));
    VPT_HIP(hipMemcpyAsync(h_ctrl, b->d_ctrl, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VPT_HIP(hipMemcpyAsync(h_ctrl + 1, second.b->d_ctrl, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VPT_HIP(hipStreamSynchronize(s));
    VPT_HIP(hipStreamSynchronize(s_out));
    for (vpt_batch* w : ws) w->pending = false;
    const uint32_t bits = uint32_t(h_ctrl[0]) | uint32_t(h_ctrl[1]);
    if (bits) {
        for (vpt_batch* w : ws) VPT_HIP(hipMemset(w->d_ctrl, 0, sizeof(uint32_t)));
        return status_from_bits(bits);
    }
    if (too_small) return fail(VPT_INVALID_ARGUMENT, ends_out ? kTokensTooSmall : kTextTooSmall);
    if (out_of_range || h_end[chunks.size() - 1] > out_cap) return fail(VPT_RUNTIME_ERROR, "vpt_tokenize_batch: the output size is out of range");
    return VPT_OK;
}
}  // namespace

// Lines in, tokenized lines out: Sentence::from_raw -> [KyteaFullwidthFilter] -> Predictor::predict -> [post-filters]
// -> [fill_tags] -> write_tokenized_text for a whole batch (the loop of predict/src/main.rs:122-176), with only the
// text crossing PCIe: char counting, scoring, tagging and the writer all run on the device.
static vpt_status tokenize_host(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, unsigned flags,
                                int tagged, uint8_t* text_out, uint64_t text_capacity, uint64_t* text_offsets_out, const vpt_pattern_tagger* t) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!text_offsets_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (flags & ~unsigned(VPT_FLAG_ALL | VPT_FLAG_CONCAT_GRAPHEMES)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (tagged && !p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    if (t && t->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: tagger: does not belong to this predictor");
    text_offsets_out[0] = 0;
    if (n_sentences == 0) return VPT_OK;
    if (!utf8 || !byte_offsets || (text_capacity && !text_out)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    const uint64_t t0 = byte_offsets[0], t1 = byte_offsets[n_sentences];
    if (t1 < t0) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: byte_offsets: must be non-decreasing");
    for (size_t i = 0; i < n_sentences; ++i)
        if (byte_offsets[i + 1] <= byte_offsets[i]) return cut_fail(vptcut::CutError::kEmptySentence);
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    vpt_batch* b = w.b;
    const size_t nbytes = size_t(t1 - t0);
    const bool with_tags = tagged && p->n_tags > 0;
    if (!with_tags) return tokenize_chunked(p, b, utf8 + t0, byte_offsets, n_sentences, flags, text_out, text_capacity, text_offsets_out);
    // NOTHING on the way needs a number from the device: the device buffers hold the whole batch and a slice of an output starts
    // where an upper bound puts it (a char is at least one byte: boundaries and chars in front of a slice <= text bytes in front
    // of it; tokenized text <= 3 bytes per text byte + the longest tag suffix per char), so copy in, char count, scoring, tagging
    // and writer are enqueued back to back; the host then waits for the event behind them, reads the size of the text from pinned
    // memory (the prefix sum's last kernel wrote it there) and copies text and offsets to where they belong.  The code can cut the
    // batch into chunks that alternate over a few lanes (streams with a workspace each, as in predict_lanes) and collect them in
    // order -- but a chunk is fifteen runtime calls, and measured on MI355X (profiles/r02_j_tokenize.txt) that enqueueing costs
    // more than the overlap returns: 100 K sentences 1.55 ms as one chunk, 1.73 .. 2.4 in 7 .. 25; a million 11.0 ms as one, 10.6 ..
    // 22.7 in 4 .. 125.  So a chunk is 256 MB of text -- one, unless the batch is larger than that (VPT_TOKENIZE_CHUNK_BYTES
    // overrides; the tests use it).
    constexpr int kMaxLanes = 4;
    const uint64_t chunk_bytes = p->knobs.tokenize_chunk_bytes;
    const uint64_t per_byte = 3 + (with_tags ? uint64_t(p->max_tag_suffix) + (t ? t->max_suffix : 0u) : 0);   // tokenized bytes per text byte, at most
    const size_t max_chunks = vptcut::tagged_max_chunks(n_sentences, nbytes, chunk_bytes);
    Lanes lanes;
    if ((st = lanes.init(p, b, int(std::min<size_t>(kMaxLanes, max_chunks)))) != VPT_OK) return st;
    if (!b->s_out) VPT_HIP(hipStreamCreateWithFlags(&b->s_out, hipStreamNonBlocking));
    if ((st = chunk_events(b, max_chunks)) != VPT_OK) return st;
    // whole-batch device buffers (lane 0's workspace owns them); the other lanes only lend their scratch
    if ((st = b->d_text.grow(nbytes + 32)) != VPT_OK) return st;
    if ((st = grow_pair(b->d_boff, b->d_ooff, vptcut::offset_slots(n_sentences, max_chunks))) != VPT_OK) return st;
    if ((st = b->d_tlab.grow(nbytes + 1)) != VPT_OK) return st;
    if ((st = b->d_tok.grow(size_t(nbytes * per_byte) + 16)) != VPT_OK) return st;
    if ((st = b->d_toff.grow(vptcut::offset_slots(n_sentences, max_chunks))) != VPT_OK) return st;
    if ((st = pinned_words(b, vptcut::tagged_pinned_words(n_sentences, max_chunks))) != VPT_OK) return st;
    uint64_t* const h_boff = b->h_off;
    uint64_t* const h_total = b->h_off + n_sentences + 1;
    for (size_t i = 0; i <= n_sentences; ++i) h_boff[i] = byte_offsets[i] - t0;
    using Chunk = vptcut::TokenizeChunk;
    std::vector<Chunk> chunks;
    for (size_t i = 0; i < n_sentences;) {
        const Chunk c = vptcut::tagged_chunk(h_boff, n_sentences, i, chunk_bytes);
        i += c.n;
        const size_t a = c.a, n = c.n, k = chunks.size();
        const uint64_t tb = c.tb, nby = c.nby, mb = c.mb;
        vpt_batch* bb = lanes[k];
        hipStream_t s = bb->own_stream;
        bb->flags = flags;
        bb->max_chars = 0;   // unknown on the host (no round trip for it): the scoring kernel takes the geometry that fits any sentence
        uint64_t* d_boff_k = b->d_boff + a + k;                   // n + 1 entries per chunk; offsets into the WHOLE text: no rebasing
        uint64_t* d_ooff_k = b->d_ooff + a + k;                   // n + 1 entries per chunk, chunk-relative
        uint8_t* d_labels_k = b->d_tlab + tb;
        VPT_HIP(hipMemcpyAsync(b->d_text + tb, utf8 + t0 + tb, size_t(nby), hipMemcpyHostToDevice, s));
        VPT_HIP(hipMemcpyAsync(d_boff_k, h_boff + a, 8 * (n + 1), hipMemcpyHostToDevice, s));
        if ((st = count_boundaries_impl(p, bb, b->d_text, d_boff_k, n, d_ooff_k, s, nby)) != VPT_OK) return st;
        const uint64_t tb_bound = nby - n;                        // boundaries of the chunk, at most
        st = vpt_predict_batch_device(p, bb, b->d_text, d_boff_k, d_ooff_k, n, tb_bound, mb, nullptr, d_labels_k, s);
        if (st != VPT_OK) return st;
        if (with_tags) {   // (no dense array: the writer takes the records)
            bb->flags = flags & VPT_FLAG_KYTEA_FULLWIDTH;
            bb->tagger = t;
            st = vpt_fill_tags_batch_device(p, bb, b->d_text, d_boff_k, d_ooff_k, n, tb_bound, d_labels_k, nullptr, s);
            if (st != VPT_OK) return st;
        }
        h_total[k] = 0;
        st = emit_device(p, bb, b->d_text, d_boff_k, d_ooff_k, n, tb_bound, d_labels_k, with_tags, b->d_tok + tb * per_byte, nby * per_byte,
                         b->d_toff + a + k, s, h_total + k);
        if (st != VPT_OK) return st;
        VPT_HIP(hipEventRecord(b->chunk_ev[k], s));
        chunks.push_back(c);
    }
    // ---- collect: chunk by chunk, in order
    uint64_t at = 0;   // tokenized bytes in front of the chunk
    std::vector<uint64_t> base(chunks.size());
    bool incomplete = false;
    st = VPT_OK;
    for (size_t k = 0; k < chunks.size() && st == VPT_OK; ++k) {
        const Chunk& c = chunks[k];
        VPT_HIP(hipEventSynchronize(b->chunk_ev[k]));
        const uint64_t total = h_total[k];
        if (total > (h_boff[c.a + c.n] - c.tb) * per_byte) { incomplete = true; break; }   // the device found the inputs inconsistent and says so below
        if (total > text_capacity || at > text_capacity - total) { st = fail(VPT_INVALID_ARGUMENT, kTextTooSmall); break; }
        base[k] = at;
        if (total) VPT_HIP(hipMemcpyAsync(text_out + at, b->d_tok + c.tb * per_byte, size_t(total), hipMemcpyDeviceToHost, b->s_out));
        VPT_HIP(hipMemcpyAsync(text_offsets_out + c.a + 1, b->d_toff + c.a + k + 1, 8 * c.n, hipMemcpyDeviceToHost, b->s_out));
        at += total;
    }
    VPT_HIP(hipStreamSynchronize(b->s_out));
    st = lanes.verdict(st);
    if (st != VPT_OK) return st;
    if (incomplete) return fail(VPT_RUNTIME_ERROR, "vpt_tokenize_batch: a chunk's output size is out of range");
    // the offsets came back relative to their chunk's text
    text_offsets_out[0] = 0;
    for (size_t k = 1; k < chunks.size(); ++k)
        for (size_t j = 1; j <= chunks[k].n; ++j) text_offsets_out[chunks[k].a + j] += base[k];
    return VPT_OK;
}

vpt_status vpt_tokenize_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, unsigned flags,
                              int tagged, uint8_t* text_out, uint64_t text_capacity, uint64_t* text_offsets_out) {
    return tokenize_host(p, utf8, byte_offsets, n_sentences, flags, tagged, text_out, text_capacity, text_offsets_out, nullptr);
}

vpt_status vpt_tokenize_batch_rules(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, unsigned flags,
                                    int tagged, uint8_t* text_out, uint64_t text_capacity, uint64_t* text_offsets_out,
                                    const void* tagger) {
    return tokenize_host(p, utf8, byte_offsets, n_sentences, flags, tagged, text_out, text_capacity, text_offsets_out, static_cast<const vpt_pattern_tagger*>(tagger));
}

// predict/src/main.rs:122-176 with --scores / --tag-scores for a batch in host buffers: the bytes the CLI writes for these lines.  labels == NULL:
// Predictor::predict and the post-filters of `flags` run here; else the caller's scores and labels are taken (the three-call path of a host filter).
vpt_status vpt_predict_listing_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, unsigned flags,
                                     unsigned listing, const int32_t* scores, const uint8_t* labels, uint8_t* out, uint64_t capacity,
                                     uint64_t* listing_offsets_out) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (flags & ~unsigned(VPT_FLAG_ALL | VPT_FLAG_LINEBREAKS_FIRST | VPT_FLAG_CONCAT_GRAPHEMES)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (listing & ~unsigned(VPT_LISTING_ALL)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: listing: unknown bit");
    if ((listing & (VPT_LISTING_TAG_SCORES | VPT_LISTING_TAGGED)) && !p->predict_tags)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    if (!listing_offsets_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    listing_offsets_out[0] = 0;
    if (n_sentences == 0) return VPT_OK;
    if (!utf8 || !byte_offsets || (capacity && !out)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    std::vector<uint64_t> ooff(n_sentences + 1);
    vpt_status st = vpt_count_boundaries(utf8, byte_offsets, n_sentences, ooff.data());   // (empty sentences and NUL are rejected here)
    if (st != VPT_OK) return st;
    if (labels && (listing & VPT_LISTING_SCORES) && ooff[n_sentences] && !scores) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: scores: must not be NULL");
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    if ((st = acquire(p, &w)) != VPT_OK) return st;
    vpt_batch* b = w.b;
    uint64_t total_b = 0, max_bytes = 0, max_chars = 0;
    if ((st = stage(b, utf8, byte_offsets, ooff.data(), n_sentences, labels, &total_b, &max_bytes, &max_chars)) != VPT_OK) return st;
    hipStream_t s = b->own_stream;
    if (labels) {
        b->flags = flags & VPT_FLAG_KYTEA_FULLWIDTH;
        if (scores && total_b) VPT_HIP(hipMemcpyAsync(b->d_scores, scores, 4 * size_t(total_b), hipMemcpyHostToDevice, s));
    } else {
        b->flags = flags;
        b->max_chars = max_chars;
        if ((st = vpt_predict_batch_device(p, b, b->d_text, b->d_boff, b->d_ooff, n_sentences, total_b, max_bytes, b->d_scores, b->d_labels, s)) != VPT_OK) return st;
    }
    if ((st = b->d_lst_out.grow(size_t(capacity) + 16)) != VPT_OK) return st;
    if ((st = b->d_lst_off.grow(n_sentences + 1)) != VPT_OK) return st;
    st = vpt_predict_listing_batch_device(p, b, b->d_text, b->d_boff, b->d_ooff, n_sentences, total_b, byte_offsets[n_sentences] - byte_offsets[0], b->d_scores,
                                          b->d_labels, listing, b->d_lst_out, capacity, b->d_lst_off, s);
    if (st != VPT_OK) return st;
    if ((st = vpt_batch_sync(b)) != VPT_OK) return st;
    return download_sized<uint8_t>(listing_offsets_out, b->d_lst_off, n_sentences, out, b->d_lst_out, capacity, "InvalidArgumentError: text_capacity: smaller than the listing");
}

// vaporetto_tantivy/src/lib.rs:183-192 for a batch in host buffers, on the caller's labels
vpt_status vpt_token_spans_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_documents,
                                 const uint64_t* out_offsets, const uint8_t* labels, uint64_t* token_offsets_out, uint32_t* token_ends_out,
                                 uint64_t capacity) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!token_offsets_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    token_offsets_out[0] = 0;
    if (n_documents == 0) return VPT_OK;
    if (!utf8 || !byte_offsets || !out_offsets || (capacity && !token_ends_out)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (out_offsets[n_documents] != out_offsets[0] && !labels) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: labels: must not be NULL");
    for (size_t i = 0; i < n_documents; ++i)
        if (byte_offsets[i + 1] > byte_offsets[i] && byte_offsets[i + 1] - byte_offsets[i] > 0xFFFFFFFFull)
            return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: text: a document must be shorter than 2^32 bytes");
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    vpt_batch* b = w.b;
    uint64_t total_b = 0;
    if ((st = stage(b, utf8, byte_offsets, out_offsets, n_documents, labels, &total_b, nullptr, nullptr)) != VPT_OK) return st;
    // the device buffer holds every end-point there can be (one per char), so a capacity that is too small is found here and nothing is
    // copied past it
    const uint64_t d_cap = total_b + n_documents;
    if ((st = b->d_tends.grow(size_t(d_cap) + 16)) != VPT_OK) return st;
    if ((st = b->d_toff.grow(n_documents + 1)) != VPT_OK) return st;
    st = spans_device(p, b, b->d_text, b->d_boff, b->d_ooff, n_documents, total_b, b->d_labels, b->d_toff, b->d_tends, d_cap, b->own_stream, nullptr, nullptr, nullptr);
    if (st != VPT_OK) return st;
    if ((st = vpt_batch_sync(b)) != VPT_OK) return st;
    return download_sized<uint32_t>(token_offsets_out, b->d_toff, n_documents, token_ends_out, b->d_tends, capacity, kTokensTooSmall);
}

// ConcatGraphemeClustersFilter on the caller's labels, host buffers
vpt_status vpt_concat_graphemes_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                      const uint64_t* out_offsets, unsigned flags, uint8_t* labels) {
    if (flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (n_sentences == 0) return VPT_OK;
    if (!utf8 || !byte_offsets || !out_offsets) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (out_offsets[n_sentences] != out_offsets[0] && !labels) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: labels: must not be NULL");
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    vpt_batch* b = w.b;
    uint64_t total_b = 0;
    if ((st = stage(b, utf8, byte_offsets, out_offsets, n_sentences, labels, &total_b, nullptr, nullptr)) != VPT_OK) return st;
    b->flags = flags;
    if (total_b == 0) {   // no label to clear: the text's own checks (Sentence::from_raw's) all the same
        std::vector<uint64_t> ooff(n_sentences + 1);
        return vpt_count_boundaries(utf8, byte_offsets, n_sentences, ooff.data());
    }
    st = vpt_concat_graphemes_batch_device(p, b, b->d_text, b->d_boff, b->d_ooff, n_sentences, total_b, b->d_labels, b->own_stream);
    if (st != VPT_OK) return st;
    VPT_HIP(hipMemcpyAsync(labels + out_offsets[0], b->d_labels, size_t(total_b), hipMemcpyDeviceToHost, b->own_stream));
    return vpt_batch_sync(b);
}

// VaporettoTokenizer::token_stream (vaporetto_tantivy/src/lib.rs:160-192) for a batch of documents: only the text goes in, the spans come back.
vpt_status vpt_token_stream_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_documents,
                                  unsigned wsconst_flags, uint64_t* token_offsets_out, uint32_t* token_ends_out, uint64_t capacity) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!token_offsets_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (wsconst_flags & ~(0x7Eu | unsigned(VPT_FLAG_CONCAT_GRAPHEMES))) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: Could not parse a wsconst value");   // lib.rs:82
    token_offsets_out[0] = 0;
    if (n_documents == 0) return VPT_OK;
    if (!utf8 || !byte_offsets || (capacity && !token_ends_out)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    // an empty document has no tokens (lib.rs:161-169) and never reaches the device: the offsets of the others, which delimit the same text
    std::vector<uint64_t> docs;
    docs.reserve(n_documents + 1);
    docs.push_back(byte_offsets[0]);
    uint64_t max_bytes = 0;
    for (size_t i = 0; i < n_documents; ++i) {
        if (byte_offsets[i + 1] < byte_offsets[i]) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: byte_offsets: must be non-decreasing");
        if (byte_offsets[i + 1] == byte_offsets[i]) continue;
        max_bytes = std::max<uint64_t>(max_bytes, byte_offsets[i + 1] - byte_offsets[i]);
        docs.push_back(byte_offsets[i + 1]);
    }
    if (max_bytes > 0xFFFFFFFFull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: text: a document must be shorter than 2^32 bytes");
    const size_t n = docs.size() - 1;
    if (n == 0) { std::fill(token_offsets_out, token_offsets_out + n_documents + 1, uint64_t(0)); return VPT_OK; }
    if (capacity < n) return fail(VPT_INVALID_ARGUMENT, kTokensTooSmall);   // (a token per document at least)
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    const unsigned flags = VPT_FLAG_KYTEA_FULLWIDTH | VPT_FLAG_SPLIT_LINEBREAKS | VPT_FLAG_LINEBREAKS_FIRST | wsconst_flags;
    std::vector<uint64_t> packed;   // (only with empty documents: the ranges of the others)
    uint64_t* const offs = n == n_documents ? token_offsets_out : (packed.resize(n + 1), packed.data());
    offs[0] = 0;
    st = tokenize_chunked(p, w.b, utf8 + docs[0], docs.data(), n, flags, nullptr, capacity, offs, token_ends_out);
    if (st != VPT_OK) return st;
    if (n != n_documents) {
        size_t k = 0;
        for (size_t i = 0; i < n_documents; ++i) {
            token_offsets_out[i] = packed[k];
            if (byte_offsets[i + 1] != byte_offsets[i]) ++k;
        }
        token_offsets_out[n_documents] = packed[n];
    }
    return VPT_OK;
}

// vpt_token_stream_batch with every token's tags and, when asked, without the tokens of a stop set: per chunk of whole documents (the tagged
// pipeline's chunks and lanes, tokenize_host) copy in, char count, scoring with the adapter's filters, fill_tags (fullwidth flag only, the
// tagger on the lane's workspace), the tagged span instance, the filter pass (without a stop set it keeps every token and writes the trivial
// starts and positions) -- enqueued back to back, nothing on the way needs a number from the device.  A chunk's arrays start where an upper
// bound puts them (a token per byte at most); the host collects the chunks in order and rebases their offsets: the filter runs per chunk, and
// a chunk holds whole documents, so the arrays do not depend on the cut.
// `tagged` == false (vpt_token_stream_ids_batch without tagger, stop set and tags): no fill_tags, the untagged span instance, and the filter
// pass without tags -- vpt_token_stream_batch's steps with starts and positions.  `vocab` != NULL: the id pass (kernels_vocab.hip) runs last
// on every chunk's finished CSR, one launch more per chunk; with NULL the launches are what they were.
// `counter` != NULL (vpt_token_stream_count_batch): the count call (kernels_vocab_count.hip, three launches) runs last on every chunk's finished
// CSR instead, and nothing is copied out: the output pointers are NULL.  A counter takes one call at a time, so a chunk's count call waits for the
// chunk before it (on another lane's stream) to be through; everything in front of it overlaps as before.  With NULL nothing changes.
namespace {
vpt_status token_stream_chunks(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_documents, unsigned wsconst_flags,
                               bool tagged, const void* tagger, const void* stop, const vpt_vocab* vocab, unsigned vocab_flags,
                               vpt_vocab_counter* counter, uint64_t* token_offsets_out, uint32_t* token_starts_out, uint32_t* token_ends_out, uint32_t* token_positions_out,
                               int32_t* token_tags_out, int32_t* token_ids_out, uint64_t capacity) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!token_offsets_out && !counter) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (wsconst_flags & ~(0x7Eu | unsigned(VPT_FLAG_CONCAT_GRAPHEMES))) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: Could not parse a wsconst value");   // lib.rs:82
    if (tagged && !p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    const vpt_pattern_tagger* t = static_cast<const vpt_pattern_tagger*>(tagger);
    const vpt_tag_stop* sp = static_cast<const vpt_tag_stop*>(stop);
    if (t && t->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: tagger: does not belong to this predictor");
    if (sp && sp->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: stop: does not belong to this predictor");
    if (vocab && vocab->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: vocab: does not belong to this predictor");
    if (counter && counter->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: counter: does not belong to this predictor");
    if ((vocab || counter) && (vocab_flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH))) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (counter && counter->known_full) return fail(VPT_INVALID_ARGUMENT, kVocabCounterFull);
    if (token_offsets_out) token_offsets_out[0] = 0;
    if (n_documents == 0) return VPT_OK;
    const uint32_t nt = tagged ? p->n_tags : 0u;
    if (!utf8 || !byte_offsets ||
        (capacity && !counter && (!token_starts_out || !token_ends_out || !token_positions_out || (nt && !token_tags_out) || (vocab && !token_ids_out))))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    std::vector<uint64_t> docs;   // an empty document has no tokens and never reaches the device (vpt_token_stream_batch)
    docs.reserve(n_documents + 1);
    docs.push_back(byte_offsets[0]);
    uint64_t max_bytes = 0;
    for (size_t i = 0; i < n_documents; ++i) {
        if (byte_offsets[i + 1] < byte_offsets[i]) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: byte_offsets: must be non-decreasing");
        if (byte_offsets[i + 1] == byte_offsets[i]) continue;
        max_bytes = std::max<uint64_t>(max_bytes, byte_offsets[i + 1] - byte_offsets[i]);
        docs.push_back(byte_offsets[i + 1]);
    }
    if (max_bytes > 0xFFFFFFFFull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: text: a document must be shorter than 2^32 bytes");
    const size_t n = docs.size() - 1;
    if (n == 0) {
        if (token_offsets_out) std::fill(token_offsets_out, token_offsets_out + n_documents + 1, uint64_t(0));
        return VPT_OK;
    }
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    vpt_batch* b = w.b;
    const unsigned flags = VPT_FLAG_KYTEA_FULLWIDTH | VPT_FLAG_SPLIT_LINEBREAKS | VPT_FLAG_LINEBREAKS_FIRST | wsconst_flags;
    const uint64_t t0 = docs[0];
    const size_t nbytes = size_t(docs[n] - t0);
    constexpr int kMaxLanes = 4;
    const uint64_t chunk_bytes = p->knobs.tokenize_chunk_bytes;
    const size_t max_chunks = vptcut::tagged_max_chunks(n, nbytes, chunk_bytes);
    Lanes lanes;
    if ((st = lanes.init(p, b, int(std::min<size_t>(kMaxLanes, max_chunks)))) != VPT_OK) return st;
    if (!b->s_out) VPT_HIP(hipStreamCreateWithFlags(&b->s_out, hipStreamNonBlocking));
    if ((st = chunk_events(b, max_chunks)) != VPT_OK) return st;
    const size_t slots = vptcut::offset_slots(n, max_chunks), tag_words = size_t(nbytes) * std::max<uint32_t>(nt, 1) + 16;
    if ((st = b->d_text.grow(nbytes + 32)) != VPT_OK) return st;
    if ((st = grow_pair(b->d_boff, b->d_ooff, slots)) != VPT_OK) return st;
    if ((st = b->d_tlab.grow(nbytes + 1)) != VPT_OK) return st;
    if ((st = b->d_toff.grow(slots)) != VPT_OK || (st = b->d_ftoff.grow(slots)) != VPT_OK) return st;
    if ((st = b->d_tends.grow(nbytes + 16)) != VPT_OK || (tagged && (st = b->d_ttags.grow(tag_words)) != VPT_OK)) return st;
    if ((st = b->d_fstarts.grow(nbytes + 16)) != VPT_OK || (st = b->d_fends.grow(nbytes + 16)) != VPT_OK || (st = b->d_fpos.grow(nbytes + 16)) != VPT_OK ||
        (tagged && (st = b->d_ftags.grow(tag_words)) != VPT_OK))
        return st;
    if (vocab && (st = b->d_fids.grow(nbytes + 16)) != VPT_OK) return st;
    if ((st = pinned_words(b, vptcut::tagged_pinned_words(n, max_chunks))) != VPT_OK) return st;
    uint64_t* const h_boff = b->h_off;
    uint64_t* const h_total = b->h_off + n + 1;
    for (size_t i = 0; i <= n; ++i) h_boff[i] = docs[i] - t0;
    using Chunk = vptcut::TokenizeChunk;
    std::vector<Chunk> chunks;
    for (size_t i = 0; i < n;) {
        const Chunk c = vptcut::tagged_chunk(h_boff, n, i, chunk_bytes);
        i += c.n;
        const size_t a = c.a, cn = c.n, k = chunks.size();
        const uint64_t tb = c.tb, nby = c.nby;
        vpt_batch* bb = lanes[k];
        hipStream_t s = bb->own_stream;
        bb->flags = flags;
        bb->max_chars = 0;
        uint64_t* d_boff_k = b->d_boff + a + k;
        uint64_t* d_ooff_k = b->d_ooff + a + k;
        uint8_t* d_labels_k = b->d_tlab + tb;
        VPT_HIP(hipMemcpyAsync(b->d_text + tb, utf8 + t0 + tb, size_t(nby), hipMemcpyHostToDevice, s));
        VPT_HIP(hipMemcpyAsync(d_boff_k, h_boff + a, 8 * (cn + 1), hipMemcpyHostToDevice, s));
        if ((st = count_boundaries_impl(p, bb, b->d_text, d_boff_k, cn, d_ooff_k, s, nby)) != VPT_OK) return st;
        const uint64_t tb_bound = nby - cn;   // boundaries of the chunk, at most
        if ((st = vpt_predict_batch_device(p, bb, b->d_text, d_boff_k, d_ooff_k, cn, tb_bound, c.mb, nullptr, d_labels_k, s)) != VPT_OK) return st;
        if (nt) {
            bb->flags = flags & VPT_FLAG_KYTEA_FULLWIDTH;
            bb->tagger = t;
            if ((st = vpt_fill_tags_batch_device(p, bb, b->d_text, d_boff_k, d_ooff_k, cn, tb_bound, d_labels_k, nullptr, s)) != VPT_OK) return st;
        }
        int32_t* const d_ttags_k = nt ? b->d_ttags + tb * nt : nullptr;
        int32_t* const d_ftags_k = nt ? b->d_ftags + tb * nt : nullptr;
        if (tagged)
            st = token_tags_device(p, bb, b->d_text, d_boff_k, d_ooff_k, cn, tb_bound, d_labels_k, b->d_toff + a + k, b->d_tends + tb, d_ttags_k, nby, s, nullptr);
        else
            st = spans_device(p, bb, b->d_text, d_boff_k, d_ooff_k, cn, tb_bound, d_labels_k, b->d_toff + a + k, b->d_tends + tb, nby, s, nullptr, nullptr, nullptr);
        if (st != VPT_OK) return st;
        h_total[k] = 0;
        st = token_filter_device(p, bb, sp, b->d_toff + a + k, b->d_tends + tb, d_ttags_k, cn, nby, b->d_ftoff + a + k, b->d_fstarts + tb,
                                 b->d_fends + tb, b->d_fpos + tb, d_ftags_k, nby, s, h_total + k, tagged);
        if (st != VPT_OK) return st;
        if (vocab) {   // the ids of the chunk's finished CSR, in the caller's text or its KyteaFullwidthFilter image
            st = token_ids_device(p, bb, vocab, b->d_text, d_boff_k, cn, b->d_ftoff + a + k, b->d_fstarts + tb, b->d_fends + tb, nby, vocab_flags,
                                  b->d_fids + tb, s);
            if (st != VPT_OK) return st;
        }
        if (counter) {   // the chunk's tokens into the counter, behind the count call of the chunk before
            if (k) VPT_HIP(hipStreamWaitEvent(s, b->chunk_ev[k - 1], 0));
            st = vocab_count_device(p, bb, counter, b->d_text, d_boff_k, cn, b->d_ftoff + a + k, b->d_fstarts + tb, b->d_fends + tb, nby, vocab_flags, s);
            if (st != VPT_OK) return st;
        }
        VPT_HIP(hipEventRecord(b->chunk_ev[k], s));
        chunks.push_back(c);
    }
    // ---- collect: chunk by chunk, in order
    std::vector<uint64_t> packed(n + 1, 0), base(chunks.size());
    uint64_t at = 0;
    bool incomplete = false;
    st = VPT_OK;
    for (size_t k = 0; k < chunks.size() && st == VPT_OK && !counter; ++k) {
        const Chunk& c = chunks[k];
        VPT_HIP(hipEventSynchronize(b->chunk_ev[k]));
        const uint64_t total = h_total[k];
        if (total > c.nby) { incomplete = true; break; }   // the device found the inputs inconsistent and says so below
        if (total > capacity || at > capacity - total) { st = fail(VPT_INVALID_ARGUMENT, kTokensTooSmall); break; }
        base[k] = at;
        if (total) {
            VPT_HIP(hipMemcpyAsync(token_starts_out + at, b->d_fstarts + c.tb, 4 * size_t(total), hipMemcpyDeviceToHost, b->s_out));
            VPT_HIP(hipMemcpyAsync(token_ends_out + at, b->d_fends + c.tb, 4 * size_t(total), hipMemcpyDeviceToHost, b->s_out));
            VPT_HIP(hipMemcpyAsync(token_positions_out + at, b->d_fpos + c.tb, 4 * size_t(total), hipMemcpyDeviceToHost, b->s_out));
            if (nt) VPT_HIP(hipMemcpyAsync(token_tags_out + at * nt, b->d_ftags + c.tb * nt, 4 * size_t(total) * nt, hipMemcpyDeviceToHost, b->s_out));
            if (vocab) VPT_HIP(hipMemcpyAsync(token_ids_out + at, b->d_fids + c.tb, 4 * size_t(total), hipMemcpyDeviceToHost, b->s_out));
        }
        VPT_HIP(hipMemcpyAsync(packed.data() + c.a + 1, b->d_ftoff + c.a + k + 1, 8 * c.n, hipMemcpyDeviceToHost, b->s_out));
        at += total;
    }
    VPT_HIP(hipStreamSynchronize(b->s_out));
    st = lanes.verdict(st);
    if (counter) {   // every lane is through: so is the counter
        counter->in_flight = false;
        counter->last_stream = nullptr;
        return st;
    }
    if (st != VPT_OK) return st;
    if (incomplete) return fail(VPT_RUNTIME_ERROR, "vpt_token_stream_tagged_batch: a chunk's output size is out of range");
    for (size_t k = 1; k < chunks.size(); ++k)
        for (size_t j = 1; j <= chunks[k].n; ++j) packed[chunks[k].a + j] += base[k];
    size_t k = 0;
    for (size_t i = 0; i < n_documents; ++i) {
        token_offsets_out[i] = packed[k];
        if (byte_offsets[i + 1] != byte_offsets[i]) ++k;
    }
    token_offsets_out[n_documents] = packed[n];
    return VPT_OK;
}
}  // namespace

vpt_status vpt_token_stream_tagged_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_documents,
                                         unsigned wsconst_flags, const void* tagger, const void* stop, uint64_t* token_offsets_out,
                                         uint32_t* token_starts_out, uint32_t* token_ends_out, uint32_t* token_positions_out, int32_t* token_tags_out,
                                         uint64_t capacity) {
    return token_stream_chunks(p, utf8, byte_offsets, n_documents, wsconst_flags, true, tagger, stop, nullptr, 0, nullptr, token_offsets_out, token_starts_out,
                               token_ends_out, token_positions_out, token_tags_out, nullptr, capacity);
}

// The token stream with every token's vocabulary id: the untagged steps when neither tagger, stop set nor tags are asked for, else the tagged ones
vpt_status vpt_token_stream_ids_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_documents,
                                      unsigned wsconst_flags, const void* tagger, const void* stop, const void* vocab, unsigned vocab_flags,
                                      uint64_t* token_offsets_out, uint32_t* token_starts_out, uint32_t* token_ends_out,
                                      uint32_t* token_positions_out, int32_t* token_tags_out, int32_t* token_ids_out, uint64_t capacity) {
    if (!vocab) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: vocab: must not be NULL");
    const bool tagged = tagger || stop || token_tags_out;
    return token_stream_chunks(p, utf8, byte_offsets, n_documents, wsconst_flags, tagged, tagger, stop, static_cast<const vpt_vocab*>(vocab), vocab_flags,
                               nullptr, token_offsets_out, token_starts_out, token_ends_out, token_positions_out, token_tags_out, token_ids_out, capacity);
}

// Every token of the stream into a vocabulary counter; nothing comes back: the untagged steps without tagger and stop set, else the tagged ones
vpt_status vpt_token_stream_count_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_documents,
                                        unsigned wsconst_flags, const void* tagger, const void* stop, void* counter, unsigned vocab_flags) {
    if (!counter) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: counter: must not be NULL");
    const bool tagged = tagger || stop;
    return token_stream_chunks(p, utf8, byte_offsets, n_documents, wsconst_flags, tagged, tagger, stop, nullptr, vocab_flags, static_cast<vpt_vocab_counter*>(counter),
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
}

// Documents in, the segment's postings out: the id stream's steps into buffers of this call (a token has a byte at least, so the text's bytes
// bound the tokens), then the WHOLE batch's token_offsets and ids to the device and the postings pass once over them -- the ids make one trip to
// the host and back, and the result cannot depend on how the stream was cut into chunks.
// (positional: also post_first [capacity + 1] and post_positions [capacity_positions], the latter from the stream's token_positions by
// postings_positions_device behind the pass)
namespace {
vpt_status token_stream_postings(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_documents,
                                 unsigned wsconst_flags, const void* tagger, const void* stop, const void* vocab, unsigned vocab_flags,
                                 uint64_t doc_base, uint64_t* term_offsets_out, uint32_t* post_docs_out, uint32_t* post_tfs_out,
                                 uint64_t capacity, uint64_t* n_postings_out, uint64_t* n_dropped_out, bool positional, uint64_t* post_first_out,
                                 uint32_t* post_positions_out, uint64_t capacity_positions, uint64_t* n_positions_out) {
    if (n_postings_out) *n_postings_out = 0;
    if (n_dropped_out) *n_dropped_out = 0;
    if (n_positions_out) *n_positions_out = 0;
    if (positional && (!post_first_out || !n_positions_out || (capacity_positions && !post_positions_out)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    const vpt_vocab* v = static_cast<const vpt_vocab*>(vocab);
    if (!v) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: vocab: must not be NULL");
    if (v->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: vocab: does not belong to this predictor");
    if (!term_offsets_out || !n_postings_out || !n_dropped_out || (capacity && (!post_docs_out || !post_tfs_out)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (v->n_keys == 0) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: n_terms: must be between 1 and 2^24");
    VPT_TRY(check_doc_range(doc_base, n_documents));
    const uint32_t n_terms = v->n_keys;
    std::fill(term_offsets_out, term_offsets_out + size_t(n_terms) + 1, uint64_t(0));
    if (positional) post_first_out[0] = 0;
    if (n_documents == 0) return VPT_OK;
    if (!utf8 || !byte_offsets) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (byte_offsets[n_documents] < byte_offsets[0]) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: byte_offsets: must be non-decreasing");
    const uint64_t cap_tok = byte_offsets[n_documents] - byte_offsets[0];
    VPT_TRY(check_pass_tokens(cap_tok));
    const bool tagged = tagger || stop;
    const uint32_t nt = tagged ? p->n_tags : 0u;
    std::vector<uint64_t> toff;
    std::vector<uint32_t> starts, ends, pos;
    std::vector<int32_t> tags, ids;
    try {
        toff.resize(n_documents + 1);
        starts.resize(size_t(cap_tok) + 1); ends.resize(size_t(cap_tok) + 1); pos.resize(size_t(cap_tok) + 1); ids.resize(size_t(cap_tok) + 1);
        tags.resize(size_t(cap_tok) * nt + 1);
    } catch (const std::bad_alloc&) {
        return fail(VPT_RUNTIME_ERROR, "out of host memory");
    }
    vpt_status st = token_stream_chunks(p, utf8, byte_offsets, n_documents, wsconst_flags, tagged, tagger, stop, v, vocab_flags, nullptr, toff.data(),
                                        starts.data(), ends.data(), pos.data(), tags.data(), ids.data(), cap_tok);
    if (st != VPT_OK) return st;
    const uint64_t n_tok = toff[n_documents];
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    if ((st = acquire(p, &w)) != VPT_OK) return st;
    vpt_batch* b = w.b;
    hipStream_t s = b->own_stream;
    // one allocation of this call, 256-byte sections: token_offsets | ids | term_offsets | docs | tfs | counts, and positional: first | order |
    // the stream's positions | the segment's positions
    vptcarve::Carver c;
    const size_t nt1 = size_t(n_tok) + 1, np1 = positional ? nt1 : 0;   // (a word of slack an array)
    const auto m_toff = c.take<uint64_t>(n_documents + 1);
    const auto m_ids = c.take<int32_t>(nt1);
    const auto m_term = c.take<uint64_t>(size_t(n_terms) + 1);
    const auto m_docs = c.take<uint32_t>(nt1);
    const auto m_tfs = c.take<uint32_t>(nt1);
    const auto m_cnt = c.take<uint64_t>(2);
    const auto m_first = c.take<uint64_t>(np1);
    const auto m_order = c.take<uint32_t>(np1);
    const auto m_pos = c.take<uint32_t>(np1);
    const auto m_ppos = c.take<uint32_t>(np1);
    DevBuf<unsigned char> mem;
    if ((st = mem.alloc(c.bytes())) != VPT_OK) return st;
    unsigned char* m = mem;
    VPT_HIP(hipMemcpyAsync(m_toff.at(m), toff.data(), 8 * (n_documents + 1), hipMemcpyHostToDevice, s));
    if (n_tok) VPT_HIP(hipMemcpyAsync(m_ids.at(m), ids.data(), 4 * size_t(n_tok), hipMemcpyHostToDevice, s));
    if (positional && n_tok) VPT_HIP(hipMemcpyAsync(m_pos.at(m), pos.data(), 4 * size_t(n_tok), hipMemcpyHostToDevice, s));
    st = postings_device(p, b, m_toff.at(m), n_documents, m_ids.at(m), n_tok, n_terms, doc_base, m_term.at(m), m_docs.at(m), m_tfs.at(m), n_tok,
                         positional ? m_first.at(m) : nullptr, positional ? m_order.at(m) : nullptr, m_cnt.at(m), s);
    if (st != VPT_OK) return st;
    if (positional) {
        st = postings_positions_device(p, b, m_toff.at(m), n_documents, n_tok, m_pos.at(m), m_term.at(m), n_terms, m_first.at(m), n_tok, m_order.at(m),
                                       m_ppos.at(m), s);
        if (st != VPT_OK) return st;
    }
    if ((st = vpt_batch_sync(b)) != VPT_OK) return st;
    uint64_t counts[2] = {0, 0};
    VPT_HIP(hipMemcpy(counts, m_cnt.at(m), 16, hipMemcpyDeviceToHost));
    *n_postings_out = counts[0];
    *n_dropped_out = counts[1];
    if (positional) *n_positions_out = n_tok - counts[1];   // the indexed tokens
    if (counts[0] > capacity) return fail(VPT_INVALID_ARGUMENT, kPostingsTooSmall);
    if (positional && *n_positions_out > capacity_positions)
        return fail(VPT_INVALID_ARGUMENT, kPositionsTooSmall);
    VPT_HIP(hipMemcpy(term_offsets_out, m_term.at(m), 8 * (size_t(n_terms) + 1), hipMemcpyDeviceToHost));
    if (counts[0]) {
        VPT_HIP(hipMemcpy(post_docs_out, m_docs.at(m), 4 * size_t(counts[0]), hipMemcpyDeviceToHost));
        VPT_HIP(hipMemcpy(post_tfs_out, m_tfs.at(m), 4 * size_t(counts[0]), hipMemcpyDeviceToHost));
    }
    if (positional) {
        VPT_HIP(hipMemcpy(post_first_out, m_first.at(m), 8 * (size_t(counts[0]) + 1), hipMemcpyDeviceToHost));
        if (*n_positions_out) VPT_HIP(hipMemcpy(post_positions_out, m_ppos.at(m), 4 * size_t(*n_positions_out), hipMemcpyDeviceToHost));
    }
    return VPT_OK;
}
}  // namespace

vpt_status vpt_token_stream_postings_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_documents,
                                           unsigned wsconst_flags, const void* tagger, const void* stop, const void* vocab, unsigned vocab_flags,
                                           uint64_t doc_base, uint64_t* term_offsets_out, uint32_t* post_docs_out, uint32_t* post_tfs_out,
                                           uint64_t capacity, uint64_t* n_postings_out, uint64_t* n_dropped_out) {
    return token_stream_postings(p, utf8, byte_offsets, n_documents, wsconst_flags, tagger, stop, vocab, vocab_flags, doc_base, term_offsets_out,
                                 post_docs_out, post_tfs_out, capacity, n_postings_out, n_dropped_out, false, nullptr, nullptr, 0, nullptr);
}

vpt_status vpt_token_stream_positional_postings_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_documents,
                                                      unsigned wsconst_flags, const void* tagger, const void* stop, const void* vocab,
                                                      unsigned vocab_flags, uint64_t doc_base, uint64_t* term_offsets_out, uint32_t* post_docs_out,
                                                      uint32_t* post_tfs_out, uint64_t* post_first_out, uint64_t capacity,
                                                      uint32_t* post_positions_out, uint64_t capacity_positions, uint64_t* n_postings_out,
                                                      uint64_t* n_dropped_out, uint64_t* n_positions_out) {
    return token_stream_postings(p, utf8, byte_offsets, n_documents, wsconst_flags, tagger, stop, vocab, vocab_flags, doc_base, term_offsets_out,
                                 post_docs_out, post_tfs_out, capacity, n_postings_out, n_dropped_out, true, post_first_out, post_positions_out,
                                 capacity_positions, n_positions_out);
}

namespace {
// a segment's arrays in an allocation of a host call, each with a word of slack; first and ppos: a positional segment's, else of count 0
struct SegmentMem {
    vptcarve::Section<uint64_t> term;
    vptcarve::Section<uint32_t> docs, tfs;
    vptcarve::Section<uint64_t> first;
    vptcarve::Section<uint32_t> ppos;
    SegmentMem(vptcarve::Carver& c, size_t n_terms, size_t n, size_t np, bool positional)
        : term(c, n_terms + 1), docs(c, n + 1), tfs(c, n + 1), first(c, positional ? n + 1 : 0), ppos(c, positional ? np + 1 : 0) {}
};

// Host segments in, the merged segment out: every segment's term_offsets and its postings (term_offsets[n_terms] of them, at most its capacity)
// go to one allocation of this call, the device merge runs once over them, and the merged arrays come back.  positional (segments:
// vpt_postings_positional_segment): with every segment's post_first (postings + 1 entries) and positions (post_first[postings] of them, at
// most its capacity_positions) beside its three arrays; else (segments: vpt_postings_segment) the position arguments are not looked at.
vpt_status postings_merge_host(const vpt_predictor* p, const void* segments, bool positional, size_t n_segments, uint32_t n_terms_out, unsigned flags,
                               uint64_t* term_offsets_out, uint32_t* post_docs_out, uint32_t* post_tfs_out, uint64_t* post_first_out, uint64_t capacity,
                               uint32_t* post_positions_out, uint64_t capacity_positions, uint64_t* n_postings_out, uint64_t* n_combined_out,
                               uint64_t* n_positions_out) {
    if (n_postings_out) *n_postings_out = 0;
    if (n_combined_out) *n_combined_out = 0;
    if (n_positions_out) *n_positions_out = 0;
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!segments || !term_offsets_out || !n_postings_out || !n_combined_out || (capacity && (!post_docs_out || !post_tfs_out)) ||
        (positional && (!post_first_out || !n_positions_out || (capacity_positions && !post_positions_out))))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    VPT_TRY(check_n_segments(n_segments));
    VPT_TRY(check_n_terms(n_terms_out));
    vptcarve::Carver c;
    std::vector<vpt_postings_positional_segment> in(n_segments), dev(n_segments);
    std::vector<SegmentMem> at;   // where the segment's arrays are in the allocation
    at.reserve(n_segments);
    uint64_t n_in = 0, np_in = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        in[s] = merge_segment(segments, positional, s);
        if (!in[s].d_term_offsets || (positional && !in[s].d_post_first) || (in[s].capacity && (!in[s].d_post_docs || !in[s].d_post_tfs)) ||
            (in[s].capacity_positions && !in[s].d_post_positions))
            return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
        if (in[s].n_terms > n_terms_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: segment: n_terms above n_terms_out");
        const uint64_t n = std::min(in[s].d_term_offsets[in[s].n_terms], in[s].capacity);   // (an end above the capacity: the device reports it)
        const uint64_t np = positional ? std::min(in[s].d_post_first[n], in[s].capacity_positions) : 0;
        VPT_TRY(check_merge_places(n_in, n));
        VPT_TRY(check_merge_positions(np_in, np));
        dev[s].n_terms = in[s].n_terms;
        dev[s].capacity = n;
        dev[s].capacity_positions = np;
        at.emplace_back(c, in[s].n_terms, size_t(n), size_t(np), positional);
        n_in += n;
        np_in += np;
    }
    const SegmentMem out(c, n_terms_out, size_t(n_in), size_t(np_in), positional);
    const auto cnt = c.take<uint64_t>(3);
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    VPT_TRY(acquire(p, &w));
    vpt_batch* b = w.b;
    hipStream_t s = b->own_stream;
    DevBuf<unsigned char> mem;
    VPT_TRY(mem.alloc(c.bytes()));
    unsigned char* m = mem;
    for (size_t k = 0; k < n_segments; ++k) {
        const size_t n = size_t(dev[k].capacity), np = size_t(dev[k].capacity_positions);
        const SegmentMem& a = at[k];
        VPT_HIP(hipMemcpyAsync(a.term.at(m), in[k].d_term_offsets, 8 * (size_t(in[k].n_terms) + 1), hipMemcpyHostToDevice, s));
        if (positional) VPT_HIP(hipMemcpyAsync(a.first.at(m), in[k].d_post_first, 8 * (n + 1), hipMemcpyHostToDevice, s));
        if (n) {
            VPT_HIP(hipMemcpyAsync(a.docs.at(m), in[k].d_post_docs, 4 * n, hipMemcpyHostToDevice, s));
            VPT_HIP(hipMemcpyAsync(a.tfs.at(m), in[k].d_post_tfs, 4 * n, hipMemcpyHostToDevice, s));
        }
        if (np) VPT_HIP(hipMemcpyAsync(a.ppos.at(m), in[k].d_post_positions, 4 * np, hipMemcpyHostToDevice, s));
        dev[k].d_term_offsets = a.term.at(m); dev[k].d_post_docs = a.docs.at(m); dev[k].d_post_tfs = a.tfs.at(m);
        dev[k].d_post_first = a.first.at(m); dev[k].d_post_positions = a.ppos.at(m);
    }
    if (positional) {
        VPT_TRY(postings_merge_positional_device(p, b, dev.data(), n_segments, n_terms_out, flags, out.term.at(m), out.docs.at(m), out.tfs.at(m),
                                                 out.first.at(m), n_in, out.ppos.at(m), np_in, cnt.at(m), s));
    } else {
        std::vector<vpt_postings_segment> plain(n_segments);
        for (size_t k = 0; k < n_segments; ++k)
            plain[k] = vpt_postings_segment{dev[k].d_term_offsets, dev[k].d_post_docs, dev[k].d_post_tfs, dev[k].n_terms, dev[k].capacity};
        VPT_TRY(postings_merge_device(p, b, plain.data(), n_segments, n_terms_out, flags, out.term.at(m), out.docs.at(m), out.tfs.at(m), n_in, cnt.at(m), s));
    }
    VPT_TRY(vpt_batch_sync(b));
    uint64_t counts[3] = {0, 0, 0};
    VPT_HIP(hipMemcpy(counts, cnt.at(m), positional ? 24 : 16, hipMemcpyDeviceToHost));
    *n_postings_out = counts[0];
    *n_combined_out = counts[1];
    if (positional) *n_positions_out = counts[2];
    if (counts[0] > capacity) return fail(VPT_INVALID_ARGUMENT, kPostingsTooSmall);
    if (positional && counts[2] > capacity_positions) return fail(VPT_INVALID_ARGUMENT, kPositionsTooSmall);
    VPT_HIP(hipMemcpy(term_offsets_out, out.term.at(m), 8 * (size_t(n_terms_out) + 1), hipMemcpyDeviceToHost));
    if (positional) VPT_HIP(hipMemcpy(post_first_out, out.first.at(m), 8 * (size_t(counts[0]) + 1), hipMemcpyDeviceToHost));
    if (counts[0]) {
        VPT_HIP(hipMemcpy(post_docs_out, out.docs.at(m), 4 * size_t(counts[0]), hipMemcpyDeviceToHost));
        VPT_HIP(hipMemcpy(post_tfs_out, out.tfs.at(m), 4 * size_t(counts[0]), hipMemcpyDeviceToHost));
    }
    if (positional && counts[2]) VPT_HIP(hipMemcpy(post_positions_out, out.ppos.at(m), 4 * size_t(counts[2]), hipMemcpyDeviceToHost));
    return VPT_OK;
}
}  // namespace

vpt_status vpt_postings_merge(const vpt_predictor* p, const void* segments, size_t n_segments, uint32_t n_terms_out, unsigned flags,
                              uint64_t* term_offsets_out, uint32_t* post_docs_out, uint32_t* post_tfs_out, uint64_t capacity, uint64_t* n_postings_out,
                              uint64_t* n_combined_out) {
    return postings_merge_host(p, segments, false, n_segments, n_terms_out, flags, term_offsets_out, post_docs_out, post_tfs_out, nullptr, capacity, nullptr,
                               0, n_postings_out, n_combined_out, nullptr);
}

vpt_status vpt_postings_merge_positional(const vpt_predictor* p, const void* segments, size_t n_segments, uint32_t n_terms_out, unsigned flags,
                                         uint64_t* term_offsets_out, uint32_t* post_docs_out, uint32_t* post_tfs_out, uint64_t* post_first_out,
                                         uint64_t capacity, uint32_t* post_positions_out, uint64_t capacity_positions, uint64_t* n_postings_out,
                                         uint64_t* n_combined_out, uint64_t* n_positions_out) {
    return postings_merge_host(p, segments, true, n_segments, n_terms_out, flags, term_offsets_out, post_docs_out, post_tfs_out, post_first_out, capacity,
                               post_positions_out, capacity_positions, n_postings_out, n_combined_out, n_positions_out);
}

// The BM25 weight of a term of document frequency df among n_documents, as tantivy's Bm25Weight computes it: one implementation for every binding.
vpt_status vpt_okapi_idf(uint64_t n_documents, uint64_t df, float* idf_out) {
    if (!idf_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (df > n_documents) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: df: above n_documents");
    const double x = (double(n_documents - df) + 0.5) / (double(df) + 0.5);
    *idf_out = float(std::log(1.0 + x));
    return VPT_OK;
}

namespace {
// The candidates of the OR search: the dfs of the slots whose term is in range.  (Bounds that do not ascend: the device reports them; such a
// list counts 0.  Counting stops at 2^32: the call refuses that.)
uint64_t search_candidates(const uint64_t* term_offsets, uint32_t n_terms, uint64_t n_post, const int32_t* query_terms, uint64_t n_slots) {
    uint64_t n_cand = 0;
    for (uint64_t s = 0; s < n_slots && n_cand < (1ull << 32); ++s) {
        const int32_t t = query_terms[s];
        if (t < 0 || uint32_t(t) >= n_terms) continue;
        const uint64_t a = term_offsets[t], e = term_offsets[uint32_t(t) + 1];
        if (e > a && e <= n_post) n_cand += e - a;
    }
    return n_cand;
}

// The places of the boolean search as the device counts them (kernels_postings_boolean.hip): per query the df of its first MUST slot of the
// smallest df, or, without a MUST slot, the dfs of its SHOULD slots; nothing for a query with a MUST slot out of range or of df 0.  (Arrays
// that are no segment's or no CSR: the device reports them; such a query or list counts 0.)
uint64_t boolean_places(const uint64_t* term_offsets, uint32_t n_terms, uint64_t n_post, const uint64_t* query_offsets, const int32_t* query_terms,
                        const uint8_t* query_occurs, uint32_t n_queries, uint64_t n_slots) {
    uint64_t places = 0;
    for (uint32_t q = 0; q < n_queries && places < (1ull << 32); ++q) {
        const uint64_t a = query_offsets[q], e = query_offsets[q + 1];
        if (a > e || e > n_slots || e - a > vpt::kSearchMaxQuerySlots) continue;
        uint64_t best = ~uint64_t(0), should = 0;
        bool must = false, dead = false;
        for (uint64_t s = a; s < e; ++s) {
            const int32_t t = query_terms[s];
            uint64_t df = 0;
            if (t >= 0 && uint32_t(t) < n_terms) {
                const uint64_t ta = term_offsets[t], tb = term_offsets[uint32_t(t) + 1];
                if (ta <= tb && tb <= n_post) df = tb - ta;
            }
            if (query_occurs[s] == VPT_OCCUR_MUST) {
                must = true;
                if (df == 0) dead = true;
                best = std::min(best, df);
            } else if (query_occurs[s] == VPT_OCCUR_SHOULD) {
                should += df;
            }
        }
        if (!dead) places += must ? best : should;
    }
    return places;
}

// The probes of the phrase search as the device counts them: per phrase that can match, the indexed tokens of its rarest term.  (Arrays that
// are no segment's or no CSR: the device reports them; a query is then counted as 0.)
uint64_t phrase_probes(const uint64_t* term_offsets, const uint64_t* post_first, uint32_t n_terms, uint64_t n_post, uint64_t n_pos,
                       const uint64_t* query_offsets, const int32_t* query_terms, uint32_t n_queries, uint64_t n_slots) {
    uint64_t n_probes = 0;
    for (uint32_t q = 0; q < n_queries && n_probes < (1ull << 32); ++q) {
        const uint64_t a = query_offsets[q], e = query_offsets[q + 1];
        if (a >= e || e > n_slots || e - a > vpt::kPhraseMaxTerms) continue;
        uint64_t best = ~uint64_t(0);
        for (uint64_t s = a; s < e && best; ++s) {
            const int32_t t = query_terms[s];
            if (t < 0 || uint32_t(t) >= n_terms) { best = 0; break; }
            const uint64_t ta = term_offsets[t], tb = term_offsets[uint32_t(t) + 1];
            if (ta >= tb || tb > n_post || post_first[ta] > post_first[tb] || post_first[tb] > n_pos) { best = 0; break; }
            best = std::min(best, post_first[tb] - post_first[ta]);
        }
        n_probes += best;
    }
    return n_probes;
}

// What a search over host arrays keeps in the one allocation of its call: the segment (phrase: with post_first and the positions), the
// documents' lengths, the query CSR (a weight a slot, phrase: a weight a query; boolean: an occur a slot), the hit arrays (phrase: with the
// frequencies), the counts.  The inputs have a word of slack each.
struct SearchMem {
    const size_t n_terms, n_post, n_pos, n_docs, n_queries, n_slots, n_out, n_slops;
    const bool phrase, boolean;
    vptcarve::Carver c{};
    vptcarve::Section<uint64_t> term{c, n_terms + 1};
    vptcarve::Section<uint32_t> docs{c, n_post + 1}, tfs{c, n_post + 1};
    vptcarve::Section<uint64_t> first{c, phrase ? n_post + 1 : 0};
    vptcarve::Section<uint32_t> pos{c, phrase ? n_pos + 1 : 0}, dl{c, n_docs + 1};
    vptcarve::Section<uint64_t> qoff{c, n_queries + 1};
    vptcarve::Section<int32_t> qterms{c, n_slots + 1};
    vptcarve::Section<float> qweights{c, phrase ? n_queries : n_slots + 1};
    vptcarve::Section<uint8_t> qoccurs{c, boolean ? n_slots + 4 : 0};
    vptcarve::Section<uint32_t> hit_docs{c, n_out};
    vptcarve::Section<float> hit_scores{c, n_out};
    vptcarve::Section<uint32_t> hit_freqs{c, phrase ? n_out : 0}, hit_counts{c, n_queries};
    vptcarve::Section<uint64_t> match_counts{c, n_queries}, counts{c, 3};
    vptcarve::Section<uint32_t> qslops{c, n_slops};   // (the sloppy phrase search with slops; behind everything else: no other offset moves)
    SearchMem(uint32_t terms, uint64_t post, uint64_t positions, uint64_t documents, uint32_t queries, uint64_t slots, uint32_t k, bool is_phrase,
              bool is_boolean, bool with_slops = false)
        : n_terms(terms), n_post(size_t(post)), n_pos(size_t(positions)), n_docs(size_t(documents)), n_queries(queries), n_slots(size_t(slots)),
          n_out(size_t(queries) * k), n_slops(with_slops ? queries : 0), phrase(is_phrase), boolean(is_boolean) {}

    // the segment, the lengths and the query CSR go up (post_first, post_positions: the phrase search's; query_occurs: the boolean search's)
    vpt_status upload(unsigned char* m, hipStream_t s, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                      const uint64_t* post_first, const uint32_t* post_positions, const uint32_t* doc_lens, const uint64_t* query_offsets,
                      const int32_t* query_terms, const float* query_weights, const uint8_t* query_occurs) const {
        VPT_HIP(hipMemcpyAsync(term.at(m), term_offsets, 8 * (n_terms + 1), hipMemcpyHostToDevice, s));
        if (n_post) {
            VPT_HIP(hipMemcpyAsync(docs.at(m), post_docs, 4 * n_post, hipMemcpyHostToDevice, s));
            VPT_HIP(hipMemcpyAsync(tfs.at(m), post_tfs, 4 * n_post, hipMemcpyHostToDevice, s));
        }
        if (phrase) VPT_HIP(hipMemcpyAsync(first.at(m), post_first, 8 * (n_post + 1), hipMemcpyHostToDevice, s));
        if (n_pos) VPT_HIP(hipMemcpyAsync(pos.at(m), post_positions, 4 * n_pos, hipMemcpyHostToDevice, s));
        if (n_docs) VPT_HIP(hipMemcpyAsync(dl.at(m), doc_lens, 4 * n_docs, hipMemcpyHostToDevice, s));
        VPT_HIP(hipMemcpyAsync(qoff.at(m), query_offsets, 8 * (n_queries + 1), hipMemcpyHostToDevice, s));
        if (n_slots) VPT_HIP(hipMemcpyAsync(qterms.at(m), query_terms, 4 * n_slots, hipMemcpyHostToDevice, s));
        if (const size_t n_weights = phrase ? n_queries : n_slots) VPT_HIP(hipMemcpyAsync(qweights.at(m), query_weights, 4 * n_weights, hipMemcpyHostToDevice, s));
        if (boolean && n_slots) VPT_HIP(hipMemcpyAsync(qoccurs.at(m), query_occurs, n_slots, hipMemcpyHostToDevice, s));
        return VPT_OK;
    }
    // an entry at or behind a query's hit count is not written on the device: zeros come back
    vpt_status clear_hits(unsigned char* m, hipStream_t s) const {
        VPT_HIP(hipMemsetAsync(m + hit_docs.offset, 0, hit_counts.offset - hit_docs.offset, s));
        return VPT_OK;
    }
    vpt_status read_back(unsigned char* m, uint64_t* counts_out, uint32_t* hit_counts_out, uint64_t* match_counts_out, uint32_t* hit_docs_out,
                         float* hit_scores_out, uint32_t* hit_freqs_out) const {
        VPT_HIP(hipMemcpy(counts_out, counts.at(m), 24, hipMemcpyDeviceToHost));
        VPT_HIP(hipMemcpy(hit_counts_out, hit_counts.at(m), 4 * n_queries, hipMemcpyDeviceToHost));
        VPT_HIP(hipMemcpy(match_counts_out, match_counts.at(m), 8 * n_queries, hipMemcpyDeviceToHost));
        VPT_HIP(hipMemcpy(hit_docs_out, hit_docs.at(m), 4 * n_out, hipMemcpyDeviceToHost));
        VPT_HIP(hipMemcpy(hit_scores_out, hit_scores.at(m), 4 * n_out, hipMemcpyDeviceToHost));
        if (phrase) VPT_HIP(hipMemcpy(hit_freqs_out, hit_freqs.at(m), 4 * n_out, hipMemcpyDeviceToHost));
        return VPT_OK;
    }
};

// A host segment, host documents' lengths and host queries in, the hits out: what the segment holds (term_offsets[n_terms] postings) goes to one
// allocation of this call, the candidates (boolean false: the OR search) or the places (the boolean search) are counted from the host's arrays,
// the device search runs once, the four outputs come back.
vpt_status postings_search_host(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs, uint32_t n_terms,
                                uint64_t doc_base, uint64_t n_documents, const uint32_t* doc_lens, const uint64_t* query_offsets,
                                const int32_t* query_terms, const float* query_weights, bool boolean, const uint8_t* query_occurs, uint32_t n_queries,
                                float k1, float b_param, float avgdl, uint32_t k, uint32_t* hit_docs_out, float* hit_scores_out,
                                uint32_t* hit_counts_out, uint64_t* match_counts_out, uint64_t* counts_out) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!term_offsets || !query_offsets || !hit_docs_out || !hit_scores_out || !hit_counts_out || !match_counts_out || !counts_out)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    VPT_TRY(check_n_terms(n_terms));
    VPT_TRY(check_n_queries(n_queries));
    VPT_TRY(check_top_k(n_queries, k));
    const uint64_t n_post = term_offsets[n_terms], n_slots = query_offsets[n_queries];
    VPT_TRY(check_search_sizes(false, n_post, n_slots));
    if ((n_post && (!post_docs || !post_tfs)) || (n_documents && !doc_lens) || (n_slots && (!query_terms || !query_weights || (boolean && !query_occurs))))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    const uint64_t n_cand = boolean ? boolean_places(term_offsets, n_terms, n_post, query_offsets, query_terms, query_occurs, n_queries, n_slots)
                                    : search_candidates(term_offsets, n_terms, n_post, query_terms, n_slots);
    VPT_TRY(check_search_sizes(false, n_cand));
    VPT_TRY(check_doc_range(0, n_documents));
    const SearchMem A(n_terms, n_post, 0, n_documents, n_queries, n_slots, k, false, boolean);
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    VPT_TRY(acquire(p, &w));
    vpt_batch* b = w.b;
    hipStream_t s = b->own_stream;
    DevBuf<unsigned char> mem;
    VPT_TRY(mem.alloc(A.c.bytes()));
    unsigned char* m = mem;
    VPT_TRY(A.upload(m, s, term_offsets, post_docs, post_tfs, nullptr, nullptr, doc_lens, query_offsets, query_terms, query_weights, query_occurs));
    VPT_TRY(A.clear_hits(m, s));
    if (!boolean)
        VPT_TRY(postings_search_device(p, b, A.term.at(m), A.docs.at(m), A.tfs.at(m), n_terms, n_post, doc_base, n_documents, A.dl.at(m), A.qoff.at(m),
                                       A.qterms.at(m), A.qweights.at(m), n_queries, n_slots, k1, b_param, avgdl, k, n_cand, A.hit_docs.at(m),
                                       A.hit_scores.at(m), A.hit_counts.at(m), A.match_counts.at(m), A.counts.at(m), s));
    else
        VPT_TRY(postings_boolean_search_device(p, b, A.term.at(m), A.docs.at(m), A.tfs.at(m), n_terms, n_post, doc_base, n_documents, A.dl.at(m),
                                               A.qoff.at(m), A.qterms.at(m), A.qweights.at(m), A.qoccurs.at(m), n_queries, n_slots, k1, b_param, avgdl, k,
                                               n_cand, A.hit_docs.at(m), A.hit_scores.at(m), A.hit_counts.at(m), A.match_counts.at(m), A.counts.at(m), s));
    VPT_TRY(vpt_batch_sync(b));
    return A.read_back(m, counts_out, hit_counts_out, match_counts_out, hit_docs_out, hit_scores_out, nullptr);
}
}  // namespace

vpt_status vpt_postings_search(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs, uint32_t n_terms,
                               uint64_t doc_base, uint64_t n_documents, const uint32_t* doc_lens, const uint64_t* query_offsets,
                               const int32_t* query_terms, const float* query_weights, uint32_t n_queries, float k1, float b_param, float avgdl,
                               uint32_t k, uint32_t* hit_docs_out, float* hit_scores_out, uint32_t* hit_counts_out, uint64_t* match_counts_out,
                               uint64_t* counts_out) {
    return postings_search_host(p, term_offsets, post_docs, post_tfs, n_terms, doc_base, n_documents, doc_lens, query_offsets, query_terms, query_weights,
                                false, nullptr, n_queries, k1, b_param, avgdl, k, hit_docs_out, hit_scores_out, hit_counts_out, match_counts_out,
                                counts_out);
}

// The boolean search over host arrays: vpt_postings_search's route with the occurs beside the weights and the places counted as the device does.
vpt_status vpt_postings_boolean_search(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                                       uint32_t n_terms, uint64_t doc_base, uint64_t n_documents, const uint32_t* doc_lens, const uint64_t* query_offsets,
                                       const int32_t* query_terms, const float* query_weights, const uint8_t* query_occurs, uint32_t n_queries, float k1,
                                       float b_param, float avgdl, uint32_t k, uint32_t* hit_docs_out, float* hit_scores_out, uint32_t* hit_counts_out,
                                       uint64_t* match_counts_out, uint64_t* counts_out) {
    return postings_search_host(p, term_offsets, post_docs, post_tfs, n_terms, doc_base, n_documents, doc_lens, query_offsets, query_terms, query_weights,
                                true, query_occurs, n_queries, k1, b_param, avgdl, k, hit_docs_out, hit_scores_out, hit_counts_out, match_counts_out,
                                counts_out);
}

namespace {
// A host positional segment, host documents' lengths and host phrases in, the hits out: what the segment holds goes to one allocation of this
// call, the probes are counted from the host's arrays as the device counts them, the device search runs once, the five outputs come back.
// sloppy: the sloppy device call, query_slops (NULL: all 0) uploaded beside the weights.
vpt_status phrase_search_host(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                              const uint64_t* post_first, const uint32_t* post_positions, uint32_t n_terms, uint64_t doc_base, uint64_t n_documents,
                              const uint32_t* doc_lens, const uint64_t* query_offsets, const int32_t* query_terms, const float* query_weights,
                              bool sloppy, const uint32_t* query_slops, uint32_t n_queries, float k1, float b_param, float avgdl, uint32_t k,
                              uint32_t* hit_docs_out, float* hit_scores_out, uint32_t* hit_freqs_out, uint32_t* hit_counts_out,
                              uint64_t* match_counts_out, uint64_t* counts_out) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!term_offsets || !post_first || !query_offsets || !query_weights || !hit_docs_out || !hit_scores_out || !hit_freqs_out || !hit_counts_out ||
        !match_counts_out || !counts_out)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    VPT_TRY(check_n_terms(n_terms));
    VPT_TRY(check_n_queries(n_queries));
    VPT_TRY(check_top_k(n_queries, k));
    const uint64_t n_post = term_offsets[n_terms], n_slots = query_offsets[n_queries];
    VPT_TRY(check_search_sizes(true, n_post, n_slots));
    const uint64_t n_pos = post_first[n_post];
    VPT_TRY(check_search_sizes(true, n_pos));
    if ((n_post && (!post_docs || !post_tfs)) || (n_pos && !post_positions) || (n_documents && !doc_lens) || (n_slots && !query_terms))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    const uint64_t n_probes = phrase_probes(term_offsets, post_first, n_terms, n_post, n_pos, query_offsets, query_terms, n_queries, n_slots);
    VPT_TRY(check_search_sizes(true, n_probes));
    VPT_TRY(check_doc_range(0, n_documents));
    const bool slops = sloppy && query_slops;
    const SearchMem A(n_terms, n_post, n_pos, n_documents, n_queries, n_slots, k, true, false, slops);
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    VPT_TRY(acquire(p, &w));
    vpt_batch* b = w.b;
    hipStream_t s = b->own_stream;
    DevBuf<unsigned char> mem;
    VPT_TRY(mem.alloc(A.c.bytes()));
    unsigned char* m = mem;
    VPT_TRY(A.upload(m, s, term_offsets, post_docs, post_tfs, post_first, post_positions, doc_lens, query_offsets, query_terms, query_weights, nullptr));
    if (slops) VPT_HIP(hipMemcpyAsync(A.qslops.at(m), query_slops, 4 * size_t(n_queries), hipMemcpyHostToDevice, s));
    VPT_TRY(A.clear_hits(m, s));
    VPT_TRY(postings_phrase_search_device(p, b, A.term.at(m), A.docs.at(m), A.tfs.at(m), A.first.at(m), A.pos.at(m), n_terms, n_post, n_pos, doc_base,
                                          n_documents, A.dl.at(m), A.qoff.at(m), A.qterms.at(m), A.qweights.at(m), n_queries, n_slots, k1, b_param, avgdl, k,
                                          n_probes, A.hit_docs.at(m), A.hit_scores.at(m), A.hit_freqs.at(m), A.hit_counts.at(m), A.match_counts.at(m),
                                          A.counts.at(m), sloppy, slops ? A.qslops.at(m) : nullptr, s));
    VPT_TRY(vpt_batch_sync(b));
    return A.read_back(m, counts_out, hit_counts_out, match_counts_out, hit_docs_out, hit_scores_out, hit_freqs_out);
}
}  // namespace

vpt_status vpt_postings_phrase_search(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                                      const uint64_t* post_first, const uint32_t* post_positions, uint32_t n_terms, uint64_t doc_base,
                                      uint64_t n_documents, const uint32_t* doc_lens, const uint64_t* query_offsets, const int32_t* query_terms,
                                      const float* query_weights, uint32_t n_queries, float k1, float b_param, float avgdl, uint32_t k,
                                      uint32_t* hit_docs_out, float* hit_scores_out, uint32_t* hit_freqs_out, uint32_t* hit_counts_out,
                                      uint64_t* match_counts_out, uint64_t* counts_out) {
    return phrase_search_host(p, term_offsets, post_docs, post_tfs, post_first, post_positions, n_terms, doc_base, n_documents, doc_lens, query_offsets,
                              query_terms, query_weights, false, nullptr, n_queries, k1, b_param, avgdl, k, hit_docs_out, hit_scores_out, hit_freqs_out,
                              hit_counts_out, match_counts_out, counts_out);
}

vpt_status vpt_postings_sloppy_phrase_search(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                                             const uint64_t* post_first, const uint32_t* post_positions, uint32_t n_terms, uint64_t doc_base,
                                             uint64_t n_documents, const uint32_t* doc_lens, const uint64_t* query_offsets,
                                             const int32_t* query_terms, const float* query_weights, const uint32_t* query_slops, uint32_t n_queries,
                                             float k1, float b_param, float avgdl, uint32_t k, uint32_t* hit_docs_out, float* hit_scores_out,
                                             uint32_t* hit_freqs_out, uint32_t* hit_counts_out, uint64_t* match_counts_out, uint64_t* counts_out) {
    return phrase_search_host(p, term_offsets, post_docs, post_tfs, post_first, post_positions, n_terms, doc_base, n_documents, doc_lens, query_offsets,
                              query_terms, query_weights, true, query_slops, n_queries, k1, b_param, avgdl, k, hit_docs_out, hit_scores_out,
                              hit_freqs_out, hit_counts_out, match_counts_out, counts_out);
}

namespace {
// What a phrase's list can hold at most: the smallest df among its terms (a document of the list has a posting of every term); 0 for a phrase
// that is empty, too long, or has a term out of range or bounds that are no list's.  The sum over the phrases always suffices as capacity_lists.
uint64_t phrase_list_bound(const uint64_t* term_offsets, uint32_t n_terms, uint64_t n_post, const int32_t* terms, uint64_t len) {
    if (len == 0 || len > vpt::kPhraseMaxTerms) return 0;
    uint64_t best = ~uint64_t(0);
    for (uint64_t j = 0; j < len; ++j) {
        const int32_t t = terms[j];
        if (t < 0 || uint32_t(t) >= n_terms) return 0;
        const uint64_t ta = term_offsets[t], tb = term_offsets[uint32_t(t) + 1];
        if (ta >= tb || tb > n_post) return 0;
        best = std::min(best, tb - ta);
    }
    return best;
}

// What the two host calls keep in the one allocation of their call: the positional segment, the phrase CSR, the lists and the lists call's
// counts; the clause search adds the documents' lengths, the slot arrays and the four outputs with the counts.  The inputs have a word of slack.
struct ClauseMem {
    const size_t n_terms, n_post, n_pos, n_docs, n_phrases, n_pslots, n_lists_cap, n_queries, n_slots, n_out, n_slops;
    vptcarve::Carver c{};
    vptcarve::Section<uint64_t> term{c, n_terms + 1};
    vptcarve::Section<uint32_t> docs{c, n_post + 1}, tfs{c, n_post + 1};
    vptcarve::Section<uint64_t> first{c, n_post + 1};
    vptcarve::Section<uint32_t> pos{c, n_pos + 1};
    vptcarve::Section<uint64_t> poff{c, n_phrases + 1};
    vptcarve::Section<int32_t> pterms{c, n_pslots + 1};
    vptcarve::Section<uint64_t> loff{c, n_phrases + 1};
    vptcarve::Section<uint32_t> ldocs{c, n_lists_cap + 1}, ltfs{c, n_lists_cap + 1};
    vptcarve::Section<uint64_t> lcounts{c, 3};
    vptcarve::Section<uint32_t> dl{c, n_docs + 1};
    vptcarve::Section<uint64_t> qoff{c, n_queries + 1};
    vptcarve::Section<int32_t> qterms{c, n_slots + 1};
    vptcarve::Section<float> qweights{c, n_slots + 1};
    vptcarve::Section<uint8_t> qoccurs{c, n_slots + 4};
    vptcarve::Section<uint32_t> hit_docs{c, n_out};
    vptcarve::Section<float> hit_scores{c, n_out};
    vptcarve::Section<uint32_t> hit_counts{c, n_queries};
    vptcarve::Section<uint64_t> match_counts{c, n_queries}, counts{c, 3};
    vptcarve::Section<uint32_t> pslops{c, n_slops};   // (the sloppy calls with slops; behind everything else)
    ClauseMem(uint32_t terms, uint64_t post, uint64_t positions, uint64_t documents, size_t phrases, size_t phrase_slots, uint64_t lists, uint32_t queries,
              uint64_t slots, uint32_t k, bool with_slops = false)
        : n_terms(terms), n_post(size_t(post)), n_pos(size_t(positions)), n_docs(size_t(documents)), n_phrases(phrases), n_pslots(phrase_slots),
          n_lists_cap(size_t(lists)), n_queries(queries), n_slots(size_t(slots)), n_out(size_t(queries) * k), n_slops(with_slops ? phrases : 0) {}

    vpt_status upload_segment(unsigned char* m, hipStream_t s, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                              const uint64_t* post_first, const uint32_t* post_positions, const uint64_t* phrase_offsets,
                              const int32_t* phrase_terms) const {
        VPT_HIP(hipMemcpyAsync(term.at(m), term_offsets, 8 * (n_terms + 1), hipMemcpyHostToDevice, s));
        if (n_post) {
            VPT_HIP(hipMemcpyAsync(docs.at(m), post_docs, 4 * n_post, hipMemcpyHostToDevice, s));
            VPT_HIP(hipMemcpyAsync(tfs.at(m), post_tfs, 4 * n_post, hipMemcpyHostToDevice, s));
        }
        VPT_HIP(hipMemcpyAsync(first.at(m), post_first, 8 * (n_post + 1), hipMemcpyHostToDevice, s));
        if (n_pos) VPT_HIP(hipMemcpyAsync(pos.at(m), post_positions, 4 * n_pos, hipMemcpyHostToDevice, s));
        VPT_HIP(hipMemcpyAsync(poff.at(m), phrase_offsets, 8 * (n_phrases + 1), hipMemcpyHostToDevice, s));
        if (n_pslots) VPT_HIP(hipMemcpyAsync(pterms.at(m), phrase_terms, 4 * n_pslots, hipMemcpyHostToDevice, s));
        return VPT_OK;
    }
};

// the arguments both host calls check of a positional host segment; *n_post, *n_pos: what it holds
vpt_status check_host_positional(const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs, const uint64_t* post_first,
                                 const uint32_t* post_positions, uint32_t n_terms, uint64_t* n_post, uint64_t* n_pos) {
    if (!term_offsets || !post_first) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    VPT_TRY(check_n_terms(n_terms));
    *n_post = term_offsets[n_terms];
    VPT_TRY(check_search_sizes(true, *n_post));
    *n_pos = post_first[*n_post];
    VPT_TRY(check_search_sizes(true, *n_pos));
    if ((*n_post && (!post_docs || !post_tfs)) || (*n_pos && !post_positions)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    return VPT_OK;
}

// Host phrases over a host positional segment in, their posting lists out: the lists call once, over one allocation of this call.
vpt_status phrase_lists_host(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                             const uint64_t* post_first, const uint32_t* post_positions, uint32_t n_terms, uint64_t doc_base, uint64_t n_documents,
                             const uint64_t* phrase_offsets, const int32_t* phrase_terms, bool sloppy, const uint32_t* phrase_slops, uint32_t n_phrases,
                             uint64_t* list_offsets_out, uint32_t* list_docs_out, uint32_t* list_tfs_out, uint64_t capacity_lists,
                             uint64_t* counts_out) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!phrase_offsets || !list_offsets_out || !counts_out || (capacity_lists && (!list_docs_out || !list_tfs_out)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    uint64_t n_post = 0, n_pos = 0;
    VPT_TRY(check_host_positional(term_offsets, post_docs, post_tfs, post_first, post_positions, n_terms, &n_post, &n_pos));
    VPT_TRY(bad_argument(n_phrases == 0 || n_phrases > vpt::kSearchMaxQueries, "InvalidArgumentError: n_phrases: must be between 1 and 2^24"));
    const uint64_t n_slots = phrase_offsets[n_phrases];
    VPT_TRY(check_search_sizes(true, n_slots));
    if (n_slots && !phrase_terms) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    VPT_TRY(check_clause_lists(n_terms, 0, capacity_lists));
    const uint64_t n_probes = phrase_probes(term_offsets, post_first, n_terms, n_post, n_pos, phrase_offsets, phrase_terms, n_phrases, n_slots);
    VPT_TRY(check_search_sizes(true, n_probes));
    VPT_TRY(check_doc_range(doc_base, n_documents));
    const bool slops = sloppy && phrase_slops;
    const ClauseMem A(n_terms, n_post, n_pos, 0, n_phrases, size_t(n_slots), capacity_lists, 0, 0, 0, slops);
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    VPT_TRY(acquire(p, &w));
    vpt_batch* b = w.b;
    hipStream_t s = b->own_stream;
    DevBuf<unsigned char> mem;
    VPT_TRY(mem.alloc(A.c.bytes()));
    unsigned char* m = mem;
    VPT_TRY(A.upload_segment(m, s, term_offsets, post_docs, post_tfs, post_first, post_positions, phrase_offsets, phrase_terms));
    if (slops) VPT_HIP(hipMemcpyAsync(A.pslops.at(m), phrase_slops, 4 * size_t(n_phrases), hipMemcpyHostToDevice, s));
    VPT_TRY(postings_phrase_lists_device(p, b, A.term.at(m), A.docs.at(m), A.tfs.at(m), A.first.at(m), A.pos.at(m), n_terms, n_post, n_pos, doc_base,
                                         n_documents, A.poff.at(m), A.pterms.at(m), n_phrases, n_slots, n_probes, A.loff.at(m), A.ldocs.at(m),
                                         A.ltfs.at(m), capacity_lists, A.lcounts.at(m), sloppy, slops ? A.pslops.at(m) : nullptr, s));
    const vpt_status st = vpt_batch_sync(b);
    VPT_HIP(hipMemcpy(counts_out, A.lcounts.at(m), 24, hipMemcpyDeviceToHost));   // (the need, when a capacity was too small)
    if (st != VPT_OK) return st;
    VPT_HIP(hipMemcpy(list_offsets_out, A.loff.at(m), 8 * (size_t(n_phrases) + 1), hipMemcpyDeviceToHost));
    const uint64_t n_entries = std::min(counts_out[1], capacity_lists);
    if (n_entries) {
        VPT_HIP(hipMemcpy(list_docs_out, A.ldocs.at(m), 4 * n_entries, hipMemcpyDeviceToHost));
        VPT_HIP(hipMemcpy(list_tfs_out, A.ltfs.at(m), 4 * n_entries, hipMemcpyDeviceToHost));
    }
    return VPT_OK;
}

// Host queries of CLAUSES over a host positional segment in, the hits out.  A clause of one term is a slot of that term; every other clause is a
// phrase: the lists call makes its list, and the slot names it.  One upload, the two device calls on one stream with no sync between them, one
// download; the probes, the list entries and the places are counted on the host from the segment's bounds (a list: at most the smallest df
// among its phrase's terms).  counts_out: the clause search's, with the phrases that have a term out of range added to the skipped slots.
// sloppy: the sloppy lists call, a phrase clause's slop from clause_slops (one per clause, NULL: all 0; a one-term clause's is not looked at).
vpt_status clause_search_host(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                              const uint64_t* post_first, const uint32_t* post_positions, uint32_t n_terms, uint64_t doc_base, uint64_t n_documents,
                              const uint32_t* doc_lens, const uint64_t* query_offsets, const uint64_t* clause_offsets, const int32_t* clause_terms,
                              const float* clause_weights, const uint8_t* clause_occurs, bool sloppy, const uint32_t* clause_slops, uint32_t n_queries,
                              float k1, float b_param, float avgdl, uint32_t k, uint32_t* hit_docs_out, float* hit_scores_out,
                              uint32_t* hit_counts_out, uint64_t* match_counts_out, uint64_t* counts_out) {
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (!query_offsets || !clause_offsets || !hit_docs_out || !hit_scores_out || !hit_counts_out || !match_counts_out || !counts_out)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    uint64_t n_post = 0, n_pos = 0;
    VPT_TRY(check_host_positional(term_offsets, post_docs, post_tfs, post_first, post_positions, n_terms, &n_post, &n_pos));
    VPT_TRY(check_n_queries(n_queries));
    VPT_TRY(check_top_k(n_queries, k));
    const uint64_t n_clauses = query_offsets[n_queries];
    VPT_TRY(check_search_sizes(false, n_clauses));
    const uint64_t n_cterms = clause_offsets[n_clauses];
    VPT_TRY(check_search_sizes(true, n_cterms));
    if ((n_documents && !doc_lens) || (n_clauses && (!clause_weights || !clause_occurs)) || (n_cterms && !clause_terms))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    for (uint32_t q = 0; q < n_queries; ++q)
        if (query_offsets[q] > query_offsets[q + 1]) return status_from_bits(vpt::kErrBadQueryCsr);
    for (uint64_t c = 0; c < n_clauses; ++c)
        if (clause_offsets[c] > clause_offsets[c + 1]) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: clause_offsets: do not describe the clauses' terms");
    VPT_TRY(check_doc_range(doc_base, n_documents));
    // the slots: a clause of one term names it, every other clause names its phrase's list
    std::vector<int32_t> slot_terms, phrase_terms;
    std::vector<uint64_t> phrase_offsets{0}, slot_bound;
    std::vector<uint32_t> phrase_slops;
    const bool slops = sloppy && clause_slops;
    uint64_t cap_lists = 0, skipped_phrases = 0;
    try {
        slot_terms.reserve(size_t(n_clauses));
        slot_bound.reserve(size_t(n_clauses));
        for (uint64_t c = 0; c < n_clauses; ++c) {
            const uint64_t a = clause_offsets[c], len = clause_offsets[c + 1] - a;
            if (len == 1) {
                const int32_t t = clause_terms[a];
                uint64_t df = 0;
                if (t >= 0 && uint32_t(t) < n_terms) {
                    const uint64_t ta = term_offsets[t], tb = term_offsets[uint32_t(t) + 1];
                    if (ta <= tb && tb <= n_post) df = tb - ta;
                }
                slot_terms.push_back(t >= 0 && uint32_t(t) < n_terms ? t : -1);   // (a value at or above n_terms would name a list)
                slot_bound.push_back(df);
                continue;
            }
            const uint64_t bound = phrase_list_bound(term_offsets, n_terms, n_post, clause_terms + a, len);
            for (uint64_t j = 0; j < len; ++j)
                if (clause_terms[a + j] < 0 || uint32_t(clause_terms[a + j]) >= n_terms) { ++skipped_phrases; break; }
            slot_terms.push_back(int32_t(n_terms + (phrase_offsets.size() - 1)));
            slot_bound.push_back(bound);
            cap_lists += bound;
            phrase_terms.insert(phrase_terms.end(), clause_terms + a, clause_terms + a + len);
            phrase_offsets.push_back(phrase_terms.size());
            if (slops) phrase_slops.push_back(clause_slops[c]);
        }
    } catch (const std::bad_alloc&) {
        return fail(VPT_RUNTIME_ERROR, "out of host memory while laying out the clauses");
    }
    const size_t n_lists = phrase_offsets.size() - 1;
    VPT_TRY(check_clause_lists(n_terms, uint32_t(std::min<size_t>(n_lists, 1u << 25)), cap_lists));
    // the places by the boolean search's rule, a list counted as its bound
    uint64_t places = 0;
    for (uint32_t q = 0; q < n_queries && places < (1ull << 32); ++q) {
        const uint64_t a = query_offsets[q], e = query_offsets[q + 1];
        if (e - a > vpt::kSearchMaxQuerySlots) continue;
        uint64_t best = ~uint64_t(0), should = 0;
        bool must = false, dead = false;
        for (uint64_t s = a; s < e; ++s) {
            if (clause_occurs[s] == VPT_OCCUR_MUST) {
                must = true;
                if (slot_bound[s] == 0) dead = true;
                best = std::min(best, slot_bound[s]);
            } else if (clause_occurs[s] == VPT_OCCUR_SHOULD) {
                should += slot_bound[s];
            }
        }
        if (!dead) places += must ? best : should;
    }
    VPT_TRY(check_search_sizes(false, places));
    const uint64_t n_probes = n_lists ? phrase_probes(term_offsets, post_first, n_terms, n_post, n_pos, phrase_offsets.data(), phrase_terms.data(),
                                                      uint32_t(n_lists), phrase_terms.size())
                                      : 0;
    VPT_TRY(check_search_sizes(true, n_probes));
    const ClauseMem A(n_terms, n_post, n_pos, n_documents, n_lists, phrase_terms.size(), cap_lists, n_queries, n_clauses, k, slops);
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    VPT_TRY(acquire(p, &w));
    vpt_batch* b = w.b;
    hipStream_t s = b->own_stream;
    DevBuf<unsigned char> mem;
    VPT_TRY(mem.alloc(A.c.bytes()));
    unsigned char* m = mem;
    VPT_TRY(A.upload_segment(m, s, term_offsets, post_docs, post_tfs, post_first, post_positions, phrase_offsets.data(), phrase_terms.data()));
    if (n_documents) VPT_HIP(hipMemcpyAsync(A.dl.at(m), doc_lens, 4 * n_documents, hipMemcpyHostToDevice, s));
    VPT_HIP(hipMemcpyAsync(A.qoff.at(m), query_offsets, 8 * (size_t(n_queries) + 1), hipMemcpyHostToDevice, s));
    if (n_clauses) {
        VPT_HIP(hipMemcpyAsync(A.qterms.at(m), slot_terms.data(), 4 * n_clauses, hipMemcpyHostToDevice, s));
        VPT_HIP(hipMemcpyAsync(A.qweights.at(m), clause_weights, 4 * n_clauses, hipMemcpyHostToDevice, s));
        VPT_HIP(hipMemcpyAsync(A.qoccurs.at(m), clause_occurs, n_clauses, hipMemcpyHostToDevice, s));
    }
    VPT_HIP(hipMemsetAsync(m + A.hit_docs.offset, 0, A.hit_counts.offset - A.hit_docs.offset, s));   // (behind a query's hit count: zeros come back)
    if (slops && n_lists) VPT_HIP(hipMemcpyAsync(A.pslops.at(m), phrase_slops.data(), 4 * n_lists, hipMemcpyHostToDevice, s));
    if (n_lists)
        VPT_TRY(postings_phrase_lists_device(p, b, A.term.at(m), A.docs.at(m), A.tfs.at(m), A.first.at(m), A.pos.at(m), n_terms, n_post, n_pos, doc_base,
                                             n_documents, A.poff.at(m), A.pterms.at(m), uint32_t(n_lists), phrase_terms.size(), n_probes, A.loff.at(m),
                                             A.ldocs.at(m), A.ltfs.at(m), cap_lists, A.lcounts.at(m), sloppy, slops ? A.pslops.at(m) : nullptr, s));
    VPT_TRY(postings_clause_search_device(p, b, A.term.at(m), A.docs.at(m), A.tfs.at(m), n_terms, n_post, A.loff.at(m), A.ldocs.at(m), A.ltfs.at(m),
                                          uint32_t(n_lists), cap_lists, doc_base, n_documents, A.dl.at(m), A.qoff.at(m), A.qterms.at(m), A.qweights.at(m),
                                          A.qoccurs.at(m), n_queries, n_clauses, k1, b_param, avgdl, k, places, A.hit_docs.at(m), A.hit_scores.at(m),
                                          A.hit_counts.at(m), A.match_counts.at(m), A.counts.at(m), s));
    VPT_TRY(vpt_batch_sync(b));
    VPT_HIP(hipMemcpy(counts_out, A.counts.at(m), 24, hipMemcpyDeviceToHost));
    counts_out[2] += skipped_phrases;
    VPT_HIP(hipMemcpy(hit_counts_out, A.hit_counts.at(m), 4 * size_t(n_queries), hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(match_counts_out, A.match_counts.at(m), 8 * size_t(n_queries), hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(hit_docs_out, A.hit_docs.at(m), 4 * A.n_out, hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(hit_scores_out, A.hit_scores.at(m), 4 * A.n_out, hipMemcpyDeviceToHost));
    return VPT_OK;
}
}  // namespace

vpt_status vpt_postings_phrase_lists(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                                     const uint64_t* post_first, const uint32_t* post_positions, uint32_t n_terms, uint64_t doc_base,
                                     uint64_t n_documents, const uint64_t* phrase_offsets, const int32_t* phrase_terms, uint32_t n_phrases,
                                     uint64_t* list_offsets_out, uint32_t* list_docs_out, uint32_t* list_tfs_out, uint64_t capacity_lists,
                                     uint64_t* counts_out) {
    return phrase_lists_host(p, term_offsets, post_docs, post_tfs, post_first, post_positions, n_terms, doc_base, n_documents, phrase_offsets,
                             phrase_terms, false, nullptr, n_phrases, list_offsets_out, list_docs_out, list_tfs_out, capacity_lists, counts_out);
}

vpt_status vpt_postings_sloppy_phrase_lists(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                                            const uint64_t* post_first, const uint32_t* post_positions, uint32_t n_terms, uint64_t doc_base,
                                            uint64_t n_documents, const uint64_t* phrase_offsets, const int32_t* phrase_terms,
                                            const uint32_t* phrase_slops, uint32_t n_phrases, uint64_t* list_offsets_out, uint32_t* list_docs_out,
                                            uint32_t* list_tfs_out, uint64_t capacity_lists, uint64_t* counts_out) {
    return phrase_lists_host(p, term_offsets, post_docs, post_tfs, post_first, post_positions, n_terms, doc_base, n_documents, phrase_offsets,
                             phrase_terms, true, phrase_slops, n_phrases, list_offsets_out, list_docs_out, list_tfs_out, capacity_lists, counts_out);
}

vpt_status vpt_postings_clause_search(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                                      const uint64_t* post_first, const uint32_t* post_positions, uint32_t n_terms, uint64_t doc_base,
                                      uint64_t n_documents, const uint32_t* doc_lens, const uint64_t* query_offsets, const uint64_t* clause_offsets,
                                      const int32_t* clause_terms, const float* clause_weights, const uint8_t* clause_occurs, uint32_t n_queries,
                                      float k1, float b_param, float avgdl, uint32_t k, uint32_t* hit_docs_out, float* hit_scores_out,
                                      uint32_t* hit_counts_out, uint64_t* match_counts_out, uint64_t* counts_out) {
    return clause_search_host(p, term_offsets, post_docs, post_tfs, post_first, post_positions, n_terms, doc_base, n_documents, doc_lens, query_offsets,
                              clause_offsets, clause_terms, clause_weights, clause_occurs, false, nullptr, n_queries, k1, b_param, avgdl, k, hit_docs_out,
                              hit_scores_out, hit_counts_out, match_counts_out, counts_out);
}

vpt_status vpt_postings_sloppy_clause_search(const vpt_predictor* p, const uint64_t* term_offsets, const uint32_t* post_docs, const uint32_t* post_tfs,
                                             const uint64_t* post_first, const uint32_t* post_positions, uint32_t n_terms, uint64_t doc_base,
                                             uint64_t n_documents, const uint32_t* doc_lens, const uint64_t* query_offsets,
                                             const uint64_t* clause_offsets, const int32_t* clause_terms, const float* clause_weights,
                                             const uint8_t* clause_occurs, const uint32_t* clause_slops, uint32_t n_queries, float k1, float b_param,
                                             float avgdl, uint32_t k, uint32_t* hit_docs_out, float* hit_scores_out, uint32_t* hit_counts_out,
                                             uint64_t* match_counts_out, uint64_t* counts_out) {
    return clause_search_host(p, term_offsets, post_docs, post_tfs, post_first, post_positions, n_terms, doc_base, n_documents, doc_lens, query_offsets,
                              clause_offsets, clause_terms, clause_weights, clause_occurs, true, clause_slops, n_queries, k1, b_param, avgdl, k,
                              hit_docs_out, hit_scores_out, hit_counts_out, match_counts_out, counts_out);
}

// ---- pinned host memory for callers that want the PCIe link at full rate
vpt_status vpt_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: out: must not be NULL");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(VPT_RUNTIME_ERROR, "no HIP device available (this library has no CPU fallback)");
    VPT_HIP(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return VPT_OK;
}
void vpt_host_free(void* ptr) { if (ptr) (void)hipHostFree(ptr); }

// Contiguous sentence ranges with about the same number of CHARACTERS each (what the scoring costs; a sentence of n chars
// has out_offsets[i+1] - out_offsets[i] + 1 of them): bounds[r] .. bounds[r+1] is shard r.
vpt_status vpt_shard_bounds(const uint64_t* out_offsets, size_t n_sentences, size_t n_shards, uint64_t* bounds) {
    if (!out_offsets || !bounds || n_shards == 0) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument or n_shards = 0");
    const uint64_t base = out_offsets[0];
    auto chars_before = [&](size_t i) { return out_offsets[i] - base + i; };
    const uint64_t total = chars_before(n_sentences);
    bounds[0] = 0;
    for (size_t r = 1; r < n_shards; ++r) {
        const uint64_t target = (unsigned __int128)(total) * r / n_shards;
        size_t lo = size_t(bounds[r - 1]), hi = n_sentences;      // first sentence with chars_before >= target
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (chars_before(mid) >= target) hi = mid; else lo = mid + 1;
        }
        bounds[r] = lo;
    }
    bounds[n_shards] = n_sentences;
    return VPT_OK;
}

// Predictor::predict over one batch on SEVERAL GPUs: shard r (vpt_shard_bounds) is scored by preds[r] -- normally
// vpt_predictor_clone_to_device copies of one predictor, one per GPU of the node -- on a host thread of its own through the
// pipelined host-buffer path, straight into its slice of the caller's outputs.  No exchange between the devices.
vpt_status vpt_predict_batch_sharded(const vpt_predictor* const* preds, size_t n_preds, const uint8_t* utf8, const uint64_t* byte_offsets,
                                     size_t n_sentences, int32_t* scores_out, uint8_t* labels_out, const uint64_t* out_offsets, unsigned flags) {
    if (!preds || n_preds == 0) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: preds: must name at least one predictor");
    for (size_t r = 0; r < n_preds; ++r)
        if (!preds[r]) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (n_sentences == 0) return VPT_OK;
    if (!utf8 || !byte_offsets || !out_offsets) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (n_preds == 1) return vpt_predict_batch_flags(preds[0], utf8, byte_offsets, n_sentences, scores_out, labels_out, out_offsets, flags);
    std::vector<uint64_t> bounds(n_preds + 1);
    vpt_status st = vpt_shard_bounds(out_offsets, n_sentences, n_preds, bounds.data());
    if (st != VPT_OK) return st;
    std::vector<vpt_status> rc(n_preds, VPT_OK);
    std::vector<std::string> msg(n_preds);
    std::vector<std::thread> th;
    for (size_t r = 0; r < n_preds; ++r)
        th.emplace_back([&, r] {
            const size_t a = size_t(bounds[r]), n = size_t(bounds[r + 1] - bounds[r]);
            if (n == 0) return;
            // the offsets stay absolute: shard r reads utf8[byte_offsets[a] ..) and writes scores_out[out_offsets[a] ..)
            rc[r] = vpt_predict_batch_flags(preds[r], utf8, byte_offsets + a, n, scores_out, labels_out, out_offsets + a, flags);
            if (rc[r] != VPT_OK) msg[r] = vpt_g_last_error;   // thread-local: carried back to the caller's thread
        });
    for (std::thread& t : th) t.join();
    for (size_t r = 0; r < n_preds; ++r)
        if (rc[r] != VPT_OK) return fail(rc[r], msg[r]);
    return VPT_OK;
}

vpt_status vpt_char_types_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences,
                                const uint64_t* out_offsets, unsigned flags, uint8_t* types_out) {
    if (flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bit");
    if (!p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: predictor: must not be NULL");
    if (n_sentences == 0) return VPT_OK;
    if (!utf8 || !byte_offsets || !out_offsets || !types_out) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    VPT_HIP(hipSetDevice(p->device));
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    vpt_batch* b = w.b;
    uint64_t total_b = 0;
    if ((st = stage(b, utf8, byte_offsets, out_offsets, n_sentences, nullptr, &total_b, nullptr, nullptr)) != VPT_OK) return st;
    const size_t total_c = size_t(total_b) + n_sentences;
    if ((st = b->d_types.grow(total_c + 16)) != VPT_OK) return st;
    b->flags = flags;
    if ((st = vpt_char_types_batch_device(p, b, b->d_text, b->d_boff, b->d_ooff, n_sentences, total_b, b->d_types, b->own_stream)) != VPT_OK) return st;
    if ((st = vpt_batch_sync(b)) != VPT_OK) return st;
    VPT_HIP(hipMemcpy(types_out + size_t(out_offsets[0]) + 0, b->d_types, total_c, hipMemcpyDeviceToHost));
    return VPT_OK;
}

vpt_status vpt_predict_one(const vpt_predictor* p, const uint8_t* utf8, size_t len, int32_t* scores, uint8_t* labels, size_t* n_boundaries) {
    uint64_t boff[2] = {0, uint64_t(len)}, ooff[2] = {0, 0};
    if (len == 0) return cut_fail(vptcut::CutError::kEmptySentence);
    vpt_status st = vpt_count_boundaries(utf8, boff, 1, ooff);
    if (st != VPT_OK) return st;
    if (n_boundaries) *n_boundaries = size_t(ooff[1]);
    return vpt_predict_batch(p, utf8, boff, 1, scores, labels, ooff);
}
