// C ABI of libvaporetto_hip.so, annotated text: Sentence::from_tokenized for a batch (sentence.rs:285-400) on the host and on the device,
// Sentence::from_partial_annotation and write_partial_annotation_text likewise (sentence.rs:516-631, 907-944), and the
// counters of the `evaluate` CLI (evaluate/src/main.rs:91-193) -- the compare kernel alone, and the whole pipeline over host lines.
#include "capi_internal.hpp"

namespace {

// One line of parse_tokenized (sentence.rs:285-400), byte by byte; appends to the outputs.  Returns 0 or the kParseErr* reason.
struct HostParseOut {
    uint8_t *raw, *labels, *tag_bytes;
    uint64_t *tag_index, *span_off;
    uint64_t n_raw = 0, n_labels = 0, n_chars = 0, n_tags = 0, n_tb = 0;
    std::string offender;   // parse_partial_line_host: the code point an invalid-boundary-character error names
};
uint32_t parse_line_host(const uint8_t* t, uint64_t len, HostParseOut& o, uint32_t* n_tags_out) {
    if (len == 0) return vpt::kParseErrNoChar;
    bool escape = false, prev_boundary = false, in_tag = false;
    uint64_t chars = 0;
    uint32_t slot = 0, n_tags = 0;
    for (uint64_t k = 0; k < len; ++k) {
        const uint8_t c = t[k];
        if (!escape && c == '\\') { escape = true; continue; }
        if (!escape && c == ' ') {
            if (chars == 0) return vpt::kParseErrStartSpace;
            if (prev_boundary) return vpt::kParseErrDoubleSpace;
            in_tag = false;
            prev_boundary = true;
            continue;
        }
        if (!escape && c == '/') {
            if (chars == 0 || prev_boundary) return vpt::kParseErrSlash;
            in_tag = true;
            o.span_off[o.n_tags++] = o.n_tb;
            n_tags = std::max(n_tags, ++slot);
            continue;
        }
        escape = false;
        if (c == 0) return vpt::kParseErrNul;
        if (in_tag) { o.tag_bytes[o.n_tb++] = c; continue; }
        if ((c & 0xC0u) != 0x80u) {   // a new char
            if (chars) o.labels[o.n_labels++] = prev_boundary ? VPT_WORD_BOUNDARY : VPT_NOT_WORD_BOUNDARY;
            o.tag_index[o.n_chars++] = o.n_tags;
            ++chars;
            slot = 0;
        }
        prev_boundary = false;
        o.raw[o.n_raw++] = c;
    }
    if (prev_boundary) return vpt::kParseErrEndSpace;
    if (chars == 0) return vpt::kParseErrNoChar;   // (the reference divides by zero here, sentence.rs:450)
    *n_tags_out = n_tags;
    return 0;
}

// One line of parse_partial_annotation (sentence.rs:516-631), code point by code point (a lead byte and the continuation bytes behind it); appends
// to the outputs.  Returns 0 or the kPartialErr* reason.
uint32_t parse_partial_line_host(const uint8_t* t, uint64_t len, HostParseOut& o, uint32_t* n_tags_out) {
    if (len == 0) return vpt::kPartialErrNoChar;
    bool escape = false, is_char = true, in_tag = false;
    uint64_t chars = 0;
    uint32_t slot = 0, n_tags = 0;
    for (uint64_t k = 0; k < len;) {
        const uint64_t k0 = k++;
        while (k < len && (t[k] & 0xC0u) == 0x80u) ++k;
        const uint8_t c = t[k0];
        if (is_char) {
            if (c == 0) return vpt::kPartialErrNul;
            if (chars) ++o.n_labels;   // (its label was stored by the mark in front of it)
            o.tag_index[o.n_chars++] = o.n_tags;
            ++chars;
            slot = 0;
            for (uint64_t q = k0; q < k; ++q) o.raw[o.n_raw++] = t[q];
            is_char = false;
            continue;
        }
        if (!escape && c == '\\') { escape = true; continue; }
        if (!escape && (c == ' ' || c == '-' || c == '|')) {
            o.labels[o.n_labels] = c == '-' ? VPT_NOT_WORD_BOUNDARY : c == '|' ? VPT_WORD_BOUNDARY : VPT_BOUNDARY_UNKNOWN;
            in_tag = false;
            is_char = true;
            continue;
        }
        if (!escape && c == '/') {
            in_tag = true;
            o.span_off[o.n_tags++] = o.n_tb;
            n_tags = std::max(n_tags, ++slot);
            continue;
        }
        escape = false;
        if (!in_tag) {
            o.offender.assign(reinterpret_cast<const char*>(t + k0), size_t(k - k0));
            return vpt::kPartialErrChar;
        }
        for (uint64_t q = k0; q < k; ++q) o.tag_bytes[o.n_tb++] = t[q];
    }
    if (is_char) return vpt::kPartialErrEnd;
    *n_tags_out = n_tags;
    return 0;
}

// One line of write_partial_annotation_text (sentence.rs:907-944); returns the bytes it takes, written to out (when given) up to `cap`.
struct HostPartialIn {
    const uint8_t *text, *labels, *tag_bytes;
    const uint64_t *tag_index, *span_off;
};
uint64_t write_partial_line_host(const HostPartialIn& in, uint64_t t0, uint64_t t1, uint64_t b0, uint64_t g0, uint8_t* out, uint64_t at, uint64_t cap) {
    uint64_t k = at, ci = 0;
    auto put = [&](uint8_t c) { if (out && k < cap) out[k] = c; ++k; };
    auto suffix = [&](uint64_t g) {
        if (!in.tag_index) return;
        const uint64_t a = in.tag_index[g];
        uint64_t e = in.tag_index[g + 1];
        while (e > a && in.span_off[e] == in.span_off[e - 1]) --e;   // up to the last Some
        for (uint64_t t = a; t < e; ++t) {
            put('/');
            for (uint64_t q = in.span_off[t]; q < in.span_off[t + 1]; ++q) put(in.tag_bytes[q]);
        }
    };
    for (uint64_t q = t0; q < t1; ++q) {
        const uint8_t c = in.text[q];
        if ((c & 0xC0u) != 0x80u) {
            if (ci) {
                suffix(g0 + ci - 1);
                const uint8_t lab = in.labels[b0 + ci - 1];
                put(lab == VPT_NOT_WORD_BOUNDARY ? '-' : lab == VPT_WORD_BOUNDARY ? '|' : ' ');
            }
            ++ci;
        }
        put(c);
    }
    suffix(g0 + ci - 1);
    return k - at;
}

// The host parsers' batch: the argument checks, the lines one after the other, the CSR arrays' last entries.  parse_line: one of the two above;
// fail_line(reason, outputs, line): the reason it returned as the call's status and message.
template <class ParseLine, class FailLine>
vpt_status parse_batch_host(const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, uint8_t* raw_out, uint64_t* raw_offsets_out,
                            uint64_t* out_offsets_out, uint8_t* labels_out, uint32_t* n_tags_out, uint64_t* tag_index_out,
                            uint64_t* span_offsets_out, uint8_t* tag_bytes_out, ParseLine parse_line, FailLine fail_line) {
    if (!byte_offsets || !raw_offsets_out || !out_offsets_out || !tag_index_out || !span_offsets_out ||
        (n_sentences && (!utf8 || !raw_out || !labels_out || !n_tags_out || !tag_bytes_out)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    HostParseOut o{raw_out, labels_out, tag_bytes_out, tag_index_out, span_offsets_out};
    raw_offsets_out[0] = 0; out_offsets_out[0] = 0;
    for (size_t i = 0; i < n_sentences; ++i) {
        if (byte_offsets[i + 1] < byte_offsets[i]) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: byte_offsets: must be non-decreasing");
        const uint32_t r = parse_line(utf8 + byte_offsets[i], byte_offsets[i + 1] - byte_offsets[i], o, n_tags_out + i);
        if (r) return fail_line(r, o, i);
        raw_offsets_out[i + 1] = o.n_raw;
        out_offsets_out[i + 1] = o.n_labels;
    }
    tag_index_out[o.n_chars] = o.n_tags;
    span_offsets_out[o.n_tags] = o.n_tb;
    return VPT_OK;
}

vpt_status parse_device_impl(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets, size_t n_sentences,
                             uint64_t capacity, uint8_t* d_raw_out, uint64_t* d_raw_offsets_out, uint64_t* d_out_offsets_out, uint8_t* d_labels_out,
                             uint32_t* d_n_tags_out, uint64_t* d_tag_index_out, uint64_t* d_span_offsets_out, uint8_t* d_tag_bytes_out,
                             hipStream_t stream, vpt::ParseKind kind) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (n_sentences >= 0xFFFFFFFFull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: n_sentences: at most 2^32-2 per call");
    if (!d_raw_offsets_out || !d_out_offsets_out || !d_tag_index_out || !d_span_offsets_out ||
        (n_sentences && (!d_utf8 || !d_byte_offsets || !d_raw_out || !d_labels_out || !d_n_tags_out || !d_tag_bytes_out)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    VPT_HIP(hipSetDevice(p->device));
    if (n_sentences == 0) {
        VPT_HIP(hipMemsetAsync(d_raw_offsets_out, 0, sizeof(uint64_t), stream));
        VPT_HIP(hipMemsetAsync(d_out_offsets_out, 0, sizeof(uint64_t), stream));
        VPT_HIP(hipMemsetAsync(d_tag_index_out, 0, sizeof(uint64_t), stream));
        VPT_HIP(hipMemsetAsync(d_span_offsets_out, 0, sizeof(uint64_t), stream));
        return VPT_OK;
    }
    vpt_status st;
    if ((st = b->d_parse_tmp.grow(2 * (n_sentences + 1))) != VPT_OK) return st;
    if ((st = b->d_scan_part.grow(vpt::scan_part_entries(n_sentences))) != VPT_OK) return st;
    vpt::ParseParams P{};
    P.text = d_utf8; P.boff = d_byte_offsets; P.n_sent = n_sentences;
    P.raw = d_raw_out; P.raw_cap = capacity; P.raw_off = d_raw_offsets_out; P.ooff = d_out_offsets_out;
    P.labels = d_labels_out; P.label_cap = capacity; P.n_tags = d_n_tags_out;
    P.tag_index = d_tag_index_out; P.index_cap = capacity + 1; P.span_off = d_span_offsets_out; P.span_cap = capacity + 1;
    P.tag_bytes = d_tag_bytes_out; P.tb_cap = capacity;
    P.tag_off = b->d_parse_tmp; P.tb_off = b->d_parse_tmp + n_sentences + 1;
    P.status = b->d_ctrl;
    VPT_HIP(vpt::launch_parse(kind, P, b->d_scan_part, stream));
    b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
    return VPT_OK;
}

vpt_status evaluate_device_impl(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_out_offsets, size_t n_sentences, const uint8_t* d_gold_labels,
                                const uint32_t* d_n_tags, const uint64_t* d_tag_index, const uint64_t* d_span_offsets, const uint8_t* d_tag_bytes,
                                const uint8_t* d_sys_labels, int sys_tags, uint64_t* d_counts, hipStream_t stream) {
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (sys_tags < VPT_EVAL_TAGS_NONE || sys_tags > VPT_EVAL_TAGS_PREDICTED) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: sys_tags: not a VPT_EVAL_TAGS_* value");
    if (n_sentences == 0) return VPT_OK;
    if (!d_out_offsets || !d_gold_labels || !d_sys_labels || !d_counts || (sys_tags != VPT_EVAL_TAGS_GOLD && !d_n_tags) ||
        (sys_tags == VPT_EVAL_TAGS_PREDICTED && (!d_tag_index || !d_span_offsets || !d_tag_bytes)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    if (sys_tags == VPT_EVAL_TAGS_PREDICTED && !p->predict_tags)
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    VPT_HIP(hipSetDevice(p->device));
    vpt::EvalParams E{};
    E.gold = d_gold_labels; E.sys = d_sys_labels; E.ooff = d_out_offsets; E.n_sent = n_sentences;
    E.gold_n_tags = d_n_tags; E.tag_index = d_tag_index; E.span_off = d_span_offsets; E.tag_bytes = d_tag_bytes;
    E.mode = uint32_t(sys_tags);
    E.counts = d_counts;
    if (sys_tags == VPT_EVAL_TAGS_PREDICTED) {
        // fill_tags' own records (the evaluate CLI runs no PatternMatchTagger), of a batch of as many sentences: the boundaries are not known here
        if (!p->n_tags) E.mode = vpt::kEvalTagsNone;   // predict_tags returns early without tag models (predictor.rs:553-555): every vector empty
        else if (const vpt_status st = tag_records_for(b, n_sentences, kBoundariesUnknown, false, &E.sys_tags); st != VPT_OK) return st;
    }
    VPT_HIP(vpt::launch_evaluate(E, stream));
    b->last_stream = stream; b->pending = true;
    return VPT_OK;
}

// vpt_evaluate_batch's device buffers for a chunk of `bytes` text bytes and `n` lines, carved out of one allocation
struct EvalLayout {
    uint8_t *text, *raw, *gold, *sys, *tag_bytes;
    uint64_t *boff, *raw_off, *ooff, *tag_index, *span_off, *counts;
    uint32_t* n_tags;
};
size_t eval_layout(unsigned char* base, uint64_t bytes, uint64_t n, EvalLayout* L) {
    size_t at = 0;
    auto take = [&](uint64_t nbytes) { unsigned char* q = base ? base + at : nullptr; at += size_t((nbytes + 255) & ~uint64_t(255)); return q; };
    L->counts = reinterpret_cast<uint64_t*>(take(8 * vpt::kEvalCounts));
    L->text = take(bytes + 16);
    L->boff = reinterpret_cast<uint64_t*>(take(8 * (n + 1)));
    L->raw = take(bytes + 16);
    L->raw_off = reinterpret_cast<uint64_t*>(take(8 * (n + 1)));
    L->ooff = reinterpret_cast<uint64_t*>(take(8 * (n + 1)));
    L->gold = take(bytes + 16);
    L->sys = take(bytes + 16);
    L->n_tags = reinterpret_cast<uint32_t*>(take(4 * n));
    L->tag_index = reinterpret_cast<uint64_t*>(take(8 * (bytes + 1)));
    L->span_off = reinterpret_cast<uint64_t*>(take(8 * (bytes + 1)));
    L->tag_bytes = take(bytes + 16);
    return at;
}

}  // namespace

vpt_status vpt_parse_tokenized_batch(const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, uint8_t* raw_out,
                                     uint64_t* raw_offsets_out, uint64_t* out_offsets_out, uint8_t* labels_out, uint32_t* n_tags_out,
                                     uint64_t* tag_index_out, uint64_t* span_offsets_out, uint8_t* tag_bytes_out) {
    return parse_batch_host(utf8, byte_offsets, n_sentences, raw_out, raw_offsets_out, out_offsets_out, labels_out, n_tags_out, tag_index_out,
                            span_offsets_out, tag_bytes_out, parse_line_host,
                            [](uint32_t reason, const HostParseOut&, uint64_t line) { return parse_fail(reason, line); });
}

vpt_status vpt_parse_tokenized_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                            size_t n_sentences, uint64_t capacity, uint8_t* d_raw_out, uint64_t* d_raw_offsets_out,
                                            uint64_t* d_out_offsets_out, uint8_t* d_labels_out, uint32_t* d_n_tags_out, uint64_t* d_tag_index_out,
                                            uint64_t* d_span_offsets_out, uint8_t* d_tag_bytes_out, void* hip_stream) {
    return parse_device_impl(p, b, d_utf8, d_byte_offsets, n_sentences, capacity, d_raw_out, d_raw_offsets_out, d_out_offsets_out, d_labels_out,
                             d_n_tags_out, d_tag_index_out, d_span_offsets_out, d_tag_bytes_out, static_cast<hipStream_t>(hip_stream),
                             vpt::ParseKind::kTokenized);
}

vpt_status vpt_parse_partial_batch(const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, uint8_t* raw_out,
                                   uint64_t* raw_offsets_out, uint64_t* out_offsets_out, uint8_t* labels_out, uint32_t* n_tags_out,
                                   uint64_t* tag_index_out, uint64_t* span_offsets_out, uint8_t* tag_bytes_out) {
    return parse_batch_host(utf8, byte_offsets, n_sentences, raw_out, raw_offsets_out, out_offsets_out, labels_out, n_tags_out, tag_index_out,
                            span_offsets_out, tag_bytes_out, parse_partial_line_host,
                            [](uint32_t reason, const HostParseOut& o, uint64_t line) { return partial_fail(reason, o.offender, line); });
}

vpt_status vpt_parse_partial_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                          size_t n_sentences, uint64_t capacity, uint8_t* d_raw_out, uint64_t* d_raw_offsets_out,
                                          uint64_t* d_out_offsets_out, uint8_t* d_labels_out, uint32_t* d_n_tags_out, uint64_t* d_tag_index_out,
                                          uint64_t* d_span_offsets_out, uint8_t* d_tag_bytes_out, void* hip_stream) {
    return parse_device_impl(p, b, d_utf8, d_byte_offsets, n_sentences, capacity, d_raw_out, d_raw_offsets_out, d_out_offsets_out, d_labels_out,
                             d_n_tags_out, d_tag_index_out, d_span_offsets_out, d_tag_bytes_out, static_cast<hipStream_t>(hip_stream),
                             vpt::ParseKind::kPartial);
}

vpt_status vpt_write_partial_batch(const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, const uint64_t* out_offsets,
                                   const uint8_t* labels, const uint32_t* n_tags, const uint64_t* tag_index, const uint64_t* span_offsets,
                                   const uint8_t* tag_bytes, uint8_t* text_out, uint64_t text_capacity, uint64_t* text_offsets_out) {
    if (!byte_offsets || !out_offsets || !text_offsets_out || (n_sentences && (!utf8 || !text_out)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if (n_tags && (!tag_index || !span_offsets)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: n_tags without the tag arrays");
    const HostPartialIn in{utf8, labels, tag_bytes, n_tags ? tag_index : nullptr, span_offsets};
    text_offsets_out[0] = 0;
    uint64_t at = 0;
    for (size_t i = 0; i < n_sentences; ++i) {
        if (byte_offsets[i + 1] < byte_offsets[i]) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: byte_offsets: must be non-decreasing");
        if (byte_offsets[i + 1] == byte_offsets[i]) return status_from_bits(vpt::kErrEmptySentence);
        uint64_t chars = 0;
        for (uint64_t q = byte_offsets[i]; q < byte_offsets[i + 1]; ++q) chars += (utf8[q] & 0xC0u) != 0x80u;
        if (out_offsets[i + 1] < out_offsets[i] || chars != out_offsets[i + 1] - out_offsets[i] + 1) return status_from_bits(vpt::kErrBadOffsets);
        if (chars > 1 && !labels) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
        for (uint64_t q = out_offsets[i]; q < out_offsets[i + 1]; ++q)
            if (labels[q] > VPT_BOUNDARY_UNKNOWN) return status_from_bits(vpt::kErrBadLabel);
        at += write_partial_line_host(in, byte_offsets[i], byte_offsets[i + 1], out_offsets[i], out_offsets[i] + i, text_out, at, text_capacity);
        text_offsets_out[i + 1] = at;
    }
    return at > text_capacity ? status_from_bits(vpt::kErrOutputTooSmall) : VPT_OK;
}

vpt_status vpt_write_partial_batch_device(const vpt_predictor* p, vpt_batch* b, const uint8_t* d_utf8, const uint64_t* d_byte_offsets,
                                          size_t n_sentences, const uint64_t* d_out_offsets, const uint8_t* d_labels, const uint32_t* d_n_tags,
                                          const uint64_t* d_tag_index, const uint64_t* d_span_offsets, const uint8_t* d_tag_bytes,
                                          uint8_t* d_text_out, uint64_t text_capacity, uint64_t* d_text_offsets_out, void* hip_stream) {
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (!p || !b || b->pred != p) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: batch: does not belong to this predictor");
    if (n_sentences >= 0xFFFFFFFFull) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: n_sentences: at most 2^32-2 per call");
    if (!d_text_offsets_out || (n_sentences && (!d_utf8 || !d_byte_offsets || !d_out_offsets || !d_labels || !d_text_out)))
        return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL device pointer");
    if (d_n_tags && (!d_tag_index || !d_span_offsets || !d_tag_bytes)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: n_tags without the tag arrays");
    VPT_HIP(hipSetDevice(p->device));
    if (n_sentences == 0) {
        VPT_HIP(hipMemsetAsync(d_text_offsets_out, 0, sizeof(uint64_t), stream));
        return VPT_OK;
    }
    vpt_status st;
    if ((st = b->d_scan_part.grow(vpt::scan_part_entries(n_sentences))) != VPT_OK) return st;
    vpt::WritePartialParams W{};
    W.text = d_utf8; W.boff = d_byte_offsets; W.ooff = d_out_offsets; W.n_sent = n_sentences; W.labels = d_labels;
    W.tag_index = d_n_tags ? d_tag_index : nullptr; W.span_off = d_span_offsets; W.tag_bytes = d_tag_bytes;
    W.out = d_text_out; W.capacity = text_capacity; W.out_off = d_text_offsets_out; W.status = b->d_ctrl;
    VPT_HIP(vpt::launch_write_partial(W, b->d_scan_part, stream));
    b->last_stream = stream; b->pending = true; b->cps_text = nullptr;
    return VPT_OK;
}

vpt_status vpt_evaluate_labels_batch_device(const vpt_predictor* p, vpt_batch* b, const uint64_t* d_out_offsets, size_t n_sentences,
                                            const uint8_t* d_gold_labels, const uint32_t* d_n_tags, const uint64_t* d_tag_index,
                                            const uint64_t* d_span_offsets, const uint8_t* d_tag_bytes, const uint8_t* d_sys_labels, int sys_tags,
                                            uint64_t* d_counts, void* hip_stream) {
    return evaluate_device_impl(p, b, d_out_offsets, n_sentences, d_gold_labels, d_n_tags, d_tag_index, d_span_offsets, d_tag_bytes, d_sys_labels,
                                sys_tags, d_counts, static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_evaluate_batch(const vpt_predictor* p, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, unsigned flags,
                              int predict_tags, uint64_t* counts_out) {
    if (!p || !byte_offsets || !counts_out || (n_sentences && !utf8)) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: NULL argument");
    if ((flags & ~unsigned(VPT_FLAG_ALL | VPT_FLAG_CONCAT_GRAPHEMES)) != 0) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: flags: unknown bits");
    if (predict_tags && !p->predict_tags) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: this predictor is created with predict_tags = false");
    for (size_t i = 0; i < n_sentences; ++i)
        if (byte_offsets[i + 1] < byte_offsets[i]) return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: byte_offsets: must be non-decreasing");
    std::memset(counts_out, 0, 8 * vpt::kEvalCounts);
    if (n_sentences == 0) return VPT_OK;
    // the system's tag vectors (evaluate/src/main.rs:103-121): fill_tags' when it runs, else what the sentence predicted holds -- from_raw's
    // none after the normalisation, the gold ones without it
    const int mode = predict_tags && p->n_tags ? VPT_EVAL_TAGS_PREDICTED : (flags & VPT_FLAG_KYTEA_FULLWIDTH) ? VPT_EVAL_TAGS_NONE : VPT_EVAL_TAGS_GOLD;
    Workspace w;
    vpt_status st = acquire(p, &w);
    if (st != VPT_OK) return st;
    vpt_batch* b = w.b;
    hipStream_t s = b->own_stream;
    VPT_HIP(hipSetDevice(p->device));
    const unsigned saved_flags = b->flags;
    struct Restore { vpt_batch* b; unsigned f; ~Restore() { b->flags = f; } } restore{b, saved_flags};
    b->flags = flags;
    // a pooled workspace may still hold the longest-sentence hint of an earlier host call (capi_host.cpp): the lines here are others
    const uint64_t saved_max_chars = b->max_chars;
    struct RestoreChars { vpt_batch* b; uint64_t v; ~RestoreChars() { b->max_chars = v; } } restore_chars{b, saved_max_chars};
    b->max_chars = 0;
    // chunks of whole lines of about eval_chunk_bytes (a longer line is a chunk of its own), one after the other on the workspace's stream;
    // the counters add up on the device
    const uint64_t budget = std::max<uint64_t>(p->knobs.eval_chunk_bytes, 1);
    uint64_t max_bytes = 0, max_lines = 0;
    for (size_t i0 = 0; i0 < n_sentences;) {
        size_t i1 = i0 + 1;
        while (i1 < n_sentences && byte_offsets[i1 + 1] - byte_offsets[i0] <= budget) ++i1;
        max_bytes = std::max<uint64_t>(max_bytes, byte_offsets[i1] - byte_offsets[i0]);
        max_lines = std::max<uint64_t>(max_lines, i1 - i0);
        i0 = i1;
    }
    EvalLayout L{};
    if ((st = b->d_eval.grow(eval_layout(nullptr, max_bytes, max_lines, &L))) != VPT_OK) return st;
    eval_layout(b->d_eval, max_bytes, max_lines, &L);
    VPT_HIP(hipMemsetAsync(L.counts, 0, 8 * vpt::kEvalCounts, s));
    std::vector<uint64_t>& boff = b->h_boff;
    for (size_t i0 = 0; i0 < n_sentences;) {
        size_t i1 = i0 + 1;
        while (i1 < n_sentences && byte_offsets[i1 + 1] - byte_offsets[i0] <= budget) ++i1;
        const size_t n = i1 - i0;
        const uint64_t t0 = byte_offsets[i0], nbytes = byte_offsets[i1] - t0;
        uint64_t longest = 0;
        boff.resize(n + 1);
        for (size_t i = 0; i <= n; ++i) {
            boff[i] = byte_offsets[i0 + i] - t0;
            if (i) longest = std::max<uint64_t>(longest, boff[i] - boff[i - 1]);
        }
        VPT_HIP(hipMemcpyAsync(L.text, utf8 + t0, size_t(nbytes), hipMemcpyHostToDevice, s));
        VPT_HIP(hipMemcpyAsync(L.boff, boff.data(), 8 * (n + 1), hipMemcpyHostToDevice, s));
        if ((st = parse_device_impl(p, b, L.text, L.boff, n, nbytes, L.raw, L.raw_off, L.ooff, L.gold, L.n_tags, L.tag_index, L.span_off,
                                    L.tag_bytes, s, vpt::ParseKind::kTokenized)) != VPT_OK)
            return st;
        // the parse's verdict before anything runs on what it wrote (a rejected line leaves no text to score), and the boundary total
        uint32_t ctrl[16] = {};
        uint64_t total_b = 0;
        VPT_HIP(hipMemcpyAsync(ctrl, b->d_ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, s));
        VPT_HIP(hipMemcpyAsync(&total_b, L.ooff + n, sizeof(total_b), hipMemcpyDeviceToHost, s));
        VPT_HIP(hipStreamSynchronize(s));
        b->pending = false;
        if (ctrl[0]) {
            VPT_HIP(hipMemset(b->d_ctrl, 0, 16 * sizeof(uint32_t)));
            return (ctrl[0] & vpt::kErrParse) ? parse_status(ctrl, i0) : status_from_bits(ctrl[0]);
        }
        if ((st = predict_device_impl(p, b, L.raw, L.raw_off, L.ooff, n, total_b, longest, nullptr, L.sys, s)) != VPT_OK) return st;
        if (mode == VPT_EVAL_TAGS_PREDICTED &&
            (st = vpt_fill_tags_batch_device(p, b, L.raw, L.raw_off, L.ooff, n, total_b, L.sys, nullptr, s)) != VPT_OK)
            return st;
        if ((st = evaluate_device_impl(p, b, L.ooff, n, L.gold, L.n_tags, L.tag_index, L.span_off, L.tag_bytes, L.sys, mode, L.counts, s)) != VPT_OK)
            return st;
        i0 = i1;
    }
    VPT_HIP(hipMemcpyAsync(counts_out, L.counts, 8 * vpt::kEvalCounts, hipMemcpyDeviceToHost, s));
    return vpt_batch_sync(b);
}
