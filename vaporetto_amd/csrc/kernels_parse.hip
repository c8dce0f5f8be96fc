// Annotated text in, labels and tags out: Sentence::from_tokenized / parse_tokenized (sentence.rs:285-400) and Sentence::from_partial_annotation
// (sentence.rs:516-631) for a batch, the partial-annotation writer, and the counters of the `evaluate` CLI (evaluate/src/main.rs:91-193).
//
// parse_lines_kernel<Syntax, kWrite>: the frame of both parsers.  A WAVE per line, the line walked in windows of 64 bytes, one byte a lane.  A syntax
// turns a window into each lane's roles (LaneRoles) and carries its own state from window to window; the frame owns the line loop, the counters
// (surface bytes, chars, tags, tag bytes, the largest slot count), the stores and the error report.  kWrite == false counts and reports the first
// error of the line; a chained scan of each count (kernels_emit.hip) places the lines; kWrite == true walks the line again and writes what it counted
// where the scans put it.
//
// TokenizedSyntax: every byte's part in the line is a function of masks over the window (ballots) and of four positions carried from the windows
// before it:
//   escaped      the previous byte is an unescaped '\\' -- the parity of the run of '\\' in front of the byte: the highest non-'\\' lane
//                below it, or the carried escape state when the run reaches the window's start;
//   tag mode     the last unescaped '/' before the byte lies after the last unescaped ' ' (a tag runs to the next unescaped '/' or ' ');
//   WordBoundary the last unescaped ' ' before a surface char lies after the last surface byte before it;
//   slot         the unescaped '/' between a char's last surface byte and the '/' in question (the frame counts them from the syntax's anchor mask).
// The ' ', '/' and '\\' bytes never occur inside a multi-byte UTF-8 sequence, so the byte-level formulation is exact.
//
// PartialSyntax / write_partial_kernel: partially annotated text both ways (Sentence::from_partial_annotation, write_partial_annotation_text;
// sentence.rs:516-631, 907-944), described where they stand.
//
// evaluate_kernel: a wave per sentence over its boundaries, 64 a window.  The char metric is four popcounts.  Nagata's word metric
// (evaluate/src/main.rs:149-191) carries `matched` from boundary to boundary; here it is a segmented scan: at an agreed WordBoundary b the
// flag is "the last disagreement before b lies before the last agreed WordBoundary before b" -- two highest-bit searches per lane.
#include "kernels.hpp"

#include "device_common.h"
#include "layout.h"

namespace vpt {
namespace {

constexpr uint32_t kParseThreads = 256;   // four waves, a line each
constexpr uint32_t kParseMaxBlocks = 8192;

__device__ __forceinline__ uint64_t lanes_below(uint32_t lane) { return (uint64_t(1) << lane) - 1u; }
// lanes 0 .. j (j <= 63: a shift by 64 would be one by 0)
__device__ __forceinline__ uint64_t lanes_upto(uint32_t j) { return j >= 63u ? ~uint64_t(0) : (uint64_t(2) << j) - 1u; }
__device__ __forceinline__ int hi_lane(uint64_t m) { return m ? 63 - __builtin_clzll(m) : -1; }
__device__ __forceinline__ uint32_t popc(uint64_t m) { return uint32_t(__builtin_popcountll(m)); }
// position (relative to the line) of the highest lane of m below `lane`, else `carry`
__device__ __forceinline__ int64_t last_below(uint64_t m, uint32_t lane, int64_t w0, int64_t carry) {
    const int j = hi_lane(m & lanes_below(lane));
    return j >= 0 ? w0 + j : carry;
}
__device__ __forceinline__ int64_t last_in(uint64_t m, int64_t w0, int64_t carry) {
    const int j = hi_lane(m);
    return j >= 0 ? w0 + j : carry;
}

// What a syntax's window step says of its lane.  The masks the frame needs are ballots of these.
struct LaneRoles {
    bool raw, lead, opener, tagb;   // a surface byte, the lead byte of a surface char, a '/' that opens a tag, a tag byte
    bool label;                     // stores the label of the boundary in front of char (chars + leads below): labels[ci - 1]
    uint32_t label_value;
    uint64_t anchorm;               // (the same in every lane) the lanes a '/' counts its slot from: the openers since the highest one below it
    uint32_t err;                   // the reason this lane rejects the line for, or 0
};

// Tokenized text (sentence.rs:285-400): ballots and four carried positions, as the header describes.
struct TokenizedSyntax {
    static constexpr uint32_t kPad = 0x41u, kStatusBit = kErrParse, kErrWord = kParseErrWord;
    struct Carry {
        int64_t last_sp = -1, last_sl = -1, last_surf = -1;   // the last unescaped ' ', unescaped '/' and surface byte
        uint32_t esc = 0;                                     // the window's last byte is an unescaped '\\'
    };
    // the lane's roles; leaves `carry` as the next window finds it
    static __device__ __forceinline__ LaneRoles step(uint32_t c, bool valid, uint32_t lane, int64_t w0, Carry& carry) {
        const uint64_t bs = __ballot(valid && c == '\\');
        // escaped: the run of '\\' right in front of the lane is odd (through the window's start: the carried state)
        const int jn = hi_lane(~bs & lanes_below(lane));
        const uint32_t esc = jn >= 0 ? uint32_t(lane - 1u - uint32_t(jn)) & 1u : (lane & 1u) ^ carry.esc;
        const bool is_sp = valid && c == ' ' && !esc, is_sl = valid && c == '/' && !esc, drop = valid && c == '\\' && !esc;
        const bool content = valid && !is_sp && !is_sl && !drop;
        const uint64_t spm = __ballot(is_sp), slm = __ballot(is_sl);
        const int64_t lsp = last_below(spm, lane, w0, carry.last_sp), lsl = last_below(slm, lane, w0, carry.last_sl);
        const bool in_tag = lsl > lsp;
        const bool surf = content && !in_tag;
        const uint64_t surfm = __ballot(surf);
        const int64_t lsurf = last_below(surfm, lane, w0, carry.last_surf);
        const bool has_surf = lsurf >= 0, prev_boundary = has_surf && lsp > lsurf;
        LaneRoles r;
        r.raw = surf; r.lead = surf && (c & 0xC0u) != 0x80u; r.opener = is_sl; r.tagb = content && in_tag;
        r.label = r.lead; r.label_value = prev_boundary ? 1u : 0u;   // at a char's lead, for the boundary in front of it
        r.anchorm = surfm;                                           // a tag's slot: the '/' since the char's last surface BYTE
        // errors in the order parse_tokenized meets them (sentence.rs:308-354)
        r.err = 0;
        if (valid && c == 0u) r.err = kParseErrNul;
        else if (is_sp && !has_surf) r.err = kParseErrStartSpace;
        else if (is_sp && prev_boundary) r.err = kParseErrDoubleSpace;
        else if (is_sl && (!has_surf || prev_boundary)) r.err = kParseErrSlash;
        carry.esc = uint32_t(__shfl(int(drop ? 1 : 0), 63));
        carry.last_sp = last_in(spm, w0, carry.last_sp);
        carry.last_sl = last_in(slm, w0, carry.last_sl);
        carry.last_surf = last_in(surfm, w0, carry.last_surf);
        return r;
    }
    static __device__ __forceinline__ uint32_t end_error(const Carry& carry, int64_t, uint64_t chars) {
        return carry.last_surf >= 0 && carry.last_sp > carry.last_surf ? kParseErrEndSpace : chars == 0 ? kParseErrNoChar : 0u;
    }
    static __device__ __forceinline__ void first_error(const ParseParams&, uint64_t, uint64_t, int64_t, int64_t, uint32_t, uint32_t) {}
};

// ---- partial annotation
//
// PartialSyntax: Sentence::from_partial_annotation (sentence.rs:516-631).  What a byte IS depends on the whole prefix here -- the code point behind a
// mark is a char whatever it is -- so the window step is a prefix scan of the transition maps of a six-state machine over five input classes:
//   states   E expect-char, A annotation, AE annotation behind a '\\', T tag, TE tag behind a '\\', X error (absorbing)
//   classes  '\\', mark (' ' '-' '|'), '/', NUL, other
// A map is 6 states x 3 bits in one word; a lead-byte lane holds the map of its class, a continuation byte the identity; composing two maps is six
// extracts, the inclusive scan six DPP steps.  The carried entry state applied to a lane's map is its state behind its byte; the lane below (or the
// entry state) gives the state in front of it, and (state in front, class) is the byte's role.  Continuation bytes take the role of their lead.
constexpr uint32_t kStE = 0, kStA = 1, kStAE = 2, kStT = 3, kStTE = 4, kStX = 5;
constexpr uint32_t pmap(uint32_t e, uint32_t a, uint32_t ae, uint32_t t, uint32_t te) {
    return e | (a << 3) | (ae << 6) | (t << 9) | (te << 12) | (kStX << 15);
}
constexpr uint32_t kMapId = pmap(kStE, kStA, kStAE, kStT, kStTE);
constexpr uint32_t kMapBackslash = pmap(kStA, kStAE, kStX, kStTE, kStT);
constexpr uint32_t kMapMark = pmap(kStA, kStE, kStX, kStE, kStT);
constexpr uint32_t kMapSlash = pmap(kStA, kStT, kStX, kStT, kStT);
constexpr uint32_t kMapNul = pmap(kStX, kStX, kStX, kStT, kStT);
constexpr uint32_t kMapOther = pmap(kStA, kStX, kStX, kStT, kStT);
// first f, then g
__device__ __forceinline__ uint32_t map_then(uint32_t f, uint32_t g) {
    uint32_t h = 0;
#pragma unroll
    for (uint32_t s = 0; s < 6; ++s) h |= ((g >> (3u * ((f >> (3u * s)) & 7u))) & 7u) << (3u * s);
    return h;
}
// inclusive scan of the maps over the wave, lane 0 first (the steps of wave_inclusive_scan; a lane without a source composes with the identity)
__device__ __forceinline__ uint32_t wave_map_scan(uint32_t x) {
    x = map_then(uint32_t(__builtin_amdgcn_update_dpp(int(kMapId), int(x), 0x111, 0xF, 0xF, false)), x);  // row_shr:1
    x = map_then(uint32_t(__builtin_amdgcn_update_dpp(int(kMapId), int(x), 0x112, 0xF, 0xF, false)), x);  // row_shr:2
    x = map_then(uint32_t(__builtin_amdgcn_update_dpp(int(kMapId), int(x), 0x114, 0xF, 0xF, false)), x);  // row_shr:4
    x = map_then(uint32_t(__builtin_amdgcn_update_dpp(int(kMapId), int(x), 0x118, 0xF, 0xF, false)), x);  // row_shr:8
    x = map_then(uint32_t(__builtin_amdgcn_update_dpp(int(kMapId), int(x), 0x142, 0xA, 0xF, false)), x);  // row_bcast:15 -> rows 1, 3
    x = map_then(uint32_t(__builtin_amdgcn_update_dpp(int(kMapId), int(x), 0x143, 0xC, 0xF, false)), x);  // row_bcast:31 -> rows 2, 3
    return x;
}

struct PartialSyntax {
    static constexpr uint32_t kPad = 0x80u, kStatusBit = kErrParsePartial, kErrWord = kPartialErrWord;
    struct Carry {
        uint32_t state = kStE, open_role = 0;   // the state behind the window, the role of its last lead byte (0 none, 1 char, 2 tag)
    };
    static __device__ __forceinline__ LaneRoles step(uint32_t c, bool valid, uint32_t lane, int64_t w0, Carry& carry) {
        // (a continuation byte that opens the line has no lead to belong to: it is one)
        const bool lead = valid && ((c & 0xC0u) != 0x80u || w0 + int64_t(lane) == 0);
        const bool is_bs = c == '\\', is_mark = c == ' ' || c == '-' || c == '|', is_sl = c == '/';
        const uint32_t own = !lead ? kMapId : is_bs ? kMapBackslash : is_mark ? kMapMark : is_sl ? kMapSlash : c == 0u ? kMapNul : kMapOther;
        const uint32_t incl = wave_map_scan(own);
        const uint32_t after = (incl >> (3u * carry.state)) & 7u;
        const uint32_t up = __shfl_up(after, 1u);
        const uint32_t before = lane == 0 ? carry.state : up;
        const bool annot = before == kStA || before == kStT;   // where '\\', marks and '/' mean something
        const bool char_lead = lead && before == kStE && c != 0u;
        const bool tag_lead = lead && (before == kStTE || (before == kStT && !is_bs && !is_mark && !is_sl));
        const uint64_t leadm = __ballot(lead), clm = __ballot(char_lead), tlm = __ballot(tag_lead);
        // a continuation byte: the role of the last lead below it
        const int jl = hi_lane(leadm & lanes_below(lane));
        const uint32_t role = lead ? (char_lead ? 1u : tag_lead ? 2u : 0u) : !valid ? 0u : jl >= 0 ? uint32_t((clm >> jl) & 1u) + 2u * uint32_t((tlm >> jl) & 1u) : carry.open_role;
        LaneRoles r;
        r.raw = role == 1u; r.lead = char_lead; r.opener = lead && annot && is_sl; r.tagb = role == 2u;
        r.label = lead && annot && is_mark; r.label_value = c == '-' ? 0u : c == '|' ? 1u : 2u;   // at the mark, for the boundary behind the char in front of it
        r.anchorm = clm;                                                                           // a tag's slot: the openers since the char's LEAD
        // the lane that enters the error state: NUL where a char is expected, else a code point that is no annotation
        r.err = lead && before != kStX && after == kStX ? (before == kStE ? kPartialErrNul : kPartialErrChar) : 0u;
        carry.state = uint32_t(__shfl(int(after), 63));
        if (leadm) {
            const int h = hi_lane(leadm);
            carry.open_role = uint32_t((clm >> h) & 1u) + 2u * uint32_t((tlm >> h) & 1u);
        }
        return r;
    }
    static __device__ __forceinline__ uint32_t end_error(const Carry& carry, int64_t len, uint64_t) {
        return len == 0 ? kPartialErrNoChar : carry.state == kStE ? kPartialErrEnd : 0u;
    }
    // The write pass meets the line's first error at byte `at`.  The count pass has settled which line each reason names: the one kPartialErrChar names
    // leaves its offender's bytes, the lead and the continuation bytes behind it (they may lie in the next window).
    static __device__ __forceinline__ void first_error(const ParseParams& P, uint64_t line, uint64_t start, int64_t len, int64_t at, uint32_t err, uint32_t lane) {
        if (err != kPartialErrChar || P.status[kPartialErrWord + kPartialErrChar] != 0xFFFFFFFFu - uint32_t(line)) return;
        uint32_t bytes = P.text[start + uint64_t(at)];
        for (int64_t k = 1; k < 4 && at + k < len; ++k) {
            const uint32_t b = P.text[start + uint64_t(at + k)];
            if ((b & 0xC0u) != 0x80u) break;
            bytes |= b << (8 * k);
        }
        if (lane == 0) P.status[kPartialErrBytesWord] = bytes;
    }
};

// The frame of both parsers: a wave per line, the line in windows of 64 bytes.  The syntax says what each byte is; the frame counts, places and stores.
template <class Syntax, bool kWrite>
__global__ __launch_bounds__(kParseThreads) void parse_lines_kernel(const ParseParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = lanes_below(lane);
    const uint64_t n_waves = uint64_t(gridDim.x) * (kParseThreads / 64);
    for (uint64_t line = uint64_t(blockIdx.x) * (kParseThreads / 64) + (threadIdx.x >> 6); line < P.n_sent; line += n_waves) {
        const uint64_t start = P.boff[line], end = P.boff[line + 1];
        const int64_t len = end > start ? int64_t(end - start) : 0;
        // bases of the line in the outputs (the write pass; the count pass leaves them at 0)
        uint64_t raw_at = 0, lab_at = 0, char_at = 0, tag_at = 0, tb_at = 0;
        if (kWrite) {
            raw_at = P.raw_off[line];
            lab_at = P.ooff[line];
            char_at = P.ooff[line] + line;
            tag_at = P.tag_off[line];
            tb_at = P.tb_off[line];
        }
        typename Syntax::Carry carry;
        uint32_t open_since_anchor = 0, n_tags = 0;   // the openers behind the last anchor lane; the line's largest slot count
        uint64_t raw = 0, chars = 0, tags = 0, tbytes = 0;
        uint32_t err = 0;   // first error of the line: the syntax's reason
        for (int64_t w0 = 0; w0 < len; w0 += 64) {
            const bool valid = w0 + int64_t(lane) < len;
            const uint32_t c = valid ? P.text[start + uint64_t(w0) + lane] : Syntax::kPad;
            const LaneRoles r = Syntax::step(c, valid, lane, w0, carry);
            const uint64_t rawm = __ballot(r.raw), leadm = __ballot(r.lead), openm = __ballot(r.opener), tagm = __ballot(r.tagb);
            const uint64_t errm = __ballot(r.err != 0);
            if (errm && !err) {
                const uint32_t f = uint32_t(__builtin_ctzll(errm));
                err = uint32_t(__shfl(int(r.err), int(f)));
                if (kWrite) Syntax::first_error(P, line, start, len, w0 + int64_t(f), err, lane);
            }
            if (!kWrite) {
                // the slot of a '/': the openers between the anchor below it and this one
                const int ja = hi_lane(r.anchorm & below);
                const uint32_t slot = ja >= 0 ? popc(openm & below & ~lanes_upto(uint32_t(ja))) : open_since_anchor + popc(openm & below);
                n_tags = r.opener && slot + 1u > n_tags ? slot + 1u : n_tags;
            } else {
                const uint64_t ci = chars + popc(leadm & below);   // char of the line
                if (r.raw) {
                    const uint64_t k = raw_at + raw + popc(rawm & below);
                    if (k < P.raw_cap) P.raw[k] = uint8_t(c);
                }
                if (r.lead && char_at + ci < P.index_cap) P.tag_index[char_at + ci] = tag_at + tags + popc(openm & below);
                if (r.label && ci > 0 && lab_at + ci - 1 < P.label_cap) P.labels[lab_at + ci - 1] = uint8_t(r.label_value);
                if (r.opener) {
                    const uint64_t k = tag_at + tags + popc(openm & below);
                    if (k < P.span_cap) P.span_off[k] = tb_at + tbytes + popc(tagm & below);
                }
                if (r.tagb) {
                    const uint64_t k = tb_at + tbytes + popc(tagm & below);
                    if (k < P.tb_cap) P.tag_bytes[k] = uint8_t(c);
                }
            }
            // carried to the next window
            if (r.anchorm) open_since_anchor = popc(openm & ~lanes_upto(uint32_t(hi_lane(r.anchorm))));
            else open_since_anchor += popc(openm);
            raw += popc(rawm);
            chars += popc(leadm);
            tags += popc(openm);
            tbytes += popc(tagm);
        }
        if (!err) err = Syntax::end_error(carry, len, chars);   // what only the line's end tells
        if (!kWrite) {
            const uint32_t nt = wave_max(n_tags);
            if (lane == 0) {
                P.raw_off[line + 1] = raw;
                P.ooff[line + 1] = chars ? chars - 1 : 0;
                P.tag_off[line + 1] = tags;
                P.tb_off[line + 1] = tbytes;
                P.n_tags[line] = nt;
                if (err) {
                    atomicOr(P.status, Syntax::kStatusBit);
                    atomicMax(P.status + Syntax::kErrWord + err, 0xFFFFFFFFu - uint32_t(line));
                }
            }
        } else if (lane == 0 && line + 1 == P.n_sent) {   // the CSR arrays' last entries
            if (char_at + chars < P.index_cap) P.tag_index[char_at + chars] = tag_at + tags;
            if (tag_at + tags < P.span_cap) P.span_off[tag_at + tags] = tb_at + tbytes;
        }
    }
}

// write_partial_kernel<kWrite>: Sentence::write_partial_annotation_text (sentence.rs:907-944), a wave per line over windows of 64 raw bytes.  A char's
// lead byte brings along what stands in front of it: the tags of the char before it ("/tag" up to the last non-empty one) and its boundary's mark;
// the line's last char leaves its tags at the line's end.  A window's sizes are one prefix sum.
__device__ __forceinline__ uint64_t partial_suffix(const WritePartialParams& P, uint64_t g, uint8_t* dst, uint64_t at) {
    if (!P.tag_index) return 0;
    const uint64_t t0 = P.tag_index[g];
    uint64_t t1 = P.tag_index[g + 1];
    while (t1 > t0 && P.span_off[t1] == P.span_off[t1 - 1]) --t1;   // up to the last Some
    if (t1 <= t0) return 0;
    const uint64_t b0 = P.span_off[t0], n = (t1 - t0) + (P.span_off[t1] - b0);
    if (dst) {
        uint64_t k = at;
        for (uint64_t t = t0; t < t1; ++t) {
            if (k < P.capacity) dst[k] = uint8_t('/');
            ++k;
            for (uint64_t q = P.span_off[t]; q < P.span_off[t + 1]; ++q, ++k)
                if (k < P.capacity) dst[k] = P.tag_bytes[q];
        }
    }
    return n;
}

template <bool kWrite>
__global__ __launch_bounds__(kParseThreads) void write_partial_kernel(const WritePartialParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = uint64_t(gridDim.x) * (kParseThreads / 64);
    for (uint64_t line = uint64_t(blockIdx.x) * (kParseThreads / 64) + (threadIdx.x >> 6); line < P.n_sent; line += n_waves) {
        const uint64_t start = P.boff[line], end = P.boff[line + 1];
        const int64_t len = end > start ? int64_t(end - start) : 0;
        const uint64_t b0 = P.ooff[line], nb = P.ooff[line + 1] >= b0 ? P.ooff[line + 1] - b0 : 0, g0 = b0 + line;
        const uint64_t out_at = kWrite ? P.out_off[line] : 0;
        uint64_t chars = 0, bytes = 0;
        uint32_t bad = len == 0 ? kErrEmptySentence : 0u;
        for (int64_t w0 = 0; w0 < len; w0 += 64) {
            const bool valid = w0 + int64_t(lane) < len;
            const uint32_t c = valid ? P.text[start + uint64_t(w0) + lane] : 0x80u;
            const bool lead = valid && (c & 0xC0u) != 0x80u;
            const uint64_t leadm = __ballot(lead);
            const uint64_t ci = chars + popc(leadm & lanes_below(lane));   // the lead's char of the line
            // a char past what out_offsets promise reads no label and no tags (the line is reported: the offsets do not match the text)
            const bool front = lead && ci > 0 && ci <= nb;
            uint32_t lab = 0;
            uint64_t sfx = 0;
            if (front) {
                lab = P.labels[b0 + ci - 1];
                sfx = partial_suffix(P, g0 + ci - 1, nullptr, 0);
            }
            if (__ballot(lab > 2u)) bad |= kErrBadLabel;
            const uint32_t mine = valid ? 1u + (front ? 1u + uint32_t(sfx) : 0u) : 0u;
            const uint32_t incl = wave_inclusive_scan(mine);
            if (kWrite && valid) {
                uint64_t k = out_at + bytes + (incl - mine);
                if (front) {
                    partial_suffix(P, g0 + ci - 1, P.out, k);
                    k += sfx;
                    if (k < P.capacity) P.out[k] = uint8_t(lab == 0u ? '-' : lab == 1u ? '|' : ' ');
                    ++k;
                }
                if (k < P.capacity) P.out[k] = uint8_t(c);
            }
            bytes += uint32_t(__shfl(int(incl), 63));
            chars += popc(leadm);
        }
        if (len > 0 && chars != nb + 1) bad |= kErrBadOffsets;
        if (lane == 0) {
            if (!bad) bytes += partial_suffix(P, g0 + nb, kWrite ? P.out : nullptr, out_at + bytes);   // the last char's tags
            if (!kWrite) {
                P.out_off[line + 1] = bytes;
                if (bad) atomicOr(P.status, bad);
            }
        }
    }
}

// ---- evaluate

// the record fill_tags left for flat char g, or ~0; [lo, hi): the records of the run of sentences that holds g (tag_records.h)
__device__ uint64_t find_record(const EvalParams& P, uint64_t lo, uint64_t hi, uint64_t g) {
    const uint64_t k = records_lower_bound(P.sys_tags.records, lo, hi, g);
    return k < hi && rec_pos(P.sys_tags.records[k]) == g && rec_has_model(P.sys_tags.records[k]) ? k : ~uint64_t(0);
}

// the tag vector of char g (sentence i) of the gold side equals that of the system side (evaluate/src/main.rs:111-122, 163, 181)
__device__ bool tags_equal(const EvalParams& P, uint64_t rec_lo, uint64_t rec_hi, uint64_t i, uint64_t g) {
    if (P.mode == kEvalTagsGold) return true;
    const uint32_t nt = P.gold_n_tags[i];
    if (P.mode == kEvalTagsNone) return nt == 0;
    if (nt != P.sys_tags.n_tags) return false;
    const uint64_t t0 = P.tag_index[g], own = P.tag_index[g + 1] - t0;
    const uint64_t rec = find_record(P, rec_lo, rec_hi, g);
    for (uint32_t j = 0; j < nt; ++j) {
        uint64_t gs = 0, gl = 0;   // gold: bytes of tag j (empty: None)
        if (j < own) { gs = P.span_off[t0 + j]; gl = P.span_off[t0 + j + 1] - gs; }
        const int32_t t = rec != ~uint64_t(0) ? P.sys_tags.rec_tags[rec * P.sys_tags.n_tags + j] : -1;
        if (t < 0 || gl == 0) {
            if ((t < 0) != (gl == 0)) return false;
            continue;
        }
        // the candidate string is stored escaped as write_tokenized_text writes it (tables.hpp, str_bytes): compare it unescaped
        const uint2 s = P.sys_tags.rec_str[rec * P.sys_tags.n_tags + j];
        uint64_t k = 0;
        for (uint32_t q = 0; q < s.y; ++q) {
            uint8_t ch = P.sys_tags.str_bytes[s.x + q];
            if (ch == '\\' && q + 1 < s.y) ch = P.sys_tags.str_bytes[s.x + ++q];
            if (k >= gl || P.tag_bytes[gs + k] != ch) return false;
            ++k;
        }
        if (k != gl) return false;
    }
    return true;
}

__global__ __launch_bounds__(kParseThreads) void evaluate_kernel(const EvalParams P) {
    __shared__ uint64_t red[kParseThreads / 64][kEvalCounts];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_waves = uint64_t(gridDim.x) * (kParseThreads / 64);
    uint64_t cnt[kEvalCounts] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t i = uint64_t(blockIdx.x) * (kParseThreads / 64) + wave; i < P.n_sent; i += n_waves) {
        const uint64_t b0 = P.ooff[i], nb = P.ooff[i + 1] - b0, g0 = b0 + i;
        int64_t last_a = -1, last_d = -2;
        uint64_t rec_lo = 0, rec_hi = 0;
        if (P.mode == kEvalTagsPredicted) { const uint64_t run = i / P.sys_tags.run_sent; records_of_runs(P.sys_tags, run, run + 1, &rec_lo, &rec_hi); }
        for (uint64_t w0 = 0; w0 < nb; w0 += 64) {
            const bool valid = w0 + lane < nb;
            const uint32_t r = valid ? P.gold[b0 + w0 + lane] : 0u, s = valid ? P.sys[b0 + w0 + lane] : 0u;
            const uint64_t agree_wb = __ballot(valid && r == s && s == kWordBoundary), dis = __ballot(valid && r != s);
            const uint64_t sys_wb = __ballot(valid && s == kWordBoundary), ref_wb = __ballot(valid && r == kWordBoundary);
            const uint64_t fp = dis & sys_wb;
            cnt[0] += popc(agree_wb);
            cnt[1] += popc(__ballot(valid && r == s && s != kWordBoundary));
            cnt[2] += popc(fp);
            cnt[3] += popc(dis & ~fp);
            cnt[4] += popc(sys_wb);
            cnt[5] += popc(ref_wb);
            const bool mine = (agree_wb >> lane) & 1u;
            const bool matched = last_below(dis, lane, int64_t(w0), last_d) < last_below(agree_wb, lane, int64_t(w0), last_a);
            const bool cor = mine && matched && tags_equal(P, rec_lo, rec_hi, i, g0 + w0 + lane);
            cnt[6] += popc(__ballot(cor));
            last_a = last_in(agree_wb, int64_t(w0), last_a);
            last_d = last_in(dis, int64_t(w0), last_d);
        }
        // the sentence's last token (evaluate/src/main.rs:181-186)
        const bool cor = last_d < last_a && tags_equal(P, rec_lo, rec_hi, i, g0 + nb);
        cnt[4] += 1; cnt[5] += 1; cnt[6] += cor ? 1 : 0; cnt[7] += 1;
    }
    if (lane == 0)
        for (uint32_t k = 0; k < kEvalCounts; ++k) red[wave][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x < kEvalCounts) {
        uint64_t v = 0;
        for (uint32_t w = 0; w < kParseThreads / 64; ++w) v += red[w][threadIdx.x];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(P.counts + threadIdx.x), (unsigned long long)v);
    }
}

uint32_t grid_for(uint64_t n) {
    const uint64_t blocks = (n + kParseThreads / 64 - 1) / (kParseThreads / 64);
    return uint32_t(blocks < kParseMaxBlocks ? (blocks ? blocks : 1) : kParseMaxBlocks);
}

// zeroes the scan's partials, then the chained scan of counts[0 .. n] in place; a total above `cap` is kErrOutputTooSmall
hipError_t scan_counts(uint64_t* counts, uint64_t n, uint64_t* scan_part, uint64_t cap, uint32_t* status, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(scan_part, 0, scan_part_entries(n) * sizeof(uint64_t), stream);
    return e != hipSuccess ? e : launch_scan(counts, n, scan_part, cap, status, nullptr, stream);
}

template <class Syntax>
hipError_t parse_with(const ParseParams& P, uint64_t* scan_part, hipStream_t stream) {
    hipLaunchKernelGGL((parse_lines_kernel<Syntax, false>), dim3(grid_for(P.n_sent)), dim3(kParseThreads), 0, stream, P);
    hipError_t e = hipGetLastError();
    uint64_t* const counts[4] = {P.raw_off, P.ooff, P.tag_off, P.tb_off};
    // the totals against what the caller's buffers hold: an output larger than them is kErrOutputTooSmall (the write pass stores nothing past them)
    const uint64_t caps[4] = {P.raw_cap, P.label_cap, P.span_cap - 1, P.tb_cap};
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = scan_counts(counts[k], P.n_sent, scan_part, caps[k], P.status, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((parse_lines_kernel<Syntax, true>), dim3(grid_for(P.n_sent)), dim3(kParseThreads), 0, stream, P);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_parse(ParseKind kind, const ParseParams& P, uint64_t* scan_part, hipStream_t stream) {
    return kind == ParseKind::kPartial ? parse_with<PartialSyntax>(P, scan_part, stream) : parse_with<TokenizedSyntax>(P, scan_part, stream);
}

hipError_t launch_write_partial(const WritePartialParams& P, uint64_t* scan_part, hipStream_t stream) {
    hipLaunchKernelGGL(write_partial_kernel<false>, dim3(grid_for(P.n_sent)), dim3(kParseThreads), 0, stream, P);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = scan_counts(P.out_off, P.n_sent, scan_part, P.capacity, P.status, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(write_partial_kernel<true>, dim3(grid_for(P.n_sent)), dim3(kParseThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_evaluate(const EvalParams& P, hipStream_t stream) {
    hipLaunchKernelGGL(evaluate_kernel, dim3(grid_for(P.n_sent)), dim3(kParseThreads), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
