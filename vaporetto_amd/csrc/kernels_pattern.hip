// PatternMatchTagger on the device (vaporetto_rules/src/sentence_filters/pattern_match_tagger.rs:21-41), behind fill_tags on its workspace and stream:
//
//   for every token (maximal run between WordBoundary labels; a token with an Unknown label inside gets nothing, as in fill_tags) and every slot
//   j < n_tags that fill_tags left None: if the token's WHOLE surface is a key of the rule table, the slot becomes rules[surface].get(j) -- which
//   may be None itself.  Slots that are Some stay.  The surfaces are those of the text as it was scored (decode_chars' words).
//
// fill_tags leaves one record per token that can have a tag model, sorted by position, run by run of `run_sent` sentences (TagParams, kernels.hpp);
// the writer reads the records of its sentences as ONE slice and depends on that order.  A rule can hit a token that has a record (its None slots
// are filled) or one that has none (a new record), so the records are MERGED into arrays of their own, in order, without a sort and without atomics:
//
//   pattern_match_kernel   a workgroup per run walks the run's chars, kPatternStep at a time, a LANE PER CHAR.  A lane whose char ends a token walks
//                          back over the labels to the token's start -- at most max_len steps: a token longer than the longest rule surface leaves
//                          at once -- hashes its code points from the decoded chars, probes the table (pattern_tagger.hpp: the slot a lane fetches
//                          first is one aligned 16-byte load) and verifies char by char.  A hit looks for the token's record among the run's (a
//                          bisection over the slice, sorted by position); with none it is a NEW record.  Per char the kernel leaves {rule + 1 | new
//                          << 31, new records of the run in front of the char} (a workgroup prefix sum carried from step to step) and per run the
//                          merged count: its records + its new ones.
//   launch_scan            the runs' merged counts -> the runs' first merged records (the chained scan of kernels_emit.hip)
//   pattern_merge_kernel   a workgroup per run again: a new record goes to (first record of the run) + (records of the run in front of its char,
//                          from the same bisection) + (new ones in front of it); a record of fill_tags moves up by the new ones in front of its
//                          char, and takes the rule's tags in its None slots when its token was hit.  The bytes the token's tags take in the
//                          tokenized text are summed again for the writer (layout.h, kTokSuffixShift).
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.hpp"
#include "pattern_tagger.hpp"

namespace vpt {
namespace {

constexpr int kPmThreads = int(kPatternStep);
constexpr int kPmWaves = kPmThreads / 64;
constexpr uint32_t kPmCharMask = 0x1FFFFFu;   // a cps word: scored scalar value | CharacterType << 24
constexpr uint32_t kPmNew = 0x80000000u;
constexpr uint32_t kPmMaxRunSent = 256;       // sentences of a front-end run, at most (tag_run_sentences); sst holds their starts and the run's end

// what both kernels know of a run: its sentences, its chars [run0, run0 + n), its records [r_lo, r_hi); ok == false: offsets or counts that do not
// fit the batch (reported by decode_chars_kernel / the scoring kernel in the batch's control word, which is looked at here: runs of such offsets can
// overlap, tag_records.h) -- the run keeps its records and gets no rule tags; records that do not fit the arrays are dropped, not clamped
struct PmRun {
    uint64_t i_a, run0, r_lo, r_hi;
    uint32_t ns, n;
    bool ok;
};
__device__ __forceinline__ PmRun pm_run(const PatternParams& P, uint64_t run) {
    PmRun R;
    R.i_a = run * P.in.run_sent;
    const uint64_t i_b = R.i_a + P.in.run_sent < P.n_sent ? R.i_a + P.in.run_sent : P.n_sent;
    R.ns = uint32_t(i_b - R.i_a);
    R.run0 = P.ooff[R.i_a] + R.i_a;
    const uint64_t run1 = P.ooff[i_b] + i_b;
    const bool recs = records_of_runs(P.in, run, run + 1, &R.r_lo, &R.r_hi);
    if (!recs) { R.r_lo = 0; R.r_hi = 0; }
#ifdef VPT_TAG_NO_OFFSETS_GATE   // (test builds, kernels_tags.hip)
    const bool gate = false;
#else
    const bool gate = (*P.status & kErrBadOffsets) != 0;
#endif
    R.ok = recs && !gate && run1 >= R.run0 && run1 <= P.total_chars && run1 - R.run0 < 0x7FFFFF00ull && R.ns <= kPmMaxRunSent;
    R.n = R.ok ? uint32_t(run1 - R.run0) : 0u;
    return R;
}

__global__ __launch_bounds__(kPmThreads) void pattern_match_kernel(const PatternParams P) {
    __shared__ uint32_t sst[kPmMaxRunSent + 1];   // the run's sentence starts, run-relative; entry ns: the run's end
    __shared__ uint32_t wtot[kPmWaves];
    __shared__ uint32_t bad;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
    const uint64_t total_b = P.total_chars - P.n_sent;
    const uint32_t mask = (1u << P.bits) - 1u;
    for (uint64_t run = blockIdx.x; run < P.in.n_runs; run += gridDim.x) {
        const PmRun R = pm_run(P, run);
        __syncthreads();   // (the run before is done with sst / wtot / bad)
        if (tid == 0) bad = 0;
        __syncthreads();
        for (uint32_t k = tid; R.ok && k <= R.ns; k += uint32_t(kPmThreads)) {   // ns + 1 entries: one more than a full run has threads
            const uint64_t i = R.i_a + k, f = P.ooff[i] + i;
            const bool in = f >= R.run0 && f - R.run0 <= R.n;
            sst[k] = in ? uint32_t(f - R.run0) : 0u;
            if (!in) bad = 1;
        }
        __syncthreads();
        for (uint32_t k = tid; R.ok && k < R.ns; k += uint32_t(kPmThreads))
            if (sst[k + 1] <= sst[k]) bad = 1;   // sentences out of order (or empty): nothing is looked up
        __syncthreads();
        const uint32_t n = R.n;
        const bool look = bad == 0;   // (else every char of the run gets an empty entry: the merge reads one per char)
        uint32_t carry = 0;   // new records of the run so far
        for (uint32_t base = 0; base < n; base += kPatternStep) {
            const uint32_t q = base + tid;
            uint32_t hit = 0;
            bool is_new = false;
            if (q < n && look) {
                uint32_t lo = 0, hi = R.ns;   // the char's sentence: the last k with sst[k] <= q
                while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (sst[mid] <= q) lo = mid; else hi = mid; }
                const uint32_t s_beg = sst[lo], s_end = sst[lo + 1];
                // char q of the run sits in sentence i_a + lo: the label behind it is labels[run0 + q - (i_a + lo)], the one in front of it one lower
                const uint64_t lab = R.run0 + q - (R.i_a + lo);
                const bool last = q + 1 == s_end;
                bool ok = last || (lab < total_b && P.labels[lab] == 1u);
                uint32_t len = 1;
                // back to the token's start: a token longer than every rule surface leaves at once, one with an Unknown label inside has no tags
                for (uint32_t p = q; ok && p > s_beg; --p, ++len) {
                    const uint64_t at = R.run0 + p - (R.i_a + lo) - 1;
                    const uint32_t b = at < total_b ? uint32_t(P.labels[at]) : 1u;
                    if (b == 1u) break;
                    if (b != 0u || len >= P.max_len) ok = false;
                }
                if (ok && len <= P.max_len) {
                    const uint32_t* const tc = P.cps + (R.run0 + q + 1 - len);
                    uint64_t h = kRuleHashSeed;
                    for (uint32_t j = 0; j < len; ++j) h = rule_hash_step(h, tc[j] & kPmCharMask);
                    h = rule_hash_finish(h, len);
                    const uint32_t fp = uint32_t(h >> 32);
                    for (uint32_t slot = uint32_t(h) & mask;; slot = (slot + 1) & mask) {   // (at most half of the slots are taken: an empty one ends every chain)
                        const uint4 e = P.slots[slot];
                        if (e.x == 0) break;
                        if (e.y == len && e.z == fp) {
                            bool same = true;
                            for (uint32_t j = 0; j < len && same; ++j) same = P.surf[e.w + j] == (tc[j] & kPmCharMask);
                            if (same) { hit = e.x; break; }
                        }
                    }
                }
                if (hit) {   // has the token a record already?
                    const uint64_t gp = R.run0 + q, k = records_lower_bound(P.in.records, R.r_lo, R.r_hi, gp);
                    is_new = !(k < R.r_hi && rec_pos(P.in.records[k]) == gp);
                }
            }
            // the new records in front of the char: a prefix sum over the workgroup, carried from step to step
            const uint64_t m = __ballot(is_new);
            if (lane == 0) wtot[wave] = uint32_t(__popcll(m));
            __syncthreads();
            uint32_t before = carry, total = 0;
#pragma unroll
            for (uint32_t k = 0; k < uint32_t(kPmWaves); ++k) {
                const uint32_t u = wtot[k];
                if (k < wave) before += u;
                total += u;
            }
            before += uint32_t(__popcll(m & ((uint64_t(1) << lane) - 1)));
            if (q < n) P.hits[R.run0 + q] = make_uint2(hit | (is_new ? kPmNew : 0u), before);
            carry += total;
            __syncthreads();   // (wtot is rewritten by the next step)
        }
        if (tid == 0) P.out_run_pref[run + 1] = (R.r_hi - R.r_lo) + carry;
    }
}

// the rule's entry for slot j as a record's words
__device__ __forceinline__ void rule_slot(const PatternParams& P, uint32_t rule, uint32_t j, int32_t* tag, uint2* str) {
    const int32_t id = P.rule_tags[size_t(rule) * P.n_tags + j];
    if (id >= 0) { *tag = -(2 + id); *str = P.id_str[id]; }
}

__global__ __launch_bounds__(kPmThreads) void pattern_merge_kernel(const PatternParams P) {
    const uint32_t tid = threadIdx.x, nt = P.n_tags;
    for (uint64_t run = blockIdx.x; run < P.in.n_runs; run += gridDim.x) {
        const PmRun R = pm_run(P, run);
        TagRecordsView out = P.in; out.run_pref = P.out_run_pref;   // (the merged records: their runs' first records come through the same accessor)
        const uint64_t o_lo = run_first_record(out, run);
        const bool have_hits = R.n != 0;   // (the first kernel left an entry per char of the run)
        // ---- the new records
        for (uint32_t q = tid; have_hits && q < R.n; q += uint32_t(kPmThreads)) {
            const uint64_t gp = R.run0 + q;
            const uint2 h = P.hits[gp];
            if (!(h.x & kPmNew)) continue;
            const uint64_t k = o_lo + (records_lower_bound(P.in.records, R.r_lo, R.r_hi, gp) - R.r_lo) + h.y;
            if (k >= P.total_chars) continue;   // (cannot be: a record per char at most)
            const uint32_t rule = (h.x & ~kPmNew) - 1u;
            uint32_t bytes = 0, last = 0;
            for (uint32_t j = 0; j < nt; ++j) {
                int32_t tag = -1;
                uint2 str = make_uint2(0u, 0u);
                rule_slot(P, rule, j, &tag, &str);
                if (tag != -1) { bytes += str.y; last = j + 1; }
                P.out_rec_tags[k * nt + j] = tag;
                P.out_rec_str[k * nt + j] = str;
                if (P.tags && tag != -1) P.tags[gp * nt + j] = tag;
            }
            bytes += last;
            P.out_records[k] = make_uint4(uint32_t(gp), uint32_t(gp >> 32), kTokModelMask | ((bytes < kTokSuffixLong ? bytes : kTokSuffixLong) << kTokSuffixShift), last);
        }
        // ---- fill_tags' records, moved up by the new ones in front of them; the None slots of a token the rules name are filled
        for (uint64_t r = R.r_lo + tid; r < R.r_hi; r += uint32_t(kPmThreads)) {
            const uint4 rec = P.in.records[r];
            const uint64_t gp = rec_pos(rec);
            uint2 h = make_uint2(0u, 0u);
            if (have_hits && gp >= R.run0 && gp - R.run0 < R.n) h = P.hits[gp];
            const uint64_t k = o_lo + (r - R.r_lo) + h.y;
            if (k >= P.total_chars) continue;
            const uint32_t model = rec.z & kTokModelMask, hit = h.x & ~kPmNew;
            bool changed = false;
            uint32_t bytes = 0, last = 0;
            for (uint32_t j = 0; j < nt; ++j) {
                int32_t tag = model ? P.in.rec_tags[r * nt + j] : -1;   // (an empty record: the passes wrote nothing for it)
                uint2 str = model ? P.in.rec_str[r * nt + j] : make_uint2(0u, 0u);
                if (tag == -1 && hit) {
                    rule_slot(P, hit - 1u, j, &tag, &str);
                    if (tag != -1) { changed = true; if (P.tags) P.tags[gp * nt + j] = tag; }
                }
                if (tag != -1) { bytes += str.y < 0x10000u ? str.y : 0x10000u; last = j + 1; }
                P.out_rec_tags[k * nt + j] = tag;
                P.out_rec_str[k * nt + j] = tag != -1 ? str : make_uint2(0u, 0u);
            }
            bytes += last;
            uint4 out = rec;
            if (changed) { out.z = (model ? model : kTokModelMask) | ((bytes < kTokSuffixLong ? bytes : kTokSuffixLong) << kTokSuffixShift); out.w = last; }
            P.out_records[k] = out;
        }
    }
}

}  // namespace

hipError_t launch_pattern_tagger(const PatternParams& P, hipStream_t stream) {
    if (P.in.n_runs == 0) return hipSuccess;
    // a workgroup per run, as many as the device holds at a time (8 of 4 waves per CU), striding over the runs
    const uint64_t cap = uint64_t(P.n_cus ? P.n_cus : 256u) * 8u;
    const dim3 grid(uint32_t(P.in.n_runs < cap ? P.in.n_runs : cap)), block(kPmThreads);
    hipLaunchKernelGGL(pattern_match_kernel, grid, block, 0, stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan(P.out_run_pref, P.in.n_runs, P.scan_state, P.total_chars, P.status, nullptr, stream, kErrBadOffsets);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pattern_merge_kernel, grid, block, 0, stream, P);
    return hipGetLastError();
}

}  // namespace vpt
