// Tag records: what a fill_tags call (or the pattern tagger's merge behind it) leaves on the workspace -- one record per token that can have a tag
// model, sorted by the token's last char, numbered run by run (TagParams, kernels.hpp) -- and the ONE set of accessors every reader goes through.
// Plain C++ (VPT_HD): the same text serves the device, the CPU build of the kernels and tests/native/tag_records_test.cpp.
// THE RUNS' BOUND.  The records are numbered by a scan over the runs' candidate counts and every array they index holds `capacity` = total_chars
// entries, so the runs the front end accepts may never cover more than total_chars chars.  Offsets that go down and up again make runs that overlap
// (each of them inside the batch on its own), so three things hold whatever the offsets say:
//   * decode_chars_kernel / the scoring kernel in front of the launches have raised kErrBadOffsets in the batch's control word (TagParams::status)
//     for such offsets: the front end and the pattern tagger then accept no run at all (no candidates, no records);
//   * the scans over run_pref have total_chars as their capacity and raise kErrBadOffsets past it;
//   * every reader takes what it reads of run_pref from the functions below, which clamp it to `capacity` -- nothing else reads run_pref -- and checks
//     a record's char against total_chars before it indexes cps, tags, model_out or scores_out with it.
#pragma once
#include <hip/hip_runtime_api.h>   // uint2, uint4
#include "layout.h"

namespace vpt {
struct TagRecordsView {
    const uint4* records;       // sorted by the token's last char
    const int32_t* rec_tags;    // [record * n_tags + slot]
    const uint2* rec_str;       // [record * n_tags + slot] {start, length} in str_bytes
    const uint64_t* run_pref;   // [n_runs + 1]
    const uint8_t* str_bytes;
    uint64_t n_runs, capacity;  // capacity = total_chars: the arrays hold that many records
    uint32_t run_sent, n_tags;
};
// the flat index of the char that ends the record's token; whether the token has tags (a tag model, or rule tags: kTokModelMask) -- else the record is empty
VPT_HD uint64_t rec_pos(const uint4& r) { return uint64_t(r.x) | (uint64_t(r.y) << 32); }
VPT_HD bool rec_has_model(const uint4& r) { return (r.z & kTokModelMask) != 0; }
// the first record of run `run` (n_runs and past it: the end of the last run's), never past the arrays; `exact`: cleared when index or value had to be bent
VPT_HD uint64_t run_first_record(const TagRecordsView& V, uint64_t run, bool* exact = nullptr) {
    const uint64_t r = run < V.n_runs ? run : V.n_runs, f = V.run_pref[r];
    if (exact && (r != run || f > V.capacity)) *exact = false;
    return f < V.capacity ? f : V.capacity;
}
VPT_HD uint64_t records_count(const TagRecordsView& V) { return run_first_record(V, V.n_runs); }
// [*lo, *hi): the records of runs [run_a, run_b), lo <= hi <= capacity whatever run_pref holds; false: not what run_pref said, it had to be bent
VPT_HD bool records_of_runs(const TagRecordsView& V, uint64_t run_a, uint64_t run_b, uint64_t* lo, uint64_t* hi) {
    bool exact = true;
    const uint64_t a = run_first_record(V, run_a, &exact), b = run_first_record(V, run_b, &exact);
    *lo = a; *hi = b < a ? a : b;
    return exact && b >= a;
}
// the first record of the slice [lo, hi) that is not in front of char gp (hi: none) -- the slice is sorted by position
VPT_HD uint64_t records_lower_bound(const uint4* records, uint64_t lo, uint64_t hi, uint64_t gp) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (rec_pos(records[mid]) < gp) lo = mid + 1; else hi = mid;
    }
    return lo;
}
}  // namespace vpt
