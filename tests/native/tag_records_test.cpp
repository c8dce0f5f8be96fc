// TEST INFRASTRUCTURE: vaporetto_amd/csrc/tag_records.h -- the accessors every reader of fill_tags' records goes through -- held to seeded random
// hand-overs, hostile ones included: run_pref that goes down, lies above the capacity or is all ~0, run indices past n_runs, no runs at all.  A
// stand-alone program (tests/test_tag_records_native.py builds it with the address and undefined-behaviour sanitizers and runs it as a child
// process); run_pref and records are heap arrays of exactly n_runs + 1 and capacity entries, so a read past either is caught.
//   tag_records_test CASES  ->  "ok CASES SLICES SEARCHES"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "tag_records.h"

using vpt::TagRecordsView;

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            std::fprintf(stderr, "case %llu kind %d line %d: %s\n", (unsigned long long)g_case, g_kind, __LINE__, #cond); \
            std::exit(1);                                                                             \
        }                                                                                             \
    } while (0)

static uint64_t g_case = 0;
static int g_kind = 0;

int main(int argc, char** argv) {
    const uint64_t cases = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1000;
    std::mt19937_64 rng(20261018);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };   // [0, n)
    uint64_t slices = 0, searches = 0;
    for (g_case = 0; g_case < cases; ++g_case) {
        // kinds of run_pref: 0 a prefix sum that fits (what fill_tags leaves), 1 inside the capacity but not monotonic, 2 values above it, 3 all ~0, 4 a mix
        const int kind = g_kind = int(g_case % 5);
        const uint64_t n_runs = g_case % 7 == 0 ? 0 : g_case % 7 == 1 ? 1 : 2 + below(40);
        const uint64_t capacity = g_case % 11 == 0 ? 0 : g_case % 11 == 1 ? 1 : 1 + below(300);
        const bool sorted = (g_case / 5) % 3 != 0;
        std::unique_ptr<uint64_t[]> pref(new uint64_t[n_runs + 1]);
        std::unique_ptr<uint4[]> records(new uint4[capacity]);
        if (kind == 0) {
            uint64_t at = 0;
            for (uint64_t r = 0; r <= n_runs; ++r) { pref[r] = at; at += below((capacity - at) / (n_runs - r + 1) * 2 + 1); if (at > capacity) at = capacity; }
            if (n_runs == 0) pref[0] = below(capacity + 1);   // (the count of a batch without runs is whatever the word holds: it is still clamped)
        }
        for (uint64_t r = 0; kind != 0 && r <= n_runs; ++r) {
            const int k = kind == 4 ? int(below(4)) : kind;
            pref[r] = k == 1 || k == 0 ? below(capacity + 1) : k == 2 ? capacity + 1 + below(below(2) ? 8 : ~uint64_t(0) - capacity - 1) : ~uint64_t(0);
        }
        // positions above 2^32 too: both words of a record's position count
        uint64_t pos = below(3) ? 0 : (uint64_t(1) << 32) - 5;
        for (uint64_t k = 0; k < capacity; ++k) {
            pos = sorted ? pos + 1 + below(4) : below(1000);
            records[k] = uint4{uint32_t(pos), uint32_t(pos >> 32), uint32_t(below(2) ? below(1u << 24) | (below(256) << 24) : below(256) << 24), 0u};
            CHECK(vpt::rec_pos(records[k]) == pos);
            CHECK(vpt::rec_has_model(records[k]) == ((records[k].z & 0xFFFFFFu) != 0));
        }
        const TagRecordsView V{records.get(), nullptr, nullptr, pref.get(), nullptr, n_runs, capacity, 64u, 2u};
        const uint64_t count = vpt::records_count(V);
        CHECK(count <= capacity);
        CHECK(count == (pref[n_runs] < capacity ? pref[n_runs] : capacity));
        for (int s = 0; s < 24; ++s) {
            // run indices: inside, at n_runs, just past it, far past it; in order and out of order
            auto index = [&]() { const uint64_t w = below(8); return w < 5 ? below(n_runs + 1) : w == 5 ? n_runs + 1 + below(3) : w == 6 ? ~uint64_t(0) - below(2) : n_runs; };
            uint64_t a = index(), b = s % 4 == 0 ? a + 1 : index();
            if (s % 4 == 1 && a > b) { const uint64_t t = a; a = b; b = t; }
            uint64_t lo = ~uint64_t(0), hi = ~uint64_t(0);
            const bool exact = vpt::records_of_runs(V, a, b, &lo, &hi);
            ++slices;
            CHECK(lo <= hi && hi <= capacity);
            CHECK(vpt::run_first_record(V, a) == lo);
            if (exact) CHECK(a <= n_runs && b <= n_runs && lo == pref[a] && hi == pref[b]);
            if (a <= n_runs && b <= n_runs && pref[a] <= pref[b] && pref[b] <= capacity) CHECK(exact && lo == pref[a] && hi == pref[b]);
            if (kind == 0 && a <= b && b <= n_runs) CHECK(exact);   // monotonic, in range: the slice is the raw pair
            for (int q = 0; q < 6; ++q) {
                uint64_t gp = q == 0 ? 0 : q == 1 ? ~uint64_t(0) : below(1200);
                if (q >= 3 && hi > lo) gp = vpt::rec_pos(records[lo + below(hi - lo)]) + below(3) - 1;   // a record's char, the one in front, the one behind
                const uint64_t k = vpt::records_lower_bound(records.get(), lo, hi, gp);
                ++searches;
                CHECK(lo <= k && k <= hi);
                if (sorted) {
                    uint64_t want = lo;
                    while (want < hi && vpt::rec_pos(records[want]) < gp) ++want;
                    CHECK(k == want);
                }
            }
        }
    }
    std::printf("ok %llu %llu %llu\n", (unsigned long long)cases, (unsigned long long)slices, (unsigned long long)searches);
    return 0;
}
