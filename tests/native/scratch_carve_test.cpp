// TEST INFRASTRUCTURE: vaporetto_amd/csrc/scratch_carve.hpp -- the carver, the sort-and-scan tail, the pass lists and the five layouts the
// postings drivers carve out of a workspace's scratch -- on the CPU (tests/test_scratch_carve_native.py builds this file alone, with the address
// and undefined-behaviour sanitizers).  The offsets and totals below are DATA: they were computed once from the hand-written offset chains the
// drivers had before the carver (capi_device.cpp at commit 7b33366) and are not recomputed here, so a layout that moves by a byte is a report.
// T = 4096 (kPostingsSortTile); train_radix_scratch and train_scan_scratch are inputs to the layouts and defined here by the sort's tile.
//
// Exit status 0 and one line "ok <layouts> <sections>", or the first failed check on stderr and 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scratch_carve.hpp"

namespace vpt {   // (kernels_train.hip: tiles of 4096 items; vpt_postings_tile checks the library's against the same two values)
static uint64_t tiles(uint64_t n) { return (n + 4095) / 4096; }
uint64_t train_scan_scratch(uint64_t n) { return tiles(n) + 1; }
uint64_t train_radix_scratch(uint64_t n) { return 256 * tiles(n); }
}  // namespace vpt

namespace {
using namespace vptcarve;

unsigned long long g_layouts, g_sections;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "layout %llu, line %d: %s\n", g_layouts, __LINE__, #cond); \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

constexpr size_t A = ~size_t(0);   // a section the driver did not have in this case: the carver's has count 0

// the descriptors' sizes (kernels.hpp: PostingsMergeSegment 48 bytes, PostingsMergePosSegment 32)
struct Seg { const void *a, *b, *c; uint64_t d, e; uint32_t f, g; };
struct PosSeg { const void *a, *b; uint64_t c, d; };
static_assert(sizeof(Seg) == 48 && sizeof(PosSeg) == 32, "the descriptors' sizes");

struct Got { size_t offset, bytes; };
template <typename T>
Got got(const Section<T>& s) { return Got{s.offset, sizeof(T) * s.count}; }
Got* tail(const SortTail& t, Got* out) { out[0] = got(t.hist); out[1] = got(t.hist_scan); out[2] = got(t.partials); return out + 3; }

// the sections in the order they were carved: each where the data says, aligned, in order, disjoint, inside the total
void check_sections(const Got* g, const size_t* want, size_t n, size_t total, size_t want_total) {
    size_t end = 0;
    for (size_t i = 0; i < n; ++i) {
        if (want[i] == A) { CHECK(g[i].bytes == 0); continue; }
        CHECK(g[i].offset == want[i]);
        CHECK(g[i].offset % kSectionAlign == 0);
        CHECK(g[i].offset >= end);                          // behind the last byte of every section in front
        CHECK(g[i].bytes == 0 || g[i].offset + g[i].bytes > end);
        end = std::max(end, g[i].offset + g[i].bytes);
        ++g_sections;
    }
    CHECK(total == want_total && end <= total && total % kSectionAlign == 0 && total - end < kSectionAlign);
    ++g_layouts;
}

// ---- the carver itself
void check_carver() {
    Carver c;
    CHECK(c.bytes() == 0);
    const auto a = c.take<uint8_t>(1);
    const auto z = c.take<uint64_t>(0);     // a count of 0 takes nothing
    const auto b = c.take<uint32_t>(64);    // exactly 256 bytes
    const auto d = c.take<uint32_t>(65);
    CHECK(a.offset == 0 && z.offset == 256 && b.offset == 256 && d.offset == 512 && c.bytes() == 1024);
    CHECK(z.count == 0 && b.count == 64);
    // two layouts over the same bytes: a copy of the carver goes on from where the first stands
    Carver other = c;
    const auto e = c.take<uint64_t>(3);
    const auto f = other.take<uint32_t>(100);
    const auto g = other.take<uint8_t>(7);
    CHECK(e.offset == 1024 && f.offset == 1024 && c.bytes() == 1280 && g.offset == 1536 && other.bytes() == 1792);
    // the typed pointers, in a buffer of exactly the total: the first and the last element of every section are inside (ASan watches)
    std::vector<unsigned char> mem(other.bytes(), 0);
    unsigned char* m = mem.data();
    *a.at(m) = 1; b.at(m)[63] = 2; d.at(m)[64] = 3; f.at(m)[99] = 4; g.at(m)[6] = 5;
    CHECK(reinterpret_cast<unsigned char*>(e.at(m)) == reinterpret_cast<unsigned char*>(f.at(m)));   // the overlay
    CHECK(mem[0] == 1 && mem[256 + 4 * 63] == 2 && mem[512 + 4 * 64] == 3 && mem[1024 + 4 * 99] == 4 && mem[1536 + 6] == 5);
    CHECK(reinterpret_cast<unsigned char*>(z.at(m)) == m + 256);
    ++g_layouts;
}

// ---- the pass lists: (word, largest value, cap) -> the passes
void check_passes() {
    struct Row { uint32_t word; uint64_t max_value; uint32_t cap, n; uint32_t v[4]; };
    static const Row rows[] = {
        {0, 0, 4, 0, {0, 0, 0, 0}},
        {0, 1, 4, 1, {0x000, 0, 0, 0}},
        {0, 255, 4, 1, {0x000, 0, 0, 0}},
        {0, 256, 4, 2, {0x000, 0x008, 0, 0}},
        {1, 257, 4, 2, {0x100, 0x108, 0, 0}},
        {0, 65536, 4, 3, {0x000, 0x008, 0x010, 0}},
        {0, 1u << 24, 4, 4, {0x000, 0x008, 0x010, 0x018}},
        {2, 0xFFFFFFFFu, 4, 4, {0x200, 0x208, 0x210, 0x218}},
        {0, 1ull << 32, 4, 4, {0x000, 0x008, 0x010, 0x018}},    // five bytes, capped: the documents of the search's key
        {1, 0xFFFFFFFFu, 2, 2, {0x100, 0x108, 0, 0}},
    };
    for (const Row& r : rows) {
        PassList p;
        p.add(r.word, r.max_value, r.cap);
        CHECK(p.n == r.n);
        for (uint32_t i = 0; i < r.n; ++i) CHECK(p.v[i] == r.v[i]);
    }
    PassList p;   // two words in turn, as the drivers build them; never past the eight entries
    p.add(1, 0xFFFFFFFFu);
    p.add(0, 257);
    CHECK(p.n == 6 && p.v[3] == 0x118 && p.v[4] == 0x000 && p.v[5] == 0x008);
    p.add(2, 0xFFFFFFFFu);
    CHECK(p.n == 8 && p.v[7] == 0x208);
    p.add(0, 1);
    CHECK(p.n == 8);
    ++g_layouts;
}

// ---- the sort-and-scan tail: n, further scan lengths -> hist, hist_scan and partials in words
void check_tail() {
    struct Row { uint64_t n, more; size_t hist, hist_scan, partials; };
    static const Row rows[] = {
        {0, 0, 0, 1, 2},   {1, 0, 256, 257, 3},       {4096, 0, 256, 257, 3},       {4097, 0, 512, 513, 4},
        {0, 257, 0, 1, 3}, {4096, 4097, 256, 257, 4}, {4097, 257, 512, 513, 4},     {4097, 3 * 4096 + 1, 512, 513, 6},
    };
    for (const Row& r : rows) {
        Carver c;
        const SortTail t(c, r.n, {r.more});
        CHECK(t.hist.count == r.hist && t.hist_scan.count == r.hist_scan && t.partials.count == r.partials);
        CHECK(t.hist.offset == 0 && t.hist_scan.offset == ((8 * r.hist + 255) & ~size_t(255)));
        ++g_layouts;
    }
}

// ---- the five drivers
struct PostingsRow { uint64_t n; size_t off[8], total; };
// n | keydoc order skey flags scan hist hist_scan partials | total
const PostingsRow kPostings[] = {
    {0, {0, 0, 0, 0, 0, 256, 256, 512}, 768},
    {1, {0, 256, 512, 768, 1024, 1280, 3328, 5632}, 5888},
    {4096, {0, 32768, 49152, 65536, 81920, 114944, 116992, 119296}, 119552},
    {4097, {0, 33024, 49664, 66304, 82944, 115968, 120064, 124416}, 124672},
};

struct MergeOrderedRow { uint32_t K; uint64_t n; uint32_t n_terms_out; int positional; size_t off[5], total; };
// K n n_terms_out positional | segs psegs range table ptable | total
const MergeOrderedRow kMergeOrdered[] = {
    {1, 0, 1, 0, {0, A, 256, 512, A}, 768},
    {1, 1, 1, 0, {0, A, 256, 512, A}, 768},
    {1, 4096, 1, 0, {0, A, 256, 512, A}, 768},
    {1, 4097, 1, 0, {0, A, 256, 512, A}, 768},
    {1, 0, 256, 0, {0, A, 256, 512, A}, 2816},
    {1, 1, 256, 0, {0, A, 256, 512, A}, 2816},
    {1, 4096, 256, 0, {0, A, 256, 512, A}, 2816},
    {1, 4097, 256, 0, {0, A, 256, 512, A}, 2816},
    {2, 0, 1, 0, {0, A, 256, 512, A}, 768},
    {2, 1, 1, 0, {0, A, 256, 512, A}, 768},
    {2, 4096, 1, 0, {0, A, 256, 512, A}, 768},
    {2, 4097, 1, 0, {0, A, 256, 512, A}, 768},
    {2, 0, 256, 0, {0, A, 256, 512, A}, 4864},
    {2, 1, 256, 0, {0, A, 256, 512, A}, 4864},
    {2, 4096, 256, 0, {0, A, 256, 512, A}, 4864},
    {2, 4097, 256, 0, {0, A, 256, 512, A}, 4864},
    {1, 0, 1, 1, {0, 256, 512, 768, 1024}, 1280},
    {1, 1, 1, 1, {0, 256, 512, 768, 1024}, 1280},
    {1, 4096, 1, 1, {0, 256, 512, 768, 1024}, 1280},
    {1, 4097, 1, 1, {0, 256, 512, 768, 1024}, 1280},
    {1, 0, 256, 1, {0, 256, 512, 768, 3072}, 5376},
    {1, 1, 256, 1, {0, 256, 512, 768, 3072}, 5376},
    {1, 4096, 256, 1, {0, 256, 512, 768, 3072}, 5376},
    {1, 4097, 256, 1, {0, 256, 512, 768, 3072}, 5376},
    {2, 0, 1, 1, {0, 256, 512, 768, 1024}, 1280},
    {2, 1, 1, 1, {0, 256, 512, 768, 1024}, 1280},
    {2, 4096, 1, 1, {0, 256, 512, 768, 1024}, 1280},
    {2, 4097, 1, 1, {0, 256, 512, 768, 1024}, 1280},
    {2, 0, 256, 1, {0, 256, 512, 768, 5120}, 9472},
    {2, 1, 256, 1, {0, 256, 512, 768, 5120}, 9472},
    {2, 4096, 256, 1, {0, 256, 512, 768, 5120}, 9472},
    {2, 4097, 256, 1, {0, 256, 512, 768, 5120}, 9472},
};

struct MergeGeneralRow { uint32_t K; uint64_t n; uint32_t n_terms_out; int positional; size_t off[13], total; };
// K n n_terms_out positional | segs psegs rec order skey flags scan ptf inv pscan hist hist_scan partials | total
const MergeGeneralRow kMergeGeneral[] = {
    {1, 0, 1, 0, {0, A, 256, 256, 256, 256, 256, A, A, A, 512, 512, 768}, 1024},
    {1, 1, 1, 0, {0, A, 256, 512, 768, 1024, 1280, A, A, A, 1536, 3584, 5888}, 6144},
    {1, 4096, 1, 0, {0, A, 256, 49408, 65792, 82176, 98560, A, A, A, 131584, 133632, 135936}, 136192},
    {1, 4097, 1, 0, {0, A, 256, 49664, 66304, 82944, 99584, A, A, A, 132608, 136704, 141056}, 141312},
    {1, 0, 256, 0, {0, A, 256, 256, 256, 256, 256, A, A, A, 512, 512, 768}, 1024},
    {1, 1, 256, 0, {0, A, 256, 512, 768, 1024, 1280, A, A, A, 1536, 3584, 5888}, 6144},
    {1, 4096, 256, 0, {0, A, 256, 49408, 65792, 82176, 98560, A, A, A, 131584, 133632, 135936}, 136192},
    {1, 4097, 256, 0, {0, A, 256, 49664, 66304, 82944, 99584, A, A, A, 132608, 136704, 141056}, 141312},
    {2, 0, 1, 0, {0, A, 256, 256, 256, 256, 256, A, A, A, 512, 512, 768}, 1024},
    {2, 1, 1, 0, {0, A, 256, 512, 768, 1024, 1280, A, A, A, 1536, 3584, 5888}, 6144},
    {2, 4096, 1, 0, {0, A, 256, 49408, 65792, 82176, 98560, A, A, A, 131584, 133632, 135936}, 136192},
    {2, 4097, 1, 0, {0, A, 256, 49664, 66304, 82944, 99584, A, A, A, 132608, 136704, 141056}, 141312},
    {2, 0, 256, 0, {0, A, 256, 256, 256, 256, 256, A, A, A, 512, 512, 768}, 1024},
    {2, 1, 256, 0, {0, A, 256, 512, 768, 1024, 1280, A, A, A, 1536, 3584, 5888}, 6144},
    {2, 4096, 256, 0, {0, A, 256, 49408, 65792, 82176, 98560, A, A, A, 131584, 133632, 135936}, 136192},
    {2, 4097, 256, 0, {0, A, 256, 49664, 66304, 82944, 99584, A, A, A, 132608, 136704, 141056}, 141312},
    {1, 0, 1, 1, {0, 256, 512, 512, 512, 512, 512, 768, 768, 768, 1024, 1024, 1280}, 1536},
    {1, 1, 1, 1, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 4608, 6912}, 7168},
    {1, 4096, 1, 1, {0, 256, 512, 49664, 66048, 82432, 98816, 131840, 148224, 164608, 197632, 199680, 201984}, 202240},
    {1, 4097, 1, 1, {0, 256, 512, 49920, 66560, 83200, 99840, 132864, 149504, 166144, 199168, 203264, 207616}, 207872},
    {1, 0, 256, 1, {0, 256, 512, 512, 512, 512, 512, 768, 768, 768, 1024, 1024, 1280}, 1536},
    {1, 1, 256, 1, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 4608, 6912}, 7168},
    {1, 4096, 256, 1, {0, 256, 512, 49664, 66048, 82432, 98816, 131840, 148224, 164608, 197632, 199680, 201984}, 202240},
    {1, 4097, 256, 1, {0, 256, 512, 49920, 66560, 83200, 99840, 132864, 149504, 166144, 199168, 203264, 207616}, 207872},
    {2, 0, 1, 1, {0, 256, 512, 512, 512, 512, 512, 768, 768, 768, 1024, 1024, 1280}, 1536},
    {2, 1, 1, 1, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 4608, 6912}, 7168},
    {2, 4096, 1, 1, {0, 256, 512, 49664, 66048, 82432, 98816, 131840, 148224, 164608, 197632, 199680, 201984}, 202240},
    {2, 4097, 1, 1, {0, 256, 512, 49920, 66560, 83200, 99840, 132864, 149504, 166144, 199168, 203264, 207616}, 207872},
    {2, 0, 256, 1, {0, 256, 512, 512, 512, 512, 512, 768, 768, 768, 1024, 1024, 1280}, 1536},
    {2, 1, 256, 1, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 4608, 6912}, 7168},
    {2, 4096, 256, 1, {0, 256, 512, 49664, 66048, 82432, 98816, 131840, 148224, 164608, 197632, 199680, 201984}, 202240},
    {2, 4097, 256, 1, {0, 256, 512, 49920, 66560, 83200, 99840, 132864, 149504, 166144, 199168, 203264, 207616}, 207872},
};

struct SearchRow { uint64_t n, ns; uint32_t nq; int boolean; size_t off[15], total; };
// n ns nq boolean | slot_df base slot_query rec hit order skey flags scan qstart hist hist_scan partials q_anchor q_flags | total
const SearchRow kSearch[] = {
    {0, 1, 1, 0, {0, 256, 512, 768, 768, 768, 768, 768, 768, 1024, 1280, 1280, 1536, 1792, 1792}, 1792},
    {1, 1, 1, 0, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 4608, 6912, 7168, 7168}, 7168},
    {4096, 1, 1, 0, {0, 256, 512, 768, 49920, 99072, 115456, 131840, 148224, 181248, 181504, 183552, 185856, 186112, 186112}, 186112},
    {4097, 1, 1, 0, {0, 256, 512, 768, 50176, 99584, 116224, 132864, 149504, 182528, 182784, 186880, 191232, 191488, 191488}, 191488},
    {0, 257, 1, 0, {0, 2304, 4608, 5888, 5888, 5888, 5888, 5888, 5888, 6144, 6400, 6400, 6656, 6912, 6912}, 6912},
    {1, 257, 1, 0, {0, 2304, 4608, 5888, 6144, 6400, 6656, 6912, 7168, 7424, 7680, 9728, 12032, 12288, 12288}, 12288},
    {4096, 257, 1, 0, {0, 2304, 4608, 5888, 55040, 104192, 120576, 136960, 153344, 186368, 186624, 188672, 190976, 191232, 191232}, 191232},
    {4097, 257, 1, 0, {0, 2304, 4608, 5888, 55296, 104704, 121344, 137984, 154624, 187648, 187904, 192000, 196352, 196608, 196608}, 196608},
    {0, 1, 257, 0, {0, 256, 512, 768, 768, 768, 768, 768, 768, 1024, 3328, 3328, 3584, 3840, 3840}, 3840},
    {1, 1, 257, 0, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 4608, 6656, 8960, 9216, 9216}, 9216},
    {4096, 1, 257, 0, {0, 256, 512, 768, 49920, 99072, 115456, 131840, 148224, 181248, 183552, 185600, 187904, 188160, 188160}, 188160},
    {4097, 1, 257, 0, {0, 256, 512, 768, 50176, 99584, 116224, 132864, 149504, 182528, 184832, 188928, 193280, 193536, 193536}, 193536},
    {0, 257, 257, 0, {0, 2304, 4608, 5888, 5888, 5888, 5888, 5888, 5888, 6144, 8448, 8448, 8704, 8960, 8960}, 8960},
    {1, 257, 257, 0, {0, 2304, 4608, 5888, 6144, 6400, 6656, 6912, 7168, 7424, 9728, 11776, 14080, 14336, 14336}, 14336},
    {4096, 257, 257, 0, {0, 2304, 4608, 5888, 55040, 104192, 120576, 136960, 153344, 186368, 188672, 190720, 193024, 193280, 193280}, 193280},
    {4097, 257, 257, 0, {0, 2304, 4608, 5888, 55296, 104704, 121344, 137984, 154624, 187648, 189952, 194048, 198400, 198656, 198656}, 198656},
    {0, 1, 1, 1, {0, 256, 512, 768, 768, 768, 768, 768, 768, 1024, 1280, 1280, 1536, 1792, 2048}, 2304},
    {1, 1, 1, 1, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 4608, 6912, 7168, 7424}, 7680},
    {4096, 1, 1, 1, {0, 256, 512, 768, 49920, 99072, 115456, 131840, 148224, 181248, 181504, 183552, 185856, 186112, 186368}, 186624},
    {4097, 1, 1, 1, {0, 256, 512, 768, 50176, 99584, 116224, 132864, 149504, 182528, 182784, 186880, 191232, 191488, 191744}, 192000},
    {0, 257, 1, 1, {0, 2304, 4608, 5888, 5888, 5888, 5888, 5888, 5888, 6144, 6400, 6400, 6656, 6912, 7168}, 7424},
    {1, 257, 1, 1, {0, 2304, 4608, 5888, 6144, 6400, 6656, 6912, 7168, 7424, 7680, 9728, 12032, 12288, 12544}, 12800},
    {4096, 257, 1, 1, {0, 2304, 4608, 5888, 55040, 104192, 120576, 136960, 153344, 186368, 186624, 188672, 190976, 191232, 191488}, 191744},
    {4097, 257, 1, 1, {0, 2304, 4608, 5888, 55296, 104704, 121344, 137984, 154624, 187648, 187904, 192000, 196352, 196608, 196864}, 197120},
    {0, 1, 257, 1, {0, 256, 512, 768, 768, 768, 768, 768, 768, 1024, 3328, 3328, 3584, 3840, 6144}, 7424},
    {1, 1, 257, 1, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 4608, 6656, 8960, 9216, 11520}, 12800},
    {4096, 1, 257, 1, {0, 256, 512, 768, 49920, 99072, 115456, 131840, 148224, 181248, 183552, 185600, 187904, 188160, 190464}, 191744},
    {4097, 1, 257, 1, {0, 256, 512, 768, 50176, 99584, 116224, 132864, 149504, 182528, 184832, 188928, 193280, 193536, 195840}, 197120},
    {0, 257, 257, 1, {0, 2304, 4608, 5888, 5888, 5888, 5888, 5888, 5888, 6144, 8448, 8448, 8704, 8960, 11264}, 12544},
    {1, 257, 257, 1, {0, 2304, 4608, 5888, 6144, 6400, 6656, 6912, 7168, 7424, 9728, 11776, 14080, 14336, 16640}, 17920},
    {4096, 257, 257, 1, {0, 2304, 4608, 5888, 55040, 104192, 120576, 136960, 153344, 186368, 188672, 190720, 193024, 193280, 195584}, 196864},
    {4097, 257, 257, 1, {0, 2304, 4608, 5888, 55296, 104704, 121344, 137984, 154624, 187648, 189952, 194048, 198400, 198656, 200960}, 202240},
};

struct PhraseRow { uint64_t n; uint32_t nq; size_t off[17], total; };
// n nq | q_anchor q_run q_probes base qstart flags plen pdoc pq hpf order skey hit scan hist hist_scan partials | total
const PhraseRow kPhrase[] = {
    {0, 1, {0, 256, 512, 768, 1024, 1280, 1280, 1280, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 1536, 1792}, 2048},
    {1, 1, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 5632, 7936}, 8192},
    {4096, 1, {0, 256, 512, 768, 1024, 1280, 17664, 34048, 50432, 66816, 83200, 99584, 115968, 165120, 198144, 200192, 202496}, 202752},
    {4097, 1, {0, 256, 512, 768, 1024, 1280, 17920, 34560, 51200, 67840, 84480, 101120, 117760, 167168, 200192, 204288, 208640}, 208896},
    {0, 257, {0, 1280, 3584, 5888, 8192, 10496, 10496, 10496, 10496, 10496, 10496, 10496, 10496, 10496, 10752, 10752, 11008}, 11264},
    {1, 257, {0, 1280, 3584, 5888, 8192, 10496, 10752, 11008, 11264, 11520, 11776, 12032, 12288, 12544, 12800, 14848, 17152}, 17408},
    {4096, 257, {0, 1280, 3584, 5888, 8192, 10496, 26880, 43264, 59648, 76032, 92416, 108800, 125184, 174336, 207360, 209408, 211712}, 211968},
    {4097, 257, {0, 1280, 3584, 5888, 8192, 10496, 27136, 43776, 60416, 77056, 93696, 110336, 126976, 176384, 209408, 213504, 217856}, 218112},
};

void check_layouts() {
    for (const PostingsRow& r : kPostings) {
        const PostingsScratch S(r.n);
        Got g[8] = {got(S.keydoc), got(S.order), got(S.skey), got(S.flags), got(S.scan)};
        tail(S.tail, g + 5);
        check_sections(g, r.off, 8, S.bytes(), r.total);
    }
    for (const MergeOrderedRow& r : kMergeOrdered) {
        const MergeScratch<Seg, PosSeg> S(r.K, r.n, uint64_t(r.n_terms_out) + 1, r.positional != 0);
        const Got g[5] = {got(S.segs), got(S.psegs), got(S.range), got(S.table), got(S.ptable)};
        check_sections(g, r.off, 5, S.bytes(true), r.total);
    }
    for (const MergeGeneralRow& r : kMergeGeneral) {
        const MergeScratch<Seg, PosSeg> S(r.K, r.n, uint64_t(r.n_terms_out) + 1, r.positional != 0);
        Got g[13] = {got(S.segs), got(S.psegs), got(S.rec), got(S.order), got(S.skey), got(S.flags), got(S.scan), got(S.ptf), got(S.inv), got(S.pscan)};
        tail(S.tail, g + 10);
        check_sections(g, r.off, 13, S.bytes(false), r.total);
        CHECK(S.rec.offset == S.range.offset);   // the two routes lay out the same bytes behind the descriptors
    }
    for (const SearchRow& r : kSearch) {
        const SearchScratch S(r.n, r.ns, r.nq, r.boolean != 0);
        Got g[15] = {got(S.slot_df), got(S.base), got(S.slot_query), got(S.rec), got(S.hit), got(S.order), got(S.skey), got(S.flags), got(S.scan), got(S.qstart)};
        Got* rest = tail(S.tail, g + 10);
        rest[0] = got(S.q_anchor); rest[1] = got(S.q_flags);
        check_sections(g, r.off, 15, S.bytes(), r.total);
        CHECK(r.boolean || (S.q_anchor.count == 0 && S.q_flags.count == 0));
    }
    for (const PhraseRow& r : kPhrase) {
        const PhraseScratch S(r.n, r.nq);
        Got g[17] = {got(S.q_anchor), got(S.q_run), got(S.q_probes), got(S.base), got(S.qstart), got(S.flags), got(S.plen), got(S.pdoc), got(S.pq), got(S.hpf),
                     got(S.order), got(S.skey), got(S.hit), got(S.scan)};
        tail(S.tail, g + 14);
        check_sections(g, r.off, 17, S.bytes(), r.total);
    }
}
}  // namespace

int main() {
    check_carver();
    check_passes();
    check_tail();
    check_layouts();
    std::printf("ok %llu %llu\n", g_layouts, g_sections);
    return 0;
}
