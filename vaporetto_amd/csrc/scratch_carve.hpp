// One allocation carved into consecutive 256-byte-aligned sections, and the five layouts the postings drivers (capi_device.cpp) carve out of a
// workspace's d_post.  A section is taken ONCE, its element type and its count together; the carver then knows the total to allocate, and the
// section gives the typed pointer into the allocation.  Two layouts over the same bytes: copy the carver where they part and go on with both.
// Free of HIP: tests/native/scratch_carve_test.cpp builds this header alone and holds every offset below to numbers written out there.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace vpt {   // (kernels.hpp) what train_radix_sort wants for n items: histogram words; what train_scan wants for n items: partials
uint64_t train_radix_scratch(uint64_t n);
uint64_t train_scan_scratch(uint64_t n);
}  // namespace vpt

namespace vptcarve {

constexpr size_t kSectionAlign = 256;

template <typename T>
struct Section;

struct Carver {
    size_t end = 0;   // where the next section starts: a multiple of kSectionAlign
    template <typename T>
    Section<T> take(size_t count);
    size_t bytes() const { return end; }   // of every section taken so far
};

template <typename T>
struct Section {
    size_t offset, count;
    Section(Carver& c, size_t n) : offset(c.end), count(n) { c.end += (sizeof(T) * n + kSectionAlign - 1) & ~(kSectionAlign - 1); }   // (n 0: no byte)
    T* at(unsigned char* m) const { return reinterpret_cast<T*>(m + offset); }
};
template <typename T>
Section<T> Carver::take(size_t count) { return Section<T>(*this, count); }

// What train_radix_sort over n places and the train_scans of the same call work in: hist | hist_scan | partials, the partials long enough for
// a scan over the histograms, one over the n places and one over each of more_scans.
struct SortTail {
    Section<uint64_t> hist, hist_scan, partials;
    SortTail(Carver& c, uint64_t n, std::initializer_list<uint64_t> more_scans = {})
        : hist(c, size_t(vpt::train_radix_scratch(n))), hist_scan(c, hist.count + 1), partials(c, scan_words(hist.count, n, more_scans) + 1) {}
    static size_t scan_words(uint64_t nh, uint64_t n, std::initializer_list<uint64_t> more_scans) {
        uint64_t w = std::max(vpt::train_scan_scratch(nh), vpt::train_scan_scratch(n));
        for (const uint64_t m : more_scans) w = std::max(w, vpt::train_scan_scratch(m));
        return size_t(w);
    }
};

// A radix pass list (train_radix_sort's word_shifts: u32 word << 8 | bit shift, least significant digit first).
struct PassList {
    uint32_t v[8], n = 0;
    // the bytes of the values 0 .. max_value of `word`, least significant first, at most `cap` of them
    void add(uint32_t word, uint64_t max_value, uint32_t cap = 4) {
        for (uint32_t k = 0; max_value && k < cap && n < 8; max_value >>= 8, ++k) v[n++] = (word << 8) | (8 * k);
    }
};

// ---- the layouts (members are carved in the order they are declared)

// vpt_postings_batch_device (PostingsParams), n token places
struct PostingsScratch {
    const size_t n;
    Carver c{};
    Section<uint32_t> keydoc{c, 2 * n}, order{c, n}, skey{c, n}, flags{c, n};
    Section<uint64_t> scan{c, n + 1};
    SortTail tail{c, n};
    explicit PostingsScratch(uint64_t places) : n(size_t(places)) {}
    size_t bytes() const { return c.bytes(); }
};

// vpt_postings_merge_device and, positional, vpt_postings_merge_positional_device (PostingsMergeParams, PostingsMergePosParams): K segments
// (Seg, PosSeg: their descriptors), n places, rows of `row` term bounds.  Behind the descriptors the ordered route (o) and the general route
// (g) lay out the same bytes; what only the positional merge has is a section of count 0 in the plain one.
template <typename Seg, typename PosSeg>
struct MergeScratch {
    const size_t K, n, row;
    const bool positional;
    Carver c{};
    Section<Seg> segs{c, K};
    Section<PosSeg> psegs{c, positional ? K : 0};
    Carver o{c};
    Section<uint32_t> range{o, 2 * K};
    Section<uint64_t> table{o, K * row}, ptable{o, positional ? K * row : 0};
    Carver g{c};
    Section<uint32_t> rec{g, 3 * n}, order{g, n}, skey{g, n}, flags{g, n};
    Section<uint64_t> scan{g, n + 1};
    Section<uint32_t> ptf{g, positional ? n : 0}, inv{g, positional ? n : 0};
    Section<uint64_t> pscan{g, positional ? n + 1 : 0};
    SortTail tail{g, n};
    MergeScratch(uint32_t n_segments, uint64_t places, uint64_t term_bounds, bool with_positions)
        : K(n_segments), n(size_t(places)), row(size_t(term_bounds)), positional(with_positions) {}
    size_t bytes(bool ordered) const { return ordered ? o.bytes() : g.bytes(); }
};

// vpt_postings_search_device and, boolean, vpt_postings_boolean_search_device and vpt_postings_clause_search_device (PostingsSearchParams,
// PostingsBooleanParams; the clause search's derived lists are the caller's arrays, not scratch): n candidate places, ns slots, nq queries
struct SearchScratch {
    const size_t n, ns, nq;
    const bool boolean;
    Carver c{};
    Section<uint64_t> slot_df{c, ns}, base{c, ns + 1};
    Section<uint32_t> slot_query{c, ns}, rec{c, 3 * n}, hit{c, 3 * n}, order{c, n}, skey{c, n}, flags{c, n};
    Section<uint64_t> scan{c, n + 1}, qstart{c, nq + 1};
    SortTail tail{c, n, {ns}};
    Section<uint64_t> q_anchor{c, boolean ? nq : 0};
    Section<uint32_t> q_flags{c, boolean ? nq : 0};
    SearchScratch(uint64_t places, uint64_t slots, uint32_t queries, bool with_occurs)
        : n(size_t(places)), ns(size_t(slots)), nq(queries), boolean(with_occurs) {}
    size_t bytes() const { return c.bytes(); }
};

// vpt_postings_phrase_search_device and vpt_postings_phrase_lists_device (PostingsPhraseParams; the lists call leaves hpf, order, skey, hit
// and the sort's histograms idle): n probe places, nq queries
struct PhraseScratch {
    const size_t n, nq;
    Carver c{};
    Section<uint32_t> q_anchor{c, nq};
    Section<uint64_t> q_run{c, nq}, q_probes{c, nq}, base{c, nq + 1}, qstart{c, nq + 1};
    Section<uint32_t> flags{c, n}, plen{c, n}, pdoc{c, n}, pq{c, n}, hpf{c, n}, order{c, n}, skey{c, n}, hit{c, 3 * n};
    Section<uint64_t> scan{c, n + 1};
    SortTail tail{c, n, {nq}};
    PhraseScratch(uint64_t places, uint32_t queries) : n(size_t(places)), nq(queries) {}
    size_t bytes() const { return c.bytes(); }
};

}  // namespace vptcarve
