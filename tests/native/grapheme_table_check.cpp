// TEST INFRASTRUCTURE: walks every scalar value 0 .. 0x10FFFF through the host-built two-stage class table the device reads
// (vaporetto_amd/csrc/tables.hpp: grapheme_table_host, grapheme_class) and compares it with grapheme_detail::class_of of
// include/vaporetto_grapheme.hpp.  Prints the table's size and "ok", or the first scalar values that differ.
#include <cstdio>

#include "tables.hpp"
#include "vaporetto_grapheme.hpp"

int main() {
    const std::vector<uint8_t>& t = vpt::grapheme_table_host();
    if (t.size() < vpt::kGraphemeBlocksAt + 256 || (t.size() - vpt::kGraphemeBlocksAt) % 256 != 0) { std::printf("size %zu\n", t.size()); return 1; }
    const size_t n_blocks = (t.size() - vpt::kGraphemeBlocksAt) / 256;
    for (uint32_t b = 0; b < vpt::kGraphemeStage1; ++b)
        if (size_t(t[2 * b]) + (size_t(t[2 * b + 1]) << 8) >= n_blocks) { std::printf("stage1[%u] names no block\n", b); return 1; }
    int bad = 0;
    for (uint32_t cp = 0; cp <= 0x10FFFFu; ++cp) {
        const uint32_t got = vpt::grapheme_class(t.data(), cp), want = vaporetto_hip::grapheme_detail::class_of(cp);
        if (got != want && ++bad <= 8) std::printf("U+%04X: table %u, class_of %u\n", cp, got, want);
    }
    if (vpt::grapheme_class(t.data(), 0x110000u) != 0 || vpt::grapheme_class(t.data(), 0x1FFFFFu) != 0) { std::printf("past U+10FFFF\n"); return 1; }
    if (bad) return 1;
    std::printf("bytes %zu blocks %zu\nok\n", t.size(), n_blocks);
    return 0;
}
