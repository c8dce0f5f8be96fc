// Example of vaporetto_tantivy's token stream over the C ABI (include/vaporetto_hip.hpp, VaporettoTokenizer): documents in, token byte spans out.
//   g++ -O2 -std=c++17 -Iinclude -o token_stream examples/token_stream.cpp -Lvaporetto_amd/lib -lvaporetto_hip -Wl,-rpath,'$ORIGIN/vaporetto_amd/lib'
//   ./token_stream model.bin [wsconst] < documents.txt       (one document per line; wsconst: chars of DRHTKOG, vaporetto_tantivy/src/lib.rs:69-86)
// One line per token: doc <TAB> position <TAB> offset_from <TAB> offset_to <TAB> text   (byte offsets into the document, as tantivy's Token holds them)
//   ./token_stream model.bin wsconst --tags [slot:tag ...] < documents.txt
// With --tags (beyond the adapter): the predictor predicts tags, every line continues with position_length and one field per tag slot ("*": None),
// and the tokens whose slot carries one of the listed tags are dropped -- position and position_length stay those before filtering.
//   ./token_stream model.bin wsconst --vocab vocab.txt < documents.txt
// With --vocab (beyond the adapter): vocab.txt holds one surface per line, line k is id k; one line per token: doc <TAB> index <TAB> id, the id of
// the token's surface (of the text as it was scored: through KyteaFullwidthFilter) or -1 -- looked up on the device, no token text comes back.
//   ./token_stream model.bin wsconst --build-vocab [min_count] < documents.txt
// With --build-vocab (beyond the adapter): the documents' token surfaces (of the text as it was scored) are counted on the device; one line per
// surface of count >= min_count: count <TAB> surface, most frequent first -- the second column is a vocab.txt for --vocab.
//   ./token_stream model.bin wsconst --postings vocab.txt [doc_base] < documents.txt
// With --postings (beyond the adapter): the documents are one segment; one line per posting, by term, then by document:
// term <TAB> document <TAB> tf, the document being doc_base + the line's index; then one line "dropped <TAB> n" for the tokens that are no entry.
//   ./token_stream model.bin wsconst --postings vocab.txt [doc_base] --segment-docs N < documents.txt
// With --segment-docs N: N documents are indexed a segment, and the segments are merged on the device; the output is the same.
//   ./token_stream model.bin wsconst --postings vocab.txt [doc_base] [--segment-docs N] --search "QUERY" [--top K] < documents.txt
// With --search: the query text is tokenised as a document is, its tokens are weighted with BM25's idf and the K (default 10) best documents of
// the index are found on the device; one line per hit, best first: document <TAB> the score's bits in hex <TAB> the score.
//   ./token_stream model.bin wsconst --postings vocab.txt [doc_base] [--segment-docs N] --phrase "QUERY" [--top K] < documents.txt
// With --phrase: the documents are indexed with positions, the query text is ONE phrase -- its tokens at consecutive positions, in order -- and
// the K best documents that hold it are found on the device; the lines of --search, plus <TAB> the phrase's occurrences in the document.
//   ./token_stream model.bin wsconst --postings vocab.txt [doc_base] [--segment-docs N] --boolean "QUERY" [--top K] < documents.txt
// With --boolean: the query text is split on spaces into clauses, +clause is required, -clause is forbidden, any other is wanted; every token
// of a clause takes the clause's occur; the lines of --search.
//   ./token_stream model.bin wsconst --postings vocab.txt [doc_base] [--segment-docs N] --boolean "QUERY" [--top K] --phrases < documents.txt
// With --phrases as the last argument: the documents are indexed with positions and a clause of several tokens is ONE exact phrase.
//   ... --phrase "QUERY" [--top K] --slop N          ... --boolean "QUERY" [--top K] --slop N --phrases
// With --slop N behind --phrase (as the last argument) or in front of --phrases: the phrase, or every phrase clause, may be off by N (0 .. 31)
// positions in all, as tantivy's PhraseQuery::set_slop; the same lines.
// With --segment-docs N the positional segments of N documents each are merged on the device with their position lists (the same lines come
// out; stderr tells "segments <TAB> n <TAB> postings <TAB> n <TAB> positions <TAB> n").
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "vaporetto_hip.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s model.bin [wsconst] < documents\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    try {
        if (argc > 3 && std::strcmp(argv[3], "--tags") == 0) {
            vaporetto_hip::TagStopFilter::Pairs stop;
            for (int a = 4; a < argc; ++a) {
                const char* colon = std::strchr(argv[a], ':');
                if (!colon) { std::fprintf(stderr, "a stop tag is slot:tag\n"); return 2; }
                stop.emplace_back(uint32_t(std::strtoul(argv[a], nullptr, 10)), std::string(colon + 1));
            }
            vaporetto_hip::VaporettoTokenizer tagged(vaporetto_hip::Model::read_slice(bytes.data(), bytes.size()).first, argv[2], 0, true, {}, stop);
            std::vector<std::string> docs;
            for (std::string l; std::getline(std::cin, l);) docs.push_back(l);
            const auto streams = tagged.token_stream_batch(docs);
            for (size_t d = 0; d < streams.size(); ++d)
                for (const vaporetto_hip::Token& t : streams[d]) {
                    std::printf("%zu\t%zu\t%zu\t%zu\t%s\t%zu", d, t.position, t.offset_from, t.offset_to, t.text.c_str(), t.position_length);
                    for (const auto& tag : t.tags) std::printf("\t%s", tag ? tag->c_str() : "*");
                    std::printf("\n");
                }
            return 0;
        }
        if (argc > 4 && std::strcmp(argv[3], "--vocab") == 0) {
            std::ifstream vf(argv[4]);
            std::vector<std::string> surfaces;
            for (std::string l; std::getline(vf, l);) surfaces.push_back(l);
            vaporetto_hip::VaporettoTokenizer plain(vaporetto_hip::Model::read_slice(bytes.data(), bytes.size()).first, argv[2]);
            const vaporetto_hip::Vocabulary vocab(plain.predictor(), surfaces);
            std::vector<std::string> docs;
            for (std::string l; std::getline(std::cin, l);) docs.push_back(l);
            const auto enc = plain.encode(docs, vocab);
            for (size_t d = 0; d < docs.size(); ++d)
                for (uint64_t k = enc.first[d]; k < enc.first[d + 1]; ++k)
                    std::printf("%zu\t%zu\t%d\n", d, size_t(k - enc.first[d]), int(enc.second[size_t(k)]));
            return 0;
        }
        if (argc > 4 && std::strcmp(argv[3], "--postings") == 0) {
            std::ifstream vf(argv[4]);
            std::vector<std::string> surfaces;
            for (std::string l; std::getline(vf, l);) surfaces.push_back(l);
            vaporetto_hip::VaporettoTokenizer plain(vaporetto_hip::Model::read_slice(bytes.data(), bytes.size()).first, argv[2]);
            const vaporetto_hip::Vocabulary vocab(plain.predictor(), surfaces);
            std::vector<std::string> docs;
            for (std::string l; std::getline(std::cin, l);) docs.push_back(l);
            size_t segment_docs = 0;
            int n_args = argc;
            const char* query = nullptr;
            const char* phrase = nullptr;
            const char* boolean = nullptr;
            uint32_t top = 10;
            bool phrases = false;
            uint32_t slop = 0;
            if (n_args > 7 && std::strcmp(argv[n_args - 1], "--phrases") == 0) { phrases = true; n_args -= 1; }
            if (n_args > 8 && std::strcmp(argv[n_args - 2], "--slop") == 0) { slop = uint32_t(std::strtoul(argv[n_args - 1], nullptr, 10)); n_args -= 2; }
            if (n_args > 6 && std::strcmp(argv[n_args - 2], "--top") == 0) { top = uint32_t(std::strtoul(argv[n_args - 1], nullptr, 10)); n_args -= 2; }
            if (n_args > 6 && std::strcmp(argv[n_args - 2], "--segment-docs") == 0) { segment_docs = std::strtoull(argv[n_args - 1], nullptr, 10); n_args -= 2; }   // (behind the query, too)
            if (n_args > 6 && std::strcmp(argv[n_args - 2], "--search") == 0) { query = argv[n_args - 1]; n_args -= 2; }
            else if (n_args > 6 && std::strcmp(argv[n_args - 2], "--phrase") == 0) { phrase = argv[n_args - 1]; n_args -= 2; }
            else if (n_args > 6 && std::strcmp(argv[n_args - 2], "--boolean") == 0) { boolean = argv[n_args - 1]; n_args -= 2; }
            if (n_args > 6 && std::strcmp(argv[n_args - 2], "--segment-docs") == 0) { segment_docs = std::strtoull(argv[n_args - 1], nullptr, 10); n_args -= 2; }
            const uint64_t doc_base = n_args > 5 ? std::strtoull(argv[5], nullptr, 10) : 0;
            vaporetto_hip::Postings post;
            if (phrase || (boolean && phrases)) {
                if (segment_docs) {
                    std::vector<std::vector<std::string>> batches;
                    for (size_t a = 0; a < docs.size(); a += segment_docs)
                        batches.emplace_back(docs.begin() + a, docs.begin() + std::min(docs.size(), a + segment_docs));
                    post = plain.index(batches, vocab, doc_base, true, true);
                    std::fprintf(stderr, "segments\t%zu\tpostings\t%zu\tpositions\t%zu\n", batches.size(), post.docs.size(), post.positions.size());
                } else {
                    post = plain.index(docs, vocab, doc_base, true, true);
                }
                if (boolean) {
                    const auto found = plain.boolean_search(post, vocab, {std::string(boolean)}, plain.doc_lens(docs, vocab), doc_base, top, 1.2f, 0.75f, true, true, slop);
                    for (const vaporetto_hip::Postings::Hit& h : found.hits[0]) {
                        uint32_t bits;
                        std::memcpy(&bits, &h.score, 4);
                        std::printf("%u\t%08x\t%.9g\n", unsigned(h.document), unsigned(bits), double(h.score));
                    }
                    return 0;
                }
                const auto found = plain.phrase_search(post, vocab, {std::string(phrase)}, plain.doc_lens(docs, vocab), doc_base, top, 1.2f, 0.75f, true, slop);
                for (const vaporetto_hip::Postings::PhraseHit& h : found.hits[0]) {
                    uint32_t bits;
                    std::memcpy(&bits, &h.score, 4);
                    std::printf("%u\t%08x\t%.9g\t%u\n", unsigned(h.document), unsigned(bits), double(h.score), unsigned(h.freq));
                }
                return 0;
            }
            if (segment_docs) {
                std::vector<std::vector<std::string>> batches;
                for (size_t a = 0; a < docs.size(); a += segment_docs)
                    batches.emplace_back(docs.begin() + a, docs.begin() + std::min(docs.size(), a + segment_docs));
                post = plain.index(batches, vocab, doc_base);
            } else {
                post = plain.index(docs, vocab, doc_base);
            }
            if (query || boolean) {
                const auto found = query ? plain.search(post, vocab, {std::string(query)}, plain.doc_lens(docs, vocab), doc_base, top)
                                         : plain.boolean_search(post, vocab, {std::string(boolean)}, plain.doc_lens(docs, vocab), doc_base, top);
                for (const vaporetto_hip::Postings::Hit& h : found.hits[0]) {
                    uint32_t bits;
                    std::memcpy(&bits, &h.score, 4);
                    std::printf("%u\t%08x\t%.9g\n", unsigned(h.document), unsigned(bits), double(h.score));
                }
                return 0;
            }
            for (size_t k = 0; k < post.n_terms(); ++k)
                for (uint64_t q = post.term_offsets[k]; q < post.term_offsets[k + 1]; ++q)
                    std::printf("%zu\t%u\t%u\n", k, unsigned(post.docs[size_t(q)]), unsigned(post.tfs[size_t(q)]));
            std::printf("dropped\t%llu\n", static_cast<unsigned long long>(post.n_dropped));
            return 0;
        }
        if (argc > 3 && std::strcmp(argv[3], "--build-vocab") == 0) {
            vaporetto_hip::VaporettoTokenizer plain(vaporetto_hip::Model::read_slice(bytes.data(), bytes.size()).first, argv[2]);
            vaporetto_hip::VocabularyCounter counter(plain.predictor(), uint64_t(1) << 20);
            std::vector<std::string> docs;
            for (std::string l; std::getline(std::cin, l);) docs.push_back(l);
            plain.count(docs, counter);
            for (const auto& e : counter.entries(argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 1))
                std::printf("%llu\t%s\n", static_cast<unsigned long long>(e.second), e.first.c_str());
            return 0;
        }
        vaporetto_hip::VaporettoTokenizer tokenizer(vaporetto_hip::Model::read_slice(bytes.data(), bytes.size()).first, argc > 2 ? argv[2] : "");
        std::vector<std::string> docs;
        for (std::string l; std::getline(std::cin, l);) docs.push_back(l);
        const auto streams = tokenizer.token_stream_batch(docs);
        for (size_t d = 0; d < streams.size(); ++d)
            for (const vaporetto_hip::Token& t : streams[d])
                std::printf("%zu\t%zu\t%zu\t%zu\t%s\n", d, t.position, t.offset_from, t.offset_to, t.text.c_str());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
