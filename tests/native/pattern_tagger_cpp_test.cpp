// Driver for vaporetto_hip::PatternMatchTagger (include/vaporetto_hip.hpp), built by tests/test_pattern_tagger_cpp.py against
// libvaporetto_hip.so (GPU) or the emulated build of the same sources (CPU tests).
//   pattern_tagger_cpp_test model.bin < lines     the rules of tests/patterntagsuite.py's case 1; prints, per line, the sentence's tags as
//   strings and its tokenized text, then the one-call tokenizer's lines, with the tagger and without
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "vaporetto_hip.hpp"

using namespace vaporetto_hip;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    try {
        Predictor predictor(Model::read_slice(bytes.data(), bytes.size()).first, true);
        const PatternMatchTagger::Rules rules = {{"漢字", {"RULE0", "RULE1", "RULE2"}}, {"う", {"no", "no", "no"}}, {"あい", {"never", "二", std::nullopt}},
                                                 {"AB", {std::nullopt, "", "sl/ash"}}, {"AB", {"last", std::nullopt, ""}}};
        const PatternMatchTagger tagger(predictor, rules);
        std::cout << "ids " << tagger.n_tags() << " suffix " << tagger.max_tag_suffix() << "\n";
        std::vector<std::string> lines;
        for (std::string l; std::getline(std::cin, l);) lines.push_back(l);
        for (const std::string& l : lines) {
            Sentence s = Sentence::from_raw(l);
            predictor.predict(s);
            s.fill_tags(&tagger);
            std::cout << "rule tags";
            for (int32_t v : s.tag_indices()) if (v <= -2) std::cout << " " << tagger.tag(uint32_t(-2 - v));
            std::cout << "\ntext " << s.write_tokenized_text(&tagger) << "\n";
            s.fill_tags();
            for (int32_t v : s.tag_indices()) if (v <= -2) { std::cout << "RULE TAG WITHOUT A TAGGER\n"; return 1; }
            std::cout << "plain " << s.write_tokenized_text() << "\n";
        }
        for (const std::string& t : predictor.tokenize(lines, true, 0, &tagger)) std::cout << "tokenize " << t << "\n";
        for (const std::string& t : predictor.tokenize(lines, true)) std::cout << "untagged " << t << "\n";
        try { PatternMatchTagger bad(predictor, {{"ok", {"t"}}, {"", {"t"}}}); } catch (const VaporettoError& e) { std::cout << "error " << e.kind() << " " << e.what() << "\n"; }
    } catch (const VaporettoError& e) {
        std::cout << "FAILED " << e.kind() << " " << e.what() << "\n";
        return 1;
    }
    return 0;
}
