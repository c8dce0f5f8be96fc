"""PatternMatchTagger, the host form (api.PatternMatchTagger.filter): the reference's own known-answer test
(vaporetto_rules/src/sentence_filters/pattern_match_tagger.rs:49-74) and the semantics the device form is compared with."""
from tests import patterntagsuite
from vaporetto_amd import api


def test_reference_known_answer():
    patterntagsuite.check_reference_kat()


def test_some_slots_stay_and_none_entries_leave_none():
    s = api.Sentence.from_tokenized("a/x b c//z d")
    api.PatternMatchTagger({"a": ["no", "A1"], "b": [None, "B1", "ignored"], "c": ["C0"], "d": []}).filter(s)
    assert s.write_tokenized_text() == "a/x/A1 b//B1 c/C0/z d"


def test_an_empty_tag_is_some_and_prints_a_trailing_slash():
    s = api.Sentence.from_tokenized("a/x/y b")
    api.PatternMatchTagger({"b": ["t", ""]}).filter(s)
    assert s.tags()[-2:] == ["t", ""] and s.write_tokenized_text() == "a/x/y b/t/"


def test_no_slots_no_tags():
    s = api.Sentence.from_tokenized("a b")
    api.PatternMatchTagger({"a": ["t"]}).filter(s)
    assert s.n_tags() == 0 and s.write_tokenized_text() == "a b"


def test_a_repeated_surface_keeps_the_last_rule():
    s = api.Sentence.from_tokenized("a/x b")
    api.PatternMatchTagger([("b", ["first"]), ("b", ["last"])]).filter(s)
    assert s.write_tokenized_text() == "a/x b/last"
