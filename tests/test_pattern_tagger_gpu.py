"""PatternMatchTagger on the MI355X through the C ABI: kernels_pattern.hip, the rule table and every entry point of
vpt_pattern_tagger_* against the host form -- the checks of tests/patterntagsuite.py."""
import pytest

from tests import patterntagsuite

pytestmark = pytest.mark.gpu


def test_reference_known_answer():
    patterntagsuite.check_reference_kat()


def test_only_the_none_slots_of_a_tagged_token_are_filled():
    patterntagsuite.check_none_slots_only()


def test_tokens_without_a_tag_model_get_records_of_their_own():
    patterntagsuite.check_tokens_without_model()


def test_the_whole_surface_or_nothing():
    patterntagsuite.check_exact_match()


def test_probe_chains_and_the_last_duplicate():
    patterntagsuite.check_probe_chains()


def test_edges_of_sentences_steps_and_batches():
    patterntagsuite.check_edges()


def test_full_runs_of_256_short_sentences():
    patterntagsuite.check_full_runs()


def test_surfaces_are_those_of_the_scored_text():
    patterntagsuite.check_fullwidth()


def test_no_tag_models_no_slots():
    patterntagsuite.check_no_tag_models()


def test_record_order_through_writer_and_pipeline_on_the_golden_model():
    patterntagsuite.check_golden_pipeline()


def test_listing_prints_rule_tags_and_no_candidates_for_them():
    patterntagsuite.check_listing()


def test_errors_by_message():
    patterntagsuite.check_errors()


def test_python_mirror_resolves_rule_tags():
    patterntagsuite.check_python_mirror()
