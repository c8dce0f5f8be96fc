"""Phrase clauses in boolean queries on the MI355X through the C ABI: the lists launch of kernels_postings_phrase.hip behind the phrase
search's, the kernels of kernels_postings_boolean.hip over a segment and derived lists, the two host calls, Postings.clause_search and
VaporettoTokenizer.boolean_search(phrases=True) against the definition of tests/clauseref.py and against the calls they are made of -- the
checks of tests/clausesuite.py.  Only sound inputs and the declared capacity and limit errors run here; the hostile lists run on the
emulator (tests/test_postings_clause_emu.py)."""
import pytest

from tests import clausesuite, vocabsuite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def fresh_predictor():
    vocabsuite._PRED.clear()
    yield
    vocabsuite._PRED.clear()


def test_no_lists_gives_the_bytes_of_the_boolean_search():
    clausesuite.check_no_lists_is_the_boolean_search()


def test_lists_of_one_term_phrases_are_the_terms_lists_and_search_as_the_terms():
    clausesuite.check_one_term_phrases_are_the_terms_lists()


def test_one_should_slot_naming_a_list_gives_the_bytes_of_the_phrase_search():
    clausesuite.check_one_should_slot_is_the_phrase_search()


def test_random_mixed_queries_over_a_postings_pass_positional_segment():
    clausesuite.check_random()


def test_addition_order_with_the_phrase_clause_first_in_the_middle_and_last():
    clausesuite.check_addition_order()


def test_anchor_choice_unmatched_phrases_vetoes_and_a_repeated_term():
    clausesuite.check_anchor_choice()


def test_a_phrase_at_the_term_limit_and_one_term_more():
    clausesuite.check_phrase_limit()


@pytest.mark.parametrize("n", ["T-1", "T", "T+1", "3T+1"])
def test_probes_entries_and_places_on_the_tile_edges_and_the_capacities(n):
    clausesuite.check_tile_edges(clausesuite.postingssuite.token_count(n))


@pytest.mark.parametrize("base", clausesuite.postingssuite.HIGH_BASES)
def test_documents_on_both_sides_of_2_31_and_up_to_the_last_document_word(base):
    clausesuite.check_high_documents(base)


def test_merged_positional_segment_postings_clause_search_and_the_phrases_keyword():
    clausesuite.check_tokenizer()


def test_an_error_of_the_lists_call_leaves_the_chained_clause_search_outputs_untouched():
    clausesuite.check_chained_errors()


def test_errors_at_the_call():
    clausesuite.check_errors()


def test_two_runs_and_a_second_workspace_give_identical_bytes():
    clausesuite.check_determinism()


def test_one_workspace_alternated_with_the_other_postings_calls_gives_the_bytes_of_fresh_ones():
    clausesuite.check_scratch_reuse()


def test_host_calls_and_postings_clause_search():
    clausesuite.check_host_call()
