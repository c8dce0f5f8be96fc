"""The BM25 top-k search with MUST / SHOULD / MUST_NOT slots on the MI355X through the C ABI: the launches of kernels_postings_boolean.hip in
front of the OR search's, the host call, Postings.boolean_search and VaporettoTokenizer.boolean_search against the definition of
tests/boolref.py -- the checks of tests/boolsuite.py.  (The hostile inputs run here in the form that has run on the emulator,
tests/test_postings_boolean_emu.py: every kernel loop is bounded, every index is clamped before use, nothing waits.)"""
import pytest

from tests import boolsuite, vocabsuite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def fresh_predictor():
    vocabsuite._PRED.clear()
    yield
    vocabsuite._PRED.clear()


def test_all_should_queries_give_the_bytes_of_the_or_search():
    boolsuite.check_all_should_is_the_or_search()


def test_random_mixed_queries_over_a_postings_pass_segment():
    boolsuite.check_random()


def test_addition_order_with_the_anchor_first_in_the_middle_and_last():
    boolsuite.check_addition_order()


def test_anchor_choice_dead_must_only_must_not_empty_queries_and_repeated_terms():
    boolsuite.check_anchor_choice()


def test_the_slot_limit_on_both_routes_and_one_slot_more():
    boolsuite.check_slot_limit()


def test_bisection_edges_in_the_lists_that_deal_out_no_places():
    boolsuite.check_bisection_edges()


@pytest.mark.parametrize("n", ["T-1", "T", "T+1", "3T+1"])
def test_places_on_the_tile_edges_on_both_routes_and_k_cuts_a_tie_group(n):
    boolsuite.check_places(boolsuite.postingssuite.token_count(n))


@pytest.mark.parametrize("base", boolsuite.postingssuite.HIGH_BASES)
def test_documents_on_both_sides_of_2_31_and_up_to_the_last_document_word(base):
    boolsuite.check_high_documents(base)


def test_merged_segment_searched_equals_one_pass_segment_searched_and_the_clause_syntax():
    boolsuite.check_merged_segment()


def test_zero_weights_k1_zero_b_zero_b_one_and_a_document_of_length_zero():
    boolsuite.check_weights_and_parameters()


def test_capacity_too_small_is_an_error_at_sync_with_the_places_needed():
    boolsuite.check_capacity()


def test_errors_at_the_call():
    boolsuite.check_errors()


def test_occur_values_above_2_are_an_error_at_sync_with_the_outputs_untouched():
    boolsuite.check_bad_occurs()


def test_hostile_input_is_an_error_at_sync_and_touches_nothing_outside():
    assert boolsuite.run_hostile() == boolsuite.N_HOSTILE


def test_two_runs_and_a_second_workspace_give_identical_bytes():
    boolsuite.check_determinism()


def test_one_workspace_through_the_five_scratch_layouts_gives_the_bytes_of_fresh_ones():
    boolsuite.check_scratch_reuse()


def test_host_call_and_postings_boolean_search():
    boolsuite.check_host_call()
