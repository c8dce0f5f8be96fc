"""The sloppy phrase search and the sloppy phrase lists on the MI355X through the C ABI: phrase_probe_kernel<true> of
kernels_postings_phrase.hip in front of the exact search's launches, the host calls, Postings.phrase_search(slop=), clause_search(slop=) and
the tokenizer's keywords against the definition of tests/sloppyref.py -- the checks of tests/sloppysuite.py.  (The hostile inputs run here in
the form that has run on the emulator, tests/test_postings_sloppy_emu.py: every kernel loop is bounded by a count, every index is bounded
before use, nothing waits.)"""
import pytest

from tests import sloppysuite, vocabsuite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def fresh_predictor():
    vocabsuite._PRED.clear()
    yield
    vocabsuite._PRED.clear()


def test_the_documented_cases_of_set_slop_at_slops_0_1_2_and_both_forms_of_the_definition_agree():
    sloppysuite.check_documented_cases()


def test_every_slop_zero_and_a_null_slops_pointer_give_the_exact_calls_bytes():
    sloppysuite.check_slop_zero()


def test_the_result_does_not_depend_on_the_anchor():
    sloppysuite.check_anchor_independence()


def test_anchor_positions_closer_than_the_slop_every_occurrence_is_counted_by_one_lane():
    sloppysuite.check_one_lane_per_occurrence()


def test_negative_occurrences_and_positions_up_to_the_last_word_with_64_slots_and_slop_31():
    sloppysuite.check_signs_and_the_top_of_the_range()


def test_slops_0_1_31_in_one_batch_a_slop_of_32_is_an_error_at_sync_64_slots_and_a_repeated_term():
    sloppysuite.check_limits()


@pytest.mark.parametrize("n", ["T-1", "T", "T+1", "3T+1"])
def test_probes_on_the_tile_edges_with_a_posting_across_a_workgroup_edge_and_the_sort_tile_edge(n):
    sloppysuite.check_probes(sloppysuite.postingssuite.token_count(n))


def test_ties_cut_by_k_k_above_the_matches_and_four_doc_bases_at_slop_2():
    sloppysuite.check_topk()


@pytest.mark.parametrize("base", sloppysuite.postingssuite.HIGH_BASES)
def test_documents_on_both_sides_of_2_31_and_up_to_the_last_document_word_at_slop_2(base):
    sloppysuite.check_high_documents(base)


def test_capacity_probes_too_small_is_an_error_at_sync_with_the_number_needed():
    sloppysuite.check_capacity()


def test_errors_at_the_call():
    sloppysuite.check_errors()


def test_two_runs_and_a_second_workspace_give_identical_bytes():
    sloppysuite.check_determinism()


def test_hostile_input_is_an_error_at_sync_or_a_bounded_result_and_touches_nothing_outside():
    assert sloppysuite.run_hostile() == sloppysuite.N_HOSTILE


def test_a_sloppy_list_in_a_should_slot_is_the_sloppy_search_and_mixed_clauses_against_clauseref():
    sloppysuite.check_clause_identities()


def test_host_calls_postings_phrase_search_and_clause_search_with_slop():
    sloppysuite.check_host_calls()


def test_tokenizer_phrase_search_and_boolean_search_with_slop():
    sloppysuite.check_tokenizer()
