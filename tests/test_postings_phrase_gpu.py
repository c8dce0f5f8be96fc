"""The position lists of a segment and the exact-phrase BM25 top-k search on the MI355X through the C ABI: the launches of
kernels_postings_phrase.hip with the trainer's sort and scan between them, the host calls, Postings.phrase_search,
Predictor.postings_packed(positions=True) and VaporettoTokenizer.phrase_search against the definitions of tests/postingsref.py and
tests/phraseref.py -- the checks of tests/phrasesuite.py.  (The hostile inputs run here in the form that has run on the emulator,
tests/test_postings_phrase_emu.py: every kernel loop is bounded, every index is clamped before use, nothing waits.)"""
import pytest

from tests import phrasesuite, vocabsuite
from vaporetto_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def fresh_predictor():
    vocabsuite._PRED.clear()
    yield
    vocabsuite._PRED.clear()


@pytest.mark.parametrize("n", ["T-1", "T", "T+1"])
def test_positions_of_a_segment_on_the_key_tile_edges_with_null_and_gapped_positions(n):
    t = api.Vocabulary.tile()
    phrasesuite.check_positions({"T-1": t - 1, "T": t, "T+1": t + 1}[n])


def test_positions_that_do_not_ascend_inside_a_posting_and_the_errors_at_the_call():
    phrasesuite.check_positions_errors()


def test_random_phrases_over_three_terms_and_a_device_made_segment():
    phrasesuite.check_random()


def test_repeated_terms_overlapping_occurrences_and_negative_starts():
    phrasesuite.check_repeats()


def test_position_gaps_break_a_phrase():
    phrasesuite.check_gaps()


def test_the_result_does_not_depend_on_the_anchor():
    phrasesuite.check_anchor_independence()


def test_a_phrase_of_one_slot_has_the_bits_of_the_or_search():
    phrasesuite.check_or_equivalence()


def test_slots_out_of_range_df0_empty_queries_and_the_length_limit():
    phrasesuite.check_query_edges()


def test_ties_cut_by_k_k_above_the_matches_and_two_doc_bases():
    phrasesuite.check_topk()


@pytest.mark.parametrize("n", ["T-1", "T", "T+1", "3T+1"])
def test_probes_on_the_tile_edges(n):
    phrasesuite.check_probes(phrasesuite.postingssuite.token_count(n))


def test_capacity_probes_too_small_is_an_error_at_sync_with_the_number_needed():
    phrasesuite.check_capacity()


def test_errors_at_the_call():
    phrasesuite.check_errors()


def test_hostile_input_is_an_error_at_sync_and_touches_nothing_outside():
    assert phrasesuite.run_hostile() == phrasesuite.N_HOSTILE


@pytest.mark.parametrize("base", phrasesuite.postingssuite.HIGH_BASES)
def test_documents_on_both_sides_of_2_31_and_up_to_the_last_document_word(base):
    phrasesuite.check_high_documents(base)   # (at the upper base with the two hostile postings, which have run on the emulator)


@pytest.mark.parametrize("n", ["T", "T+1", "2T+1"])
def test_k_cuts_a_tie_group_on_the_tile_edges_and_a_phrase_ends_on_them(n):
    phrasesuite.check_tile_edge_ties(phrasesuite.postingssuite.token_count(n))


def test_two_runs_and_a_second_workspace_give_identical_bytes():
    phrasesuite.check_determinism()


def test_host_call_and_postings_phrase_search():
    phrasesuite.check_host_call()


def test_index_batch_with_positions_and_tokenizer_phrase_search():
    phrasesuite.check_tokenizer()
