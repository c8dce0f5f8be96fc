"""The vocabulary counter on the MI355X through the C ABI: the counter handle, the three count kernels, finish, the one host call and the
tokenizer's build_vocab against the restatement of tests/vocabcountref.py -- the checks of tests/vocabcountsuite.py.  (The full counter and the
hostile CSRs run here after they have run on the emulator, tests/test_vocab_count_emu.py: every kernel loop is bounded, nothing waits.)"""
import pytest

from tests import vocabcountsuite, vocabsuite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def fresh_predictor():
    vocabsuite._PRED.clear()
    yield
    vocabsuite._PRED.clear()


@pytest.mark.parametrize("fullwidth", [False, True])
def test_random_documents_match_restatement_and_a_second_counter(fullwidth):
    vocabcountsuite.check_random(43, fullwidth)


def test_accumulation_over_three_calls_equals_one_call():
    vocabcountsuite.check_accumulation()


def test_contention_every_lane_on_one_slot():
    vocabcountsuite.check_contention()


def test_probe_chains_shared_home_slot_and_wrap_around():
    vocabcountsuite.check_probing()


def test_fingerprint_twins_are_two_keys():
    vocabcountsuite.check_twins()


def test_skip_rules_and_length_bounds():
    vocabcountsuite.check_skip_rules()


def test_fullwidth_image_is_the_key():
    vocabcountsuite.check_fullwidth()


def test_tokens_and_empty_documents_on_both_sides_of_every_tile_edge():
    vocabcountsuite.check_edges()


def test_full_is_reported_sticky_and_cleared_by_reset():
    vocabcountsuite.check_full()


def test_finish_order_ties_and_cuts():
    vocabcountsuite.check_finish()


def test_build_vocab_round_trip_bincount_equals_counts():
    vocabcountsuite.check_round_trip()


def test_one_call_pipeline_equals_the_steps_and_does_not_depend_on_chunks():
    vocabcountsuite.check_pipeline()


def test_errors():
    vocabcountsuite.check_errors()


def test_hostile_csr_is_an_error_at_sync_and_touches_nothing_outside():
    assert vocabcountsuite.run_hostile() == vocabsuite.N_HOSTILE
