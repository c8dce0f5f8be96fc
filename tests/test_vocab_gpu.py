"""Vocabulary ids of the token stream on the MI355X through the C ABI: the vocabulary handle, token_ids_kernel, the one host call and the tokenizer
class against the restatement of tests/vocabref.py -- the checks of tests/vocabsuite.py.  (The hostile CSRs run here after they have run on the
emulator, tests/test_vocab_emu.py: an error at the sync, the guard words around every caller array intact.)"""
import pytest

from tests import vocabsuite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def fresh_predictor():
    vocabsuite._PRED.clear()
    yield
    vocabsuite._PRED.clear()


@pytest.mark.parametrize("fullwidth", [False, True])
def test_random_documents_match_restatement_unfiltered_and_filtered(fullwidth):
    vocabsuite.check_random(41, fullwidth)


def test_tokens_and_empty_documents_on_both_sides_of_every_tile_edge():
    vocabsuite.check_edges()


def test_length_bound():
    vocabsuite.check_length_bound()


def test_probe_chains_shared_home_slot_and_wrap_around():
    vocabsuite.check_probing()


def test_fingerprint_twin_that_is_no_key_is_unknown():
    vocabsuite.check_verification()


def test_handle_unk_ids_sizes_and_surfaces():
    vocabsuite.check_handle()


def test_errors():
    vocabsuite.check_errors()


def test_one_call_pipeline_equals_the_steps_and_does_not_depend_on_chunks():
    vocabsuite.check_pipeline()


def test_hostile_csr_is_an_error_at_sync_and_touches_nothing_outside():
    assert vocabsuite.run_hostile() == vocabsuite.N_HOSTILE
