"""The postings pass on the CPU emulator (tests/native/hipemu): the four launches with the trainer's sort and scan between them, the host call and
the tokenizer's index_batch against the definition of tests/postingsref.py -- the checks of tests/postingssuite.py.  The hostile CSRs run in a
child process (hipemu checks the red zones around every allocation when the workspace goes, and aborts when one is touched).  The largest
cases here have 2 T + 1 tokens (T = vpt_postings_tile): the emulator runs a lane as a fiber, and 3 T + 1 adds time and no path."""
import gc
import os
import subprocess
import sys

import pytest

from tests import devmem, emu, postingssuite, vocabsuite
from vaporetto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    devmem.EMULATED = True
    vocabsuite._PRED.clear()
    yield
    vocabsuite._PRED.clear()
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


def test_random_csrs_match_the_definition_with_and_without_positions():
    postingssuite.check_random(47)


@pytest.mark.parametrize("n", ["1", "63", "64", "65", "255", "256", "257", "T-1", "T", "T+1", "2T+1"])
def test_token_counts_on_the_edges(n):
    postingssuite.check_token_counts(postingssuite.token_count(n))


@pytest.mark.parametrize("n_terms", postingssuite.N_TERMS_EDGES)
def test_n_terms_on_the_pass_edges(n_terms):
    postingssuite.check_n_terms(n_terms)


def test_runs_across_wave_round_and_tile_edges_of_the_sorted_order():
    postingssuite.check_runs()


def test_empty_documents_on_both_sides_of_every_key_tile_edge():
    postingssuite.check_empty_documents()


def test_dropped_tokens_are_counted_and_indexed_nowhere():
    postingssuite.check_dropped()


def test_stability_token_order_ascends_and_covers_the_indexed_tokens_once():
    postingssuite.check_stability()


def test_doc_base_shifts_the_documents_and_one_more_is_refused():
    postingssuite.check_doc_base()


def test_capacity_too_small_is_an_error_at_sync_with_the_number_needed():
    postingssuite.check_capacity()


def test_two_runs_and_a_second_workspace_give_identical_bytes():
    postingssuite.check_determinism()


def test_hostile_csr_is_an_error_at_sync_and_touches_nothing_outside():
    r = subprocess.run([sys.executable, "-m", "tests.postingssuite", "--emu-hostile"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    print(out, r.stderr.decode()[-3000:])
    assert r.returncode == 0, (out[-500:], r.stderr.decode()[-2000:])
    assert out.strip().endswith("ran %d cases" % postingssuite.N_HOSTILE)


def test_errors_at_the_call():
    postingssuite.check_errors()


def test_one_call_pipeline_equals_the_steps_and_does_not_depend_on_chunks():
    postingssuite.check_pipeline()


def test_one_call_pipeline_with_tag_models_and_a_stop_set():
    postingssuite.check_pipeline_stop_set()


def test_counter_vocabulary_and_postings_agree():
    postingssuite.check_three_features_agree()
