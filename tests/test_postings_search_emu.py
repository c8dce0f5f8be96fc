"""The BM25 top-k search on the CPU emulator (tests/native/hipemu): the launches of kernels_postings_search.hip with the trainer's sort and scan
between them, the host call, Postings.search and VaporettoTokenizer.search against the definition of tests/searchref.py -- the checks of
tests/searchsuite.py.  The hostile inputs run in a child process (hipemu checks the red zones around every allocation when the workspace goes,
and aborts when one is touched)."""
import gc
import os
import subprocess
import sys

import pytest

from tests import devmem, emu, searchsuite, vocabsuite
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


def test_random_queries_over_a_postings_pass_segment_and_the_addition_order():
    searchsuite.check_random()


def test_equal_documents_tie_by_ascending_document_and_k_cuts_a_tie_group():
    searchsuite.check_ties()


def test_slots_repeated_df0_out_of_range_empty_queries_and_the_slot_limit():
    searchsuite.check_slots()


@pytest.mark.parametrize("n", ["T-1", "T", "T+1", "3T+1"])
def test_candidates_and_matches_on_the_tile_edges(n):
    searchsuite.check_candidates(searchsuite.postingssuite.token_count(n))


def test_merged_segment_searched_equals_one_pass_segment_searched():
    searchsuite.check_merged_segment()


def test_zero_weights_k1_zero_b_zero_b_one_and_a_document_of_length_zero():
    searchsuite.check_weights_and_parameters()


def test_bm25_idf_is_the_definition():
    searchsuite.check_idf()


def test_capacity_too_small_is_an_error_at_sync_with_the_number_needed():
    searchsuite.check_capacity()


def test_errors_at_the_call():
    searchsuite.check_errors()


def hostile_child(flag, n_cases):
    r = subprocess.run([sys.executable, "-m", "tests.searchsuite", flag], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    print(out, r.stderr.decode()[-3000:])
    assert r.returncode == 0, (out[-500:], r.stderr.decode()[-2000:])
    assert out.strip().endswith("ran %d cases" % n_cases)


def test_hostile_input_is_an_error_at_sync_and_touches_nothing_outside():
    hostile_child("--emu-hostile", searchsuite.N_HOSTILE)


@pytest.mark.parametrize("base", searchsuite.postingssuite.HIGH_BASES)
def test_documents_on_both_sides_of_2_31_and_up_to_the_last_document_word(base):
    searchsuite.check_high_documents(base, hostile=False)


def test_hostile_postings_outside_a_range_that_ends_at_the_last_document_word():
    hostile_child("--emu-hostile-high", searchsuite.N_HOSTILE_HIGH)


@pytest.mark.parametrize("n", ["T", "T+1", "2T+1"])
def test_k_cuts_a_tie_group_on_the_tile_edges_and_a_query_ends_on_them(n):
    searchsuite.check_tile_edge_ties(searchsuite.postingssuite.token_count(n))


def test_two_runs_and_a_second_workspace_give_identical_bytes():
    searchsuite.check_determinism()


def test_host_call_and_postings_search():
    searchsuite.check_host_call()
