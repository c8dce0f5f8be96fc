"""The postings merge on the CPU emulator (tests/native/hipemu): the ordered route's three launches, the general route's launches with the
trainer's sort and scan between them, the host call and the tokenizer's index_batches against the definitions of tests/postingsmergeref.py and
tests/postingsref.py -- the checks of tests/postingsmergesuite.py.  The hostile segments run in a child process (hipemu checks the red zones
around every allocation when the workspace goes, and aborts when one is touched)."""
import gc
import os
import subprocess
import sys

import pytest

from tests import devmem, emu, postingsmergesuite, vocabsuite
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


def test_ordered_merge_of_contiguous_groups_equals_one_pass_on_both_routes():
    postingsmergesuite.check_ordered_equals_one_pass(47)


def test_general_merge_of_documents_and_of_tokens_dealt_at_random():
    postingsmergesuite.check_general(21)


@pytest.mark.parametrize("base", postingsmergesuite.postingssuite.HIGH_BASES)
def test_segments_on_both_sides_of_2_31_and_up_to_the_last_document_word_on_both_routes(base):
    postingsmergesuite.check_high_documents(base)


def test_broken_promise_is_an_error_at_sync_and_touching_ranges_are_not():
    postingsmergesuite.check_broken_promise()


def test_vocabulary_growth_segments_with_fewer_terms():
    postingsmergesuite.check_vocabulary_growth()


@pytest.mark.parametrize("n", ["T-1", "T", "T+1", "3T+1"])
def test_input_postings_on_the_tile_edges(n):
    postingsmergesuite.check_input_postings(postingsmergesuite.postingssuite.token_count(n))


def test_edges_one_term_many_terms_spare_capacity_empty_segment_and_one_segment():
    postingsmergesuite.check_edges()


def test_the_most_segments_with_one_posting_each():
    postingsmergesuite.check_segment_limit()


def test_capacity_too_small_is_an_error_at_sync_with_the_number_needed():
    postingsmergesuite.check_capacity()


def test_hostile_segment_is_an_error_at_sync_and_touches_nothing_outside():
    r = subprocess.run([sys.executable, "-m", "tests.postingsmergesuite", "--emu-hostile"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    out = r.stdout.decode()
    print(out, r.stderr.decode()[-3000:])
    assert r.returncode == 0, (out[-500:], r.stderr.decode()[-2000:])
    assert out.strip().endswith("ran %d cases" % postingsmergesuite.N_HOSTILE)


def test_tf_sum_above_32_bits_is_an_error_and_the_largest_sum_is_not():
    postingsmergesuite.check_tf_overflow()


def test_errors_at_the_call():
    postingsmergesuite.check_errors()


def test_two_runs_and_a_second_workspace_give_identical_bytes():
    postingsmergesuite.check_determinism()


def test_host_call_and_postings_merge():
    postingsmergesuite.check_host_call()


def test_index_batches_equals_index_batch_of_the_concatenation():
    postingsmergesuite.check_index_batches()
