"""The merge of positional segments on the CPU emulator (tests/native/hipemu): the ordered route's tables, copy and pcopy, the general route's
ranks, scans, first and pcopy behind the merge's own launches, the host call, Postings.merge(positions=True) and the tokenizer's
index_batches(positions=True) against the definitions of tests/positionsmergeref.py and tests/phraseref.py -- the checks of
tests/positionsmergesuite.py.  The hostile segments run in a child process (hipemu checks the red zones around every allocation when the
workspace goes, and aborts when one is touched)."""
import gc
import os
import subprocess
import sys

import pytest

from tests import devmem, emu, positionsmergesuite, vocabsuite
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


def test_ordered_merge_of_device_made_ranges_equals_one_pass_on_both_routes():
    positionsmergesuite.check_ordered_equals_one_pass()


def test_general_merge_of_tokens_dealt_at_random_equals_one_pass():
    positionsmergesuite.check_general()


@pytest.mark.parametrize("base", positionsmergesuite.postingssuite.HIGH_BASES)
def test_segments_on_both_sides_of_2_31_and_up_to_the_last_document_word_merged_and_searched(base):
    positionsmergesuite.check_high_documents(base)


def test_position_places_on_the_workgroup_edges_and_a_segment_boundary_inside_a_wave():
    positionsmergesuite.check_position_places()


@pytest.mark.parametrize("n", ["T-1", "T", "T+1", "3T+1"])
def test_positions_on_the_scan_tile_edges(n):
    positionsmergesuite.check_positions_on_the_scan_tile(positionsmergesuite.postingssuite.token_count(n))


def test_edges_one_posting_last_segment_term_spare_capacity_and_one_segment():
    positionsmergesuite.check_edges()


def test_phrase_search_over_the_merged_segment_has_the_definitions_score_bits():
    positionsmergesuite.check_phrase_search_over_the_merge()


def test_capacities_too_small_are_errors_at_sync_with_the_numbers_needed():
    positionsmergesuite.check_capacity()


def test_errors_at_the_call():
    positionsmergesuite.check_errors()


def test_positions_that_do_not_ascend_or_repeat_across_segments():
    positionsmergesuite.check_bad_positions()


def test_hostile_segment_is_an_error_at_sync_and_touches_nothing_outside():
    r = subprocess.run([sys.executable, "-m", "tests.positionsmergesuite", "--emu-hostile"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    out = r.stdout.decode()
    print(out, r.stderr.decode()[-3000:])
    assert r.returncode == 0, (out[-500:], r.stderr.decode()[-2000:])
    assert out.strip().endswith("ran %d cases" % positionsmergesuite.N_HOSTILE)


def test_two_runs_and_a_second_workspace_give_identical_bytes():
    positionsmergesuite.check_determinism()


def test_host_call_and_postings_merge_with_positions():
    positionsmergesuite.check_host_call()


def test_index_batches_with_positions_equals_index_batch_of_the_concatenation():
    positionsmergesuite.check_index_batches()
