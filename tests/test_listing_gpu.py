"""The predict CLI's listings on the MI355X: the checks of tests/listingsuite.py against the restatement of tests/listingref.py."""
import pytest

from tests import listingsuite

pytestmark = pytest.mark.gpu


def test_known_answers():
    listingsuite.check_kat()


def test_formatting_edges():
    listingsuite.check_edges()


def test_tag_block_edges_with_forced_tokens():
    listingsuite.check_forced_tokens()


def test_extreme_scores():
    listingsuite.check_extreme_scores()


def test_batches_every_combination_host_and_device():
    listingsuite.check_batches(400)


def test_errors():
    listingsuite.check_errors()


def test_bad_offsets_across_front_end_runs():
    listingsuite.check_bad_offsets_across_runs()
