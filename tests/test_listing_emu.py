"""The predict CLI's listings on the CPU emulator (tests/native/hipemu): kernels_listing.hip and its host pipeline against the restatement of
tests/listingref.py -- the checks of tests/listingsuite.py."""
import gc

import pytest

from tests import devmem, emu, listingsuite
from vaporetto_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    devmem.EMULATED = True
    yield
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


def test_known_answers():
    listingsuite.check_kat()


def test_formatting_edges():
    listingsuite.check_edges()


def test_tag_block_edges_with_forced_tokens():
    listingsuite.check_forced_tokens()


def test_extreme_scores():
    listingsuite.check_extreme_scores()


def test_batches_every_combination_host_and_device():
    listingsuite.check_batches(120)


def test_errors():
    listingsuite.check_errors()


def test_bad_offsets_across_front_end_runs():
    listingsuite.check_bad_offsets_across_runs()
