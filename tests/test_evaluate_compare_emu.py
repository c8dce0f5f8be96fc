"""The evaluate compare kernel alone on the CPU emulator (tests/native/hipemu): vpt_evaluate_labels_batch_device on label vectors, texts and
gold lines of the tests' own against the restatement of tests/evalref.py -- the checks of tests/evalsuite.py."""
import gc

import pytest

from tests import devmem, emu, evalsuite
from vaporetto_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    devmem.EMULATED = True
    evalsuite.reset()
    yield
    evalsuite.reset()
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


def test_matched_carried_from_window_to_window_in_modes_gold_and_none():
    evalsuite.check_window_carries()


def test_counts_are_added_to_what_the_buffer_holds():
    evalsuite.check_counts_add_up()


def test_workgroups_with_idle_waves_and_the_grid_stride_loop():
    evalsuite.check_grid()


def test_predicted_tags_escaped_candidates_every_kind_of_difference_and_the_run_lookup():
    evalsuite.check_predicted_tags()
