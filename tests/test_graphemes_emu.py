"""ConcatGraphemeClustersFilter on the device, on the CPU emulator (tests/native/hipemu): kernels_graphemes.hip, the flag through every
pipeline of the C ABI and the two caller-labels entry points against the host filter -- the checks of tests/graphemesuite.py, the random
counts cut and the long runs reduced to the cases around one and two tile edges."""
import gc

import pytest

from tests import devmem, emu, graphemesuite, tokensuite
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


def test_reference_known_answers():
    graphemesuite.check_reference_kat()


def test_random_strings_over_every_class():
    graphemesuite.check_random(n=200)


def test_state_across_wave_workgroup_and_tile_edges():
    graphemesuite.check_edges(full=False)


def test_classes_are_those_of_the_scored_text():
    graphemesuite.check_fullwidth()


@pytest.mark.parametrize("wc,wt", tokensuite.WINDOWS)
def test_one_call_equals_the_three_call_composition(wc, wt):
    graphemesuite.check_pipelines(21 + wc, wc, wt)


def test_evaluate_counters():
    graphemesuite.check_evaluate()


def test_fill_tags_sees_the_filtered_labels():
    graphemesuite.check_tagged()


@pytest.mark.parametrize("case", graphemesuite.G_KAT, ids=[c["name"] for c in graphemesuite.G_KAT])
def test_adapter_kats_with_g_through_the_c_abi(case):
    graphemesuite.check_kat_cabi(case)


def test_errors_and_the_flag_clear():
    graphemesuite.check_errors()
