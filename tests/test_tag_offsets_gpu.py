"""Hostile out_offsets over several front-end runs (tests/tagoffsetsuite.py) on the device: error-path contract tests -- the expected outcome of
every case is a status word at sync, guard words that nobody touched, and a workspace that gives the oracle's tags right afterwards."""
import pytest

from tests import tagoffsetsuite

pytestmark = pytest.mark.gpu
_ran = {}


@pytest.mark.parametrize("variant", tagoffsetsuite.VARIANTS)
@pytest.mark.parametrize("batch", tagoffsetsuite.BATCHES)
def test_hostile_offsets_stay_inside_the_batch(batch, variant):
    _ran[(batch, variant)] = tagoffsetsuite.run_group(batch, variant)
    assert _ran[(batch, variant)] == tagoffsetsuite.CASES_PER_BATCH[batch]


def test_every_case_ran():
    if len(_ran) != len(tagoffsetsuite.BATCHES) * len(tagoffsetsuite.VARIANTS):
        pytest.skip("a selection of the cases was run")
    assert sum(_ran.values()) == tagoffsetsuite.N_CASES == 123
