"""The evaluate compare kernel alone on the MI355X: vpt_evaluate_labels_batch_device on label vectors, texts and gold lines of the tests' own
against the restatement of tests/evalref.py -- the checks of tests/evalsuite.py, the system side of mode PREDICTED from the CPU oracle."""
import pytest

from tests import evalsuite
from vaporetto_amd import build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_hip()
    evalsuite.reset()
    yield
    evalsuite.reset()


def test_matched_carried_from_window_to_window_in_modes_gold_and_none():
    evalsuite.check_window_carries()


def test_counts_are_added_to_what_the_buffer_holds():
    evalsuite.check_counts_add_up()


def test_workgroups_with_idle_waves_and_the_grid_stride_loop():
    evalsuite.check_grid()


def test_predicted_tags_escaped_candidates_every_kind_of_difference_and_the_run_lookup():
    evalsuite.check_predicted_tags()
