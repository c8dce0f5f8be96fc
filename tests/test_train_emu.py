"""The trainer's kernels and host driver on the CPU emulator (tests/native/hipemu) against the restatement of tests/trainref.py:
the key table and the CSR, the TRON weights and iteration counts, the model bytes, determinism, and the errors."""
import pytest

from tests import emu, trainsuite
from vaporetto_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    yield
    _lib._lib = saved


@pytest.mark.parametrize("case", trainsuite.CASES)
def test_keys_and_csr_match_restatement(case):
    trainsuite.check_matrix(case)


@pytest.mark.parametrize("case,solver", [(trainsuite.CASES[0], 0), (trainsuite.CASES[0], 2), (trainsuite.CASES[1], 2),
                                         (trainsuite.CASES[2], 0), (trainsuite.CASES[2], 2)])
def test_tron_weights_model_and_determinism(case, solver):
    trainsuite.check_solver(case, solver)


def test_errors():
    trainsuite.check_errors()


def test_shaped_matrix_exact():
    """The "medium" shaped corpus (about 17 000 rows, 72 000 feature occurrences, three levels of X^T v, columns of 4 095 / 4 096 /
    4 097 nonzeros).  On the emulator this check takes 0.6 s, a label vector of the next test (both solvers) 0.8 s and the solve 10 s,
    against 25 s for the slowest test above, so the corpus is used at its full size."""
    trainsuite.check_shaped_matrix("medium")


@pytest.mark.parametrize("labels", ["random", "all_but_one", "alternating"])
def test_shaped_gnorm0_exact_and_stats_bounded(labels):
    trainsuite.check_shaped_stats("medium", labels)


def test_shaped_solve():
    trainsuite.check_shaped_solve("medium")
