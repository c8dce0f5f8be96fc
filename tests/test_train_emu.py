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
