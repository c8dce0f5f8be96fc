"""Solver 5 (Trainer(l1r=True)) on the CPU emulator (tests/native/hipemu) against the restatement of tests/l1ref.py: the kernel of
vaporetto_amd/csrc/kernels_train_l1.hip on all three of its paths, the host driver's groups, order and stopping rule (the emulated
build also verifies that no row occurs twice in a group), the stats, the sparse model's bytes, determinism, and the errors."""
import pytest

from tests import emu, l1suite
from vaporetto_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    yield
    _lib._lib = saved


@pytest.mark.parametrize("case", l1suite.CASES)
def test_solver5_weights_stats_model_and_determinism(case):
    l1suite.check_solver5(case)   # 200 sentences, the GPU shape: a case takes seconds here


def test_errors():
    l1suite.check_errors()
