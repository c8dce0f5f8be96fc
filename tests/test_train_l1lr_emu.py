"""Solver 6 (Trainer(l1r_lr=True)) on the CPU emulator (tests/native/hipemu) against the restatement of tests/l1lrref.py: the kernels of
vaporetto_amd/csrc/kernels_train_l1lr.hip on all three of their column paths, the host driver's groups, order and stopping rules (the
emulated build also verifies that no row occurs twice in a group), the stats, the sparse model's bytes, determinism, and the errors."""
import pytest

from tests import emu, l1lrsuite
from vaporetto_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    yield
    _lib._lib = saved


@pytest.mark.parametrize("case", l1lrsuite.CASES)
def test_solver6_weights_stats_model_and_determinism(case):
    l1lrsuite.check_solver6(case)   # 200 sentences, the GPU shape: a case takes seconds here


def test_errors_and_non_interference():
    l1lrsuite.check_errors()
