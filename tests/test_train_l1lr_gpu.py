"""Solver 6 (Trainer(l1r_lr=True), L1-regularised logistic regression) on the MI355X against the restatement of tests/l1lrref.py: the
checks of tests/l1lrsuite.py."""
import pytest

from tests import l1lrsuite

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", l1lrsuite.CASES)
def test_solver6_weights_stats_model_and_determinism(case):
    l1lrsuite.check_solver6(case)


def test_errors_and_non_interference():
    l1lrsuite.check_errors()
