"""The restatement of solver 6 (tests/l1lrref.py) on its own: the column groups share no row on the suite's corpora -- what lets the
library update a group in one launch --, and its solution against the liblinear that scikit-learn bundles.  sklearn's liblinear shrinks
and draws its order from its own generator, so only objectives are compared; the zero shares of both are printed (l1lrsuite.MIN_ZERO
was set below them)."""
import functools

import numpy as np
import pytest

from tests import l1lrref, l1ref, trainsuite
from tests.test_train_l1_ref import NESTED, problem

EPS, COST = 0.01, 1.0
CASES = trainsuite.CASES + [NESTED]


@functools.lru_cache(maxsize=None)
def sklearn_weights(case, n_sent=200):
    """liblinear's solve_l1r_lr through scikit-learn: bias 1.0 inside the L1 norm, the same C and tolerance."""
    import warnings

    from sklearn.linear_model import LogisticRegression
    keys, X, y = problem(case, n_sent)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = LogisticRegression(penalty="l1", solver="liblinear", C=COST, tol=EPS, intercept_scaling=1, max_iter=1000).fit(X[:, :-1], y)
    return np.append(m.coef_.ravel(), m.intercept_)


@functools.lru_cache(maxsize=None)
def restatement(case, n_sent=200):
    keys, X, y = problem(case, n_sent)
    sol = l1lrref.solve(X, y, keys, COST, EPS)
    sol[0].flags.writeable = False
    return sol


@pytest.mark.parametrize("case", CASES)
def test_groups_share_no_row(case):
    keys, X, y = problem(case)
    gs = l1ref.groups(keys)
    assert sorted(j for g in gs for j in g) == list(range(len(keys) + 1))
    for g in gs:
        assert l1ref.rows_disjoint(X, g)


def test_violation_is_zero_only_at_an_optimum():
    """The independent check itself: at w = 0 it is the integer formula of the suite's gnorm0 check, and it falls along the solve."""
    case = CASES[0]
    keys, X, y = problem(case)
    w, newton, sweeps, halvings, g0, gn = restatement(case)
    G2 = np.asarray(2 * (X.T @ (y < 0)) - X.sum(axis=0)).ravel()   # 2 Grad at w = 0, C = 1: integers
    v0 = float(np.where(G2 + 2 < 0, -(G2 + 2), np.where(G2 - 2 > 0, G2 - 2, 0)).sum()) / 2
    assert l1lrref.violation(X, y, 0 * w, COST) == v0 == g0
    assert l1lrref.violation(X, y, w, COST) <= l1lrref.tolerance(y, EPS) * v0 * (1 + 1e-9)
    assert l1lrref.objective(X, y, w, COST) < l1lrref.objective(X, y, 0 * w, COST)


@pytest.mark.parametrize("case", CASES)
def test_restatement_against_sklearn_liblinear(case):
    pytest.importorskip("sklearn")
    keys, X, y = problem(case)
    w, newton, sweeps, halvings, g0, gn = restatement(case)
    ws = sklearn_weights(case)
    fo, fs = l1lrref.objective(X, y, w, COST), l1lrref.objective(X, y, ws, COST)
    tol = l1lrref.tolerance(y, EPS)
    v_zero = l1lrref.violation(X, y, 0 * w, COST)
    print("seed %d: %d Newton iterations, %d sweeps, %d halvings, objective %.6f against %.6f (gap %.2e), violation / violation(0) %.2e "
          "(liblinear %.2e, tol %.2e), zero weights %.1f %% (liblinear %.1f %%)"
          % (case[0], newton, sweeps, halvings, fo, fs, abs(fo - fs) / fs, l1lrref.violation(X, y, w, COST) / v_zero,
             l1lrref.violation(X, y, ws, COST) / v_zero, tol, 100 * float((w == 0).mean()), 100 * float((ws == 0).mean())))
    assert abs(fo - fs) <= 1e-3 * fs
    assert gn <= tol * g0 and 1 <= newton < l1lrref.MAX_NEWTON
