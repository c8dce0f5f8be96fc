"""The restatement of solver 5 (tests/l1ref.py) on its own: the column groups share no row on the suite's corpora -- what lets the
library update a group in one launch -- and its solution against the liblinear that scikit-learn bundles."""
import functools

import numpy as np
import pytest

from tests import l1ref, trainref, trainsuite

NESTED = (5, 2, 2, 1, 1, 1, True)   # tests/test_train_ref.py: dictn = 1 over nested words, counts above 1
EPS, COST = 0.01, 1.0


@functools.lru_cache(maxsize=None)
def problem(case, n_sent=200):
    """(keys, X with the bias column, y) of the case's corpus by the restatement; shared, read-only."""
    seed, charw, charn, typew, typen, dictn, with_dict = case
    sents = trainsuite.corpus(seed, n_sent)
    words = trainsuite.dictionary(sents, seed) if with_dict else []
    r = trainref.RefTrainer(charw, charn, typew, typen, words, dictn)
    for s, lab in sents:
        r.add_example(s, lab)
    keys, ptr, cols, cnt, y = r.matrix()
    y.flags.writeable = False
    return keys, trainref.design(ptr, cols, cnt, len(keys)), y


@functools.lru_cache(maxsize=None)
def sklearn_weights(case, n_sent=200):
    """liblinear's solve_l1r_l2_svc through scikit-learn: bias 1.0 inside the L1 norm, the same C and tolerance."""
    import warnings

    from sklearn.svm import LinearSVC
    keys, X, y = problem(case, n_sent)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = LinearSVC(penalty="l1", loss="squared_hinge", dual=False, C=COST, tol=EPS, intercept_scaling=1, max_iter=1000).fit(X[:, :-1], y)
    return np.append(m.coef_.ravel(), m.intercept_)


@pytest.mark.parametrize("case", trainsuite.CASES + [NESTED])
def test_groups_share_no_row(case):
    keys, X, y = problem(case)
    gs = l1ref.groups(keys)
    assert sorted(j for g in gs for j in g) == list(range(len(keys) + 1))
    for g in gs:
        assert l1ref.rows_disjoint(X, g)
        kinds = {trainref.decode_key(keys[j])[0] if j < len(keys) else "bias" for j in g}
        assert len(kinds) == 1
        if kinds & {"dict", "bias"}:
            assert len(g) == 1
    assert gs[-1] == [len(keys)]
    assert len(gs) > 3 and max(len(g) for g in gs) > 1


def test_generator_is_splitmix64():
    rng = l1ref.SplitMix64(0)   # the published vector of splitmix64 from state 0
    assert [rng.next() for _ in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    order = list(range(10))
    l1ref.shuffle(order, l1ref.SplitMix64())
    assert sorted(order) == list(range(10)) and order != list(range(10))


@pytest.mark.parametrize("case", trainsuite.CASES)
def test_restatement_against_sklearn_liblinear(case):
    pytest.importorskip("sklearn")
    keys, X, y = problem(case)
    w, sweeps, halvings, v0, v = l1ref.solve(X, y, keys, COST, EPS)
    ws = sklearn_weights(case)
    fo, fs = l1ref.objective_l1(X, y, w, COST), l1ref.objective_l1(X, y, ws, COST)
    tol = l1ref.tolerance(y, EPS)
    print("seed %d: %d sweeps, %d halvings, objective %.6f against %.6f, violation / violation(0) %.2e (liblinear %.2e, tol %.2e), nonzero %d / %d"
          % (case[0], sweeps, halvings, fo, fs, l1ref.violation(X, y, w, COST) / l1ref.violation(X, y, 0 * w, COST),
             l1ref.violation(X, y, ws, COST) / l1ref.violation(X, y, 0 * w, COST), tol, np.count_nonzero(w), len(w)))
    assert abs(fo - fs) <= 1e-3 * fs
    assert v <= tol * v0 and sweeps < l1ref.MAX_SWEEPS
