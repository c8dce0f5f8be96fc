"""The restatement of solver 5 for tag problems (tests/tagl1ref.py) on its own, without the library: the groups of every problem of the
suite's corpora and shapes share no row -- what lets the kernel update a group between two barriers --, its solutions meet liblinear's
stopping rule at their own weights but on a recorded few, and its objective is that of the liblinear scikit-learn bundles."""
import numpy as np
import pytest

from tests import l1ref, tagl1suite, tagtrainref

CORPORA = sorted(tagl1suite.CASES)


@pytest.mark.parametrize("name", CORPORA + sorted(tagl1suite.SHAPES))
def test_groups_share_no_row(name):
    _, ref = tagl1suite.reference(name)
    assert ref
    for tok, p, X, _, _ in ref:
        gs = l1ref.groups(p["keys"])
        assert sorted(j for g in gs for j in g) == list(range(len(p["keys"]) + 1)) and gs[-1] == [len(p["keys"])]
        assert all(l1ref.rows_disjoint(X, g) for g in gs), tok


def test_restatement_meets_the_stopping_rule_but_on_the_recorded_pairs():
    misses, pairs = set(), 0
    for name in CORPORA:
        for tok, p, X, W, st in tagl1suite.reference(name)[1]:
            for c, y in tagtrainref.class_targets(p):
                pairs += 1
                if not l1ref.violation(X, y, W[c], tagl1suite.COST) <= l1ref.tolerance(y, tagl1suite.EPS) * l1ref.violation(X, y, 0 * W[c], tagl1suite.COST):
                    misses.add((name, tok, p["slot"], c))
                    print(name, tok, p["slot"], c, st[c])
                assert st[c][0] < l1ref.MAX_SWEEPS, (name, tok, p["slot"], c)   # what the seeds are chosen for
    assert misses == tagl1suite.REF_MISSES
    assert len(misses) <= 0.05 * pairs, (len(misses), pairs)


@pytest.mark.parametrize("name", sorted(tagl1suite.SHAPES))
def test_shapes_hold_what_they_promise(name):
    counts, n_class, path, _ = tagl1suite.SHAPES[name]
    ((tok, p, X, W, st),) = tagl1suite.reference(name)[1]
    assert tok == "X" and len(p["candidates"]) == n_class and tagl1suite.fits(p) == (path == 1)
    col_len = np.diff(X.tocsc().indptr)
    gs = l1ref.groups(p["keys"])
    if name == "lane_wave":
        assert {63, 64, 65} <= set(col_len.tolist())
    if name == "wave_block":
        assert {1023, 1024, 1025} <= set(col_len.tolist())
    if name == "wide":
        assert max(len(g) for g in gs) > 256 and n_class >= 4
    if name == "limit":
        assert len(p["keys"]) + 1 + len(p["y"]) == tagl1suite.LDS_DOUBLES
    if name == "past_limit":
        assert len(p["keys"]) + 1 + len(p["y"]) == tagl1suite.LDS_DOUBLES + 1
    for c, y in tagtrainref.class_targets(p):
        assert l1ref.violation(X, y, W[c], tagl1suite.COST) <= l1ref.tolerance(y, tagl1suite.EPS) * l1ref.violation(X, y, 0 * W[c], tagl1suite.COST)
        assert st[c][0] < l1ref.MAX_SWEEPS


def test_a_shape_and_a_corpus_have_halvings():
    assert all(st[c][1] > 0 for _, p, _, _, st in tagl1suite.reference("halvings")[1] for c, _ in tagtrainref.class_targets(p))
    assert any(st[c][1] > 0 for _, p, _, _, st in tagl1suite.reference("small")[1] for c, _ in tagtrainref.class_targets(p))


@pytest.mark.parametrize("name", CORPORA + ["lane_wave", "wide", "halvings"])
def test_restatement_against_sklearn_liblinear(name):
    """Every (problem, class) of the case within 1e-3 relative of liblinear's objective, as tests/l1suite.py compares the boundary model.

    Both are solved with the suite's eps, chosen for this bound (tests/tagl1suite.py)."""
    pytest.importorskip("sklearn")
    import warnings

    from sklearn.svm import LinearSVC
    for tok, p, X, W, _ in tagl1suite.reference(name)[1]:
        for c, y in tagtrainref.class_targets(p):
            w = W[c]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m = LinearSVC(penalty="l1", loss="squared_hinge", dual=False, C=tagl1suite.COST, tol=tagl1suite.EPS, intercept_scaling=1,
                              max_iter=1000, random_state=0).fit(X[:, :-1], y)
            ws = np.append(m.coef_.ravel(), m.intercept_)
            fo, fs = l1ref.objective_l1(X, y, w, tagl1suite.COST), l1ref.objective_l1(X, y, ws, tagl1suite.COST)
            assert abs(fo - fs) <= 1e-3 * fs, (tok, p["slot"], c, fo, fs)
