"""TEST INFRASTRUCTURE: the checks of solver 6 (Trainer(l1r_lr=True), SolverType.L1RegularizedLogistic) shared by the emulator tests
(tests/test_train_l1lr_emu.py) and the GPU tests (tests/test_train_l1lr_gpu.py), against the restatement of tests/l1lrref.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import l1lrref, l1suite, trainref, trainsuite
from tests.test_train_l1_ref import NESTED
from vaporetto_amd import _lib, api

# EPS: the restatement and scikit-learn's liblinear agree within the bar of 1e-3 at l1suite's 0.01 (gaps seen: 7.2e-4, 4.5e-5, 1.7e-4,
# 1.8e-4 on seeds 1, 2, 3, 5), so it was not lowered
EPS, COST = 0.01, 1.0
CASES = trainsuite.CASES + [NESTED]
# (seed, sentences) on which the library's Newton-iteration and inner-sweep counts were seen equal to the restatement's on both the
# emulator and the MI355X; elsewhere exp, log and sums in another order may move a decision by an iteration
STABLE = {(1, 200), (2, 200), (3, 200), (5, 200)}
# the share of weights that must be exactly 0.0.  Measured at 200 sentences: the restatement 95.2 %, 82.6 %, 98.0 %, 84.7 % on seeds 1,
# 2, 3, 5, scikit-learn's liblinear 95.4 %, 82.8 %, 98.0 %, 85.1 %
MIN_ZERO = 0.8

trainer = l1suite.trainer
n_ngram_weights = l1suite.n_ngram_weights


@functools.lru_cache(maxsize=None)
def reference(case, n_sent):
    """(keys, (ptr, cols, cnt), X, y, the restatement's solution): computed once, shared, read-only."""
    seed, charw, charn, typew, typen, dictn, with_dict = case
    sents = trainsuite.corpus(seed, n_sent)
    words = trainsuite.dictionary(sents, seed) if with_dict else []
    r = trainref.RefTrainer(charw, charn, typew, typen, words, dictn)
    for s, lab in sents:
        r.add_example(s, lab)
    keys, ptr, cols, cnt, y = r.matrix()
    X = trainref.design(ptr, cols, cnt, len(keys))
    sol = l1lrref.solve(X, y, keys, COST, EPS)
    sol[0].flags.writeable = y.flags.writeable = False
    return keys, (ptr, cols, cnt), X, y, sol


def violation0_exact(X, y):
    """The violation sum at w = 0 with C = 1, in integers: 2 Grad_j = 2 sum_{y = -1} x - sum x."""
    Xi = X.astype(np.int64)
    G2 = np.asarray(2 * (Xi.T @ (y < 0).astype(np.int64)) - np.asarray(Xi.sum(axis=0)).ravel()).ravel()
    v2 = np.where(G2 + 2 < 0, -(G2 + 2), np.where(G2 - 2 > 0, G2 - 2, 0))
    return int(v2.sum()) / 2


def check_solver6(case, n_sent=200):
    t, words = trainer(case, n_sent, l1r_lr=True)
    keys, (ptr, cols, cnt), X, y, (wr, newton_r, sweeps_r, halv_r, _, _) = reference(case, n_sent)
    col_len = np.diff(X.tocsc().indptr)
    assert col_len.min() == 1 and (col_len > 256).sum() > 1 and col_len[-1] > 1024   # every path of the kernels; the bias on the workgroup's
    model = t.train_bytes(EPS, COST, 6)
    w, b, gkeys = t.weights()
    stats = t.last_stats()
    assert gkeys == keys                                                            # 1
    wg = np.append(w, b)
    fg, fr = l1lrref.objective(X, y, wg, COST), l1lrref.objective(X, y, wr, COST)
    tol = l1lrref.tolerance(y, EPS)
    vg, v_zero = l1lrref.violation(X, y, wg, COST), l1lrref.violation(X, y, 0 * wg, COST)
    zero = float((wg == 0.0).mean())
    print("seed %d, %d sentences: %d Newton iterations (restatement %d), %d sweeps (%d; the restatement halved %d times), objective %.9g (%.9g), "
          "violation / violation(0) %.3g (tol %.3g), stats %.17g / %.17g, zero weights %.1f %%"
          % (case[0], n_sent, stats["iterations"], newton_r, stats["cg_steps"], sweeps_r, halv_r, fg, fr, vg / v_zero, tol, stats["gnorm"],
             stats["gnorm0"], 100 * zero))
    assert stats["gnorm0"] == violation0_exact(X, y) == v_zero                      # 2
    assert abs(fg - fr) <= 1e-3 * fr                                                # 3
    try:
        import sklearn  # noqa: F401
    except ImportError:
        pass
    else:
        if n_sent == 200:
            from tests.test_train_l1lr_ref import sklearn_weights
            fs = l1lrref.objective(X, y, sklearn_weights(case), COST)
            assert abs(fg - fs) <= 1e-3 * fs
    # 4: the violations are |G_j +- 1| or a one-sided part of it, so their sum moves by at most sum_j |dG_j| <= sqrt(n) |dG|_2, and
    # stats_bounds bounds |dG|_2 for an fp64 gradient of the logistic loss summed in any order (G is its gradient without the w term)
    bound = np.sqrt(len(wg)) * trainref.stats_bounds(ptr, cols, cnt, y, w, b, COST, 0)[3]
    assert vg <= tol * v_zero + bound
    assert stats["gnorm"] <= tol * stats["gnorm0"] and 1 <= stats["iterations"] <= 100
    assert abs(stats["objective"] - fg) <= 1e-9 * fg                                # 5
    assert zero >= MIN_ZERO                                                         # 6
    dense = t.train_bytes(EPS, COST, 2)
    assert n_ngram_weights(model) < n_ngram_weights(dense)
    charw, typew, dictn = case[1], case[3], case[5]
    assert model == trainref.build_model(keys, w, b, charw, typew, words, dictn if words else 0)   # 7
    assert t.train_bytes(EPS, COST, 6) == model
    t2, _ = trainer(case, n_sent, l1r_lr=True)
    assert t2.train_bytes(EPS, COST, 6) == model
    assert t2.last_stats() == stats
    if (case[0], n_sent) in STABLE:
        assert (stats["iterations"], stats["cg_steps"]) == (newton_r, sweeps_r)     # 8
    return stats


def check_errors():                                                                 # 9
    case = trainsuite.CASES[1]
    plain, _ = trainer(case, 20)
    with pytest.raises(api.VaporettoError, match="solver: only 0 and 2 are implemented"):
        plain.train_bytes(EPS, COST, 6)
    l1, _ = trainer(case, 20, l1r=True)
    with pytest.raises(api.VaporettoError, match="solver: only 0, 2 and 5 are implemented"):
        l1.train_bytes(EPS, COST, 6)
    lr, _ = trainer(case, 20, l1r_lr=True)
    for solver in (0, 2):
        assert lr.train_bytes(EPS, COST, solver) == plain.train_bytes(EPS, COST, solver)
    for solver in (1, 3, 4, 5, 7):
        with pytest.raises(api.VaporettoError, match="solver: only 0, 2 and 6 are implemented"):
            lr.train_bytes(EPS, COST, solver)
    assert lr.train_bytes(EPS, COST, 6)
    both, _ = trainer(case, 20, l1r=True, l1r_lr=True)
    for solver in (0, 2):
        assert both.train_bytes(EPS, COST, solver) == plain.train_bytes(EPS, COST, solver)
    assert both.train_bytes(EPS, COST, 5) == l1.train_bytes(EPS, COST, 5)
    assert both.train_bytes(EPS, COST, 6) == lr.train_bytes(EPS, COST, 6)
    for solver in (1, 3, 4, 7):
        with pytest.raises(api.VaporettoError, match="solver: only 0, 2, 5 and 6 are implemented"):
            both.train_bytes(EPS, COST, solver)
    for kw in (dict(train_tags=True), dict(train_tags=True, l1r=True), dict(train_tags=True, l1r=True, l1r_tags=True)):
        tags, _ = trainer(case, 20, l1r_lr=True, **kw)
        with pytest.raises(api.VaporettoError, match="solver 6: tag models are trained with solvers 0, 2 and 5 only"):
            tags.train_bytes(EPS, COST, 6)
    for flags in (2, 3, 1 << 31, 16 | 2, 16 | 8, 16 | 32):
        prm = _lib.TrainParams(2, 2, 2, 1, 0, flags)
        h = C.c_void_p()
        assert _lib.load().vpt_trainer_create(C.addressof(prm), None, None, 0, 0, C.byref(h)) == _lib.VPT_INVALID_ARGUMENT
        assert "flags: " in _lib.last_error()
