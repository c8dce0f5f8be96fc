"""TEST INFRASTRUCTURE: the checks of solver 5 (Trainer(l1r=True), SolverType.L1RegularizedL2LossSVC) shared by the emulator tests
(tests/test_train_l1_emu.py) and the GPU tests (tests/test_train_l1_gpu.py), against the restatement of tests/l1ref.py."""
import functools

import numpy as np
import pytest

from tests import l1ref, trainref, trainsuite
from tests.test_train_l1_ref import NESTED, sklearn_weights
from vaporetto_amd import api, modelfmt

EPS, COST = 0.01, 1.0
CASES = trainsuite.CASES + [NESTED]
# (seed, sentences) on which the library's sweep count was seen equal to the restatement's on both the emulator and the GPU; elsewhere
# sums in another order may move the stopping decision by a sweep
STABLE = {(1, 200), (2, 200), (3, 200), (5, 200)}
# the share of weights that must be exactly 0.0.  Measured with liblinear and with the restatement alike: 79 %, 48 % and 90 % on the
# suite's cases; the nested case (seed 5) was measured before the bar was put to it: 47 %
MIN_ZERO = 0.4


def trainer(case, n_sent, **kw):
    seed, charw, charn, typew, typen, dictn, with_dict = case
    sents = trainsuite.corpus(seed, n_sent)
    words = trainsuite.dictionary(sents, seed) if with_dict else []
    t = api.Trainer(charw, charn, typew, typen, words, dictn if words else 0, **kw)
    utf8, boff = api.pack_texts([s.encode("utf-8") for s, _ in sents])
    t.add_packed(utf8, boff, np.concatenate([lab for _, lab in sents]))
    return t, words


@functools.lru_cache(maxsize=None)
def reference(case, n_sent):
    """(keys, X, y, the restatement's solution): computed once, shared, read-only."""
    seed, charw, charn, typew, typen, dictn, with_dict = case
    sents = trainsuite.corpus(seed, n_sent)
    words = trainsuite.dictionary(sents, seed) if with_dict else []
    r = trainref.RefTrainer(charw, charn, typew, typen, words, dictn)
    for s, lab in sents:
        r.add_example(s, lab)
    keys, ptr, cols, cnt, y = r.matrix()
    X = trainref.design(ptr, cols, cnt, len(keys))
    sol = l1ref.solve(X, y, keys, COST, EPS)
    sol[0].flags.writeable = y.flags.writeable = False
    return keys, X, y, sol


def n_ngram_weights(model_bytes):
    m = modelfmt.decode_model(model_bytes)[0]
    return sum(int(np.count_nonzero(d.weights)) for part in (m.char_ngram_model, m.type_ngram_model) for d in part)


def check_solver5(case, n_sent=200):
    t, words = trainer(case, n_sent, l1r=True)
    keys, X, y, (wr, sweeps_r, halv_r, _, _) = reference(case, n_sent)
    col_len = np.diff(X.tocsc().indptr)
    assert col_len.min() == 1 and (col_len > 256).sum() > 1 and col_len[-1] > 1024   # every path of the kernel; the bias on the workgroup's
    model = t.train_bytes(EPS, COST, 5)
    w, b, gkeys = t.weights()
    stats = t.last_stats()
    assert gkeys == keys                                                            # 1
    wg = np.append(w, b)
    fg, fr = l1ref.objective_l1(X, y, wg, COST), l1ref.objective_l1(X, y, wr, COST)
    tol = l1ref.tolerance(y, EPS)
    vg, v_zero = l1ref.violation(X, y, wg, COST), l1ref.violation(X, y, 0 * wg, COST)
    zero = float((wg == 0.0).mean())
    print("seed %d, %d sentences: %d sweeps (restatement %d), %d halvings (%d), objective %.9g (%.9g), violation / violation(0) %.3g (tol %.3g), "
          "stats %.3g / %.3g, zero weights %.1f %%" % (case[0], n_sent, stats["iterations"], sweeps_r, stats["cg_steps"], halv_r, fg, fr,
                                                     vg / v_zero, tol, stats["gnorm"], stats["gnorm0"], 100 * zero))
    assert abs(fg - fr) <= 1e-3 * fr                                                # 2
    try:
        import sklearn  # noqa: F401
    except ImportError:
        pass
    else:
        if n_sent == 200:
            fs = l1ref.objective_l1(X, y, sklearn_weights(case), COST)
            assert abs(fg - fs) <= 1e-3 * fs                                        # 3
    assert vg <= tol * v_zero                                                       # 4
    assert stats["gnorm"] <= tol * stats["gnorm0"] and 1 <= stats["iterations"] < 1000   # 5
    assert abs(stats["objective"] - fg) <= 1e-9 * fg                                # 6
    assert zero >= MIN_ZERO                                                         # 7
    dense = t.train_bytes(EPS, COST, 2)
    assert n_ngram_weights(model) < n_ngram_weights(dense)                          # 8
    charw, typew, dictn = case[1], case[3], case[5]
    assert model == trainref.build_model(keys, w, b, charw, typew, words, dictn if words else 0)   # 9
    assert t.train_bytes(EPS, COST, 5) == model                                     # 10
    t2, _ = trainer(case, n_sent, l1r=True)
    assert t2.train_bytes(EPS, COST, 5) == model
    assert t2.last_stats() == stats
    if (case[0], n_sent) in STABLE:
        assert stats["iterations"] == sweeps_r                                      # 11
    return stats


def check_errors():
    case = trainsuite.CASES[1]
    plain, _ = trainer(case, 20)
    with pytest.raises(api.VaporettoError, match="solver: only 0 and 2 are implemented"):
        plain.train_bytes(EPS, COST, 5)
    both, _ = trainer(case, 20, l1r=True, train_tags=True)
    with pytest.raises(api.VaporettoError, match="solver 5: tag models are trained with solvers 0 and 2 only"):
        both.train_bytes(EPS, COST, 5)
    l1, _ = trainer(case, 20, l1r=True)
    for solver in (0, 2):
        assert l1.train_bytes(EPS, COST, solver) == plain.train_bytes(EPS, COST, solver)
    for solver in (1, 3, 4, 6, 7):
        with pytest.raises(api.VaporettoError, match="solver: only 0, 2 and 5 are implemented"):
            l1.train_bytes(EPS, COST, solver)
    assert l1.train_bytes(EPS, COST, 5)
