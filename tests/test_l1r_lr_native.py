"""vaporetto_amd/csrc/l1r_lr.h -- the one transcript of liblinear's solve_l1r_lr (newGLMNET) that the device kernels and the host driver
share -- over a third backend: tests/native/l1r_lr_test.cpp instantiates the algorithm over a dense fp64 matrix with sequential sums,
is compiled by g++ from l1r_lr.h alone with the address and undefined-behaviour sanitizers, runs as a child process on small seeded
problems, and its weights and its three counts (Newton iterations, inner sweeps, line-search halvings) are held to the restatement
(tests/l1lrref.py).  CPU only.

The problems are those of tests/test_l1r_native.py (3-5 features per template, two count columns, the bias).  ONE_POSITIVE has a
single +1 row, so that min(pos, neg) = 1: the floor of the tolerance.  HALVING is built so that a line search must halve.  From w = 0
the quadratic model bounds the loss from above (every D_i is at its maximum C / 4), so a first step is always accepted, and a large C
alone never made the restatement halve on the seeded problems (searched: C up to 1e7, counts scaled up to 60).  What does: 100 rows
+1 with count 1 of one feature, 2 rows -1 with count 5 of it and count 1 of a second feature, C = 0.7.  After the first iterations
the two -1 rows sit far on the wrong side, where D is nearly 0; the model then underestimates the curvature along the way back,
the step overshoots, and the L1 term makes the objective rise.  The restatement is asserted to halve there, and the program to halve
as often."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import l1lrref, l1ref, trainref
from tests.test_l1r_native import problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "l1r_lr_test.cpp")
PROBLEMS = [(1, 1.0), (2, 1.0), (3, 0.25), (4, 4.0), (5, 1.0)]
ONE_POSITIVE = (7, 1.0)
HALVING = (0, 0.7)
ALL = PROBLEMS + [ONE_POSITIVE, HALVING]
EPS = 0.01


def make(key):
    if key == HALVING:
        X, y = np.zeros((102, 2)), np.ones(102)
        X[:100, 0], X[100:, 0], X[100:, 1], y[100:] = 1, 5, 1, -1
        return X, y, [trainref.key_of(("dict", 1, "L")), trainref.key_of(("dict", 1, "R"))]
    X, y, keys = problem(key[0])
    if key == ONE_POSITIVE:
        y = -np.ones(len(y))
        y[0] = 1.0
    return X, y, keys


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("l1r_lr") / "l1r_lr_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "vaporetto_amd", "csrc"), "-o", exe, SRC])
    lines = ["%d" % len(ALL)]
    for key in ALL:
        X, y, keys = make(key)
        gs = l1ref.groups(keys)
        lines.append("%d %d %r %r %d" % (X.shape[0], X.shape[1], EPS, key[1], len(gs)))
        lines += ["%d %s" % (len(g), " ".join("%d" % j for j in g)) for g in gs]
        lines += ["%d %s" % (t, " ".join("%d" % v for v in row)) for row, t in zip(X, y)]
    out = subprocess.run([exe], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True, timeout=120).stdout.decode().split("\n")
    res = {}
    for k, key in enumerate(ALL):
        st, w = out[2 * k].split(), out[2 * k + 1].split()
        assert st[0] == "stats" and w[0] == "w"
        res[key] = (dict(newton=int(st[1]), sweeps=int(st[2]), halvings=int(st[3]), v0=float(st[4]), v=float(st[5])), np.array([float(v) for v in w[1:]]))
    return res


@pytest.mark.parametrize("seed,cost", ALL)
def test_dense_backend_against_the_restatement(results, seed, cost):
    X, y, keys = make((seed, cost))
    st, w = results[(seed, cost)]
    Xb = sp.csr_matrix(np.hstack([X, np.ones((len(y), 1))]))
    for g in l1ref.groups(keys):
        assert l1ref.rows_disjoint(Xb, g)
    wr, newton, sweeps, halvings, v0, v = l1lrref.solve(Xb, y, keys, cost, EPS)
    print("seed %d C %g: %s, restatement %d Newton iterations %d sweeps %d halvings" % (seed, cost, st, newton, sweeps, halvings))
    # the same steps in the same order; only the order of the sums inside a column or over the rows differs
    assert (st["newton"], st["sweeps"], st["halvings"]) == (newton, sweeps, halvings)
    assert 1 <= newton < l1lrref.MAX_NEWTON
    assert np.linalg.norm(w - wr) <= 1e-9 * np.linalg.norm(wr)
    assert np.array_equal(w == 0, wr == 0)
    tol = l1lrref.tolerance(y, EPS)
    assert abs(st["v0"] - v0) <= 1e-9 * v0 and st["v"] <= tol * st["v0"]
    assert l1lrref.violation(Xb, y, w, cost) <= tol * l1lrref.violation(Xb, y, 0 * w, cost) * (1 + 1e-9)
    if (seed, cost) == ONE_POSITIVE:
        assert int((y > 0).sum()) == 1 and tol == EPS / len(y)
    if (seed, cost) == HALVING:
        assert halvings > 0
