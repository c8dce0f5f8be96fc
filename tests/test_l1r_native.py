"""vaporetto_amd/csrc/l1r.h -- the one transcript of liblinear's solve_l1r_l2_svc column step and of the sweep order that the device
kernel and the host driver share -- over a third backend: tests/native/l1r_test.cpp instantiates the step over a dense fp64 matrix with
sequential sums, is compiled by g++ from l1r.h alone with the address and undefined-behaviour sanitizers, runs as a child process on
small seeded problems, and its weights are held to the restatement (tests/l1ref.py).  CPU only.

The problems: features in templates that share no row (one feature of a template per row, as the trainer's n-grams), two count
columns that share rows (as dictionary columns do) and the bias; OVERSHOOT has a large C and few rows, so that the full Newton step of
some columns passes the kink and the line search halves."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import l1ref, trainref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "l1r_test.cpp")
PROBLEMS = [(1, 1.0), (2, 1.0), (3, 0.25), (4, 4.0), (5, 1.0)]
OVERSHOOT = (6, 1000.0)
EPS = 0.01


def problem(seed, few_rows=False):
    """(X without the bias, y, keys): 3 templates of 3 .. 5 features, one feature of each per row, then two columns of counts 0 .. 3."""
    rng = np.random.default_rng(seed)
    rows = int(rng.integers(6, 10)) if few_rows else int(rng.integers(30, 80))
    sizes = [int(rng.integers(3, 6)) for _ in range(3)]
    X = np.zeros((rows, sum(sizes) + 2))
    keys, at = [], 0
    for tpl, size in enumerate(sizes):
        X[np.arange(rows), at + rng.integers(0, size, rows)] = 1.0
        keys += [trainref.key_of(("char", chr(0x3042 + k), tpl - 1)) for k in range(size)]   # rel_position tells the templates apart
        at += size
    X[:, at:] = rng.integers(0, 4, (rows, 2)) * (rng.random((rows, 2)) < 0.5)
    keys += [trainref.key_of(("dict", 1, "L")), trainref.key_of(("dict", 1, "R"))]
    y = np.where((X @ rng.normal(size=X.shape[1]) + 0.5 * rng.normal(size=rows) > 0) ^ (rng.random(rows) < 1 / 7), 1.0, -1.0)
    y[0], y[1] = 1.0, -1.0
    assert X[:, at:].max() > 1
    return X, y, keys


ALL = PROBLEMS + [OVERSHOOT]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("l1r") / "l1r_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "vaporetto_amd", "csrc"), "-o", exe, SRC])
    lines = ["%d" % len(ALL)]
    for seed, cost in ALL:
        X, y, keys = problem(seed, (seed, cost) == OVERSHOOT)
        gs = l1ref.groups(keys)
        lines.append("%d %d %r %r %d" % (X.shape[0], X.shape[1], EPS, cost, len(gs)))
        lines += ["%d %s" % (len(g), " ".join("%d" % j for j in g)) for g in gs]
        lines += ["%d %s" % (t, " ".join("%d" % v for v in row)) for row, t in zip(X, y)]
    out = subprocess.run([exe], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True, timeout=120).stdout.decode().split("\n")
    res = {}
    for k, key in enumerate(ALL):
        st, w = out[2 * k].split(), out[2 * k + 1].split()
        assert st[0] == "stats" and w[0] == "w"
        res[key] = (dict(sweeps=int(st[1]), halvings=int(st[2]), v0=float(st[3]), v=float(st[4])), np.array([float(v) for v in w[1:]]))
    return res


@pytest.mark.parametrize("seed,cost", ALL)
def test_dense_backend_against_the_restatement(results, seed, cost):
    X, y, keys = problem(seed, (seed, cost) == OVERSHOOT)
    st, w = results[(seed, cost)]
    Xb = sp.csr_matrix(np.hstack([X, np.ones((len(y), 1))]))
    for g in l1ref.groups(keys):
        assert l1ref.rows_disjoint(Xb, g)
    wr, sweeps, halvings, v0, v = l1ref.solve(Xb, y, keys, cost, EPS)
    print("seed %d C %g: %s, restatement %d sweeps %d halvings" % (seed, cost, st, sweeps, halvings))
    # the same steps in the same order; only the order of the sums inside a column differs
    assert (st["sweeps"], st["halvings"]) == (sweeps, halvings)
    assert np.linalg.norm(w - wr) <= 1e-9 * np.linalg.norm(wr)
    assert np.array_equal(w == 0, wr == 0)
    assert abs(st["v0"] - v0) <= 1e-9 * v0 and st["v"] <= l1ref.tolerance(y, EPS) * st["v0"]
    if (seed, cost) == OVERSHOOT:
        assert st["halvings"] > 0
