"""vaporetto_amd/csrc/tron.h -- the one transcript of liblinear's TRON that the host driver and the in-kernel solver share -- over a
third backend: tests/native/tron_test.cpp instantiates the template over a dense fp64 matrix with sequential sums, is compiled with g++
and run on small seeded 0/1 problems, and its weights and stats are held to the restatement (tests/trainref.py's tron).  CPU only.

The seeds: the restatement was run on seeds 1 .. 40 of `problem`, as generated and with a single positive row, with its dot products,
norms and matrix products taken by numpy and again summed in index order; on every one the iteration and CG counts of solver 0 were
the same both ways (problems this small are that well conditioned), so the counts of the seeds below do not hang on the order of
the sums.  For solver 2 the counts are not asserted: the generalised Hessian jumps where a margin crosses 1, and the order of the
sums alone can change the path (the note in tests/trainsuite.py, check_solver)."""
import os
import subprocess

import numpy as np
import pytest

from tests import trainref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tron_test.cpp")
EPS, COST = 0.01, 1.0
SEEDS = (1, 2, 3, 4, 5, 6)
ONE_POSITIVE = 7   # a problem with a single positive row: min(pos, neg) = 1, the floor of liblinear's tolerance


def problem(seed, one_positive=False):
    """(X, y): 12 .. 40 rows of 4 .. 10 0/1 features; the target follows a random linear rule, one in seven flipped."""
    rng = np.random.default_rng(seed)
    rows, features = int(rng.integers(12, 41)), int(rng.integers(4, 11))
    X = (rng.random((rows, features)) < 0.4).astype(np.float64)
    y = np.where((X @ rng.normal(size=features) + 0.3 * rng.normal(size=rows) > 0) ^ (rng.random(rows) < 1 / 7), 1.0, -1.0)
    if one_positive:
        y[:] = -1.0
        y[int(rng.integers(0, rows))] = 1.0
    return X, y


PROBLEMS = [(seed, solver, False) for solver in (0, 2) for seed in SEEDS] + [(ONE_POSITIVE, solver, True) for solver in (0, 2)]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tron") / "tron_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "vaporetto_amd", "csrc"), "-o", exe, SRC])
    lines = ["%d" % len(PROBLEMS)]
    for seed, solver, one in PROBLEMS:
        X, y = problem(seed, one)
        lines.append("%d %d %d %r %r" % (X.shape[0], X.shape[1], solver, EPS, COST))
        lines += ["%d %s" % (t, " ".join("%d" % v for v in row)) for row, t in zip(X, y)]
    out = subprocess.run([exe], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True, timeout=120).stdout.decode().split("\n")
    res = {}
    for k, key in enumerate(PROBLEMS):
        st, w = out[2 * k].split(), out[2 * k + 1].split()
        assert st[0] == "stats" and w[0] == "w"
        res[key] = (dict(iterations=int(st[1]), cg_steps=int(st[2]), gnorm0=float(st[3]), gnorm=float(st[4]), objective=float(st[5])),
                    np.array([float(v) for v in w[1:]]))
    return res


@pytest.mark.parametrize("seed,solver,one", PROBLEMS)
def test_dense_backend_against_the_restatement(results, seed, solver, one):
    X, y = problem(seed, one)
    assert (int((y > 0).sum()) == 1) == one
    st, w = results[(seed, solver, one)]
    rows, features = X.shape
    Xb = np.hstack([X, np.ones((rows, 1))])
    wr, it, cg, g0, _ = trainref.tron(Xb, y, COST, EPS, solver)
    print("seed %d solver %d: %s, restatement %d iterations %d CG steps" % (seed, solver, st, it, cg))
    assert st["iterations"] >= 1
    assert np.linalg.norm(w - wr) <= 1e-7 * np.linalg.norm(wr)
    pos = int((y > 0).sum())
    assert st["gnorm"] <= EPS * max(min(pos, rows - pos), 1) / rows * st["gnorm0"]
    # the norm of the first gradient within the bound of fp64 summation in any order, from the matrix alone
    ptr, cols = np.arange(rows + 1) * features, np.tile(np.arange(features), rows)
    _, gnorm0, _, bound = trainref.stats_bounds(ptr, cols, X.ravel(), y, np.zeros(features), 0.0, COST, solver)
    assert abs(st["gnorm0"] - float(gnorm0)) <= bound
    if solver == 0:
        assert (st["iterations"], st["cg_steps"]) == (it, cg)
