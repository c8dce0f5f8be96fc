"""TEST INFRASTRUCTURE: the restatement of solver 6 for tag problems: tests/l1lrref.py's loop (liblinear's newGLMNET by groups that share
no row, its seeded order carried across sweeps and Newton iterations, no shrinking) over a tag problem of tests/tagtrainref.py -- the
0/1 matrix of tagtrainref.design, the targets of tagtrainref.class_targets, the groups of tests/tagl1ref.py (the templates of the
problem's keys in sorted order, the bias last and alone).  Every class starts from w = 0 and the seed; two candidates are one solve,
mirrored."""
import numpy as np

from tests import l1lrref, tagl1ref, tagtrainref

groups = tagl1ref.groups


def solve(p, eps, cost):
    """(weights [classes][features + 1], [(Newton iterations, inner sweeps, halvings, first violation sum, last violation sum)] per class)."""
    X = tagtrainref.design(p)
    k = len(p["candidates"])
    W = np.zeros((k, X.shape[1]))
    stats = [None] * k
    for c, y in tagtrainref.class_targets(p):
        w, newton, sweeps, halvings, g0, gn = l1lrref.solve(X, y, p["keys"], cost, eps)
        W[c], stats[c] = w, (newton, sweeps, halvings, g0, gn)
    if k == 2:
        W[1], stats[1] = -W[0], stats[0]
    return W, stats
