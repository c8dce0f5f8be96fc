"""TEST INFRASTRUCTURE: the restatement of solver 5 for tag problems: tests/l1ref.py's loop (liblinear's solve_l1r_l2_svc by groups that
share no row, its seeded order, no shrinking) over a tag problem of tests/tagtrainref.py -- the 0/1 matrix of tagtrainref.design, the
targets of tagtrainref.class_targets, the groups the templates (kind, number of context symbols, rel_position) of the problem's keys
in sorted order with the bias last and alone.  A tag example has at most one feature per template (tag_trainer.rs:79-100), so a
template's columns share no row.  Every class starts from w = 0 and the seed."""
import numpy as np

from tests import l1ref, tagtrainref


def groups(p):
    return l1ref.groups(p["keys"])


def solve(p, eps, cost):
    """(weights [classes][features + 1], [(sweeps, halvings, first violation sum, last violation sum)] per class)."""
    X = tagtrainref.design(p)
    k = len(p["candidates"])
    W = np.zeros((k, X.shape[1]))
    stats = [None] * k
    for c, y in tagtrainref.class_targets(p):
        w, sweeps, halvings, v0, v = l1ref.solve(X, y, p["keys"], cost, eps)
        W[c], stats[c] = w, (sweeps, halvings, v0, v)
    if k == 2:
        W[1], stats[1] = -W[0], stats[0]
    return W, stats
