"""TEST INFRASTRUCTURE: a restatement of the trainer's solver 6 (vaporetto_amd/csrc/l1r_lr.h, capi_train.cpp solve_l1r_lr) in numpy, fp64.

liblinear's solve_l1r_lr (newGLMNET) for  |w|_1 + C sum log(1 + exp(-y_i w.x_i)),  the bias a column of ones inside the norm, with the
library's order and divergences: the columns in the groups of tests/l1ref.py, permuted anew per inner sweep by Fisher-Yates over
splitmix64 from a fixed seed carried across sweeps and Newton iterations; no shrinking at either level; a column's sum x D xTd taken on
its own and added to Grad_j + (wpd_j - w_j) nu; the trial weights put back to w after 20 refused line-search trials.  A group is updated
over whole arrays: its columns share no row, so that is coordinate descent over them one by one.  Sums are numpy's, not the library's
tiles, and exp and log are numpy's, so a stopping decision can fall an iteration apart.

`violation` and `objective` are evaluated from w alone, sharing nothing with `solve`; `violation` in np.longdouble.
"""
import numpy as np

from tests import l1ref

NU, SIGMA = 1e-12, 0.01
MAX_NEWTON, MAX_SWEEPS, MAX_LINESEARCH = 100, 1000, 20


def objective(X, y, w, C):
    """|w|_1 + C sum log(1 + exp(-y w.x)), the bias (X's last column of ones) inside the norm."""
    return float(np.abs(w).sum() + C * np.logaddexp(0.0, -y * (X @ w)).sum())


def _violations(w, G):
    Gp, Gn = G + 1, G - 1
    return np.where(w == 0, np.where(Gp < 0, -Gp, np.where(Gn > 0, Gn, 0.0)), np.where(w > 0, np.abs(Gp), np.abs(Gn)))


def violation(X, y, w, C):
    """The sum of the columns' violations at w, from w alone in np.longdouble: G_j = C sum_i x_ij (sigma(w.x_i) - [y_i = +1])."""
    ext = np.longdouble
    M = X.tocoo()
    z = np.zeros(X.shape[0], ext)
    np.add.at(z, M.row, M.data.astype(ext) * np.asarray(w, ext)[M.col])
    gz = ext(C) * (1 / (1 + np.exp(-z)) - (np.asarray(y) > 0))
    G = np.zeros(X.shape[1], ext)
    np.add.at(G, M.col, M.data.astype(ext) * gz[M.row])
    return float(_violations(np.asarray(w, ext), G).sum())


tolerance = l1ref.tolerance


def solve(X, y, keys, C, eps):
    """(w, Newton iterations, inner sweeps, line-search halvings, first violation sum, last violation sum) from w = 0."""
    Xc = X.tocsc()
    Xc.sort_indices()
    indptr, rows, vals = Xc.indptr, Xc.indices, Xc.data.astype(np.float64)
    n, l = X.shape[1], X.shape[0]
    col_of = np.repeat(np.arange(n), np.diff(indptr))
    gs = []
    for g in l1ref.groups(keys):
        g = np.asarray(g)
        nz = np.concatenate([np.arange(indptr[j], indptr[j + 1]) for j in g])
        gs.append((g, rows[nz], vals[nz], np.repeat(np.arange(len(g)), np.diff(indptr)[g])))
    neg = y < 0
    w, wpd = np.zeros(n), np.zeros(n)
    e = np.ones(l)
    xjneg = np.bincount(col_of, np.where(neg[rows], C * vals, 0.0), n)

    def refresh(e):
        t = 1 / (1 + e)
        return C * t, C * e * t * t

    tau, D = refresh(e)
    tol = tolerance(y, eps)
    rng, order = l1ref.SplitMix64(), list(range(len(gs)))
    inner_eps, w_norm = 1.0, 0.0
    newton = sweeps = halvings = 0
    g0 = gn = 0.0
    while newton < MAX_NEWTON:
        hdiag = NU + np.bincount(col_of, vals * vals * D[rows], n)
        grad = -np.bincount(col_of, vals * tau[rows], n) + xjneg
        gn = float(_violations(w, grad).sum())
        if newton == 0:
            g0 = gn
        if gn <= tol * g0:
            break
        xTd = np.zeros(l)
        it = 0
        while it < MAX_SWEEPS:
            l1ref.shuffle(order, rng)
            viol = np.zeros(n)
            for gi in order:
                g, r, val, col = gs[gi]
                wp = wpd[g]
                G = grad[g] + (wp - w[g]) * NU + np.bincount(col, val * D[r] * xTd[r], len(g))
                H = hdiag[g]
                viol[g] = _violations(wp, G)
                Gp, Gn = G + 1, G - 1
                z = np.where(Gp < H * wp, -Gp / H, np.where(Gn > H * wp, -Gn / H, -wp))
                z[np.abs(z) < 1e-12] = 0.0
                z = np.minimum(np.maximum(z, -10.0), 10.0)
                wpd[g] = np.where(z != 0, wp + z, wp)
                move = z[col] != 0
                xTd[r[move]] += z[col][move] * val[move]
            it += 1
            if float(viol.sum()) <= inner_eps * g0:
                break
        sweeps += it
        w_norm_new = float(np.abs(wpd).sum())
        delta = float((grad * (wpd - w)).sum()) + (w_norm_new - w_norm)
        negsum = float(np.where(neg, C * xTd, 0.0).sum())
        for k in range(MAX_LINESEARCH):
            ex = np.exp(xTd)
            en = e * ex
            cond = w_norm_new - w_norm + negsum - SIGMA * delta + float((C * np.log((1 + en) / (ex + en))).sum())
            if cond <= 0:
                w_norm = w_norm_new
                w = wpd.copy()
                e = en
                tau, D = refresh(e)
                break
            wpd = (w + wpd) * 0.5
            xTd = xTd * 0.5
            w_norm_new = float(np.abs(wpd).sum())
            delta *= 0.5
            negsum *= 0.5
            halvings += 1
        else:
            e = np.exp(X @ w)
            wpd = w.copy()
        if it == 1:
            inner_eps *= 0.25
        newton += 1
    return w, newton, sweeps, halvings, g0, gn
