"""TEST INFRASTRUCTURE: a restatement of the trainer's solver 5 (vaporetto_amd/csrc/l1r.h, capi_train.cpp solve_l1r) in numpy, fp64.

liblinear's solve_l1r_l2_svc -- coordinate descent for  |w|_1 + C sum max(0, b_i)^2,  b_i = 1 - y_i w.x_i, the bias a column of ones
inside the norm -- with the library's order: the columns in groups that share no row (a template (kind, n-gram length, rel_position)
of the char and type features; every dictionary column and the bias alone), the groups permuted anew per sweep by Fisher-Yates over
splitmix64 from a fixed seed, no shrinking, b written once per accepted step, a step dropped after 20 halvings.  A group is updated
over whole arrays: its columns share no row, so that is coordinate descent over them one by one.  Sums are numpy's, not the library's
tiles, so a stopping decision can fall a sweep apart.
"""
import numpy as np

from tests import trainref

SEED = 0x5EED5EED5EED5EED
_M64 = (1 << 64) - 1
SIGMA, MAX_LINESEARCH, MAX_SWEEPS = 0.01, 20, 1000


class SplitMix64:
    def __init__(self, seed=SEED):
        self.state = seed

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & _M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)


def shuffle(order, rng):
    for i in range(len(order) - 1, 0, -1):
        j = rng.next() % (i + 1)
        order[i], order[j] = order[j], order[i]


def groups(keys):
    """The column groups in the library's order; the bias is column len(keys), last and alone."""
    tpl, alone = {}, []
    for j, k in enumerate(keys):
        f = trainref.decode_key(k)
        if f[0] == "dict":
            alone.append(j)
        else:
            tpl.setdefault((0 if f[0] == "char" else 1, len(f[1]), f[2] + 16), []).append(j)
    return [tpl[k] for k in sorted(tpl)] + [[j] for j in alone] + [[len(keys)]]


def rows_disjoint(X, group):
    """No row has a nonzero in two columns of the group (X: trainref.design, CSR or CSC)."""
    sub = X.tocsc()[:, group]
    return int(np.diff(sub.tocsr().indptr).max(initial=0)) <= 1


def objective_l1(X, y, w, C):
    b = 1 - y * (X @ w)
    return np.abs(w).sum() + C * (b[b > 0] ** 2).sum()


def _violations(w, G):
    Gp, Gn = G + 1, G - 1
    return np.where(w == 0, np.where(Gp < 0, -Gp, np.where(Gn > 0, Gn, 0.0)), np.where(w > 0, np.abs(Gp), np.abs(Gn)))


def violation(X, y, w, C):
    """The sum of the columns' violations at w (what a sweep would sum if it moved nothing)."""
    b = 1 - y * (X @ w)
    G = -2 * C * (X.T @ (y * np.where(b > 0, b, 0.0)))
    return float(_violations(w, G).sum())


def tolerance(y, eps):
    pos = int((y > 0).sum())
    return eps * max(min(pos, len(y) - pos), 1) / len(y)


def solve(X, y, keys, C, eps):
    """(w, sweeps, halvings, first violation sum, last violation sum) from w = 0."""
    Xc = X.tocsc()
    Xc.sort_indices()
    indptr, rows, vals = Xc.indptr, Xc.indices, Xc.data * y[Xc.indices]   # v = x y
    n = X.shape[1]
    xj_sq = C * np.add.reduceat(np.append(vals * vals, 0.0), indptr[:-1])
    gs = []
    for g in groups(keys):
        g = np.asarray(g)
        nz = np.concatenate([np.arange(indptr[j], indptr[j + 1]) for j in g])
        gs.append((g, nz, np.repeat(np.arange(len(g)), np.diff(indptr)[g])))
    w, b = np.zeros(n), np.ones(len(y))
    tol = tolerance(y, eps)
    rng, order = SplitMix64(), list(range(len(gs)))
    sweeps = halvings = 0
    v0 = v = 0.0
    while sweeps < MAX_SWEEPS:
        shuffle(order, rng)
        viol = np.zeros(n)
        for gi in order:
            g, nz, col = gs[gi]
            r, val = rows[nz], vals[nz]
            bb = b[r]
            act = bb > 0
            G = -2 * np.bincount(col, np.where(act, C * val * bb, 0.0), len(g))
            H = np.maximum(2 * np.bincount(col, np.where(act, C * val * val, 0.0), len(g)), 1e-12)
            wj = w[g]
            viol[g] = _violations(wj, G)
            Gp, Gn = G + 1, G - 1
            d = np.where(Gp < H * wj, -Gp / H, np.where(Gn > H * wj, -Gn / H, -wj))
            d[np.abs(d) < 1e-12] = 0.0
            delta = np.abs(wj + d) - np.abs(wj) + G * d
            cond = np.abs(wj + d) - np.abs(wj) - SIGMA * delta
            for k in np.flatnonzero((d != 0) & (xj_sq[g] * d * d + G * d + cond > 0)):   # the few steps that need the data
                m = col == k
                bk, vk = bb[m], val[m]
                loss_old = C * (bk[bk > 0] ** 2).sum()
                dk, dl = d[k], delta[k]
                for it in range(MAX_LINESEARCH):
                    c = abs(wj[k] + dk) - abs(wj[k]) - SIGMA * dl
                    if xj_sq[g[k]] * dk * dk + G[k] * dk + c <= 0:
                        break
                    bn = bk - dk * vk
                    if c + C * (bn[bn > 0] ** 2).sum() - loss_old <= 0:
                        break
                    dk, dl = dk * 0.5, dl * 0.5
                    halvings += 1
                else:
                    dk = 0.0
                d[k] = dk
            w[g] = wj + d
            b[r] = bb - d[col] * val
        v = float(viol.sum())
        if sweeps == 0:
            v0 = v
        sweeps += 1
        if v <= tol * v0:
            break
    return w, sweeps, halvings, v0, v
