"""TEST INFRASTRUCTURE: a restatement of the reference's boundary trainer (vaporetto/src/trainer.rs) in plain Python / numpy.

- gen_features / RefTrainer.add_example: Trainer::gen_features and add_example (trainer.rs:260-350), features in the reference's order;
- keys: the library's 128-bit feature keys (include/vaporetto_hip.h, Trainer section), so that the sorted key table and the CSR compare;
- tron: liblinear's TRON for solvers 0 (l2r_lr_fun) and 2 (l2r_l2_svc_fun) as scikit-learn bundles it (tron.cpp, linear.cpp), in fp64;
- build_model: quantisation and the model layout (trainer.rs:352-487), encoded by modelfmt.encode_model.
"""
import math

import numpy as np

from vaporetto_amd import modelfmt
from vaporetto_amd.api import CharacterType

_SH = (99, 78, 57, 36, 15)
_WHERE = {"L": 0, "I": 1, "R": 2}


def char_type(c):
    return int(CharacterType.get_type(c))


def gen_features(text, charw, charn, typew, typen, dict_words=(), dictn=0):
    """Per boundary its features as ("char", str, rel) / ("type", tuple, rel) / ("dict", length, "L"|"I"|"R"), reference order."""
    n = len(text)
    types = [char_type(c) for c in text]
    ex = [[] for _ in range(n - 1)]
    for i in range(n - 1):
        for m in range(charn):
            for j in range(max(0, i + 1 - charw), max(0, min(i + 1 + charw, n) - m)):
                ex[i].append(("char", text[j:j + m + 1], j - i - 1))
        for m in range(typen):
            for j in range(max(0, i + 1 - typew), max(0, min(i + 1 + typew, n) - m)):
                ex[i].append(("type", tuple(types[j:j + m + 1]), j - i - 1))
    words = set(dict_words)
    if words:
        maxl = max(len(w) for w in words)
        # find_overlapping_iter: every occurrence of every word, in order of its end (then start)
        for end in range(1, n + 1):
            for start in range(max(0, end - maxl), end):
                if text[start:end] not in words:
                    continue
                length = min(end - start, dictn)
                if start != 0:
                    ex[start - 1].append(("dict", length, "L"))
                for b in range(start, end - 1):
                    ex[b].append(("dict", length, "I"))
                if end != n:
                    ex[end - 1].append(("dict", length, "R"))
    return ex


def key_of(f):
    kind = {"char": 0, "type": 1, "dict": 2}[f[0]]
    if kind == 2:
        return (2 << 120) | (f[1] << 99) | (_WHERE[f[2]] << 78)
    cs = [ord(c) for c in f[1]] if kind == 0 else list(f[1])
    v = kind << 120
    for k, c in enumerate(cs):
        v |= c << _SH[k]
    return v | (len(cs) << 5) | (f[2] + 16)


def decode_key(v):
    kind = (v >> 120) & 3
    if kind == 2:
        return ("dict", (v >> 99) & 0x1FFFFF, "LIR"[(v >> 78) & 0x1FFFFF])
    ln, rel = (v >> 5) & 7, (v & 31) - 16
    cs = [(v >> _SH[k]) & 0x1FFFFF for k in range(ln)]
    return ("char", "".join(map(chr, cs)), rel) if kind == 0 else ("type", tuple(cs), rel)


class RefTrainer:
    def __init__(self, charw, charn, typew, typen, dict_words=(), dictn=0):
        self.p = (charw, charn, typew, typen)
        self.dict_words, self.dictn = list(dict_words), dictn
        self.rows, self.labels = [], []

    def add_example(self, text, labels):
        for feats, lab in zip(gen_features(text, *self.p, self.dict_words, self.dictn), labels):
            row = {}
            for f in feats:
                k = key_of(f)
                row[k] = row.get(k, 0) + 1
            self.rows.append(row)
            self.labels.append(int(lab))

    def matrix(self):
        """(sorted keys, row_ptr, cols, counts, y)"""
        keys = sorted({k for r in self.rows for k in r})
        col = {k: j for j, k in enumerate(keys)}
        ptr, cols, cnt = [0], [], []
        for r in self.rows:
            for j, c in sorted((col[k], c) for k, c in r.items()):
                cols.append(j)
                cnt.append(c)
            ptr.append(len(cols))
        y = np.where(np.array(self.labels) == 1, 1.0, -1.0)
        return keys, np.array(ptr, np.int64), np.array(cols, np.int64), np.array(cnt, np.float64), y


def design(ptr, cols, cnt, nd):
    """scipy CSR of the examples with the bias column (1.0) last."""
    import scipy.sparse as sp
    nr = len(ptr) - 1
    X = sp.csr_matrix((cnt, cols, ptr), shape=(nr, nd))
    return sp.hstack([X, np.ones((nr, 1))], format="csr")


def objective(X, y, w, C, solver):
    z = y * (X @ w)
    if solver == 0:
        loss = np.where(z >= 0, np.log1p(np.exp(-np.abs(z))), -z + np.log1p(np.exp(z.clip(max=0))))
        return 0.5 * w @ w + C * loss.sum()
    d = 1 - z
    return 0.5 * w @ w + C * (d[d > 0] ** 2).sum()


def gradient(X, y, w, C, solver):
    z = y * (X @ w)
    if solver == 0:
        s = 1 / (1 + np.exp(-z))
        return w + X.T @ (C * (s - 1) * y)
    act = z < 1
    return w + 2 * X.T @ np.where(act, C * y * (z - 1), 0.0)


def tron(X, y, C, eps, solver, max_iter=1000):
    """liblinear tron.cpp (CG without a preconditioner, eps_cg = 0.1) from w = 0; returns (w, iterations, cg steps, |g0|, |g|)."""
    n = X.shape[1]
    pos = int((y > 0).sum())
    eps = eps * max(min(pos, len(y) - pos), 1) / len(y)
    state = {}

    def fun(w):
        state["z"] = X @ w
        return objective(X, y, w, C, solver)

    def grad(w):
        yz = y * state["z"]
        if solver == 0:
            s = 1 / (1 + np.exp(-yz))
            state["D"] = C * s * (1 - s)
            return w + X.T @ (C * (s - 1) * y)
        act = yz < 1
        state["D"] = np.where(act, 2 * C, 0.0)
        return w + X.T @ np.where(act, 2 * C * y * (yz - 1), 0.0)

    def hv(v):
        return v + X.T @ (state["D"] * (X @ v))

    def trcg(delta, g):
        s = np.zeros(n)
        r = -g.copy()
        d = r.copy()
        cgtol = 0.1 * np.linalg.norm(g)
        it = 0
        rTr = r @ r
        while True:
            if np.linalg.norm(r) <= cgtol:
                break
            it += 1
            Hd = hv(d)
            alpha = rTr / (d @ Hd)
            s += alpha * d
            if np.linalg.norm(s) > delta:
                s -= alpha * d
                std, sts, dtd, dsq = s @ d, s @ s, d @ d, delta * delta
                rad = math.sqrt(std * std + dtd * (dsq - sts))
                alpha = (dsq - sts) / (std + rad) if std >= 0 else (rad - std) / dtd
                s += alpha * d
                r -= alpha * Hd
                break
            r -= alpha * Hd
            rnew = r @ r
            d = r + (rnew / rTr) * d
            rTr = rnew
        return s, r, it

    eta0, eta1, eta2, sigma1, sigma2, sigma3 = 1e-4, 0.25, 0.75, 0.25, 0.5, 4
    w = np.zeros(n)
    f = fun(w)
    g = grad(w)
    delta = gnorm1 = gnorm = np.linalg.norm(g)
    search = not gnorm <= eps * gnorm1
    it, cg_total = 1, 0
    while it <= max_iter and search:
        s, r, cg = trcg(delta, g)
        cg_total += cg
        w_new = w + s
        gs = g @ s
        prered = -0.5 * (gs - s @ r)
        fnew = fun(w_new)
        actred = f - fnew
        snorm = np.linalg.norm(s)
        if it == 1:
            delta = min(delta, snorm)
        alpha = sigma3 if fnew - f - gs <= 0 else max(sigma1, -0.5 * (gs / (fnew - f - gs)))
        if actred < eta0 * prered:
            delta = min(max(alpha, sigma1) * snorm, sigma2 * delta)
        elif actred < eta1 * prered:
            delta = max(sigma1 * delta, min(alpha * snorm, sigma2 * delta))
        elif actred < eta2 * prered:
            delta = max(sigma1 * delta, min(alpha * snorm, sigma3 * delta))
        else:
            delta = max(delta, min(alpha * snorm, sigma3 * delta))
        if actred > eta0 * prered:
            it += 1
            w, f = w_new, fnew
            g = grad(w)
            gnorm = np.linalg.norm(g)
            if gnorm <= eps * gnorm1:
                break
        if f < -1.0e32:
            break
        if abs(actred) <= 0 and prered <= 0:
            break
        if abs(actred) <= 1.0e-12 * abs(f) and abs(prered) <= 1.0e-12 * abs(f):
            break
    return w, it - 1, cg_total, gnorm1, gnorm


def build_model(keys, w, bias, charw, typew, dict_words, dictn) -> bytes:
    """trainer.rs:376-487 from fp64 weights (key order) and the bias; Model::to_vec."""
    wmax = max([abs(bias)] + [abs(x) for x in w])
    m = wmax / 32767
    if m == 0:
        raise ValueError("all weights are zero")
    cw, tw = {}, {}
    dw = [[0, 0, 0] for _ in range(dictn)]
    for k, x in zip(keys, w):
        q = int(x / m)   # to_int_unchecked: toward zero
        if q == 0:
            continue
        f = decode_key(k)
        if f[0] == "dict":
            dw[f[1] - 1][_WHERE[f[2]]] = q
            continue
        ln = len(f[1])
        mp, ng = (cw, f[1]) if f[0] == "char" else (tw, bytes(f[1]))
        mp.setdefault(ng, [0] * (2 * charw - ln + 1))[charw - ln - f[2]] = q
    recs = []
    for word in dict_words:
        ln = len(word)
        d = dw[min(ln, dictn) - 1]
        ws = [d[1]] * (ln + 1)
        ws[0], ws[-1] = d[0], d[2]
        recs.append(modelfmt.WordWeightRecord(word, ws, ""))
    md = modelfmt.ModelData(
        char_ngram_model=[modelfmt.NgramData(k, cw[k]) for k in sorted(cw)],
        type_ngram_model=[modelfmt.NgramData(k, tw[k]) for k in sorted(tw)],
        dict_model=recs, bias=int(bias / m), char_window_size=charw, type_window_size=typew)
    return modelfmt.encode_model(md)
