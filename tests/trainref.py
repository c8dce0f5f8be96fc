"""TEST INFRASTRUCTURE: a restatement of the reference's boundary trainer (vaporetto/src/trainer.rs) in plain Python / numpy.

- gen_features / RefTrainer.add_example: Trainer::gen_features and add_example (trainer.rs:260-350), features in the reference's order;
- keys: the library's 128-bit feature keys (include/vaporetto_hip.h, Trainer section), so that the sorted key table and the CSR compare;
- fast_matrix: RefTrainer.matrix() over a packed corpus in vectorised numpy, for corpora of 10^5 rows (tests/test_train_ref.py holds
  it to RefTrainer); column_sums / gnorm0_squared / stats_bounds: what vpt_train_stats must hold, from that matrix alone;
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


def pack_corpus(sents):
    """(code points, chars per sentence, labels) of [(text, labels)]: what fast_matrix reads."""
    cps = np.array([ord(c) for s, _ in sents for c in s], np.int64)
    lens = np.array([len(s) for s, _ in sents], np.int64)
    return cps, lens, np.concatenate([np.asarray(lab, np.uint8) for _, lab in sents])


def _or_shift(hi, lo, c, s):
    """hi:lo |= c << s, for symbols c below 2^21 (uint64 words of a 128-bit key)."""
    c = c.astype(np.uint64)
    if s >= 64:
        hi |= c << np.uint64(s - 64)
        return
    lo |= c << np.uint64(s)   # the bits past 63 fall off the low word ...
    if s + 21 > 64:
        hi |= c >> np.uint64(64 - s)   # ... and arrive here


def keys_as_ints(keys):
    """The (n, 2) array of (low, high) words as Python ints, for a comparison with RefTrainer.matrix() or Trainer.weights()."""
    return [int(lo) | (int(hi) << 64) for lo, hi in keys]


def fast_matrix(cps, lens, labels, charw, charn, typew, typen, dict_words=(), dictn=0):
    """RefTrainer.matrix() without a Python loop per boundary: Trainer::gen_features (trainer.rs:260-318) and add_example (:321-350)
    stated per (kind, n-gram length, relative position) and per dictionary word over whole arrays.

    cps: the corpus' code points, sentence after sentence; lens: chars per sentence; labels: one per boundary.  Returns (keys, row_ptr,
    cols, counts, y): the sorted distinct keys as an (n, 2) uint64 array of (low, high) words -- the form vpt_trainer_weights gives
    them in -- and the CSR with rows in corpus order, columns in key order and a feature's occurrences at a boundary as its count."""
    from vaporetto_amd.api import _types_of
    cps, lens = np.asarray(cps, np.int64), np.asarray(lens, np.int64)
    assert lens.min() >= 1 and lens.sum() == len(cps)
    n_sent = len(lens)
    types = _types_of(cps).astype(np.int64)
    cbase = np.cumsum(lens) - lens                       # a sentence's first char
    rbase = np.concatenate([[0], np.cumsum(lens - 1)])   # ... and first boundary (row)
    total_b = int(rbase[-1])
    assert len(labels) == total_b
    sent = np.repeat(np.arange(n_sent), lens - 1)
    p = np.arange(total_b) - rbase[sent]                 # the boundary between chars p and p + 1 of its sentence
    n = lens[sent]
    g0 = cbase[sent] + p + 1                             # the char at relative position 0
    rows, his, los = [], [], []
    # n-grams of m + 1 symbols starting at j = p + 1 + rel: max(0, p + 1 - w) <= j and j + m < min(p + 1 + w, n)
    for kind, (w, ng, sym) in enumerate(((charw, charn, cps), (typew, typen, types))):
        for m in range(ng):
            for rel in range(-w, w - m):
                j = p + 1 + rel
                r = np.flatnonzero((j >= 0) & (j + m < n))
                hi = np.full(len(r), kind << 56, np.uint64)
                lo = np.full(len(r), ((m + 1) << 5) | (rel + 16), np.uint64)
                for k in range(m + 1):
                    _or_shift(hi, lo, sym[g0[r] + rel + k], _SH[k])
                rows.append(r)
                his.append(hi)
                los.append(lo)
    # find_overlapping_iter: every occurrence of every word inside a sentence; Left of its first char, Right of its last, Inside between
    csent = np.repeat(np.arange(n_sent), lens)
    cloc = np.arange(len(cps)) - cbase[csent]
    for word in sorted(set(dict_words)):
        ln = len(word)
        if ln > len(cps):
            continue
        ok = np.ones(len(cps) - ln + 1, bool)
        for k, c in enumerate(word):
            ok &= cps[k:len(cps) - ln + 1 + k] == ord(c)
        at = np.flatnonzero(ok)
        at = at[cloc[at] + ln <= lens[csent[at]]]
        r0, a = rbase[csent[at]], cloc[at]
        left, right = a != 0, a + ln != lens[csent[at]]
        inside = np.repeat(r0 + a, ln - 1) + np.tile(np.arange(ln - 1), len(at))
        for where, r in ((0, (r0 + a - 1)[left]), (1, inside), (2, (r0 + a + ln - 1)[right])):
            rows.append(r)
            his.append(np.full(len(r), (2 << 56) | (min(ln, dictn) << 35) | (where << 14), np.uint64))
            los.append(np.zeros(len(r), np.uint64))
    rows, hi, lo = np.concatenate(rows), np.concatenate(his), np.concatenate(los)
    order = np.lexsort((lo, hi))
    first = np.ones(len(order), bool)
    first[1:] = (hi[order][1:] != hi[order][:-1]) | (lo[order][1:] != lo[order][:-1])
    col = np.empty(len(order), np.int64)
    col[order] = np.cumsum(first) - 1
    keys = np.stack([lo[order][first], hi[order][first]], axis=1)
    nd = len(keys)
    assert total_b * nd < 2 ** 62
    code, cnt = np.unique(rows * nd + col, return_counts=True)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(code // nd, minlength=total_b))]).astype(np.int64)
    y = np.where(np.asarray(labels) == 1, 1.0, -1.0)
    return keys, ptr, code % nd, cnt.astype(np.float64), y


def column_lengths(cols, nd):
    return np.bincount(cols, minlength=nd)


def xtv_levels(col_len, seg=64):
    """Levels of the trainer's segmented X^T v (capi_train.cpp csc_levels): a level cuts every column into segments of `seg` values, and
    the last level is the one that leaves one segment per column."""
    levels, ln = 0, np.asarray(col_len)
    while True:
        ln = (ln + seg - 1) // seg
        levels += 1
        if np.all(ln == 1):
            return levels


def column_sums(ptr, cols, cnt, y, nd):
    """sum_i x_ij y_i per column in int64, and sum_i y_i: exact."""
    cols = np.asarray(cols, np.int64)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    t = np.asarray(cnt).astype(np.int64) * np.asarray(y).astype(np.int64)[rows]
    order = np.argsort(cols, kind="stable")
    return _segment_sums(t[order], np.searchsorted(cols[order], np.arange(nd)), np.int64), int(np.asarray(y).astype(np.int64).sum())


def gnorm0_squared(ptr, cols, cnt, y, nd):
    """S = sum_j (sum_i x_ij y_i)^2 + (sum_i y_i)^2 in Python integers.  At w = 0 every row's gz is -2 C y (solver 2) or -C y / 2
    (solver 0: 1 / (1 + exp(-0)) is exactly 0.5), so with C = 1 the squared norm of the first gradient is 4 S or S / 4, and every
    partial sum on the way is an integer multiple of 1/2 below 2^53: exact in fp64 in any order."""
    cs, b = column_sums(ptr, cols, cnt, y, nd)
    return sum(int(v) * int(v) for v in cs) + b * b


def check_gnorm0(stats, ptr, cols, cnt, y, nd, solver):
    """stats["gnorm0"] of a training with C = 1 is the square root of gnorm0_squared's integer times 4 (solver 2) or 1/4 (solver 0),
    bit for bit."""
    S = gnorm0_squared(ptr, cols, cnt, y, nd)
    assert 4 * S < 2 ** 53
    want = math.sqrt(4 * S) if solver == 2 else math.sqrt(S / 4)
    assert stats["gnorm0"] == want, (stats["gnorm0"], want, S)


_U = 2.0 ** -53
_EXT = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else None


def _segment_sums(t, start, dtype):
    """Sums of t[start[k] : start[k + 1]] (the last to the end; a segment may be empty) in `dtype`; dtype None: extended precision,
    np.longdouble where it has a 64-bit significand, else math.fsum."""
    start = np.asarray(start, np.int64)
    ends = np.append(start[1:], len(t))
    full = ends > start
    if dtype is None and _EXT is None:
        return np.array([math.fsum(t[a:e]) for a, e in zip(start, ends)])
    out = np.zeros(len(start), dtype or _EXT)
    if full.any():
        out[full] = np.add.reduceat(t.astype(out.dtype), start[full])
    return out


def _total(t):
    return np.sum(t.astype(_EXT)) if _EXT is not None else math.fsum(t)


def stats_bounds(ptr, cols, cnt, y, w, b, C, solver):
    """(f, |g|, bound on f, bound on |g|) at weights w and bias b: the objective and gradient norm of liblinear's l2r_lr_fun (solver 0) /
    l2r_l2_svc_fun (solver 2) in extended precision, and how far an fp64 evaluation that sums in any order may lie from them.

    A sum of n fp64 terms t_i in any order is within (n - 1) 2^-53 sum |t_i| of the exact sum.  That gives dz_i for z = Xw + b; it
    reaches the loss through its Lipschitz constant (2 C |1 - y z| for solver 2, C for solver 0) and gz through 2 C or C / 4 (gz is
    continuous at y z = 1, so a row whose activity flips within rounding stays inside); then the sums over rows and over a column's
    nonzeros add their own term.  The whole is doubled for second-order terms and the few ulps of exp, log and the products.  Nothing
    in it is measured on the code under test."""
    ext = _EXT if _EXT is not None else np.float64
    ptr, cols = np.asarray(ptr, np.int64), np.asarray(cols, np.int64)
    w, cnt = np.asarray(w, np.float64), np.asarray(cnt, np.float64)
    nr, nd = len(ptr) - 1, len(w)
    row_len = np.diff(ptr)
    rows = np.repeat(np.arange(nr), row_len)
    wx, bx = w.astype(ext), ext(b)
    z = _segment_sums(cnt.astype(ext) * wx[cols], ptr[:-1], None) + bx
    dz = row_len * _U * (_segment_sums(np.abs(cnt * w[cols]), ptr[:-1], np.float64) + abs(b))   # row_len + 1 terms
    yz = y.astype(ext) * z
    if solver == 0:
        loss = C * np.where(yz >= 0, np.log1p(np.exp(-np.abs(yz))), -yz + np.log1p(np.exp(np.minimum(yz, 0))))
        gz = C * (1 / (1 + np.exp(-yz)) - 1) * y
        lip_loss, lip_gz = np.full(nr, float(C)), C / 4
    else:
        d = np.maximum(1 - yz, 0)
        loss = C * d * d
        gz = -2 * C * y * d
        lip_loss, lip_gz = 2 * C * np.abs(1 - yz).astype(np.float64), 2 * C
    reg = (_total(wx * wx) + bx * bx) / 2
    f = reg + _total(loss)
    bound_f = nd * _U * float(reg) + (nr - 1) * _U * float(_total(np.abs(loss))) + float(np.sum(lip_loss * dz)) + _U * float(f)
    # g_j = w_j + sum_i x_ij gz_i (len_j + 1 terms), the bias: b + sum_i gz_i (nr + 1 terms)
    order = np.argsort(cols, kind="stable")
    start = np.searchsorted(cols[order], np.arange(nd))
    col_len = np.diff(np.append(start, len(cols)))
    tg = (cnt.astype(ext) * gz[rows])[order]
    g = np.append(wx + _segment_sums(tg, start, None), bx + _total(gz))
    dg = (col_len * _U * (np.abs(w) + _segment_sums(np.abs(tg).astype(np.float64), start, np.float64))
          + lip_gz * _segment_sums((cnt * dz[rows])[order], start, np.float64))
    dg_b = nr * _U * (abs(b) + float(np.sum(np.abs(gz)))) + lip_gz * float(np.sum(dz))
    gnorm = np.sqrt(_total(g * g))
    bound_g = float(np.sqrt(np.sum(dg * dg) + dg_b * dg_b)) + nd * _U * float(gnorm) / 2   # the norm's own sum of nd + 1 squares
    return f, gnorm, 2 * bound_f, 2 * bound_g


def check_stats(stats, ptr, cols, cnt, y, w, b, C, solver):
    """stats["objective"] and stats["gnorm"] are f and |g| at (w, b) within stats_bounds; returns the two error / bound ratios."""
    f, gnorm, bf, bg = stats_bounds(ptr, cols, cnt, y, w, b, C, solver)
    ext = type(f)
    rf, rg = float(abs(ext(stats["objective"]) - f)) / bf, float(abs(ext(stats["gnorm"]) - gnorm)) / bg
    assert rf <= 1 and rg <= 1, (rf, rg, float(f), float(gnorm), bf, bg)
    return rf, rg


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
