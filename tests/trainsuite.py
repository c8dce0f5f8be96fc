"""TEST INFRASTRUCTURE: the trainer checks shared by the emulator tests (tests/test_train_emu.py) and the GPU tests
(tests/test_train_gpu.py), against the restatement of tests/trainref.py."""
import functools
import math

import numpy as np
import pytest

from tests import trainref
from vaporetto_amd import api

ALPHABET = "0１9aZｚあいうかがカタナーン漢字東京。、!?-　 \U00020B9F\U0002000B"


def corpus(seed, n_sent=200, max_len=24, unknown=0.1):
    """Seeded sentences (text, labels): every char type, non-BMP chars, one-char sentences, some Unknown labels."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_sent):
        n = 1 if i % 17 == 0 else int(rng.integers(2, max_len))
        text = "".join(ALPHABET[k] for k in rng.integers(0, len(ALPHABET), n))
        lab = (rng.random(n - 1) < 0.4).astype(np.uint8)
        lab[rng.random(n - 1) < unknown] = 2
        out.append((text, lab))
    return out


def dictionary(sents, seed):
    """Words that occur in the corpus, nested and overlapping ones among them (a word and its prefixes / suffixes)."""
    rng = np.random.default_rng(seed + 1)
    words = set()
    for text, _ in sents[:40]:
        if len(text) >= 4:
            a = int(rng.integers(0, len(text) - 3))
            w = text[a:a + 4]
            words.update({w, w[:2], w[1:3], w[2:]})
    return sorted(words)


CASES = [  # (seed, charw, charn, typew, typen, dictn, with dictionary)
    (1, 3, 3, 2, 2, 4, True),
    (2, 2, 2, 2, 2, 2, True),
    (3, 4, 5, 1, 3, 1, False),
]


def run_pair(case, solver, n_sent=200):
    seed, charw, charn, typew, typen, dictn, with_dict = case
    sents = corpus(seed, n_sent)
    words = dictionary(sents, seed) if with_dict else []
    t = api.Trainer(charw, charn, typew, typen, words, dictn if words else 0)
    utf8, boff = api.pack_texts([s.encode("utf-8") for s, _ in sents])
    t.add_packed(utf8, boff, np.concatenate([lab for _, lab in sents]))
    r = trainref.RefTrainer(charw, charn, typew, typen, words, dictn)
    for s, lab in sents:
        r.add_example(s, lab)
    return t, r, words


STABLE = {(1, 0), (3, 0), (3, 2)}   # (seed, solver) whose TRON path does not depend on the order of the sums


def quantised(w):
    """trainer.rs:376-400: trunc(w / (max |w| / 32767)), the bias included (the last entry)."""
    m = np.abs(w).max() / 32767
    return np.trunc(w / m).astype(np.int64)


def check_matrix(case):
    t, r, _ = run_pair(case, 2)
    keys, ptr, cols, cnt, _ = r.matrix()
    assert t.n_features() == len(keys)
    gptr, gcols, gcnt = t.csr()
    assert np.array_equal(gptr.astype(np.int64), ptr)
    assert np.array_equal(gcols.astype(np.int64), cols)
    assert np.array_equal(gcnt.astype(np.float64), cnt)
    t.train_bytes(0.1, 1.0, 2)
    assert t.weights()[2] == keys


def check_solver(case, solver, eps=0.01, cost=1.0):
    t, r, words = run_pair(case, solver)
    model = t.train_bytes(eps, cost, solver)
    w, b, keys = t.weights()
    stats = t.last_stats()
    k, ptr, cols, cnt, y = r.matrix()
    assert keys == k
    X = trainref.design(ptr, cols, cnt, len(k))
    wr, it, cg, g0, _ = trainref.tron(X, y, cost, eps, solver)
    wg = np.append(w, b)
    # the stopping rule, recomputed from the CSR (1 % slack for summation order)
    pos = int((y > 0).sum())
    tol = eps * max(min(pos, len(y) - pos), 1) / len(y)
    g = trainref.gradient(X, y, wg, cost, solver)
    assert np.linalg.norm(g) <= tol * np.linalg.norm(trainref.gradient(X, y, np.zeros_like(wg), cost, solver)) * 1.01
    # Only the summation order differs from the restatement, but CG amplifies it over its steps, and the L2-loss SVC's generalised
    # Hessian jumps where a margin y z crosses 1: on some corpora the paths part (seed 1 / solver 2 takes 6 or 8 iterations, seed 2 /
    # solver 0 32 or 35 CG steps, depending on the order of the sums alone).  Where the path is stable (STABLE) the iteration and CG
    # counts are equal, the weights agree to 1e-7 and quantised weights differ only at integer steps; everywhere both solutions satisfy the
    # stopping rule and their objectives agree to 1e-3.
    fg, fr = trainref.objective(X, y, wg, cost, solver), trainref.objective(X, y, wr, cost, solver)
    assert abs(fg - fr) <= 1e-3 * abs(fr)
    if (case[0], solver) in STABLE:
        assert (stats["iterations"], stats["cg_steps"]) == (it, cg)
        assert np.linalg.norm(wg - wr) / np.linalg.norm(wr) <= 1e-7
        # truncation flips a quantised weight only where the weight lies within rounding of an integer step, by one.  Features that
        # always occur together share a weight, so one such weight flips a group: 40 of 29574 (99.86 %) on seed 3 / solver 2.
        qg, qr = quantised(wg), quantised(wr)
        diff = np.flatnonzero(qg != qr)
        assert len(diff) <= 0.005 * len(qg) and np.abs(qg - qr).max() <= 1
        u = wr[diff] / (np.abs(wr).max() / 32767)
        assert np.all(np.abs(u - np.round(u)) < 1e-2)
    # the library's model is the restatement's quantisation of the library's weights, byte for byte
    charw, typew, dictn = case[1], case[3], case[5]
    assert model == trainref.build_model(keys, w, b, charw, typew, words, dictn if words else 0)
    # two trainings: identical bytes
    assert t.train_bytes(eps, cost, solver) == model
    t2, _, _ = run_pair(case, solver)
    assert t2.train_bytes(eps, cost, solver) == model
    return model


# ---------------------------------------------------------------------------------------------------- shaped corpora
# With charw = charn = typew = typen = 1 a boundary has four n-gram features: the char and the type on either side.  A char planted k
# times, never first or last in its sentence, therefore owns two columns of exactly k nonzeros.  The dictionary's words nest and
# overlap and all fall into the bucket min(len, dictn) = 1, so its three columns (Left, Inside, Right) carry counts above 1.
SHAPED_PARAMS = (1, 1, 1, 1)
SHAPED_WORDS = ["カキ", "カキク", "キク", "キクケ"]
SHAPED_DICTN = 1
PLANTED = (1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)    # the edges of seg_count_kernel and xtv_level_kernel, levels 1 and 2
PLANTED_LARGE = (262143, 262144, 262145)                       # ... and of level 3
_MARK0, _DIST0, _N_DIST, _PHRASE = 0x4E00, 0x5000, 2200, "カキクケ"   # planted Kanji, Kanji that occur once, the text the words lie in
_HEAD, _TAIL, _LONE, _A, _I = ord("ノ"), ord("。"), ord("ん"), ord("あ"), ord("い")
_SEEDS = {"medium": 41, "large": 42}
_TILE, _SEG = 4096, 64                                         # kernels_train.hip: kTile (256 threads * 16) and kSeg


@functools.lru_cache(maxsize=None)
def shaped_corpus(size):
    """"medium" or "large": (code points, chars per sentence).  A regular sentence is _HEAD, a stretch of the shuffled body, _TAIL; in
    front of every seventh sentence and at the very end stands a sentence of one char (no boundary).  Whole arrays, no loop per char.

    "large" adds 262143 あ and 2 い to the body and ends its last regular sentence with あ in place of _TAIL.  No other char is
    Hiragana, so the columns (あ, -1), (あ, 0) and (Hiragana, -1) have 262143, 262144 and 262145 nonzeros: the three lengths around
    64^3 from one stretch of text, not three."""
    rng = np.random.default_rng(_SEEDS[size])
    planted = [(_MARK0 + k, n) for k, n in enumerate(PLANTED)]
    if size == "large":
        planted += [(_A, PLANTED_LARGE[0]), (_I, 2)]
    n_phrase = 300 if size == "medium" else 3000
    # the body's tokens: a planted char, a char that occurs once, or the phrase (0; kept whole)
    tok = np.concatenate([np.full(n, c) for c, n in planted] + [np.arange(_DIST0, _DIST0 + _N_DIST), np.zeros(n_phrase, np.int64)])
    tok = tok[rng.permutation(len(tok))]
    ln = np.where(tok == 0, len(_PHRASE), 1)
    src = np.repeat(np.arange(len(tok)), ln)
    within = np.arange(len(src)) - np.repeat(np.cumsum(ln) - ln, ln)
    body = np.where(tok[src] == 0, np.array([ord(c) for c in _PHRASE])[within], tok[src])
    # stretches of 1 .. 38 chars
    cut = np.cumsum(rng.integers(1, 39, len(body)))
    start = np.concatenate([[0], cut[cut < len(body)]])
    lens = np.diff(np.append(start, len(body))) + 2
    s0 = np.cumsum(lens) - lens
    cps = np.full(int(lens.sum()), -1, np.int64)
    cps[s0], cps[s0 + lens - 1] = _HEAD, _TAIL
    cps[cps == -1] = body
    if size == "large":
        cps[-1] = _A
    at = np.arange(0, len(lens), 7)
    cps = np.append(np.insert(cps, s0[at], _LONE), _LONE)
    lens = np.append(np.insert(lens, at, 1), 1)
    cps.flags.writeable = lens.flags.writeable = False
    return cps, lens


@functools.lru_cache(maxsize=None)
def shaped_reference(size):
    """(keys, row_ptr, cols, counts) of the corpus by trainref.fast_matrix: computed once, shared, read-only."""
    cps, lens = shaped_corpus(size)
    out = trainref.fast_matrix(cps, lens, np.zeros(int((lens - 1).sum()), np.uint8), *SHAPED_PARAMS, SHAPED_WORDS, SHAPED_DICTN)[:4]
    for a in out:
        a.flags.writeable = False
    return out


def check_shape(size):
    """What the corpus is for, asserted on the restatement's matrix alone: a generator that misses a shape fails here."""
    cps, lens = shaped_corpus(size)
    keys, ptr, cols, cnt = shaped_reference(size)
    n_rows, nd = len(ptr) - 1, len(keys)
    col_len = trainref.column_lengths(cols, nd)
    occ = int(cnt.sum())
    lone = np.flatnonzero(lens == 1)
    assert lens[-1] == 1 and len(lone) > 2 and lone[0] == 0 and np.all(np.diff(lone) > 1)   # interleaved, and the last sentence
    assert cnt.max() > 1 and (cnt > 1).sum() >= 0.005 * len(cnt)                             # dictionary words sharing a bucket
    assert n_rows > _TILE and nd > _TILE                                                     # dot_kernel: a second pass over both
    assert set(PLANTED) <= set(col_len.tolist())
    if size == "medium":
        assert _TILE < col_len.max() <= _SEG ** 3 and trainref.xtv_levels(col_len, _SEG) == 3
    else:
        assert col_len.max() > _SEG ** 3 and trainref.xtv_levels(col_len, _SEG) == 4
        assert set(PLANTED_LARGE) <= set(col_len.tolist())
        # the type unigram all those boundaries share
        hira = trainref.key_of(("type", (trainref.char_type("あ"),), -1))
        assert col_len[trainref.keys_as_ints(keys).index(hira)] == PLANTED_LARGE[2]
        # scan_top_kernel walks the tile sums 256 at a time: its carry loop runs more than once over the occurrence flags
        assert occ > 256 * _TILE and math.ceil(occ / _TILE) > 256


LABELS = ("random", "all_but_one", "alternating", "learnable")


def shaped_labels(size, name):
    """random: a 40 / 60 split; all_but_one: WordBoundary everywhere but at one row; alternating: by row index, about 5 % Unknown (which
    trains as -1); learnable: decided by the char behind the boundary, 10 % flipped (for a real solve)."""
    cps, lens = shaped_corpus(size)
    n = int((lens - 1).sum())
    rng = np.random.default_rng(_SEEDS[size] + 7 + LABELS.index(name))
    if name == "random":
        return (rng.random(n) < 0.4).astype(np.uint8)
    if name == "all_but_one":
        lab = np.ones(n, np.uint8)
        lab[n // 3] = 0
        return lab
    if name == "alternating":
        lab = (np.arange(n) % 2).astype(np.uint8)
        lab[rng.random(n) < 0.05] = 2
        return lab
    right = np.delete(cps, np.cumsum(lens) - lens)   # every char but a sentence's first: the char behind each boundary
    return ((right % 3 == 0) ^ (rng.random(n) < 0.1)).astype(np.uint8)


def shaped_trainer(size, labels):
    cps, lens = shaped_corpus(size)
    utf8 = np.frombuffer(cps.astype("<u4").tobytes().decode("utf-32-le").encode("utf-8"), np.uint8)
    nbytes = 1 + (cps >= 0x80) + (cps >= 0x800) + (cps >= 0x10000)
    boff = np.concatenate([[0], np.cumsum(nbytes)[np.cumsum(lens) - 1]]).astype(np.uint64)
    t = api.Trainer(*SHAPED_PARAMS, SHAPED_WORDS, SHAPED_DICTN)
    t.add_packed(utf8, boff, labels)
    return t


def loose_eps(y):
    """TRON's relative tolerance is eps * min(pos, neg) / l (liblinear's train_one); 0.9 stops it at the first step that takes a tenth
    off the gradient.  At 1 it would not start, and a trainer without weights has no stats to read."""
    pos = int((y > 0).sum())
    return 0.9 * len(y) / min(pos, len(y) - pos)


def check_shaped_matrix(size):
    """(a) the key table and the CSR equal the restatement's, element for element."""
    check_shape(size)
    keys, ptr, cols, cnt = shaped_reference(size)
    labels = shaped_labels(size, "random")
    t = shaped_trainer(size, labels)
    assert t.n_features() == len(keys)
    gptr, gcols, gcnt = t.csr()
    assert np.array_equal(gptr.astype(np.int64), ptr)
    assert np.array_equal(gcols.astype(np.int64), cols)
    assert np.array_equal(gcnt.astype(np.float64), cnt)
    t.train_bytes(loose_eps(np.where(labels == 1, 1.0, -1.0)), 1.0, 2)
    assert t.weights()[2] == trainref.keys_as_ints(keys)


def check_shaped_stats(size, name):
    """(b) gnorm0 bit for bit and (c) objective and gnorm at the returned weights within the fp64 summation bound, for both solvers
    after a step or two of TRON; returns {solver: (objective error / bound, gnorm error / bound)}."""
    check_shape(size)
    keys, ptr, cols, cnt = shaped_reference(size)
    labels = shaped_labels(size, name)
    y = np.where(labels == 1, 1.0, -1.0)
    t = shaped_trainer(size, labels)
    ratios = {}
    for solver in (2, 0):
        t.train_bytes(loose_eps(y), 1.0, solver)
        stats = t.last_stats()
        w, b, _ = t.weights()
        assert stats["iterations"] >= 1
        trainref.check_gnorm0(stats, ptr, cols, cnt, y, len(keys), solver)
        ratios[solver] = trainref.check_stats(stats, ptr, cols, cnt, y, w, b, 1.0, solver)
    print("error / bound (objective, gnorm) %s %s: %s" % (size, name, ratios))
    return ratios


def check_shaped_determinism(size, eps=0.1):
    """(d) two trainers fed the same corpus: the same model bytes and the same stats.  On a device the insert table's compare-and-swap
    winners differ from run to run; the order of the key sort has to hide that."""
    labels = shaped_labels(size, "learnable")
    t1, t2 = shaped_trainer(size, labels), shaped_trainer(size, labels)
    m1, m2 = t1.train_bytes(eps, 1.0, 2), t2.train_bytes(eps, 1.0, 2)
    assert m1 == m2
    assert t1.last_stats() == t2.last_stats()
    assert t1.last_stats()["iterations"] >= 1


def check_shaped_solve(size, eps=0.01, cost=1.0, solver=2):
    """(e) a real solve: check_solver's stopping rule and objective against trainref.tron over the restatement's matrix, and (c) at the
    solution.  The pair is not in STABLE: whether its path is the restatement's step for step has not been established."""
    keys, ptr, cols, cnt = shaped_reference(size)
    labels = shaped_labels(size, "learnable")
    y = np.where(labels == 1, 1.0, -1.0)
    t = shaped_trainer(size, labels)
    t.train_bytes(eps, cost, solver)
    w, b, gkeys = t.weights()
    stats = t.last_stats()
    assert gkeys == trainref.keys_as_ints(keys)
    X = trainref.design(ptr, cols, cnt, len(keys))
    wr = trainref.tron(X, y, cost, eps, solver)[0]
    wg = np.append(w, b)
    pos = int((y > 0).sum())
    tol = eps * max(min(pos, len(y) - pos), 1) / len(y)
    g = trainref.gradient(X, y, wg, cost, solver)
    assert np.linalg.norm(g) <= tol * np.linalg.norm(trainref.gradient(X, y, np.zeros_like(wg), cost, solver)) * 1.01
    fg, fr = trainref.objective(X, y, wg, cost, solver), trainref.objective(X, y, wr, cost, solver)
    assert abs(fg - fr) <= 1e-3 * abs(fr)
    trainref.check_gnorm0(stats, ptr, cols, cnt, y, len(keys), solver)
    ratios = trainref.check_stats(stats, ptr, cols, cnt, y, w, b, cost, solver)
    print("error / bound (objective, gnorm) %s solve: %s, %d iterations, %d CG steps" % (size, ratios, stats["iterations"], stats["cg_steps"]))
    return ratios


def check_errors():
    with pytest.raises(api.VaporettoError, match="typew"):
        api.Trainer(2, 2, 3, 2)
    with pytest.raises(api.VaporettoError, match="charn"):
        api.Trainer(2, 6, 2, 2)
    with pytest.raises(api.VaporettoError, match="typen"):
        api.Trainer(2, 2, 2, 0)
    with pytest.raises(api.VaporettoError, match="charw"):
        api.Trainer(17, 2, 2, 2)
    with pytest.raises(api.VaporettoError, match="dictn"):
        api.Trainer(2, 2, 2, 2, ["あ"], 0)
    with pytest.raises(api.VaporettoError, match="empty word"):
        api.Trainer(2, 2, 2, 2, ["あ", ""], 2)
    # a dictionary word that is no well-formed UTF-8 (an overlong NUL): through the C ABI, api.Trainer takes str
    import ctypes as C
    from vaporetto_amd import _lib
    prm = _lib.TrainParams(2, 2, 2, 2, 2, 0)
    word, off, h = (C.c_uint8 * 2)(0xC0, 0x80), (C.c_uint64 * 2)(0, 2), C.c_void_p()
    assert _lib.load().vpt_trainer_create(C.addressof(prm), word, off, 1, 0, C.byref(h)) == _lib.VPT_INVALID_ARGUMENT
    assert "dict_words: invalid UTF-8" in _lib.last_error()
    t = api.Trainer(2, 2, 2, 2)
    t.add_packed(*api.pack_texts(["あいう".encode()]), np.array([1, 0], np.uint8))
    for solver in (1, 3, 4, 5, 6, 7):
        with pytest.raises(api.VaporettoError, match="only 0 and 2 are implemented"):
            t.train_bytes(0.1, 1.0, solver)
    one = api.Trainer(2, 2, 2, 2)
    one.add_packed(*api.pack_texts(["あいう".encode()]), np.array([1, 1], np.uint8))
    with pytest.raises(api.VaporettoError, match="WordBoundary"):
        one.train_bytes(0.1, 1.0, 2)
    with pytest.raises(api.VaporettoError, match="labels"):
        one.add_packed(*api.pack_texts(["あい".encode()]), np.array([3], np.uint8))
