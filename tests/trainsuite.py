"""TEST INFRASTRUCTURE: the trainer checks shared by the emulator tests (tests/test_train_emu.py) and the GPU tests
(tests/test_train_gpu.py), against the restatement of tests/trainref.py."""
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
