"""The restatement of tests/trainref.py against the reference's own vectors: Trainer::gen_features' KATs check_features_3322 and
check_features_2222_dict (trainer.rs:502-868), recorded literal for literal in tests/golden/train_features_kat.json."""
import json
import os

import pytest

from tests import trainref, trainsuite
from vaporetto_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "train_features_kat.json"), encoding="utf-8"))


@pytest.mark.parametrize("name", sorted(KAT))
def test_gen_features_kat(name):
    k = KAT[name]
    s = api.Sentence.from_tokenized(k["tokenized"])
    ex = trainref.gen_features(s.as_raw_text(), k["charw"], k["charn"], k["typew"], k["typen"], k["dict"], k["dictn"])
    assert len(ex) == len(k["boundaries"])
    for b in k["boundaries"]:
        want = [(f[0], tuple(f[1]) if f[0] == "type" else f[1], f[2]) for f in b["features"]]
        assert ex[b["index"]] == want, b["index"]
        assert int(s.boundaries()[b["index"]]) == int(getattr(api.CharacterBoundary, b["label"]))


# trainref.fast_matrix is what the shaped corpora of tests/trainsuite.py are checked against; it is trusted only because it equals the
# per-boundary restatement here: on the suite's cases, and with dictn = 1 over nested words (every word in one bucket, counts above 1)
NESTED = (5, 2, 2, 1, 1, 1, True)


@pytest.mark.parametrize("case", trainsuite.CASES + [NESTED])
def test_fast_matrix_equals_restatement(case):
    import numpy as np
    seed, charw, charn, typew, typen, dictn, with_dict = case
    sents = trainsuite.corpus(seed, 200)
    words = trainsuite.dictionary(sents, seed) if with_dict else []
    r = trainref.RefTrainer(charw, charn, typew, typen, words, dictn)
    for s, lab in sents:
        r.add_example(s, lab)
    keys, ptr, cols, cnt, y = r.matrix()
    fkeys, fptr, fcols, fcnt, fy = trainref.fast_matrix(*trainref.pack_corpus(sents), charw, charn, typew, typen, words, dictn)
    assert trainref.keys_as_ints(fkeys) == keys
    assert np.array_equal(fptr, ptr) and np.array_equal(fcols, cols) and np.array_equal(fcnt, cnt) and np.array_equal(fy, y)
    if case == NESTED:
        assert any(a != b and a in b for a in words for b in words) and cnt.max() > 1
        assert {trainref.decode_key(k)[1] for k in keys if trainref.decode_key(k)[0] == "dict"} == {1}


def test_shaped_corpora_hold_their_shapes():
    trainsuite.check_shape("medium")
    trainsuite.check_shape("large")


def test_keys_round_trip():
    for f in [("char", "\U00020B9Fあ", -3), ("type", (1, 6, 3), 2), ("dict", 4, "R"), ("char", "abcde", -16)]:
        assert trainref.decode_key(trainref.key_of(f)) == f


@pytest.mark.parametrize("text,want", [  # sentence.rs:643-672
    ("ま-ぁ|良-い|だ-ろ-う", "まぁ 良い だろう"),
    ("ま-ぁ/名詞/マー|社-長/名詞/シャチョー|は/助詞/ワ|火-星 猫|だ/助動詞/ダ", "まぁ/名詞/マー 社長/名詞/シャチョー は/助詞/ワ だ/助動詞/ダ"),
    ("ま-ぁ/名詞/マー|社-長/名詞/シャチョー|は/助詞/ワ|火/名詞/ヒ-星|猫|だ/助動詞/ダ",
     "まぁ/名詞/マー 社長/名詞/シャチョー は/助詞/ワ 火星 猫 だ/助動詞/ダ"),
])
def test_from_partial_annotation_doc_vectors(text, want):
    assert api.Sentence.from_partial_annotation(text).write_tokenized_text() == want


def test_from_partial_annotation_boundaries_and_errors():
    s = api.Sentence.from_partial_annotation("a|b-c d/x\\/y")
    assert s.as_raw_text() == "abcd" and list(s.boundaries()) == [1, 0, 2]
    assert s.n_tags() == 1 and s.tags() == [None, None, None, "x/y"]
    for bad, msg in [("", "must contain at least one character"), ("a|", "invalid annotation"), ("ab", "invalid boundary character: 'b'"),
                     ("a|\0", "must not contain NULL"), ("a|bc", "invalid boundary character: 'c'")]:
        with pytest.raises(api.VaporettoError, match=msg):
            api.Sentence.from_partial_annotation(bad)


# the restatement's TRON against the liblinear that scikit-learn bundles (bias 1.0, the same C and tolerance, max_iter 1000).  On the
# seed-1 corpus the L2-loss SVC's paths part (6 against 8 iterations): its generalised Hessian jumps where a margin y z crosses 1, and
# the two codes sum in different orders; both stop by the same rule, at objectives 3e-4 apart.  Everywhere else they agree.
@pytest.mark.parametrize("solver", [0, 2])
@pytest.mark.parametrize("case", trainsuite.CASES)
def test_tron_against_sklearn_liblinear(case, solver):
    pytest.importorskip("sklearn")
    import warnings

    import numpy as np
    from sklearn.linear_model import LogisticRegression
    from sklearn.svm import LinearSVC

    seed, charw, charn, typew, typen, dictn, with_dict = case
    sents = trainsuite.corpus(seed, 200)
    words = trainsuite.dictionary(sents, seed) if with_dict else []
    r = trainref.RefTrainer(charw, charn, typew, typen, words, dictn)
    for s, lab in sents:
        r.add_example(s, lab)
    keys, ptr, cols, cnt, y = r.matrix()
    X = trainref.design(ptr, cols, cnt, len(keys))
    w, it, _, _, _ = trainref.tron(X, y, 1.0, 0.01, solver)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = (LogisticRegression(solver="liblinear", C=1.0, tol=0.01, max_iter=1000) if solver == 0 else
             LinearSVC(dual=False, C=1.0, tol=0.01, max_iter=1000)).fit(X[:, :-1], y)
    ws = np.append(m.coef_.ravel(), m.intercept_)
    fo, fs = trainref.objective(X, y, w, 1.0, solver), trainref.objective(X, y, ws, 1.0, solver)
    if solver == 2 and seed == 1:
        assert abs(fo - fs) <= 1e-3 * fs
        return
    assert abs(fo - fs) <= 1e-6 * fs
    assert it == int(np.max(m.n_iter_))
