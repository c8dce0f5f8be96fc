"""The restatement of tests/tagtrainref.py pinned on the CPU, without the library's trainer: hand-worked feature sets, its per-class
weights against the liblinear that scikit-learn bundles, the mapping the reference's own tagged corpus gives, and the margins of the
corpus whose tags an adjacent char decides."""
import os

import numpy as np
import pytest

from tests import tagtrainref, tagtrainsuite, trainref
from vaporetto_amd import api, modelfmt

HERE = os.path.dirname(os.path.abspath(__file__))


def _feats(text, start, end):
    types = [trainref.char_type(c) for c in text]
    return tagtrainref.token_features(text, types, start, end, 2, 1), types


def test_features_of_a_token_at_the_start():
    # "あい|う|え": token [0, 2); charn 2: n-grams of 3 and 4 chars covering it; typen 1: of 3 chars
    f, ty = _feats("あいうえ", 0, 2)
    assert f == [("char", "あいう", 1), ("char", "あいうえ", 2), ("type", tuple(ty[0:3]), 1)]


def test_features_of_a_token_in_the_middle():
    # "あ|い|うえ": token [1, 2): i runs over end - len .. start
    f, ty = _feats("あいうえ", 1, 2)
    assert f == [("char", "あい", 0), ("char", "いう", 1), ("char", "あいう", 1), ("char", "いうえ", 2),
                 ("type", tuple(ty[0:2]), 0), ("type", tuple(ty[1:3]), 1)]


def test_features_of_a_token_at_the_end_and_of_a_whole_sentence():
    f, ty = _feats("あいうえ", 2, 4)
    assert f == [("char", "いうえ", 0), ("char", "あいうえ", 0), ("type", tuple(ty[1:4]), 0)]
    # a combination that a sentence edge cuts is absent, never shortened
    assert _feats("あ", 0, 1)[0] == []
    assert _feats("あい", 0, 2)[0] == []


def test_keys_hold_the_context_alone():
    f, _ = _feats("あいうえ", 1, 2)
    keys = [tagtrainref.key_of(x, 1) for x in f]
    assert len(set(keys)) == len(keys)
    assert trainref.decode_key(keys[0]) == ("char", "あ", 0) and trainref.decode_key(keys[3]) == ("char", "うえ", 2)
    assert trainref.decode_key(keys[2]) == ("char", "あう", 1)


def test_token_ranges_skip_unknown():
    assert list(tagtrainref.token_ranges([1, 2, 1, 0], 5)) == [(0, 1), (3, 5)]
    assert list(tagtrainref.token_ranges([0, 2], 3)) == []
    assert list(tagtrainref.token_ranges([], 1)) == [(0, 1)]
    # two skipped tokens in a row, then a token: it starts behind the last WordBoundary, [5, 6).  (The reference's TokenIterator adds
    # `i + 1` to `start` at every skip of one call, sentence.rs:1279-1281, and would start it at 7, past the sentence: the library and
    # this restatement share the documented divergence, DESIGN "Tag-model training".)
    assert list(tagtrainref.token_ranges([2, 1, 0, 2, 1], 6)) == [(5, 6)]


def test_golden_corpus_gives_the_reference_models_mapping():
    lines = [l for l in open(os.path.join(HERE, "golden", "docs.tok"), encoding="utf-8").read().split("\n") if l]
    r = tagtrainref.RefTagTrainer(3, 3)
    for l in lines:
        s = api.Sentence.from_tokenized(l)
        r.add_example(s.as_raw_text(), s.boundaries(), s.n_tags(), s.tags())
    models = r.models()
    md = modelfmt.decode_model(open(os.path.join(HERE, "golden", "model.bin"), "rb").read())[0]
    assert len(md.tag_models) == 8
    assert {m["token"]: m["tags"] for m in models} == {m.token: m.tags for m in md.tag_models}
    by = {m["token"]: m for m in models}
    assert by["まぁ"]["tags"] == [["名詞", "副詞"], ["マー"]]
    assert [p["slot"] for p in by["まぁ"]["problems"]] == [0]
    assert all(not m["problems"] for t, m in by.items() if t != "まぁ")
    W, _ = tagtrainref.solve(by["まぁ"]["problems"][0], 0.01, 1.0, 2)
    assert np.array_equal(W[1], -W[0])
    assert [m["token"] for m in models] == sorted(by, key=lambda s: s.encode())


@pytest.mark.parametrize("solver", [0, 2])
def test_per_class_weights_against_sklearn_liblinear(solver):
    pytest.importorskip("sklearn")
    import warnings

    from sklearn.linear_model import LogisticRegression
    from sklearn.svm import LinearSVC
    params = tagtrainsuite.CASES["small"]
    r = tagtrainref.RefTagTrainer(params[4], params[6], tagtrainsuite.TAG_DICTIONARY)
    for s in tagtrainsuite.corpus(params[0], params[1], params[2]):
        r.add_example(*s)
    n = 0
    for m in r.models():
        for p in m["problems"]:
            X = tagtrainref.design(p)
            W, stats = tagtrainref.solve(p, 0.01, 1.0, solver)
            k = len(p["candidates"])
            for c in range(k):
                # one binary fit per class; scikit-learn reports a binary problem for its second class (+1 here)
                y = np.where(p["y"] == c, 1.0, -1.0)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    mdl = (LogisticRegression(solver="liblinear", C=1.0, tol=0.01, max_iter=1000) if solver == 0 else
                           LinearSVC(dual=False, C=1.0, tol=0.01, max_iter=1000, intercept_scaling=1)).fit(X[:, :-1], y)
                ws = np.append(mdl.coef_.ravel(), mdl.intercept_)
                fo, fs = trainref.objective(X, y, W[c], 1.0, solver), trainref.objective(X, y, ws, 1.0, solver)
                assert abs(fo - fs) <= 1e-6 * fs, (m["token"], p["slot"], c)
                assert stats[c][0] == int(np.max(mdl.n_iter_)), (m["token"], p["slot"], c)
                n += 1
    assert n > 10


def test_decided_corpus_margins():
    """The restatement-trained model reproduces every gold tag of the decided corpus with an integer score gap of at least 2 between the
    best and the second candidate: larger than any truncation flip of a quantised weight."""
    params = tagtrainsuite.DECIDED
    r = tagtrainref.RefTagTrainer(params[4], params[6])
    sents = tagtrainsuite.decided_corpus()
    for s in sents:
        r.add_example(*s)
    n = 0
    for m in r.models():
        for p in m["problems"]:
            W, _ = tagtrainref.solve(p, 0.01, 1.0, 2)
            Q = np.trunc(W / (max(1e-6, np.abs(W).max()) / 32767))
            scores = tagtrainref.design(p) @ Q.T
            order = np.sort(scores, axis=1)
            assert np.array_equal(scores.argmax(axis=1), p["y"]), m["token"]
            assert (order[:, -1] - order[:, -2]).min() >= 2, m["token"]
            n += len(p["y"])
    assert n > 300
