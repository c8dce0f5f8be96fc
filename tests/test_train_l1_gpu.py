"""Solver 5 (Trainer(l1r=True), L1-regularised L2-loss SVC) on the MI355X against the restatement of tests/l1ref.py (the checks of
tests/l1suite.py), and a sparse model trained on the golden corpus, predicted with the library and held to the CPU oracle."""
import os

import numpy as np
import pytest

from tests import l1suite
from vaporetto_amd import api

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("case", l1suite.CASES)
def test_solver5_weights_stats_model_and_determinism(case):
    l1suite.check_solver5(case)


def test_errors():
    l1suite.check_errors()


def test_golden_corpus_trains_a_sparse_model_the_oracle_agrees_on():
    """docs.tok with its tags stripped, trained with solver 5 (eps 0.01, C 1): the library's predictor and the CPU oracle give the same
    scores and labels for the model, bit for bit.  An L1 model need not separate its training set, so the count is printed and not
    asserted; recorded on the MI355X: it re-splits 2 of the 2 sentences exactly, with 11 of 224 weights nonzero after 40 sweeps."""
    from oracle import cbind
    lines = [l for l in open(os.path.join(HERE, "golden", "docs.tok"), encoding="utf-8").read().split("\n") if l]
    sents = [api.Sentence.from_tokenized(" ".join(tok.split("/")[0] for tok in l.split(" "))) for l in lines]   # --ignore-tags
    t = api.Trainer(3, 3, 3, 3, l1r=True)
    t.add_examples(sents)
    mbytes = t.train_bytes(0.01, 1.0, int(api.SolverType.L1RegularizedL2LossSVC))
    w, b, _ = t.weights()
    pred = api.Predictor(api.Model.read_slice(mbytes)[0], False, device=0)
    utf8, boff = api.pack_texts([s.as_raw_text().encode("utf-8") for s in sents])
    scores, labels, ooff = pred.predict_packed(utf8, boff)
    o_scores, o_labels, o_ooff, _ = cbind.OraclePredictor(mbytes).predict_batch(utf8, boff)
    assert np.array_equal(scores, o_scores) and np.array_equal(labels, o_labels) and np.array_equal(ooff, o_ooff)
    exact = 0
    for s in sents:
        r = api.Sentence.from_raw(s.as_raw_text())
        pred.predict(r)
        exact += list(r.iter_tokens()) == list(s.iter_tokens())
    print("solver 5 on docs.tok: %d of %d sentences re-split exactly, %d of %d weights nonzero, %d model bytes, %s"
          % (exact, len(sents), int(np.count_nonzero(w)), len(w), len(mbytes), t.last_stats()))
    assert np.count_nonzero(w) < len(w)
