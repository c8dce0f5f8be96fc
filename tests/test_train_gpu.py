"""The trainer on the MI355X against the restatement of tests/trainref.py (the checks of tests/trainsuite.py), plus a model trained
on the golden corpus and one on a synthetic corpus, predicted with the library and checked against the CPU oracle."""
import os

import numpy as np
import pytest

from tests import trainref, trainsuite
from vaporetto_amd import api

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("case", trainsuite.CASES)
def test_keys_and_csr_match_restatement(case):
    trainsuite.check_matrix(case)


@pytest.mark.parametrize("solver", [0, 2])
@pytest.mark.parametrize("case", trainsuite.CASES)
def test_tron_weights_model_and_determinism(case, solver):
    trainsuite.check_solver(case, solver)


def test_errors():
    trainsuite.check_errors()


# The shaped corpora of tests/trainsuite.py: "medium" (three levels of X^T v) and "large" (four levels, a scan of more than 256 tiles).
@pytest.mark.parametrize("size", ["medium", "large"])
def test_shaped_matrix_exact(size):
    trainsuite.check_shaped_matrix(size)


@pytest.mark.parametrize("labels", ["random", "all_but_one", "alternating"])
@pytest.mark.parametrize("size", ["medium", "large"])
def test_shaped_gnorm0_exact_and_stats_bounded(size, labels):
    """Observed error / bound on one MI355X, over both sizes, the three label vectors and both solvers: objective between 1.6e-7 and
    5.2e-5, gnorm between 1.9e-8 and 1.2e-4 (the largest at "medium", all_but_one, solver 0); at the solution of test_shaped_solve
    1.8e-5 and 9.0e-6.  The bound itself is about 4e-12 of the objective and 2e-10 of gnorm; dropping one row of "medium" from the
    reference moves either by more than 10^6 bounds."""
    trainsuite.check_shaped_stats(size, labels)


def test_shaped_determinism_at_scale():
    trainsuite.check_shaped_determinism("large")


def test_shaped_solve():
    trainsuite.check_shaped_solve("medium")


def test_golden_corpus_trains_a_model_that_splits_it():
    lines = [l for l in open(os.path.join(HERE, "golden", "docs.tok"), encoding="utf-8").read().split("\n") if l]
    sents = []
    for l in lines:
        s = api.Sentence.from_tokenized(" ".join(tok.split("/")[0] for tok in l.split(" ")))   # --ignore-tags
        sents.append(s)
    t = api.Trainer(3, 3, 3, 3)
    t.add_examples(sents)
    model = t.train(0.01, 1.0, api.SolverType.L2RegularizedL2LossSVC)
    pred = api.Predictor(model, False, device=0)
    for s in sents:
        r = api.Sentence.from_raw(s.as_raw_text())
        pred.predict(r)
        assert list(r.iter_tokens()) == list(s.iter_tokens())


def test_synthetic_corpus_agreement_and_oracle():
    from oracle import cbind
    rng = np.random.default_rng(7)
    texts = ["".join(trainsuite.ALPHABET[k] for k in rng.integers(0, 20, int(rng.integers(4, 40)))) for _ in range(20000)]
    raw = open(os.path.join(HERE, "golden", "model.bin"), "rb").read()
    labeler = api.Predictor(api.Model.read_slice(raw)[0], False, device=0)
    utf8, boff = api.pack_texts([x.encode() for x in texts])
    _, labels, _ = labeler.predict_packed(utf8, boff)
    t = api.Trainer(3, 3, 3, 3)
    t.add_packed(utf8, boff, labels)
    mbytes = t.train_bytes(0.01, 1.0, 2)
    pred = api.Predictor(api.Model.read_slice(mbytes)[0], False, device=0)
    scores, plabels, ooff = pred.predict_packed(utf8, boff)
    o_scores, o_labels, _, _ = cbind.OraclePredictor(mbytes).predict_batch(utf8, boff)
    assert np.array_equal(scores, o_scores) and np.array_equal(plabels, o_labels)
    w, b, keys = t.weights()
    ref_model = trainref.build_model(keys, w, b, 3, 3, [], 0)
    assert ref_model == mbytes
    agree = float((plabels == labels).mean())
    assert agree >= 0.95, agree
