"""Tokenized text and the `evaluate` CLI on the MI355X: the parse kernel bit for bit against the host parser, vpt_evaluate_batch /
Predictor.evaluate against the restatement (tests/evalref.py) fed with the library's own predict / fill_tags output (themselves pinned to the
CPU oracle by tests/test_gpu_parity.py), the chunked path, and the CLI's stdout end to end."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import devmem, evalref, kat
from tests.evalsuite import merge_tokens, oracle_system as _oracle_system
from tests.test_evaluate_cli import KAT_GOLD, MODES, _expected
from tests.test_tokenized_parse import _expect, check_parsed, random_line
from vaporetto_amd import _lib, api, build
from vaporetto_amd.modelfmt import encode_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_hip()


def _predictor(model, tags=True):
    return api.Predictor(api.Model.read_slice(model)[0], tags)


def test_parse_kernel_matches_host_parser():
    """100 K random lines of 1 - 4 000 chars (lengths log-uniform), bit for bit against the host parser, a sample against the restatement"""
    rng = random.Random(5)
    pool = [random_line(rng, 1) for _ in range(5000)]
    lines = []
    for _ in range(100000):
        n = max(1, int(math.exp(rng.uniform(0.0, math.log(4000.0)))) // 3)   # tokens average about 3 chars
        lines.append(" ".join(rng.choices(pool, k=n)))
    rng.shuffle(lines)
    enc = [ln.encode("utf-8") for ln in lines]
    utf8, boff = api.pack_texts(enc)
    p = _predictor(encode_model(kat.predictor_test_model()))
    d = p.parse_tokenized_packed(utf8, boff)
    h = api.parse_tokenized_host(enc)
    for k in h:
        assert np.array_equal(np.asarray(d[k]), np.asarray(h[k])), k
    check_parsed(d, lines[:2000], _expect(lines[:2000]))
    assert max(len(ln) for ln in lines) > 3000


def test_parse_kernel_reports_the_first_failing_line():
    p = _predictor(encode_model(kat.predictor_test_model()))
    utf8, boff = api.pack_texts([b"a b"] * 50 + [b"a /b"] + [b"a b"] * 10 + [b" x"])
    with pytest.raises(api.VaporettoError) as e:
        p.parse_tokenized_packed(utf8, boff)
    assert str(e.value) == "InvalidArgumentError: tokenized_text: a slash must follow a character (line 50)"


@pytest.mark.parametrize("mode", sorted(MODES))
def test_kat_hand_counts(mode):
    p = _predictor(encode_model(kat.predictor_test_model()))
    for gold in KAT_GOLD:
        r = p.evaluate([gold[0]], **MODES[mode])
        assert {k: r[k] for k in _expected(gold, mode)} == _expected(gold, mode), gold[0]


def _corpus(pred, texts):
    """gold lines: the model's own tokenization (tagged) with a seeded share of boundaries flipped"""
    rng = random.Random(3)
    toks = pred.tokenize(texts, tagged=pred.n_tags() > 0)
    out = []
    for t in toks:
        if rng.random() < 0.3 and " " in t:
            k = t.index(" ")
            t = t[:k] + t[k + 1:] if "/" not in t[:k] else t
        out.append(t)
    return out


@pytest.mark.parametrize("wsconst", [(), (5,), (5, 3), ("G",)], ids=["none", "K", "KH", "G"])
@pytest.mark.parametrize("predict_tags,no_norm", [(False, False), (False, True), (True, False), (True, True)])
def test_evaluate_matches_restatement(wsconst, predict_tags, no_norm):
    models = [("model.bin", open(os.path.join(ROOT, "tests", "golden", "model.bin"), "rb").read()),
              ("kat", encode_model(kat.predictor_test_model()))]
    texts = ["まぁ社長は火星猫だ", "まぁ良いだろう", "この人は地球人だ", "火星猫", "Ｒｕｓｔで良いプログラミング体験を！", "ab 12 cd"] * 7
    for name, raw in models:
        pred = _predictor(raw)
        lines = _corpus(pred, texts) + open(os.path.join(ROOT, "tests", "golden", "docs.tok"), encoding="utf-8").read().splitlines()
        types = [t for t in wsconst if t != "G"]
        got = pred.evaluate(lines, predict_tags=predict_tags, wsconst=wsconst, no_norm=no_norm)
        want = evalref.evaluate(lines, _oracle_system(raw, pred._model.tag_models(), types, "G" in wsconst, predict_tags),
                                predict_tags=predict_tags, no_norm=no_norm)
        assert {k: got[k] for k in want} == want, name


def test_evaluate_over_several_front_end_runs():
    """fill_tags numbers its records run by run of at most 256 sentences and the compare finds a sentence's records through its run: 720 lines
    are three runs at least, so sentences of run 1 and 2 are compared -- the one call, and the compare alone on a workspace of the test's own
    (which says how fill_tags cut the batch), both against the restatement over the oracle's system side."""
    keys = ("tp", "tn", "fp", "fn", "n_sys", "n_ref", "n_cor", "n_sentences")
    texts = ["まぁ社長は火星猫だ", "まぁ良いだろう", "この人は地球人だ", "火星猫", "Ｒｕｓｔで良いプログラミング体験を！", "ab 12 cd"] * 120
    for name, raw in (("model.bin", open(os.path.join(ROOT, "tests", "golden", "model.bin"), "rb").read()), ("kat", encode_model(kat.predictor_test_model()))):
        pred = _predictor(raw)
        lines = _corpus(pred, texts)
        want = evalref.evaluate(lines, _oracle_system(raw, pred._model.tag_models(), [], False, True), predict_tags=True)
        assert want["n_cor"] > 0 and want["n_cor"] < want["n_ref"]
        got = pred.evaluate(lines, predict_tags=True)
        assert {k: got[k] for k in want} == want, name
        # call by call: parse, predict, fill_tags (the records stay on the workspace), the compare
        h = api.parse_tokenized_host([ln.encode("utf-8") for ln in lines])
        _, sys_l, ooff = pred.predict_packed(h["raw"], h["raw_offsets"], fullwidth=True)
        assert np.array_equal(ooff, h["out_offsets"])
        S, nb = len(lines), int(ooff[-1])
        pad = lambda a: np.concatenate([a, np.zeros(32, a.dtype)])
        d = {k: devmem.put(pad(v)) for k, v in h.items()}
        d_sys, d_counts = devmem.put(pad(sys_l)), devmem.zeros(8, np.uint64)
        batch = api.DeviceBatch(pred)
        batch.set_flags(_lib.VPT_FLAG_KYTEA_FULLWIDTH)
        batch.fill_tags(d["raw"].ptr, d["raw_offsets"].ptr, d["out_offsets"].ptr, S, nb, d_sys.ptr, 0, devmem.stream())
        st = _lib.load().vpt_evaluate_labels_batch_device(pred.handle, batch._h, d["out_offsets"].ptr, S, d["labels"].ptr, d["n_tags"].ptr, d["tag_index"].ptr,
                                                          d["span_offsets"].ptr, d["tag_bytes"].ptr, d_sys.ptr, _lib.VPT_EVAL_TAGS_PREDICTED, d_counts.ptr,
                                                          devmem.stream())
        assert st == _lib.VPT_OK, _lib.last_error()
        batch.sync()
        assert batch.last_plan()["tag_runs"] >= 3, name
        assert dict(zip(keys, (int(c) for c in d_counts.get()))) == {k: want[k] for k in keys}, name


def test_chunked_path_gives_the_same_counts():
    raw = open(os.path.join(ROOT, "tests", "golden", "model.bin"), "rb").read()
    pred = _predictor(raw)
    lines = _corpus(pred, ["まぁ社長は火星猫だ", "まぁ良いだろう", "火星猫"] * 200)
    want = pred.evaluate(lines, predict_tags=True)
    os.environ["VPT_EVAL_CHUNK_BYTES"] = "700"
    try:
        small = _predictor(raw)
    finally:
        del os.environ["VPT_EVAL_CHUNK_BYTES"]
    got = small.evaluate(lines, predict_tags=True)
    assert {k: got[k] for k in ("tp", "tn", "fp", "fn", "n_sys", "n_ref", "n_cor", "n_sentences")} == \
        {k: want[k] for k in ("tp", "tn", "fp", "fn", "n_sys", "n_ref", "n_cor", "n_sentences")}
    bad = lines[:300] + ["a  b"] + lines[300:]
    with pytest.raises(api.VaporettoError) as e:
        small.evaluate(bad)
    assert str(e.value).endswith("must not contain consecutive whitespaces (line 300)")


def test_evaluate_after_short_host_predicts():
    """a pooled workspace that a host predict call left with a short longest-sentence hint scores long gold lines all the same; the counters are
    the restatement's over the oracle's system side (a tenth of the gold tokens are merged ones)"""
    raw = open(os.path.join(ROOT, "tests", "golden", "model.bin"), "rb").read()
    pred = _predictor(raw)
    lines = [merge_tokens(" ".join(["火星", "猫", "は", "まぁ", "社長"] * n), n) for n in (300, 2000)]   # 2 400 and 16 000 chars
    first = pred.evaluate(lines, predict_tags=True)
    want = evalref.evaluate(lines, _oracle_system(raw, pred._model.tag_models(), [], False, True), predict_tags=True)
    assert {k: first[k] for k in want} == want and min(want["fp"], want["tp"]) > 0
    # (untagged gold lines are never correct against predicted tags) without them the word metric counts: tokens 16 000 chars into a sentence
    plain, want = pred.evaluate(lines), evalref.evaluate(lines, _oracle_system(raw, pred._model.tag_models(), [], False, False))
    assert {k: plain[k] for k in want} == want and 0 < want["n_cor"] < want["n_ref"]
    pred.predict_packed(*api.pack_texts([b"ab", b"cd"]))
    again = pred.evaluate(lines, predict_tags=True)
    assert again == first or all(again[k] == first[k] for k in ("tp", "tn", "fp", "fn", "n_sys", "n_ref", "n_cor", "n_sentences"))


def test_cli_stdout(tmp_path):
    model = tmp_path / "kat.model"
    model.write_bytes(encode_model(kat.predictor_test_model()))
    stdin = ("\n".join(g[0] for g in KAT_GOLD) + "\n\n").encode("utf-8")
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, "-m", "vaporetto_amd.evaluate", "--model", str(model), "--predict-tags", "--metric", "word"],
                         input=stdin, capture_output=True, timeout=300, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    cor = sum(g[4]["pred"] for g in KAT_GOLD)
    n_sys, n_ref = sum(g[2] for g in KAT_GOLD), sum(g[3] for g in KAT_GOLD)
    p, r = cor / n_sys, cor / n_ref
    from vaporetto_amd.evaluate import rust_f64
    assert run.stdout.decode() == "Precision: %s\nRecall: %s\nF1: %s\n" % (rust_f64(p), rust_f64(r), rust_f64(2.0 * p * r / (p + r)))
    ours = [ln for ln in run.stderr.decode().splitlines() if not ln.startswith("/opt/")]   # (the driver's libdrm may add a line of its own)
    assert ours == ["Loading model file...", "Start tokenization"]
    run = subprocess.run([sys.executable, "-m", "vaporetto_amd.evaluate", "--model", str(model)], input=stdin, capture_output=True,
                         timeout=300, env=env, cwd=ROOT)
    tp, tn, fp, fn = (sum(g[1][k] for g in KAT_GOLD) for k in range(4))
    assert run.stdout.decode().endswith("TP: %d, TN: %d, FP: %d, FN: %d\n" % (tp, tn, fp, fn))
