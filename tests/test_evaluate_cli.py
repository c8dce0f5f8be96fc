"""The `evaluate` CLI (evaluate/src/main.rs:91-193) without a GPU: hand-derived counters for the reference's pinned predictor output,
checked against the restatement (tests/evalref.py) and against the library's whole pipeline (vpt_evaluate_batch: parse, predict,
fill_tags and the compare kernel) on the CPU emulator; Rust's float formatting; from_tokenized / write_tokenized_text round trips."""
import os

import numpy as np
import pytest

from tests import devmem, emu, evalref, kat
from tests.evalsuite import merge_tokens, oracle_system
from vaporetto_amd import _lib, api, build
from vaporetto_amd import evaluate as cli
from vaporetto_amd.modelfmt import encode_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# predictor.rs:861-903: create_test_model() on この人は地球人だ predicts この|人|は|地球|人|だ, and with fill_tags
# 人 (char 2) = [名詞, ヒト], 地球 (char 5) = [名詞, チキュー], 人 (char 6) = [接尾辞, ジン], every other char [None, None].
KAT_TEXT = "この人は地球人だ"
SYS_LABELS = [0, 1, 1, 1, 0, 1, 1]
SYS_TAGS = [kat.PREDICT_TAGS_EXPECTED[2 * c:2 * c + 2] for c in range(8)]

# gold line -> ((tp, tn, fp, fn), n_sys, n_ref, n_cor for the system tag vectors {predicted, none (normalised), gold (--no-norm)}).
# By hand, boundaries after chars 0..6, W = WordBoundary, N = not:
KAT_GOLD = [
    # exact, with the predicted tags: gold = system = N W W W N W W: TP 5 (the W), TN 2.  Word: 6 tokens each side, every agreed W
    # starts matched; predicted tags equal at chars 1, 2, 3, 5, 6 and the last char 7 -> 6; empty system vectors never equal the
    # gold's two slots -> 0; the gold's own tags -> 6
    ("この 人/名詞/ヒト は 地球/名詞/チキュー 人/接尾辞/ジン だ", (5, 2, 0, 0), 6, 6, {"pred": 6, "none": 0, "gold": 6}),
    # exact, no tags (n_tags 0): the predicted vectors have 2 slots -> 0; empty = empty -> 6; gold -> 6
    ("この 人 は 地球 人 だ", (5, 2, 0, 0), 6, 6, {"pred": 0, "none": 6, "gold": 6}),
    # merged: gold N W N W N N W against N W W W N W W: b2 and b5 are FP -> TP 3 TN 2 FP 2.  n_sys 5 + 1, n_ref 3 + 1; matched: b1
    # correct (この), b2 breaks it, b3 is agreed but not matched (resets), b5 breaks, b6 not matched (resets), the end is matched (だ) -> 2
    ("この 人は 地球人 だ", (3, 2, 2, 0), 6, 4, {"pred": 0, "none": 2, "gold": 2}),
    # split: gold N W W W W W W: b4 is FN -> TP 5 TN 1 FN 1; n_sys 6, n_ref 7; b1 b2 b3 correct, b4 breaks, b5 not matched, b6 and the
    # end correct -> 5
    ("この 人 は 地 球 人 だ", (5, 1, 0, 1), 6, 7, {"pred": 0, "none": 5, "gold": 5}),
    # a wrong tag on 地球 (マンホーム, the candidate the model did not choose): the predicted vectors differ at char 5 only -> 5
    ("この 人/名詞/ヒト は 地球/名詞/マンホーム 人/接尾辞/ジン だ", (5, 2, 0, 0), 6, 6, {"pred": 5, "none": 0, "gold": 6}),
    # one slot against the model's two: vectors of different lengths are never equal -> 0; empty against one slot -> 0
    ("この 人/名詞 は 地球/名詞 人/接尾辞 だ", (5, 2, 0, 0), 6, 6, {"pred": 0, "none": 0, "gold": 6}),
]
MODES = {"pred": dict(predict_tags=True, no_norm=False), "none": dict(predict_tags=False, no_norm=False),
         "gold": dict(predict_tags=False, no_norm=True)}


def _expected(gold, mode):
    _, (tp, tn, fp, fn), n_sys, n_ref, cor = gold
    return dict(tp=tp, tn=tn, fp=fp, fn=fn, n_sys=n_sys, n_ref=n_ref, n_cor=cor[mode], n_sentences=1)


def _pinned_system(predict_tags):
    def system(raws, normalised):
        assert raws == [KAT_TEXT] * len(raws)
        return [SYS_LABELS] * len(raws), ([SYS_TAGS] * len(raws) if predict_tags else None)
    return system


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("gold", KAT_GOLD, ids=lambda g: g[0])
def test_hand_counts_against_restatement(gold, mode):
    o = MODES[mode]
    got = evalref.evaluate([gold[0]], _pinned_system(o["predict_tags"]), **o)
    assert got == _expected(gold, mode)


def test_rust_float_formatting():
    assert [cli.rust_f64(x) for x in (1.0, 0.5, 0.1, 1e-5, float("nan"), 0.0, 2 / 3, 1e21, 123.0)] == \
        ["1", "0.5", "0.1", "0.00001", "NaN", "0", "0.6666666666666666", "1000000000000000000000", "123"]


def test_report_lines():
    r = api.evaluation_result([3, 2, 2, 0, 6, 4, 2, 1])
    assert cli.report(r, "char") == "Precision: 0.6\nRecall: 1\nF1: 0.7499999999999999\nTP: 3, TN: 2, FP: 2, FN: 0\n"
    assert cli.report(r, "word") == "Precision: 0.3333333333333333\nRecall: 0.5\nF1: 0.4\n"
    assert cli.report(api.evaluation_result([0] * 8), "char").startswith("Precision: NaN\nRecall: NaN\nF1: NaN\n")


def test_lines_split_like_rust():
    assert cli.split_lines(b"a b\r\n\nc\n") == ["a b", "", "c"]
    assert cli.split_lines(b"a\rb") == ["a\rb"]
    assert cli.split_lines(b"x\na\r") == ["x", "a\r"]             # '\r' is stripped only in front of '\n'
    with pytest.raises(UnicodeDecodeError):
        cli.split_lines(b"\xff\n")
    assert cli.split_lines(b"") == []


def test_tokenized_round_trip_docs_tok():
    build.build_hip()
    for line in open(os.path.join(ROOT, "tests", "golden", "docs.tok"), encoding="utf-8").read().splitlines():
        if line:
            assert api.Sentence.from_tokenized(line).write_tokenized_text() == line


# ---- the whole pipeline on the CPU emulator

@pytest.fixture(scope="module")
def emulated():
    lib = emu.load()
    saved = _lib._lib
    _lib._lib = lib
    devmem.EMULATED = True
    yield lib
    import gc
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


def test_evaluate_batch_hand_counts_on_emulator(emulated):
    pred = api.Predictor(api.Model.read_slice(encode_model(kat.predictor_test_model()))[0], True)
    for gold in KAT_GOLD:
        for mode, o in MODES.items():
            r = pred.evaluate([gold[0], ""], **o)          # the empty line is skipped (evaluate/src/main.rs:94)
            assert {k: r[k] for k in _expected(gold, mode)} == _expected(gold, mode), (gold[0], mode)
    # several sentences at once add up
    r = pred.evaluate([g[0] for g in KAT_GOLD], predict_tags=True)
    assert r["n_cor"] == sum(g[4]["pred"] for g in KAT_GOLD) and r["n_sentences"] == len(KAT_GOLD)
    with pytest.raises(api.VaporettoError) as e:
        pred.evaluate(["この 人", "この  人"])
    assert str(e.value) == "InvalidArgumentError: tokenized_text: must not contain consecutive whitespaces (line 1)"


def test_evaluate_after_short_host_predicts_on_emulator(emulated):
    """a pooled workspace that a host predict call left with a short longest-sentence hint scores long gold lines all the same; the counters are
    the restatement's over the oracle's system side (a tenth of the gold tokens are merged ones)"""
    raw = open(os.path.join(ROOT, "tests", "golden", "model.bin"), "rb").read()
    pred = api.Predictor(api.Model.read_slice(raw)[0], True)
    line = merge_tokens(" ".join(["火星", "猫", "は", "まぁ", "社長"] * 200), 200)   # 1 600 chars
    first = pred.evaluate([line])
    want = evalref.evaluate([line], oracle_system(raw, pred._model.tag_models(), [], False, False))
    assert {k: first[k] for k in want} == want and min(want["fp"], want["tp"]) > 0 and 0 < want["n_cor"] < want["n_ref"]
    utf8, boff = api.pack_texts([b"ab", b"cd"])
    pred.predict_packed(utf8, boff)
    again = pred.evaluate([line], predict_tags=True)
    assert again["tp"] + again["fn"] == first["tp"] + first["fn"] and again["n_sentences"] == 1
    assert {k: again[k] for k in ("tp", "tn", "fp", "fn")} == {k: first[k] for k in ("tp", "tn", "fp", "fn")}


def test_error_names_the_input_line_with_empty_lines_on_emulator(emulated):
    pred = api.Predictor(api.Model.read_slice(encode_model(kat.predictor_test_model()))[0], True)
    with pytest.raises(api.VaporettoError) as e:
        pred.evaluate(["この 人", "", "", "この 人", "", "この  人"])
    assert str(e.value) == "InvalidArgumentError: tokenized_text: must not contain consecutive whitespaces (line 5)"
