"""`python -m vaporetto_amd.train --train-tags --l1r-lr --l1r-lr-tags --solver 6` in process, with the emulated library
(tests/native/hipemu) swapped in: the model file against the equivalent api.Trainer's bytes, tag models present and read by
`predict --predict-tags`, and the refusals of --l1r-lr-tags without both others and of --solver 6 without it."""
import gc
import io
import os
import sys

import pytest

from tests import devmem, emu
from tests.test_train_tags_cli import DICT, PART, TOK, run, write
from vaporetto_amd import _lib, api, modelfmt
from vaporetto_amd import predict as predict_cli


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    devmem.EMULATED = True
    yield
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


class _Std:
    def __init__(self, data=b""):
        self.buffer = io.BytesIO(data)


def _trainer():
    fw = api.KyteaFullwidthFilter()
    dsents = [api.Sentence.from_tokenized(ln) for ln in DICT]
    words = sorted({fw.filter(w) for s in dsents for w in s.iter_tokens()})
    tag_dictionary = [(fw.filter(tk.surface()), tk.tags()) for s in dsents for tk in s.tokens()]
    t = api.Trainer(2, 2, 2, 2, words, 4, train_tags=True, tag_dictionary=tag_dictionary, l1r_lr=True, l1r_lr_tags=True)
    t.add_examples([api.Sentence.from_tokenized(ln) for ln in TOK], fullwidth=True)
    t.add_examples([api.Sentence.from_partial_annotation(ln) for ln in PART], fullwidth=True)
    return t


def test_l1r_lr_tags_solver6_equals_trainer_bytes_and_predict_reads_it(tmp_path, monkeypatch, capsys):
    files = ["--tok", write(tmp_path, "a.tok", TOK), "--part", write(tmp_path, "b.part", PART), "--dict", write(tmp_path, "c.dict", DICT)]
    rc, model = run(tmp_path, *files, "--train-tags", "--l1r-lr", "--l1r-lr-tags", "--solver", "6")
    assert rc == 0
    md, used = modelfmt.decode_model(model)
    assert used == len(model) and md.tag_models
    t = _trainer()
    assert t.train_bytes(0.01, 1.0, 6) == model
    assert t.train_bytes(0.01, 1.0, 2) != model
    # the flag changes nothing for the TRON solvers
    rc, dense = run(tmp_path, *files, "--train-tags", "--l1r-lr", "--l1r-lr-tags", "--solver", "2")
    assert rc == 0 and dense == t.train_bytes(0.01, 1.0, 2)
    # predict --predict-tags reads the model
    path = os.path.join(str(tmp_path), "m6.model")
    with open(path, "wb") as f:
        f.write(model)
    text = "".join(api.Sentence.from_tokenized(ln).as_raw_text() + "\n" for ln in TOK[:3])
    stdout = _Std()
    monkeypatch.setattr(sys, "stdin", _Std(text.encode("utf-8")))
    monkeypatch.setattr(sys, "stdout", stdout)
    assert predict_cli.main(["--model", path, "--predict-tags"]) == 0
    out = stdout.buffer.getvalue().decode("utf-8").splitlines()
    assert len(out) == 3 and all(ln.strip() for ln in out)


def test_l1r_lr_tags_needs_both_others(tmp_path, capsys):
    tok = write(tmp_path, "ok.tok", TOK)
    assert run(tmp_path, "--tok", tok, "--l1r-lr", "--l1r-lr-tags", "--solver", "6")[0] == 1
    assert "--l1r-lr-tags needs both --l1r-lr and --train-tags" in capsys.readouterr().err
    assert run(tmp_path, "--tok", tok, "--train-tags", "--l1r-lr-tags", "--solver", "6")[0] == 1
    assert "--l1r-lr-tags needs both --l1r-lr and --train-tags" in capsys.readouterr().err
    # without the new flag solver 6 on a tag trainer is refused with the old text
    assert run(tmp_path, "--tok", tok, "--train-tags", "--l1r-lr", "--solver", "6")[0] == 1
    assert "solver 6: tag models are trained with solvers 0, 2 and 5 only" in capsys.readouterr().err
