"""`python -m vaporetto_amd.train --l1r --train-tags --l1r-tags --solver 5` in process, with the emulated library (tests/native/hipemu)
swapped in: the model file against the equivalent api.Trainer's bytes, tag models present, and the refusal of --l1r-tags alone."""
import pytest

from tests import emu
from tests.test_train_tags_cli import DICT, PART, TOK, run, write
from vaporetto_amd import _lib, api, modelfmt


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    yield
    _lib._lib = saved


def _trainer():
    fw = api.KyteaFullwidthFilter()
    dsents = [api.Sentence.from_tokenized(ln) for ln in DICT]
    words = sorted({fw.filter(w) for s in dsents for w in s.iter_tokens()})
    tag_dictionary = [(fw.filter(tk.surface()), tk.tags()) for s in dsents for tk in s.tokens()]
    t = api.Trainer(2, 2, 2, 2, words, 4, train_tags=True, tag_dictionary=tag_dictionary, l1r=True, l1r_tags=True)
    t.add_examples([api.Sentence.from_tokenized(ln) for ln in TOK], fullwidth=True)
    t.add_examples([api.Sentence.from_partial_annotation(ln) for ln in PART], fullwidth=True)
    return t


def test_l1r_tags_solver5_equals_trainer_bytes(tmp_path):
    files = ["--tok", write(tmp_path, "a.tok", TOK), "--part", write(tmp_path, "b.part", PART), "--dict", write(tmp_path, "c.dict", DICT)]
    rc, model = run(tmp_path, *files, "--l1r", "--train-tags", "--l1r-tags", "--solver", "5")
    assert rc == 0
    md, used = modelfmt.decode_model(model)
    assert used == len(model) and md.tag_models
    assert any(m.char_ngram_model or m.type_ngram_model for m in md.tag_models)
    t = _trainer()
    assert t.train_bytes(0.01, 1.0, 5) == model
    assert t.train_bytes(0.01, 1.0, 2) != model
    # the third flag changes nothing for the TRON solvers
    rc, dense = run(tmp_path, *files, "--l1r", "--train-tags", "--l1r-tags", "--solver", "2")
    assert rc == 0 and dense == t.train_bytes(0.01, 1.0, 2)


def test_l1r_tags_needs_both_others(tmp_path, capsys):
    tok = write(tmp_path, "ok.tok", TOK)
    assert run(tmp_path, "--tok", tok, "--l1r", "--l1r-tags", "--solver", "5")[0] == 1
    assert "--l1r-tags needs both --l1r and --train-tags" in capsys.readouterr().err
    assert run(tmp_path, "--tok", tok, "--train-tags", "--l1r-tags", "--solver", "5")[0] == 1
    assert "--l1r-tags needs both --l1r and --train-tags" in capsys.readouterr().err
