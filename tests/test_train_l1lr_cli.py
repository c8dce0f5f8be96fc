"""`python -m vaporetto_amd.train --l1r-lr --solver 6` in process, with the emulated library (tests/native/hipemu) swapped in: the model
file against api.Trainer(l1r_lr=True)'s bytes, read by the predictor's loader, and the refusal without --l1r-lr."""
import numpy as np
import pytest

from tests import emu
from tests.test_train_cli import DICT, PART, TOK, run, write
from vaporetto_amd import _lib, api, modelfmt


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    yield
    _lib._lib = saved


def test_l1r_lr_solver6_writes_a_model_predict_loads(tmp_path):
    rc, model = run(tmp_path, "--tok", write(tmp_path, "a.tok", TOK), "--part", write(tmp_path, "b.part", PART),
                    "--dict", write(tmp_path, "c.dict", DICT), "--l1r-lr", "--solver", "6")
    assert rc == 0
    md, used = modelfmt.decode_model(model)
    assert used == len(model) and md.char_window_size == 2 and not md.tag_models
    words = sorted({w for ln in DICT for w in ln.split(" ")})
    t = api.Trainer(2, 2, 2, 2, words, 4, l1r_lr=True)
    sents = [api.Sentence.from_tokenized(ln) for ln in TOK] + [api.Sentence.from_partial_annotation(ln) for ln in PART]
    utf8, boff = api.pack_texts([s.as_raw_text().encode() for s in sents])
    t.add_packed(utf8, boff, np.concatenate([s.boundaries() for s in sents]), fullwidth=True)
    assert t.train_bytes(0.01, 1.0, 6) == model
    assert t.train_bytes(0.01, 1.0, 2) != model
    # the predictor of the predict CLI loads it and splits a training sentence with it
    pred = api.Predictor(api.Model.read_slice(model)[0], False, device=0)
    s = api.Sentence.from_raw(sents[0].as_raw_text())
    pred.predict(s)
    assert "".join(s.iter_tokens()) == sents[0].as_raw_text()
    # --l1r-lr alone changes nothing for the TRON solvers
    rc, dense = run(tmp_path, "--tok", write(tmp_path, "a.tok", TOK), "--part", write(tmp_path, "b.part", PART),
                    "--dict", write(tmp_path, "c.dict", DICT), "--l1r-lr", "--solver", "2")
    assert rc == 0 and dense == t.train_bytes(0.01, 1.0, 2)


def test_solver6_refusals(tmp_path, capsys):
    tok = write(tmp_path, "ok.tok", TOK)
    assert run(tmp_path, "--tok", tok, "--solver", "6")[0] == 1
    assert "solver: only 0 and 2 are implemented" in capsys.readouterr().err
    assert run(tmp_path, "--tok", tok, "--l1r", "--solver", "6")[0] == 1
    assert "solver: only 0, 2 and 5 are implemented" in capsys.readouterr().err
    assert run(tmp_path, "--tok", tok, "--l1r-lr", "--solver", "6", "--train-tags")[0] == 1
    assert "solver 6: tag models are trained with solvers 0, 2 and 5 only" in capsys.readouterr().err
