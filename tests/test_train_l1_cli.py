"""`python -m vaporetto_amd.train --l1r --solver 5` in process, with the emulated library (tests/native/hipemu) swapped in: the model
file against api.Trainer(l1r=True)'s bytes, and the refusal together with --train-tags."""
import os

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


def test_l1r_solver5_equals_trainer_bytes(tmp_path):
    rc, model = run(tmp_path, "--tok", write(tmp_path, "a.tok", TOK), "--part", write(tmp_path, "b.part", PART),
                    "--dict", write(tmp_path, "c.dict", DICT), "--l1r", "--solver", "5")
    assert rc == 0
    md, used = modelfmt.decode_model(model)
    assert used == len(model) and md.char_window_size == 2 and not md.tag_models
    words = sorted({w for ln in DICT for w in ln.split(" ")})
    t = api.Trainer(2, 2, 2, 2, words, 4, l1r=True)
    sents = [api.Sentence.from_tokenized(ln) for ln in TOK] + [api.Sentence.from_partial_annotation(ln) for ln in PART]
    utf8, boff = api.pack_texts([s.as_raw_text().encode() for s in sents])
    t.add_packed(utf8, boff, np.concatenate([s.boundaries() for s in sents]), fullwidth=True)
    assert t.train_bytes(0.01, 1.0, 5) == model
    assert t.train_bytes(0.01, 1.0, 2) != model
    # --l1r alone changes nothing for the TRON solvers
    rc, dense = run(tmp_path, "--tok", write(tmp_path, "a.tok", TOK), "--part", write(tmp_path, "b.part", PART),
                    "--dict", write(tmp_path, "c.dict", DICT), "--l1r", "--solver", "2")
    assert rc == 0 and dense == t.train_bytes(0.01, 1.0, 2)


def test_solver5_refusals(tmp_path, capsys):
    tok = write(tmp_path, "ok.tok", TOK)
    assert run(tmp_path, "--tok", tok, "--l1r", "--solver", "5", "--train-tags")[0] == 1
    assert "solver 5: tag models are trained with solvers 0 and 2 only" in capsys.readouterr().err
    assert run(tmp_path, "--tok", tok, "--solver", "5")[0] == 1
    assert "only 0 and 2 are implemented" in capsys.readouterr().err
    assert run(tmp_path, "--tok", tok, "--l1r", "--solver", "6")[0] == 1
    assert "only 0, 2 and 5 are implemented" in capsys.readouterr().err
