"""`python -m vaporetto_amd.train` in process, with the emulated library (tests/native/hipemu) swapped in: --tok, --part and --dict
together, the model file against api.Trainer's bytes, KyteaFullwidthFilter through the device decode, tags, and errors that name the
file and line."""
import os

import numpy as np
import pytest

from tests import emu
from vaporetto_amd import _lib, api, modelfmt, train

TOK = ["ＡＢＣ は テスト です", "これ は テスト です", "123 円 で 買った", "東京 に 行く"]
PART = ["こ-れ|は|テ-ス-ト", "か ら-だ"]
DICT = ["テスト", "東京 タワー", "これ"]


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    yield
    _lib._lib = saved


def write(tmp_path, name, lines):
    p = os.path.join(str(tmp_path), name)
    with open(p, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    return p


def run(tmp_path, *args):
    out = os.path.join(str(tmp_path), "model.bin")
    rc = train.main(list(args) + ["--model", out, "--charw", "2", "--charn", "2", "--typew", "2", "--typen", "2"])
    return rc, (open(out, "rb").read() if rc == 0 else None)


def test_tok_part_dict_equal_trainer_bytes(tmp_path):
    rc, model = run(tmp_path, "--tok", write(tmp_path, "a.tok", TOK), "--part", write(tmp_path, "b.part", PART),
                    "--dict", write(tmp_path, "c.dict", DICT), "--solver", "2")
    assert rc == 0
    md, used = modelfmt.decode_model(model)
    assert used == len(model) and md.char_window_size == 2 and not md.tag_models
    fw = api.KyteaFullwidthFilter()
    words = sorted({w for ln in DICT for w in ln.split(" ")})
    assert [r.word for r in md.dict_model] == words
    t = api.Trainer(2, 2, 2, 2, words, 4)
    sents = [api.Sentence.from_tokenized(ln) for ln in TOK] + [api.Sentence.from_partial_annotation(ln) for ln in PART]
    utf8, boff = api.pack_texts([s.as_raw_text().encode() for s in sents])
    t.add_packed(utf8, boff, np.concatenate([s.boundaries() for s in sents]), fullwidth=True)
    assert t.train_bytes(0.01, 1.0, 2) == model
    # without the normalisation the fullwidth Roman letters make other features: another model
    t2 = api.Trainer(2, 2, 2, 2, words, 4)
    t2.add_packed(utf8, boff, np.concatenate([s.boundaries() for s in sents]), fullwidth=False)
    assert t2.train_bytes(0.01, 1.0, 2) != model
    rc, raw_model = run(tmp_path, "--tok", write(tmp_path, "a.tok", TOK), "--part", write(tmp_path, "b.part", PART),
                        "--dict", write(tmp_path, "c.dict", DICT), "--solver", "2", "--no-norm")
    assert rc == 0 and raw_model == t2.train_bytes(0.01, 1.0, 2)


def test_errors_name_file_and_line(tmp_path, capsys):
    bad = write(tmp_path, "bad.tok", ["これ は", "これ  は"])
    assert run(tmp_path, "--tok", bad, "--solver", "2")[0] == 1
    assert "bad.tok:2: " in capsys.readouterr().err
    tagged = write(tmp_path, "tagged.tok", ["これ は", "これ/代名詞 は"])
    assert run(tmp_path, "--tok", tagged, "--solver", "2")[0] == 1
    assert "tagged.tok:2: carries tags" in capsys.readouterr().err
    rc, model = run(tmp_path, "--tok", tagged, "--solver", "2", "--ignore-tags")
    assert rc == 0 and not modelfmt.decode_model(model)[0].tag_models
    part = write(tmp_path, "bad.part", ["こ-れ", "こ*れ"])
    assert run(tmp_path, "--part", part, "--tok", tagged, "--ignore-tags", "--solver", "2")[0] == 1
    err = capsys.readouterr().err
    assert "bad.part:2: " in err and "invalid boundary character" in err
    d = write(tmp_path, "tagged.dict", ["テスト/名詞"])
    assert run(tmp_path, "--tok", write(tmp_path, "ok.tok", TOK), "--dict", d, "--solver", "2")[0] == 1
    assert "tagged.dict:1: carries tags" in capsys.readouterr().err
    assert run(tmp_path, "--tok", write(tmp_path, "ok.tok", TOK), "--solver", "5")[0] == 1
    assert "only 0 and 2 are implemented" in capsys.readouterr().err


def test_trainer_rejects_tags_unless_ignored():
    s = api.Sentence.from_tokenized("これ/代名詞 は")
    with pytest.raises(api.VaporettoError, match="carries tags"):
        api.Trainer(2, 2, 2, 2).add_examples([s])
    t = api.Trainer(2, 2, 2, 2, ignore_tags=True)
    t.add_examples([s, api.Sentence.from_tokenized("は これ")])
    assert t.n_features() > 0
