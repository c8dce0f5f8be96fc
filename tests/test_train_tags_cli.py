"""`python -m vaporetto_amd.train --train-tags` in process, with the emulated library (tests/native/hipemu) swapped in: --tok, --part and
--dict together against api.Trainer(train_tags=True, tag_dictionary=...)'s bytes, a dictionary-only surface, --no-norm, and errors."""
import os

import pytest

from tests import emu
from vaporetto_amd import _lib, api, modelfmt, train

TOK = ["ABC/名詞 は/助詞 テスト/名詞 です/助動詞", "これ/代名詞 は/助詞/ワ テスト/名詞 です", "ABC/記号 で 買った/動詞", "東京 に 行く",
       "は/感動詞 と 言う", "テスト/動詞 は/助詞 する"]
PART = ["こ-れ/代名詞|は/助詞|テ-ス-ト", "か ら-だ/名詞"]
DICT = ["テスト/名詞", "東京/名詞/トーキョー タワー/名詞", "これ", "XY/記号"]


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


def _api_bytes(fullwidth):
    fw = api.KyteaFullwidthFilter()
    norm = fw.filter if fullwidth else (lambda s: s)
    dsents = [api.Sentence.from_tokenized(ln) for ln in DICT]
    words = sorted({norm(w) for s in dsents for w in s.iter_tokens()})
    tag_dictionary = [(norm(tk.surface()), tk.tags()) for s in dsents for tk in s.tokens()]
    t = api.Trainer(2, 2, 2, 2, words, 4, train_tags=True, tag_dictionary=tag_dictionary)
    t.add_examples([api.Sentence.from_tokenized(ln) for ln in TOK], fullwidth=fullwidth)
    t.add_examples([api.Sentence.from_partial_annotation(ln) for ln in PART], fullwidth=fullwidth)
    return t.train_bytes(0.01, 1.0, 2)


def test_tok_part_dict_equal_trainer_bytes(tmp_path, capsys):
    files = ["--tok", write(tmp_path, "a.tok", TOK), "--part", write(tmp_path, "b.part", PART), "--dict", write(tmp_path, "c.dict", DICT)]
    rc, model = run(tmp_path, *files, "--solver", "2", "--train-tags")
    assert rc == 0
    err = capsys.readouterr().err
    md, used = modelfmt.decode_model(model)
    assert used == len(model)
    assert "Tags: %d/%d\n" % (len(md.tag_models), len(md.tag_models)) in err and err.count("Tags: ") == 1
    assert model == _api_bytes(True)
    by = {m.token: m for m in md.tag_models}
    # normalised surfaces, tags as they are; a dictionary-only surface with its fixed tags
    assert by["ＡＢＣ"].tags == [["名詞", "記号"]] and (by["ＡＢＣ"].char_ngram_model or by["ＡＢＣ"].type_ngram_model)
    assert by["ＸＹ"].tags == [["記号"]] and not by["ＸＹ"].bias
    assert by["東京"].tags == [["名詞"], ["トーキョー"]] and by["タワー"].tags == [["名詞"], []]   # its line has two slots
    assert by["は"].tags == [["助詞", "感動詞"], ["ワ"]]
    assert [m.token for m in md.tag_models] == sorted(by, key=lambda s: s.encode())
    # --no-norm: other surfaces, another model
    rc, raw_model = run(tmp_path, *files, "--solver", "2", "--train-tags", "--no-norm")
    assert rc == 0 and raw_model != model and raw_model == _api_bytes(False)
    assert {"ABC", "XY"} <= {m.token for m in modelfmt.decode_model(raw_model)[0].tag_models}
    # without the flag the tags stay an error, and --ignore-tags a model without tag models
    assert run(tmp_path, *files, "--solver", "2")[0] == 1
    assert "a.tok:1: carries tags" in capsys.readouterr().err
    rc, plain = run(tmp_path, *files, "--solver", "2", "--ignore-tags")
    assert rc == 0 and not modelfmt.decode_model(plain)[0].tag_models


def test_errors_name_file_and_line(tmp_path, capsys):
    bad = write(tmp_path, "bad.tok", ["これ/代名詞 は", "これ  は"])
    assert run(tmp_path, "--tok", bad, "--solver", "2", "--train-tags")[0] == 1
    assert "bad.tok:2: " in capsys.readouterr().err
    part = write(tmp_path, "bad.part", ["こ-れ/代名詞", "こ*れ"])
    assert run(tmp_path, "--part", part, "--solver", "2", "--train-tags")[0] == 1
    assert "bad.part:2: " in capsys.readouterr().err
    assert run(tmp_path, "--tok", write(tmp_path, "ok.tok", TOK), "--solver", "5", "--train-tags")[0] == 1
    assert "only 0 and 2 are implemented" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run(tmp_path, "--tok", write(tmp_path, "ok.tok", TOK), "--solver", "2", "--train-tags", "--ignore-tags")
    assert e.value.code == 2
    assert "exclude each other" in capsys.readouterr().err
