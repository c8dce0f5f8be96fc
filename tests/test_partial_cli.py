"""`python -m vaporetto_amd.train --part` in process, with the emulated library (tests/native/hipemu) swapped in: the corpus goes through the
batch parser (vpt_parse_partial_batch), not through a Sentence per line, and trains the model the same sentences train through add_examples."""
import os

import pytest

from tests import emu
from vaporetto_amd import _lib, api, train

PART = ["こ-れ|は|テ-ス-ト", "か ら-だ", "東-京|に|行-く", "a||-b", "こ-れ|は|東-京"]
TAGGED = ["こ-れ/代名詞|は/助詞|テ-ス-ト/名詞", "か ら-だ/名詞", "東-京/名詞/トーキョー|に/助詞|行-く/動詞", "こ-れ/代名詞|は/助詞|東-京/名詞//"]


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
    rc = train.main(list(args) + ["--model", out, "--charw", "2", "--charn", "2", "--typew", "2", "--typen", "2", "--solver", "2"])
    return rc, (open(out, "rb").read() if rc == 0 else None)


@pytest.fixture
def no_sentence_per_line(monkeypatch):
    """the sentences the comparison needs are parsed first; the CLI itself must not parse a line through the Sentence restatement"""
    real = api.Sentence.from_partial_annotation

    def parsed(lines):
        return [real(ln) for ln in lines]

    def refuse(text):
        raise AssertionError("the train CLI parsed a line through Sentence.from_partial_annotation")
    yield parsed, lambda: monkeypatch.setattr(api.Sentence, "from_partial_annotation", staticmethod(refuse))


def test_ignore_tags_equals_add_examples(tmp_path, no_sentence_per_line):
    parsed, forbid = no_sentence_per_line
    sents = parsed(PART + TAGGED)
    forbid()
    rc, model = run(tmp_path, "--part", write(tmp_path, "a.part", PART + TAGGED), "--ignore-tags")
    assert rc == 0
    t = api.Trainer(2, 2, 2, 2, [], 4, ignore_tags=True)
    t.add_examples(sents, fullwidth=True)
    assert t.train_bytes(0.01, 1.0, 2) == model


def test_train_tags_equals_add_examples(tmp_path, no_sentence_per_line):
    parsed, forbid = no_sentence_per_line
    sents = parsed(PART + TAGGED)
    forbid()
    rc, model = run(tmp_path, "--part", write(tmp_path, "a.part", PART + TAGGED), "--train-tags")
    assert rc == 0
    t = api.Trainer(2, 2, 2, 2, [], 4, train_tags=True)
    t.add_examples(sents, fullwidth=True)
    assert t.train_bytes(0.01, 1.0, 2) == model
    assert t.n_tag_models() > 0


def test_messages_name_file_and_line(tmp_path, capsys, no_sentence_per_line):
    no_sentence_per_line[1]()
    bad = write(tmp_path, "bad.part", ["こ-れ", "こ-れ|は", "こ\\漢れ"])
    assert run(tmp_path, "--part", bad)[0] == 1
    assert "bad.part:3: InvalidArgumentError: partial_annotation_text: contains an invalid boundary character: '漢'\n" in capsys.readouterr().err
    assert run(tmp_path, "--part", write(tmp_path, "end.part", ["こ-れ", "こ-れ|"]))[0] == 1
    assert "end.part:2: InvalidArgumentError: partial_annotation_text: invalid annotation\n" in capsys.readouterr().err
    tagged = write(tmp_path, "tagged.part", ["こ-れ", "こ-れ/|は", "こ/代-れ"])   # (an empty tag is no tag)
    assert run(tmp_path, "--part", tagged)[0] == 1
    assert "tagged.part:3: carries tags" in capsys.readouterr().err
