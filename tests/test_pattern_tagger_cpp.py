"""vaporetto_hip::PatternMatchTagger (include/vaporetto_hip.hpp) against the Python mirror on case 1 of tests/patterntagsuite.py: a C++ driver
(tests/native/pattern_tagger_cpp_test.cpp) is compiled and run on that case's model and sentences; every sentence's rule tags, its tokenized
text with and without the tagger and the one-call tokenizer's lines must be what api.PatternMatchTagger gives on the same library.
On the CPU the driver links the emulated build of the kernel sources (test infrastructure); `-m gpu` links the product."""
import os
import subprocess

import pytest

from tests import patterntagsuite
from vaporetto_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pattern_tagger_cpp_test.cpp")
RULES = [("漢字", ["RULE0", "RULE1", "RULE2"]), ("う", ["no", "no", "no"]), ("あい", ["never", "二", None]), ("AB", [None, "", "sl/ash"]),
         ("AB", ["last", None, ""])]
LINES = patterntagsuite.docs(1, 60) + patterntagsuite.docs_of_tokens(1, 20)[0]


def _build(lib_path: str, out: str) -> str:
    d, name = os.path.dirname(lib_path), os.path.basename(lib_path)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", out, SRC,
                           "-L" + d, "-l:" + name, "-Wl,-rpath," + d])
    return out


def _expected(model_bytes: bytes) -> str:
    pred = api.Predictor(api.Model.read_slice(model_bytes)[0], True)
    tagger = api.PatternMatchTagger(RULES)
    out = ["ids %d suffix %d" % (tagger.n_tags(pred), tagger.max_tag_suffix(pred))]
    any_rule = False
    for l in LINES:
        s = api.Sentence.from_raw(l)
        pred.predict(s)
        utf8, boff = api.pack_texts([l.encode("utf-8")])
        dense = pred.fill_tags_packed(utf8, boff, api.count_boundaries(utf8, boff), s.boundaries(), tagger=tagger)
        out.append("rule tags" + "".join(" " + tagger.tag(pred, -2 - int(v)) for v in dense.ravel() if v <= -2))
        any_rule = any_rule or bool((dense <= -2).any())
        s.fill_tags()
        plain = s.write_tokenized_text()
        tagger.filter(s)
        out.append("text " + s.write_tokenized_text())
        out.append("plain " + plain)
    assert any_rule
    out += ["tokenize " + t for t in pred.tokenize(LINES, tagged=True, tagger=tagger)]
    out += ["untagged " + t for t in pred.tokenize(LINES, tagged=True)]
    out.append("error 1 InvalidArgumentError: rules: a surface must contain at least one character (rule 1)")
    return "\n".join(out) + "\n"


def _run(exe: str, model_path: str) -> str:
    return subprocess.run([exe, model_path], input="\n".join(LINES).encode("utf-8"), stdout=subprocess.PIPE, check=True,
                          timeout=600).stdout.decode("utf-8")


def _model(tmp_path):
    raw = api.Model(patterntagsuite.tagged_model()).to_vec()
    path = str(tmp_path / "case1_model.bin")
    with open(path, "wb") as fh:
        fh.write(raw)
    return raw, path


def test_cpp_pattern_tagger_on_the_emulated_sources(tmp_path, monkeypatch):
    from tests import emu
    lib = emu.build_emulated()
    exe = _build(lib, str(tmp_path / "pattern_tagger_cpp_test"))
    monkeypatch.setattr(_lib, "_lib", emu.load())     # the Python mirror on the same (emulated) library
    raw, path = _model(tmp_path)
    assert _run(exe, path) == _expected(raw)


@pytest.mark.gpu
def test_cpp_pattern_tagger_on_the_gpu(tmp_path):
    exe = _build(_lib.LIB_PATH, str(tmp_path / "pattern_tagger_cpp_test"))
    raw, path = _model(tmp_path)
    assert _run(exe, path) == _expected(raw)
