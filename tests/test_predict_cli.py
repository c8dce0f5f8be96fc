"""`python -m vaporetto_amd.predict` in process, with the emulated library (tests/native/hipemu) swapped in, on tests/golden/model.bin: the
reference's documented outputs, and streams with empty lines, NUL lines, CRLF endings and no final newline under every flag combination
against tests/listingref.py applied line by line."""
import gc
import io
import itertools
import os
import sys

import pytest

from tests import devmem, emu, listingref
from vaporetto_amd import _lib, predict
from vaporetto_amd.evaluate import split_lines

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = os.path.join(HERE, "golden", "model.bin")
RAW = open(MODEL, "rb").read()


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


def run(argv, data, monkeypatch):
    stdin, stdout, stderr = _Std(data), _Std(), io.StringIO()
    monkeypatch.setattr(sys, "stdin", stdin)
    monkeypatch.setattr(sys, "stdout", stdout)
    monkeypatch.setattr(sys, "stderr", stderr)
    rc = predict.main(["--model", MODEL] + argv)
    return rc, stdout.buffer.getvalue(), stderr.getvalue()


def expected(data: bytes, predict_tags=False, scores=False, tag_scores=False, no_norm=False, wsconst=""):
    out = []
    for ln in split_lines(data):
        if not ln or "\0" in ln:
            out.append(b"\n")
        else:
            out += listingref.listing_lines(RAW, [ln], scores=scores, tag_scores=tag_scores, tagged=predict_tags, fullwidth=not no_norm,
                                            wsconst=wsconst, no_norm_order=no_norm)
    return b"".join(out)


def test_documented_outputs(monkeypatch):
    data = "まぁ社長は火星猫だ\nまぁ良いだろう\n".encode()
    rc, out, err = run([], data, monkeypatch)
    assert rc == 0 and out.decode() == "まぁ 社長 は 火星 猫 だ\nまぁ 良い だろう\n"
    assert err.startswith("Loading model file...\nStart tokenization\nElapsed: ") and err.endswith(" [sec]\n")
    rc, out, _ = run(["--predict-tags"], data, monkeypatch)
    assert rc == 0 and out.decode() == ("まぁ/名詞/マー 社長/名詞/シャチョー は/助詞/ワ 火星/名詞/カセー 猫/名詞/ネコ だ/助動詞/ダ\n"
                                        "まぁ/副詞/マー 良い/形容詞/ヨイ だろう/助動詞/ダロー\n")


STREAM = "まぁ社長は火星猫だ\r\n\nまぁ\0良い\nA1 b/c\\d\n\n火星猫\r\nまぁ良いだろう\r".encode()


@pytest.mark.parametrize("tags,scores,tag_scores,no_norm", [c for c in itertools.product([False, True], repeat=4) if c[0] or not c[2]])
def test_stream_with_rejected_lines(monkeypatch, tags, scores, tag_scores, no_norm):
    argv = (["--predict-tags"] if tags else []) + (["--scores"] if scores else []) + (["--tag-scores"] if tag_scores else []) + (["--no-norm"] if no_norm else [])
    rc, out, _ = run(argv, STREAM, monkeypatch)
    assert rc == 0
    assert out == expected(STREAM, tags, scores, tag_scores, no_norm)


@pytest.mark.parametrize("ws", ["D", "R", "H", "T", "K", "O", "G", "DRHTKOG"])
def test_wsconst(monkeypatch, ws):
    argv = ["--scores", "--predict-tags", "--tag-scores"] + [x for c in ws for x in ("--wsconst", c)]
    rc, out, _ = run(argv, STREAM, monkeypatch)
    assert rc == 0 and out == expected(STREAM, True, True, True, False, ws)


def test_tag_scores_needs_predict_tags(monkeypatch):
    with pytest.raises(SystemExit) as e:
        run(["--tag-scores"], b"a\n", monkeypatch)
    assert e.value.code == 2


def test_invalid_utf8(monkeypatch):
    rc, out, err = run([], b"abc\n\xff\xfe\n", monkeypatch)
    assert rc == 1 and "Error: stream did not contain valid UTF-8" in err
    assert out == b"abc\n"   # the lines in front of the failing one are printed, as the reference's reader gives them one by one
    rc, out, err = run(["--scores"], "火星猫\n\nまぁ".encode() + b"\xe3\x81", monkeypatch)
    assert rc == 1 and "Error: stream did not contain valid UTF-8" in err and out == expected("火星猫\n\n".encode(), scores=True)


def test_rejected_lines_at_both_ends(monkeypatch):
    """The "\\n" of rejected lines is spliced into the arena by offset: runs of them in front, in the middle, behind the last good line."""
    data = "\n\n\0\n火星猫\n\n\n\nまぁ良いだろう\n\n\0x\n\n".encode()
    for argv, kw in (([], {}), (["--scores", "--predict-tags", "--tag-scores"], dict(predict_tags=True, scores=True, tag_scores=True))):
        rc, out, _ = run(argv, data, monkeypatch)
        assert rc == 0 and out == expected(data, **kw)
    rc, out, _ = run(["--scores"], b"\n\n\n", monkeypatch)
    assert rc == 0 and out == b"\n\n\n"


def test_chunks_give_the_same_bytes(monkeypatch):
    data = STREAM + b"\n" + STREAM + b"\n" + "火星猫だ\n".encode() * 7
    rc, whole, _ = run(["--scores", "--predict-tags", "--tag-scores"], data, monkeypatch)
    monkeypatch.setattr(predict, "_CHUNK_LINES", 3)
    rc2, cut, _ = run(["--scores", "--predict-tags", "--tag-scores"], data, monkeypatch)
    assert rc == 0 and rc2 == 0 and whole == cut and whole == expected(data, True, True, True)
