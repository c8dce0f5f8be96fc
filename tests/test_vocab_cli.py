"""`python -m vaporetto_amd.vocab` in process, with the emulated library (tests/native/hipemu) swapped in, on tests/golden/model.bin: the listing
is a collections.Counter over the tokens `python -m vaporetto_amd.predict` prints for the same lines, in the counter's finish order, under the
normalisation, wsconst and cut options; empty and NUL lines are no documents."""
import collections
import gc
import io
import os
import sys

import pytest

from tests import devmem, emu
from vaporetto_amd import _lib, api, predict, vocab

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = os.path.join(HERE, "golden", "model.bin")
DATA = ("まぁ社長は火星猫だ\nまぁ良いだろう\n\n火星猫はAB09だ\nまぁ\0だ\n社長はＡＢ０９だろう\r\nまぁ社長は火星猫だ").encode()


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


def run(main, argv, data, monkeypatch):
    stdin, stdout, stderr = _Std(data), _Std(), io.StringIO()
    monkeypatch.setattr(sys, "stdin", stdin)
    monkeypatch.setattr(sys, "stdout", stdout)
    monkeypatch.setattr(sys, "stderr", stderr)
    rc = main(["--model", MODEL] + argv)
    return rc, stdout.buffer.getvalue().decode(), stderr.getvalue()


def expected(argv, no_norm, min_count, max_size, monkeypatch):
    rc, text, _ = run(predict.main, argv + (["--no-norm"] if no_norm else []), DATA, monkeypatch)
    assert rc == 0
    norm = api.KyteaFullwidthFilter()
    counts = collections.Counter((t if no_norm else norm.filter(t)) for line in text.split("\n") for t in line.split(" ") if t and "\0" not in line)
    rows = sorted(((s, c) for s, c in counts.items() if c >= min_count), key=lambda x: (-x[1], x[0]))
    return "".join("%d\t%s\n" % (c, s) for s, c in (rows[:max_size] if max_size else rows))


@pytest.mark.parametrize("wsconst", [[], ["--wsconst", "D", "--wsconst", "R"]])
@pytest.mark.parametrize("no_norm", [False, True])
def test_listing_is_the_counter_of_the_predict_cli_tokens(wsconst, no_norm, monkeypatch):
    for min_count, max_size in ((1, 0), (2, 0), (1, 3)):
        argv = wsconst + (["--no-norm"] if no_norm else []) + ["--min-count", str(min_count), "--max-size", str(max_size)]
        rc, out, err = run(vocab.main, argv, DATA, monkeypatch)
        assert rc == 0, err
        assert out == expected(wsconst, no_norm, min_count, max_size, monkeypatch)
        assert wsconst or out.startswith("4\tは\n3\tまぁ\n3\t火星\n")   # count descending, then code points


def test_full_counter_and_empty_input(monkeypatch):
    rc, out, err = run(vocab.main, ["--max-keys", "2"], DATA, monkeypatch)
    assert rc == 1 and out == "" and "vocab counter: full" in err
    rc, out, err = run(vocab.main, [], b"", monkeypatch)
    assert rc == 0 and out == ""
    rc, out, err = run(vocab.main, [], b"\xff\xfe\n", monkeypatch)
    assert rc == 1 and "valid UTF-8" in err
