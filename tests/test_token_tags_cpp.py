"""include/vaporetto_hip.hpp's tagged VaporettoTokenizer (predict_tags, TagStopFilter, Token::tags) through the --tags block of
examples/token_stream.cpp against the Python mirror, which tests/tokentagsuite.py holds to the restatement: compiled against the emulated build
of the kernel sources on the CPU, against the product with -m gpu."""
import gc
import os
import subprocess

import pytest

from tests import devmem, patterntagsuite
from vaporetto_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOP = [(0, "p"), (2, "カ"), (0, "nowhere")]


def _check(lib_path, tmp_path):
    d, name = os.path.dirname(lib_path), os.path.basename(lib_path)
    exe = str(tmp_path / "token_stream")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "token_stream.cpp"), "-L" + d, "-l:" + name, "-Wl,-rpath," + d])
    raw = api.Model(patterntagsuite.tagged_model(31)).to_vec()
    model = str(tmp_path / "model.bin")
    open(model, "wb").write(raw)
    texts = patterntagsuite.docs(5, 80, lo=1, hi=40) + ["う", "漢字う"]
    for stop in ([], STOP):
        tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", predict_tags=True, stop_tags=stop or None)
        want = "".join("%d\t%d\t%d\t%d\t%s\t%d%s\n" % (i, t.position, t.offset_from, t.offset_to, t.text, t.position_length,
                                                          "".join("\t" + ("*" if g is None else g) for g in t.tags))
                       for i, doc in enumerate(tok.token_stream_batch(texts)) for t in doc)
        out = subprocess.run([exe, model, "DR", "--tags"] + ["%d:%s" % p for p in stop], input=("\n".join(texts) + "\n").encode("utf-8"),
                             stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode("utf-8")
        assert out == want, stop
        assert ("\t*" in out) and any(len(l.split("\t")) == 9 for l in out.splitlines())
    bad = subprocess.run([exe, model, "", "--tags", "7:x"], input=b"a\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert bad.returncode == 1 and b"slot must be smaller" in bad.stderr


def test_cpp_tagged_tokenizer_on_the_emulated_sources(tmp_path):
    from tests import emu
    saved = _lib._lib
    _lib._lib = emu.load()
    devmem.EMULATED = True
    try:
        _check(emu.build_emulated(), tmp_path)
    finally:
        gc.collect()
        devmem.EMULATED = False
        _lib._lib = saved


@pytest.mark.gpu
def test_cpp_tagged_tokenizer_on_the_gpu(tmp_path):
    _check(_lib.LIB_PATH, tmp_path)
