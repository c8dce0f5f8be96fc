"""include/vaporetto_hip.hpp's VaporettoTokenizer through examples/token_stream.cpp against the adapter's expected tokens
(tests/golden/token_stream_kat.json): compiled against the emulated build of the kernel sources on the CPU, against the product with -m gpu."""
import json
import os
import subprocess

import pytest

from vaporetto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "token_stream_kat.json"), encoding="utf-8"))
CASES = [c for c in KAT["cases"] if "\n" not in c["text"] and "\r" not in c["text"]]   # (the example reads a document per line)


def _check(lib_path, tmp_path):
    d, name = os.path.dirname(lib_path), os.path.basename(lib_path)
    exe = str(tmp_path / "token_stream")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "token_stream.cpp"), "-L" + d, "-l:" + name, "-Wl,-rpath," + d])
    model = os.path.join(ROOT, "tests", "golden", KAT["model"])
    for ws in sorted({c["wsconst"] for c in CASES}):
        cases = [c for c in CASES if c["wsconst"] == ws]
        out = subprocess.run([exe, model, ws], input=("\n".join(c["text"] for c in cases) + "\n").encode("utf-8"), stdout=subprocess.PIPE,
                             check=True, timeout=600).stdout.decode("utf-8")
        want = "".join("%d\t%d\t%d\t%d\t%s\n" % (d, t[3], t[1], t[2], t[0]) for d, c in enumerate(cases) for t in c["tokens"])
        assert out == want, ws
    bad = subprocess.run([exe, model, "X"], input=b"a\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert bad.returncode == 1 and b"Could not parse a wsconst value" in bad.stderr


def test_cpp_tokenizer_on_the_emulated_sources(tmp_path):
    from tests import emu
    _check(emu.build_emulated(), tmp_path)


@pytest.mark.gpu
def test_cpp_tokenizer_on_the_gpu(tmp_path):
    _check(_lib.LIB_PATH, tmp_path)
