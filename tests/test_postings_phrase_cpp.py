"""include/vaporetto_hip.hpp's VaporettoTokenizer::index with positions, Postings::phrase_search and VaporettoTokenizer::phrase_search through
the --phrase flag of examples/token_stream.cpp: the hit lines -- document, the score's bits in hex, the score, the frequency -- must be those
of the definition (tests/phraseref.py) over the documents' encoded ids.  Compiled against the emulated build of the kernel sources on the CPU,
against the product with -m gpu."""
import gc
import os
import subprocess

import pytest

from tests import devmem, kat, phraseref, phrasesuite, postingssuite
from vaporetto_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(lib_path, tmp_path):
    d, name = os.path.dirname(lib_path), os.path.basename(lib_path)
    exe = str(tmp_path / "token_stream")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "token_stream.cpp"), "-L" + d, "-l:" + name, "-Wl,-rpath," + d])
    raw, _ = kat.load_fixture("tantivy_model.bin")
    model = str(tmp_path / "model.bin")
    open(model, "wb").write(raw)
    texts = postingssuite.fixture_corpus()
    plain = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR")
    surfaces = sorted({api.KyteaFullwidthFilter().filter(t.text) for doc in plain.token_stream_batch(texts) for t in doc})
    keys = surfaces
    vocab_file = str(tmp_path / "vocab.txt")
    open(vocab_file, "w", encoding="utf-8").write("".join(k + "\n" for k in keys))
    tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", vocab=keys)
    stdin = ("\n".join(texts) + "\n").encode("utf-8")
    toff, ids = tok.encode_batch(texts)
    docs = [ids[int(toff[i]):int(toff[i + 1])].tolist() for i in range(len(texts))]
    df = [sum(1 for doc in docs if t in doc) for t in range(len(keys))]

    def example(*args):
        return subprocess.run([exe, model, "DR", "--postings", vocab_file] + list(args), input=stdin, stdout=subprocess.PIPE, check=True,
                              timeout=600).stdout.decode("utf-8")
    seen = 0
    for query in ("東京🙂", "火星猫は東京だ", "まぁ良いだろう", "猫は東京", "東京特許許可局"):   # (the first: a token that is no entry, no hit)
        qoff, qids = tok.encode_batch([query])
        phrase = qids.tolist()
        assert len(phrase) > 1 and (query != "東京🙂" or -1 in phrase)
        weight = phraseref.phrase_weight(len(texts), df, [t for t in phrase if 0 <= t < len(keys)])
        for base in ([], ["70000"]):
            doc_base = int(base[0]) if base else 0
            want, ref = phrasesuite.example_lines(docs, len(keys), doc_base, phrase, weight, 3)
            assert example(*base, "--phrase", query, "--top", "3") == "".join(l + "\n" for l in want), (query, base)
            seen += len(want)
    want, ref = phrasesuite.example_lines(docs, len(keys), doc_base, phrase, weight, 100)
    assert example(*base, "--phrase", query) == "".join(l + "\n" for l in want[:10])   # --top defaults to 10
    assert seen >= 10


def test_cpp_phrase_search_on_the_emulated_sources(tmp_path):
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
def test_cpp_phrase_search_on_the_gpu(tmp_path):
    _check(_lib.LIB_PATH, tmp_path)
