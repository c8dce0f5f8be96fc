"""include/vaporetto_hip.hpp's Postings::boolean_search and VaporettoTokenizer::boolean_search through the --boolean flag of
examples/token_stream.cpp: the hit lines -- document, the score's bits in hex, the score -- must be those of the definition (tests/boolref.py)
over the Python mirror's postings, with the clause syntax (`+` MUST, `-` MUST_NOT, every token of a clause a slot), with and without
--segment-docs.  Compiled against the emulated build of the kernel sources on the CPU, against the product with -m gpu."""
import gc
import os
import subprocess

import numpy as np
import pytest

from tests import boolref, devmem, kat, postingssuite, searchref
from vaporetto_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, M, N = boolref.SHOULD, boolref.MUST, boolref.MUST_NOT
QUERIES = (("+猫 東京特許許可局", [("猫", M), ("東京特許許可局", S)]),
           ("まぁ  +だろう -東京特許許可局 +", [("まぁ", S), ("だろう", M), ("東京特許許可局", N)]),
           ("東京特許許可局 -猫 -", [("東京特許許可局", S), ("猫", N)]))


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
    keys = [x for j, x in enumerate(surfaces) if j % 3 != 1]
    vocab_file = str(tmp_path / "vocab.txt")
    open(vocab_file, "w", encoding="utf-8").write("".join(k + "\n" for k in keys))
    tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", vocab=keys)
    stdin = ("\n".join(texts) + "\n").encode("utf-8")
    toff, _ = tok.encode_batch(texts)
    dl = np.diff(toff.astype(np.int64)).astype(np.uint32)

    def example(*args):
        return subprocess.run([exe, model, "DR", "--postings", vocab_file] + list(args), input=stdin, stdout=subprocess.PIPE, check=True,
                              timeout=600).stdout.decode("utf-8")

    def lines(ref):
        return "".join("%d\t%08x\t%s\n" % (doc, searchref.bits(s), "%.9g" % float(s)) for doc, s in ref.hits[0])
    seen = 0
    for text, clauses in QUERIES:
        for base in ([], ["70000"]):
            doc_base = int(base[0]) if base else 0
            post = tok.index_batch(texts, doc_base)
            df = post.df()
            slots = []
            for clause, occur in clauses:
                _, ids = tok.encode_batch([clause])
                slots += [(int(t), occur, searchref.idf(len(texts), int(df[t])) if 0 <= t < len(keys) and occur != N else np.float32(0)) for t in ids]
            ref = boolref.BoolRef(post.term_offsets, post.docs, post.tfs, doc_base, dl, [slots], 3)
            assert example(*base, "--boolean", text, "--top", "3") == lines(ref), (text, base)
            seen += len(ref.hits[0])
    assert ref.vetoes["must_not"] >= 1 and seen >= 12
    # (the last query and doc_base) over merged segments, all matches; --top defaults to 10
    ref = boolref.BoolRef(post.term_offsets, post.docs, post.tfs, doc_base, dl, [slots], 100)
    want = lines(ref)
    assert example(*base, "--segment-docs", "7", "--boolean", text, "--top", "100") == want and ref.match_counts[0] > 10
    assert example(*base, "--boolean", text) == "".join(want.splitlines(True)[:10])


def test_cpp_boolean_search_on_the_emulated_sources(tmp_path):
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
def test_cpp_boolean_search_on_the_gpu(tmp_path):
    _check(_lib.LIB_PATH, tmp_path)
