"""include/vaporetto_hip.hpp's Postings::clause_search and VaporettoTokenizer::boolean_search(..., phrases) through the --phrases flag of
examples/token_stream.cpp --postings --boolean: the hit lines -- document, the score's bits in hex, the score -- must be those of the Python
path (VaporettoTokenizer.boolean_search(phrases=True)) and of the definition (tests/clauseref.py) over the encoded ids, with and without
--segment-docs; without --phrases the lines stay those of every token as a slot.  Compiled against the emulated build of the kernel sources
on the CPU, against the product with -m gpu."""
import gc
import os
import subprocess

import numpy as np
import pytest

from tests import boolref, clauseref, devmem, kat, phraseref, postingssuite, searchref
from vaporetto_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, M, N = boolref.SHOULD, boolref.MUST, boolref.MUST_NOT
QUERIES = (("火星猫は 東京だ -まぁ良い", [("火星猫は", S), ("東京だ", S), ("まぁ良い", N)]),
           ("+東京特許許可局 猫", [("東京特許許可局", M), ("猫", S)]),
           ("まぁ  +だろう -東京特許許可局 +", [("まぁ", S), ("だろう", M), ("東京特許許可局", N)]))


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
    toff, ids = tok.encode_batch(texts)
    docs = [ids[int(toff[i]):int(toff[i + 1])].tolist() for i in range(len(texts))]

    def example(*args):
        return subprocess.run([exe, model, "DR", "--postings", vocab_file] + list(args), input=stdin, stdout=subprocess.PIPE, check=True,
                              timeout=600).stdout.decode("utf-8")

    def lines(hits):
        return "".join("%d\t%08x\t%s\n" % (doc, searchref.bits(s), "%.9g" % float(s)) for doc, s in hits)
    seen = phrase_clauses = 0
    for text, clauses in QUERIES:
        for base in ([], ["70000"]):
            doc_base = int(base[0]) if base else 0
            post = tok.index_batch(texts, doc_base, positions=True)
            df = post.df()
            query = []
            for clause, occur in clauses:
                terms = tok.encode_batch([clause])[1].tolist()
                phrase_clauses += len(terms) > 1
                weight = np.float32(0) if occur == N else phraseref.phrase_weight(len(texts), df, [t for t in terms if 0 <= t < len(keys)])
                query.append((terms, occur, weight))
            ref = clauseref.of_clauses(docs, len(keys), doc_base, [query], 3)
            hits, _ = tok.boolean_search(post, [text], 3, phrases=True)
            assert lines(hits[0]) == lines(ref.hits[0])
            assert example(*base, "--boolean", text, "--top", "3", "--phrases") == lines(ref.hits[0]), (text, base)
            seen += len(ref.hits[0])
    assert phrase_clauses >= 8 and seen >= 8
    # (the last query and doc_base) over merged positional segments, all matches; --top defaults to 10; without --phrases: every token a slot
    ref = clauseref.of_clauses(docs, len(keys), doc_base, [query], 100)
    want = lines(ref.hits[0])
    assert example(*base, "--segment-docs", "7", "--boolean", text, "--top", "100", "--phrases") == want and ref.match_counts[0] >= 3
    assert example(*base, "--boolean", text, "--phrases") == "".join(want.splitlines(True)[:10])
    old, _ = tok.boolean_search(tok.index_batch(texts, doc_base), [text], 100)
    assert example(*base, "--boolean", text, "--top", "100") == lines(old[0]) != want


def test_cpp_clause_search_on_the_emulated_sources(tmp_path):
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
def test_cpp_clause_search_on_the_gpu(tmp_path):
    _check(_lib.LIB_PATH, tmp_path)
