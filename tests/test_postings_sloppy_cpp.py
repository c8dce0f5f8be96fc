"""include/vaporetto_hip.hpp's slop arguments -- Postings::phrase_search, Postings::clause_search, VaporettoTokenizer::phrase_search and
boolean_search -- through the --slop flag of examples/token_stream.cpp, beside --phrase and beside --boolean --phrases: the hit lines must be
those of the definition (tests/sloppyref.py) over the documents' encoded ids.  Compiled against the emulated build of the kernel sources on
the CPU, against the product with -m gpu."""
import gc
import os
import subprocess

import numpy as np
import pytest

from tests import clauseref, devmem, kat, postingssuite, sloppyref, sloppysuite
from vaporetto_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


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
    keys = sorted({api.KyteaFullwidthFilter().filter(t.text) for doc in plain.token_stream_batch(texts) for t in doc})
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

    def weight_of(terms):
        return sloppyref.phrase_weight(len(texts), df, [t for t in terms if 0 <= t < len(keys)])
    seen = gained = 0
    for query in ("火星だ", "猫東京", "火星猫は東京だ", "東京特許許可局", "東京🙂"):
        phrase = tok.encode_batch([query])[1].tolist()
        assert len(phrase) > 1
        for base, slop in (([], 0), ([], 2), (["70000"], 2), ([], 31)):
            doc_base = int(base[0]) if base else 0
            want, ref = sloppysuite.example_lines(docs, len(keys), doc_base, phrase, weight_of(phrase), slop, 3)
            assert example(*base, "--phrase", query, "--top", "3", "--slop", str(slop)) == "".join(l + "\n" for l in want), (query, base, slop)
            seen += len(want)
            gained += slop == 2 and ref.match_counts[0] > sloppyref.SloppyRef(docs, len(keys), doc_base, [phrase], [F(1)], [0], 3).match_counts[0]
    assert example("--phrase", "火星猫は東京だ", "--slop", "0") == example("--phrase", "火星猫は東京だ")   # slop 0: the exact call's lines
    assert seen >= 10 and gained >= 1
    # beside --boolean --phrases: the slop of every phrase clause
    for query in ("+火星だ 猫", "猫東京 -まぁ", "+東京特許許可局 火星だ"):
        clauses = []
        for clause in query.split(" "):
            occur = clauseref.MUST if clause[0] == "+" else clauseref.MUST_NOT if clause[0] == "-" else clauseref.SHOULD
            terms = tok.encode_batch([clause.lstrip("+-")])[1].tolist()
            clauses.append((terms, occur, F(0) if occur == clauseref.MUST_NOT else weight_of(terms)))
        for slop in (0, 2):
            ref = sloppysuite.of_clauses(docs, len(keys), 0, [clauses], slop, 4)
            want = ["%d\t%08x\t%.9g" % (d, sloppyref.bits(s), float(s)) for d, s in ref.hits[0]]
            assert example("--boolean", query, "--top", "4", "--slop", str(slop), "--phrases") == "".join(l + "\n" for l in want), (query, slop)
            seen += len(want)
    assert seen >= 14


def test_cpp_slop_on_the_emulated_sources(tmp_path):
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
def test_cpp_slop_on_the_gpu(tmp_path):
    _check(_lib.LIB_PATH, tmp_path)
