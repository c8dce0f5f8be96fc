"""include/vaporetto_hip.hpp's Postings::merge with positions and VaporettoTokenizer::index over several batches with positions, through
--segment-docs N --phrase of examples/token_stream.cpp: the hit lines -- document, the score's bits in hex, the score, the frequency -- must
be those of the definition (tests/phraseref.py) over the documents' encoded ids, the same as without --segment-docs, and stderr must tell that
segments were really merged and how many postings and positions the merged segment holds (tests/positionsmergeref.py).  Compiled against the
emulated build of the kernel sources on the CPU, against the product with -m gpu."""
import gc
import os
import subprocess

import pytest

from tests import devmem, kat, phraseref, phrasesuite, positionsmergeref, postingssuite
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
    keys = sorted({api.KyteaFullwidthFilter().filter(t.text) for doc in plain.token_stream_batch(texts) for t in doc})
    vocab_file = str(tmp_path / "vocab.txt")
    open(vocab_file, "w", encoding="utf-8").write("".join(k + "\n" for k in keys))
    tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", vocab=keys)
    stdin = ("\n".join(texts) + "\n").encode("utf-8")
    toff, ids = tok.encode_batch(texts)
    docs = [ids[int(toff[i]):int(toff[i + 1])].tolist() for i in range(len(texts))]
    df = [sum(1 for doc in docs if t in doc) for t in range(len(keys))]
    whole = positionsmergeref.PositionsMergeRef.of_documents(docs, len(keys))
    n_postings, n_positions = whole.n_out, len(whole.arrays()[4])

    def example(*args):
        r = subprocess.run([exe, model, "DR", "--postings", vocab_file] + list(args), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True,
                           timeout=600)
        return r.stdout.decode("utf-8"), r.stderr.decode("utf-8")
    seen = 0
    for query in ("火星猫は東京だ", "猫は東京"):
        qoff, qids = tok.encode_batch([query])
        phrase = qids.tolist()
        weight = phraseref.phrase_weight(len(texts), df, [t for t in phrase if 0 <= t < len(keys)])
        for base, n in (([], 2), (["70000"], 7)):
            doc_base = int(base[0]) if base else 0
            want, ref = phrasesuite.example_lines(docs, len(keys), doc_base, phrase, weight, 3)
            one, err1 = example(*base, "--phrase", query, "--top", "3")
            assert "segments" not in err1
            flags = ["--segment-docs", str(n), "--phrase", query] if base else ["--phrase", query, "--segment-docs", str(n)]   # (either order)
            out, err = example(*base, *flags, "--top", "3")
            assert out == one == "".join(l + "\n" for l in want), (query, base, n)
            assert err.split() == ["segments", str((len(texts) + n - 1) // n), "postings", str(n_postings), "positions", str(n_positions)], err
            seen += len(want)
    assert seen >= 4 and len(texts) > 14


def test_cpp_phrase_search_over_merged_segments_on_the_emulated_sources(tmp_path):
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
def test_cpp_phrase_search_over_merged_segments_on_the_gpu(tmp_path):
    _check(_lib.LIB_PATH, tmp_path)
