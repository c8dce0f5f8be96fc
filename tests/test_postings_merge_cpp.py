"""include/vaporetto_hip.hpp's Postings::merge and VaporettoTokenizer::index over several batches through the --segment-docs flag of
examples/token_stream.cpp: the output with the flag (N documents a segment, the segments merged on the device) must be the output without it,
and the Python mirror's (VaporettoTokenizer.index_batch, which tests/postingssuite.py holds to the definition).  Compiled against the emulated
build of the kernel sources on the CPU, against the product with -m gpu."""
import gc
import os
import subprocess

import pytest

from tests import devmem, patterntagsuite
from vaporetto_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(lib_path, tmp_path):
    d, name = os.path.dirname(lib_path), os.path.basename(lib_path)
    exe = str(tmp_path / "token_stream")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "token_stream.cpp"), "-L" + d, "-l:" + name, "-Wl,-rpath," + d])
    raw = api.Model(patterntagsuite.tagged_model(31)).to_vec()
    model = str(tmp_path / "model.bin")
    open(model, "wb").write(raw)
    texts = patterntagsuite.docs(5, 41, lo=1, hi=40) + ["う", "", "AB０９", "漢字う"]
    plain = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR")
    surfaces = sorted({api.KyteaFullwidthFilter().filter(t.text) for doc in plain.token_stream_batch(texts) for t in doc})
    keys = surfaces[::2]
    vocab_file = str(tmp_path / "vocab.txt")
    open(vocab_file, "w", encoding="utf-8").write("".join(k + "\n" for k in keys))
    tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", vocab=keys)
    stdin = ("\n".join(texts) + "\n").encode("utf-8")

    def example(*args):
        return subprocess.run([exe, model, "DR", "--postings", vocab_file] + list(args), input=stdin, stdout=subprocess.PIPE, check=True,
                              timeout=600).stdout.decode("utf-8")
    for base in ([], ["70000"]):
        post = tok.index_batch(texts, int(base[0]) if base else 0)
        want = "".join("%d\t%d\t%d\n" % (k, int(post.docs[q]), int(post.tfs[q])) for k in range(len(keys))
                       for q in range(int(post.term_offsets[k]), int(post.term_offsets[k + 1]))) + "dropped\t%d\n" % post.n_dropped
        without = example(*base)
        assert without == want and len(post) >= 20 and post.n_dropped > 0
        for n in ("2", "7", str(len(texts) + 5)):
            assert example(*base, "--segment-docs", n) == without, n


def test_cpp_segment_docs_on_the_emulated_sources(tmp_path):
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
def test_cpp_segment_docs_on_the_gpu(tmp_path):
    _check(_lib.LIB_PATH, tmp_path)
