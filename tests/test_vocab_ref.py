"""The restatement of the vocabulary ids (tests/vocabref.py) held to a plain dict lookup on the surfaces of tests/golden/docs.tok, its hash to
hand-computed words, and the searches the suite relies on (same home slot, fingerprint twins) shown to succeed for the hash that ships.  CPU only."""
import os

import numpy as np

from tests import vocabref

HERE = os.path.dirname(os.path.abspath(__file__))


def golden_tokens():
    lines = open(os.path.join(HERE, "golden", "docs.tok"), encoding="utf-8").read().splitlines()
    return [[t.split("/")[0] for t in line.split(" ")] for line in lines if line]


def test_ids_are_a_dict_lookup_on_the_golden_surfaces():
    docs = golden_tokens()
    assert docs[0] == ["まぁ", "社長", "は", "火星", "猫", "だ"]
    distinct = []
    for d in docs:
        for t in d:
            if t not in distinct:
                distinct.append(t)
    keys = distinct[::2]   # every other surface is a key
    vocab = {s: k for k, s in enumerate(keys)}
    raws = ["".join(d).encode("utf-8") for d in docs]
    toff, ends = [0], []
    for d in docs:
        at = 0
        for t in d:
            at += len(t.encode("utf-8"))
            ends.append(at)
        toff.append(len(ends))
    starts = [0 if k in toff[:-1] else ends[k - 1] for k in range(len(ends))]
    flat = [t for d in docs for t in d]
    want = [vocab.get(t, -7) for t in flat]
    assert list(vocabref.ids_from_csr(raws, toff, None, ends, vocab, -7, False)) == want
    assert list(vocabref.ids_from_csr(raws, toff, starts, ends, vocab, -7, False)) == want
    assert -7 in want and 0 in want
    # a CSR without the second token of every document: starts carry what the neighbour no longer tells
    keep = [k for k in range(len(ends)) if k - 1 not in toff[:-1]]
    f_off = [sum(1 for k in keep if k < t) for t in toff]
    got = vocabref.ids_from_csr(raws, f_off, [starts[k] for k in keep], [ends[k] for k in keep], vocab, -7, False)
    assert list(got) == [want[k] for k in keep]


def test_normalised_lookup_sees_the_fullwidth_image():
    vocab = {"ＡＢ": 0, "AB": 1, "あ": 2}
    raw = "ABＡＢあ".encode("utf-8")
    assert list(vocabref.ids_from_csr([raw], [0, 3], None, [2, 8, 11], vocab, -1, False)) == [1, 0, 2]
    assert list(vocabref.ids_from_csr([raw], [0, 3], None, [2, 8, 11], vocab, -1, True)) == [0, 0, 2]


def test_hash_words():
    # FNV-1a over no char is the seed; the finish of seed ^ 0 by hand
    x = vocabref.SEED
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & vocabref.M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & vocabref.M64
    assert vocabref.surface_hash("") == x ^ (x >> 33)
    words = ["あ", "漢字", "AB09", "𠮷", "é"]
    many = [int(vocabref.hash_many(np.array([[ord(c) for c in w]], np.uint64))[0]) for w in words]
    assert many == [vocabref.surface_hash(w) for w in words]
    assert len(set(many)) == len(words)


def test_placement_is_linear_probing_with_load_at_most_a_half():
    for n in (1, 2, 3, 4, 5, 8, 9, 100, 1000):
        keys = ["w%d" % k for k in range(n)]
        bits, slots, where = vocabref.place(keys)
        assert (1 << bits) >= 2 * n and (n == 1 or (1 << bits) < 4 * n)
        assert sorted(s[0] for s in slots if s is not None) == list(range(n))
        for k, (h, slot, probes) in enumerate(where):
            assert slot == (h + probes - 1) & ((1 << bits) - 1)
            assert all(slots[(h + j) & ((1 << bits) - 1)] is not None for j in range(probes))   # no empty slot in front of a key on its chain


def test_the_searches_of_the_suite_succeed():
    three = vocabref.find_same_home(8, 15, 3)
    assert len(set(three)) == 3 and all(vocabref.home(s, 4) == 15 for s in three)
    _, _, where = vocabref.place(three + ["x1", "x2", "x3", "x4", "x5"])
    assert [w[1] for w in where[:3]] == [15, 0, 1]   # the chain wraps around the table's end
    twins = vocabref.find_fingerprint_twins(3)
    assert twins is not None
    a, b = twins
    assert a != b and len(a) == len(b) and vocabref.fingerprint(a) == vocabref.fingerprint(b) and vocabref.home(a, 3) == vocabref.home(b, 3)
