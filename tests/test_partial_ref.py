"""The oracle of the partial-annotation tests, pinned without a device: the reference's own unit tests and doc examples (tests/golden/partial_kat.json)
through the host restatement (api.Sentence.from_partial_annotation, Sentence.write_partial_annotation_text) and through the host C ABI
(vpt_parse_partial_batch, vpt_write_partial_batch)."""
import json
import os

import numpy as np
import pytest

from vaporetto_amd import api, build

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partial_kat.json"), encoding="utf-8"))
TAG_KEYS = ("n_tags", "tag_index", "span_offsets", "tag_bytes")


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_hip()


def _sentence_of(p):
    """a Sentence from the arrays the host parser wrote for one line"""
    s = api.Sentence.from_raw(bytes(p["raw"]).decode("utf-8"))
    s._boundaries = p["labels"].copy()
    nt, ti, so, tb = int(p["n_tags"][0]), p["tag_index"], p["span_offsets"], bytes(p["tag_bytes"])
    for c in range(len(s)):
        own = [tb[int(so[k]):int(so[k + 1])].decode("utf-8") for k in range(int(ti[c]), int(ti[c + 1]))]
        s._tags += [t if t else None for t in own + [""] * (nt - len(own))]
    s._n_tags = nt
    return s


@pytest.mark.parametrize("vec", KAT["parse"], ids=lambda v: v["text"][:10])
def test_parse_vectors(vec):
    s = api.Sentence.from_partial_annotation(vec["text"])
    h = _sentence_of(api.parse_partial_host([vec["text"].encode("utf-8")]))
    for x in (s, h):
        if "raw" in vec:
            assert x.as_raw_text() == vec["raw"]
            assert list(x.boundaries()) == vec["boundaries"]
            assert list(x.char_types()) == vec["char_types"]
            assert x.char_to_str_pos() == vec["char_to_str_pos"]
            assert len(x.boundary_scores()) == 0
        if "tokenized" in vec:
            assert x.write_tokenized_text() == vec["tokenized"]
    assert s.tags() == h.tags() and s.n_tags() == h.n_tags()


@pytest.mark.parametrize("vec", KAT["parse_errors"], ids=lambda v: v["message"][-12:])
def test_parse_error_vectors(vec):
    with pytest.raises(api.VaporettoError) as e:
        api.Sentence.from_partial_annotation(vec["text"])
    assert e.value.kind == "InvalidArgument" and str(e.value) == vec["message"]
    with pytest.raises(api.VaporettoError) as e:
        api.parse_partial_host([b"a", vec["text"].encode("utf-8")])
    assert e.value.kind == "InvalidArgument" and str(e.value) == vec["message"] + " (line 1)"


@pytest.mark.parametrize("vec", KAT["write"], ids=lambda v: v["partial"][:10])
def test_write_vectors(vec):
    if vec["from"] == "raw":
        s = api.Sentence.from_raw(vec["text"])
        p = None
    elif vec["from"] == "tokenized":
        s = api.Sentence.from_tokenized(vec["text"])
        p = api.parse_tokenized_host([vec["text"].encode("utf-8")])
    else:
        s = api.Sentence.from_partial_annotation(vec["text"])
        p = api.parse_partial_host([vec["text"].encode("utf-8")])
    if "set_boundary" in vec:
        s.boundaries_mut()[vec["set_boundary"][0]] = vec["set_boundary"][1]
        p["labels"][vec["set_boundary"][0]] = vec["set_boundary"][1]
    assert s.write_partial_annotation_text() == vec["partial"]
    if p is None:   # from_raw: every boundary Unknown, no tags
        utf8, boff = api.pack_texts([vec["text"].encode("utf-8")])
        n = len(vec["text"]) - 1
        text, toff = api.write_partial_host(utf8, boff, np.array([0, n], np.uint64), np.full(n, 2, np.uint8))
    else:
        text, toff = api.write_partial_host(p["raw"], p["raw_offsets"], p["out_offsets"], p["labels"], *[p[k] for k in TAG_KEYS])
    assert bytes(text).decode("utf-8") == vec["partial"] and list(toff) == [0, len(vec["partial"].encode("utf-8"))]
    # what was written parses back to the same sentence
    back = api.Sentence.from_partial_annotation(vec["partial"])
    assert back.as_raw_text() == s.as_raw_text() and list(back.boundaries()) == list(s.boundaries())
