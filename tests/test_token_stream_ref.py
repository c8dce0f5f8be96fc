"""The restatement of vaporetto_tantivy's token_stream (tests/tokenref.py) against the adapter's own expected tokens
(tests/golden/token_stream_kat.json: the doc example and the tests of vaporetto_tantivy/src/lib.rs, recorded as data, plus the two
filter-order examples), on tantivy_model.bin.  CPU only."""
import json
import os

import pytest

from tests import tokenref

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "token_stream_kat.json"), encoding="utf-8"))
MODEL = open(os.path.join(HERE, "golden", KAT["model"]), "rb").read()


@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_restatement_gives_the_adapters_tokens(case):
    assert tokenref.token_stream(MODEL, case["text"], case["wsconst"]) == case["tokens"]


def test_the_order_examples_differ_under_the_librarys_flag_order():
    """What makes the order visible: wsconst first, linebreaks second (the library's VPT_FLAG_* order) gives other tokens."""
    import numpy as np
    labels = np.zeros(3, dtype=np.uint8)
    adapter = tokenref.filter_labels("a\n\nb", labels, "O")
    assert list(adapter) == [1, 0, 1]
    swapped = tokenref.filter_labels("a\n\nb", tokenref.filter_labels("a\n\nb", labels, "")[:] * 0, "")   # linebreaks last: every boundary set
    assert list(swapped) == [1, 1, 1]


def test_bad_wsconst_is_rejected():
    with pytest.raises(tokenref.WsconstError, match="Could not parse a wsconst value"):
        tokenref.token_stream(MODEL, "a", "X")
