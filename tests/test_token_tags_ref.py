"""The restatement of the tagged token spans (tests/tokentagref.py) held to hand-written cases whose expected tokens are literals.  CPU only: the
host forms alone (api.Sentence tags as lists, no predictor)."""
from tests import tokentagref
from vaporetto_amd.modelfmt import TagModel


def test_tokens_carry_the_tags_of_their_last_char():
    # "これは" + "テスト": two slots; tags sit at the token's last char (sentence.rs:1068)
    text, labels = "これはテスト", [0, 1, 1, 0, 0]
    tags = [None, None, "名詞", "コレ", "助詞", None, None, None, None, None, "名詞", None]
    assert tokentagref.tokens_of(text, labels, tags, 2) == [
        [0, 6, 0, ("名詞", "コレ")],
        [6, 9, 1, ("助詞", None)],
        [9, 18, 2, ("名詞", None)],
    ]


def test_byte_offsets_count_the_callers_bytes():
    # 1-, 2-, 3- and 4-byte chars; one slot; a single-char document
    assert tokentagref.tokens_of("aé漢🤌", [1, 0, 1], [None, None, "x", ""], 1) == [[0, 1, 0, (None,)], [1, 6, 1, ("x",)], [6, 10, 2, ("",)]]
    assert tokentagref.tokens_of("a", [], ["t"], 1) == [[0, 1, 0, ("t",)]]


def test_no_slots_no_tags():
    assert tokentagref.tokens_of("ab", [1], [], 0) == [[0, 1, 0, ()], [1, 2, 1, ()]]


def test_vocabulary_walk_is_first_appearance_over_models_slots_candidates():
    class M:
        tag_models = [TagModel("a", [["名", "動"], [], ["カ"]], bias=[]), TagModel("b", [["動", "x"], ["名"]], bias=[]), TagModel("c", [[""], ["x", "y"]], bias=[])]
    assert tokentagref.walk_vocabulary(M) == ["名", "動", "カ", "x", "", "y"]
