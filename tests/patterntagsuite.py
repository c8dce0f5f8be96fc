"""PatternMatchTagger on the device (vaporetto_rules/src/sentence_filters/pattern_match_tagger.rs; include/vaporetto_hip.h, vpt_pattern_tagger_*;
vaporetto_amd/csrc/kernels_pattern.hip), run on the CPU emulator by tests/test_pattern_tagger_emu.py and on the MI355X by
tests/test_pattern_tagger_gpu.py.

The oracle is the host form: fill_tags (without a tagger), api.PatternMatchTagger.filter on every sentence, write_tokenized_text.  Every
comparison is byte for byte.  The host form itself is pinned by the reference's own known-answer test (check_reference_kat)."""
import os
import random

import numpy as np
import pytest

from tests import devmem, randmodel
from vaporetto_amd import _lib, api
from vaporetto_amd.modelfmt import TagModel

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_MODEL = open(os.path.join(HERE, "golden", "model.bin"), "rb").read()
FW = _lib.VPT_FLAG_KYTEA_FULLWIDTH
ALPHA = list("あいう漢字AB09")

# pattern_match_tagger.rs:51-73
KAT_INPUT = "これ/名詞/ソレ は テスト/名詞 です//デス"
KAT_RULES = {"これ": ["代名詞", "コレ"], "は": ["助詞", "ワ"], "テスト": ["名詞", "テスト"], "です": ["助動詞", "デス"]}
KAT_EXPECTED = "これ/名詞/ソレ は/助詞/ワ テスト/名詞/テスト です/助動詞/デス"


def check_reference_kat():
    s = api.Sentence.from_tokenized(KAT_INPUT)
    api.PatternMatchTagger(KAT_RULES).filter(s)
    assert s.write_tokenized_text() == KAT_EXPECTED


def golden_predictor():
    return api.Predictor(api.Model.read_slice(GOLDEN_MODEL)[0], True, device=0)


def tagged_model(seed=11, with_tags=True):
    """A random boundary model over ALPHA whose tag models leave slots None: three slots at most (n_tags == 3), candidate lists that are
    empty, models with fewer slots than n_tags."""
    m = randmodel.rand_model(seed, alphabet=ALPHA, wc=2, wt=2, n_tag_models=0)
    if with_tags:
        m.tag_models += [TagModel("漢字", [["名", "動"], [], ["カ"]], bias=[3, -2]),    # slot 1 has no candidate: None
                         TagModel("あい", [["x"]], bias=[]),                              # one slot: slots 1, 2 are None
                         TagModel("う", [["p", "q"], ["r"], ["s", "t"]], bias=[1, 2, 5, 4]),   # tagged fully
                         TagModel("09", [[], [], []], bias=[])]                            # a tag model that tags nothing
    return m


def predictor_of(m, predict_tags=True):
    return api.Predictor(api.Model.read_slice(api.Model(m).to_vec())[0], predict_tags, device=0)


def pack(texts):
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    return utf8, boff, api.count_boundaries(utf8, boff)


def lines_of(text, toff):
    raw = bytes(text)
    return [raw[int(toff[i]):int(toff[i + 1])] for i in range(len(toff) - 1)]


def oracle(pred, texts, ooff, labels, tagger, fullwidth=False):
    """-> (the tokenized lines as bytes, every sentence's tags): fill_tags, the host filter, write_tokenized_text.  Under `fullwidth` tags and
    rules see the normalised text and the caller's text is printed (predict/src/main.rs:154-170)."""
    norm = api.KyteaFullwidthFilter()
    sents = []
    for i, t in enumerate(texts):
        s = api.Sentence.from_raw(norm.filter(t) if fullwidth else t)
        s._boundaries = np.array(labels[int(ooff[i]):int(ooff[i + 1])], dtype=np.uint8)
        sents.append(s)
    pred.fill_tags_batch(sents)
    lines, tags = [], []
    for s, t in zip(sents, texts):
        if tagger is not None:
            tagger.filter(s)
        tags.append(list(s.tags()))
        s._text = t
        lines.append(s.write_tokenized_text().encode("utf-8"))
    return lines, tags


def resolve(pred, tagger, texts, ooff, labels, dense, fullwidth=False):
    """The dense int32 array of a fill_tags call as strings, per sentence: >= 0 through the tag model of the token, -(2 + id) through the tagger."""
    norm = api.KyteaFullwidthFilter()
    models = {tm.token: tm for tm in pred._model.tag_models()}
    nt = dense.shape[1]
    out = []
    for i, t in enumerate(texts):
        t = norm.filter(t) if fullwidth else t
        g0, n = int(ooff[i]) + i, len(t)
        row = [None] * (n * nt)
        start = 0
        for e in range(n):
            last = e == n - 1 or labels[int(ooff[i]) + e] == 1
            for j in range(nt):
                v = int(dense[g0 + e, j])
                if not last:
                    assert v == -1, (i, e, j, v)
                elif v >= 0:
                    row[e * nt + j] = models[t[start:e + 1]].tags[j][v]
                elif v <= -2:
                    row[e * nt + j] = tagger.tag(pred, -2 - v)
            if last:
                start = e + 1
        out.append(row)
    return out


def device_calls(pred, tagger, utf8, boff, ooff, labels, fullwidth=False):
    """On a workspace of the caller's: fill_tags with the dense array, expand_tags, write_tagged.  -> (dense, lines)"""
    S, nb, nt = len(boff) - 1, len(labels), pred.n_tags()
    total_c = nb + S
    d_text, d_boff, d_ooff = devmem.put(np.concatenate([utf8, np.zeros(32, np.uint8)])), devmem.put(boff), devmem.put(ooff)
    d_lab = devmem.put(np.concatenate([labels, np.zeros(16, np.uint8)]))
    guard = 8
    d_tags = devmem.put(np.full(total_c * max(nt, 1) + guard, 0x5A5A5A5A, np.int32))
    d_tags2 = devmem.put(np.full(total_c * max(nt, 1) + guard, 0x5A5A5A5A, np.int32))
    cap = 3 * len(utf8) + total_c * (pred.max_tag_suffix() + (tagger.max_tag_suffix(pred) if tagger is not None else 0)) + 16
    d_out, d_off = devmem.zeros(cap + 16, np.uint8), devmem.zeros(S + 1, np.uint64)
    batch = api.DeviceBatch(pred)
    batch.set_flags(FW if fullwidth else 0)
    batch.set_pattern_tagger(tagger)
    st = devmem.stream()
    batch.fill_tags(d_text.ptr, d_boff.ptr, d_ooff.ptr, S, nb, d_lab.ptr, d_tags.ptr, st)
    batch.expand_tags(S, nb, d_tags2.ptr, st)
    batch.write_tagged(d_text.ptr, d_boff.ptr, d_ooff.ptr, S, nb, d_lab.ptr, 0, d_out.ptr, cap, d_off.ptr, st)
    batch.sync()
    a, b = d_tags.get(), d_tags2.get()
    if nt:
        assert np.array_equal(a, b), "vpt_expand_tags_batch_device differs from the dense array of the fill_tags call"
        assert (a[total_c * nt:] == 0x5A5A5A5A).all()
    toff = d_off.get()
    return a[:total_c * nt].reshape(total_c, nt) if nt else np.zeros((total_c, 0), np.int32), lines_of(d_out.get(int(toff[S])), toff)


def check_all(pred, texts, rules, fullwidth=False, expect_rule_tags=True, labels=None):
    """Every path against the oracle, on the labels predict gives (the one-call pipeline too) or on the caller's; twice."""
    tagger = api.PatternMatchTagger(rules)
    utf8, boff, ooff = pack(texts)
    predicted = labels is None
    if predicted:
        _, labels, _ = pred.predict_packed(utf8, boff, fullwidth=fullwidth)
    want, want_tags = oracle(pred, texts, ooff, labels, tagger, fullwidth)
    plain, _ = oracle(pred, texts, ooff, labels, None, fullwidth)
    assert (want != plain) == expect_rule_tags
    for _ in range(2):   # two runs give identical bytes
        text, toff = pred.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, fullwidth=fullwidth, tagger=tagger)
        got = lines_of(text, toff)
        bad = [i for i in range(len(texts)) if got[i] != want[i]]
        assert not bad, (bad[:4], got[bad[0]].decode(), want[bad[0]].decode())
        if predicted:
            tok = pred.tokenize(texts, tagged=True, fullwidth=fullwidth, tagger=tagger)
            assert [t.encode("utf-8") for t in tok] == want
        dense, lines = device_calls(pred, tagger, utf8, boff, ooff, labels, fullwidth)
        assert lines == want
        assert resolve(pred, tagger, texts, ooff, labels, dense, fullwidth) == want_tags
        host_dense = pred.fill_tags_packed(utf8, boff, ooff, labels, fullwidth=fullwidth, tagger=tagger)
        assert np.array_equal(host_dense, dense)
    # with the tagger unset: what the calls give today, bit for bit
    text0, toff0 = pred.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, fullwidth=fullwidth)
    assert lines_of(text0, toff0) == plain
    dense0, lines0 = device_calls(pred, None, utf8, boff, ooff, labels, fullwidth)
    assert lines0 == plain and np.array_equal(dense0, pred.fill_tags_packed(utf8, boff, ooff, labels, fullwidth=fullwidth))
    assert (dense0 >= -1).all()
    return want


def docs(seed, n, extra=(), lo=1, hi=30):
    rng = random.Random(seed)
    words = ["漢字", "あい", "う", "09", "AB", "字漢", "B0"] + list(extra)
    out = []
    for _ in range(n):
        k = rng.randint(lo, hi)
        t = ""
        while len(t) < k:
            t += rng.choice(words) if rng.random() < 0.6 else rng.choice(ALPHA)
        out.append(t)
    return out


def docs_of_tokens(seed, n, extra=()):
    """-> (texts, labels): sentences of whole words, every word a token"""
    rng = random.Random(seed)
    words = ["漢字", "あい", "う", "09", "AB", "字漢", "B0", "A", "0", "い"] + list(extra)
    texts, labels = [], []
    for _ in range(n):
        toks = [rng.choice(words) for _ in range(rng.randint(1, 12))]
        texts.append("".join(toks))
        lab = []
        for t in toks:
            lab += [0] * (len(t) - 1) + [1]
        labels += lab[:-1]
    return texts, np.array(labels, np.uint8)


def check_none_slots_only():
    """Case 1: a token whose tag model leaves a slot None gets that slot alone; one the model tags fully is unchanged though a rule names it."""
    pred = predictor_of(tagged_model())
    assert pred.n_tags() == 3
    rules = {"漢字": ["RULE0", "RULE1", "RULE2"], "う": ["no", "no", "no"], "あい": ["never", "二", None]}
    check_all(pred, docs(1, 200), rules)
    texts, labels = docs_of_tokens(1, 100)
    want = check_all(pred, texts, rules, labels=labels)
    joined = b" ".join(want).decode()
    assert "/RULE1/カ" in joined and "RULE0" not in joined and "RULE2" not in joined and "/no" not in joined
    assert "あい/x/二" in joined and "never" not in joined


def check_tokens_without_model():
    """Case 2: lists shorter and longer than n_tags, a None in the middle with Some("") last (a trailing '/'); escapes in a rule tag."""
    pred = predictor_of(tagged_model())
    rules = {"AB": ["short"], "字漢": ["a", "b", "c", "ignored", "too"], "B0": ["first", None, ""], "A": [None, "sl/ash sp\\"], "0": []}
    check_all(pred, docs(2, 200), rules)
    texts, labels = docs_of_tokens(2, 100)
    want = check_all(pred, texts, rules, labels=labels)
    joined = b" ".join(want).decode()
    assert "AB/short " in joined + " " and "字漢/a/b/c " in joined + " " and "ignored" not in joined
    assert "B0/first// " in joined + " "
    assert "A//sl\\/ash\\ sp\\\\" in joined


def check_exact_match():
    """Case 3: the whole surface or nothing; a token one char longer than the longest surface."""
    pred = golden_predictor()
    rules = {"東京": ["地名", "トーキョー"], "東京都": ["地名", "トーキョート"]}
    tagger = api.PatternMatchTagger(rules)
    texts = ["東京", "東京都", "東京都庁", "東京都庁舎", "は東京都"]
    utf8, boff, ooff = pack(texts)
    nt = pred.n_tags()
    for labels in (np.zeros(int(ooff[-1]), np.uint8), ):   # every sentence one token, but the last: は | 東京都
        labels[int(ooff[4])] = 1
        want, _ = oracle(pred, texts, ooff, labels, tagger)
        assert want == ["東京/地名/トーキョー".encode(), "東京都/地名/トーキョート".encode(), "東京都庁".encode(), "東京都庁舎".encode(),
                        "は/助詞/ワ 東京都/地名/トーキョート".encode()]
        text, toff = pred.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, tagger=tagger)
        assert lines_of(text, toff) == want
        dense, lines = device_calls(pred, tagger, utf8, boff, ooff, labels)
        assert lines == want and dense.shape[1] == nt
    assert tagger.info(pred)["max_surface_chars"] == 3


def chain_rules(n=2000, seed=3):
    rng = random.Random(seed)
    pool = list("あいう漢字AB09カキ")
    pairs, seen = [], set()
    while len(pairs) < n:
        s = "".join(rng.choice(pool) for _ in range(rng.randint(1, 6)))
        if s in seen:
            continue
        seen.add(s)
        pairs.append((s, ["T%d" % (len(pairs) % 37), None if len(pairs) % 5 == 0 else "U%d" % len(pairs)]))
    return pairs


def check_probe_chains():
    """Case 4: 2 000 surfaces (collisions occur), every 7th of them in the text as a token of its own; a duplicate surface keeps the last rule."""
    pred = predictor_of(tagged_model())
    pairs = chain_rules()
    pairs.append((pairs[14][0], ["LAST", "WINS", "x"]))   # (14 is a multiple of 7: it is in the text)
    tagger = api.PatternMatchTagger(pairs)
    info = tagger.info(pred)
    assert info["n_keys"] == 2000 and 0.25 < info["n_keys"] / info["n_slots"] <= 0.5
    surfaces = [p[0] for p in pairs[0:2000:7]]
    rng = random.Random(5)
    texts, labels = [], []
    for _ in range(120):
        toks = [rng.choice(surfaces) if rng.random() < 0.7 else rng.choice(ALPHA) for _ in range(rng.randint(1, 8))]
        texts.append("".join(toks))
        lab = []
        for t in toks:
            lab += [0] * (len(t) - 1) + [1]
        labels += lab[:-1]
    utf8, boff, ooff = pack(texts)
    labels = np.array(labels, np.uint8)
    want, want_tags = oracle(pred, texts, ooff, labels, tagger)
    joined = b" ".join(want).decode()
    assert "/LAST/WINS/x" in joined and joined.count("/T") > 100
    text, toff = pred.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, tagger=tagger)
    assert lines_of(text, toff) == want
    dense, lines = device_calls(pred, tagger, utf8, boff, ooff, labels)
    assert lines == want and resolve(pred, tagger, texts, ooff, labels, dense) == want_tags


def check_edges():
    """Case 5."""
    pred = predictor_of(tagged_model())
    tile = api.PatternMatchTagger.tile()
    assert tile >= 64
    rules = {"A": ["one"], "AB09": ["straddle", None, "s"], "漢字": [None, "mid"], "B": ["lastlast"]}
    tagger = api.PatternMatchTagger(rules)
    # a one-char sentence; a sentence that is one token; tokens across multiples of the kernel's step, counted from the start of their front-end
    # run, in the run's first sentence and in one further on; a rule hit on the last token of the last sentence
    def straddling(start, spots):
        """A sentence that begins `start` chars into its run, with a rule surface across every run-relative position k * tile in `spots`."""
        t = ""
        for k, w in spots:
            at = k * tile - 1 - start   # the surface's first char is the step's last one
            assert at >= len(t)
            t += "う" * (at - len(t)) + w
        return t + "う"
    long1 = straddling(0, [(1, "AB09"), (2, "漢字"), (3, "AB09"), (4, "AB09")])
    head = [long1, "A", "AB09", "あ"]
    start2 = sum(len(t) for t in head)
    k2 = start2 // tile + 1
    long2 = straddling(start2, [(k2, "AB09"), (k2 + 1, "漢字")])
    texts = head + [long2, "あいB"]
    per = run_sentences(len(texts), sum(len(t) for t in texts))
    assert per >= 5   # (the first five sentences are one run: the positions above are run-relative)
    for t, start in ((long1, 0), (long2, start2)):
        crossed = 0
        for w in ("AB09", "漢字"):
            at = t.find(w)
            while at >= 0:
                first, last = start + at, start + at + len(w) - 1
                assert first // tile + 1 == last // tile and first % tile == tile - 1   # spans k * tile - 1 and k * tile
                crossed += 1
                at = t.find(w, at + 1)
        assert crossed == (4 if start == 0 else 2)
    utf8, boff, ooff = pack(texts)
    labels = np.ones(int(ooff[-1]), np.uint8)
    for i, t in enumerate(texts):   # every char a token, but the rule surfaces
        for w in ("AB09", "漢字"):
            at = t.find(w)
            while at >= 0:
                labels[int(ooff[i]) + at:int(ooff[i]) + at + len(w) - 1] = 0
                at = t.find(w, at + 1)
    want, want_tags = oracle(pred, texts, ooff, labels, tagger)
    assert want[1] == b"A/one" and want[2] == "AB09/straddle//s".encode() and want[-1].endswith(b" B/lastlast")
    assert want[0].count(b"AB09/straddle//s") == 3 and want[0].count("/mid/カ".encode()) == 1
    assert want[4].count(b"AB09/straddle//s") == 1 and want[4].count("/mid/カ".encode()) == 1
    for _ in range(2):
        text, toff = pred.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, tagger=tagger)
        assert lines_of(text, toff) == want
        dense, lines = device_calls(pred, tagger, utf8, boff, ooff, labels)
        assert lines == want and resolve(pred, tagger, texts, ooff, labels, dense) == want_tags
    # an Unknown label inside a token: no rule tags for it (the dense array; the writer rejects such labels)
    lab2 = labels.copy()
    lab2[int(ooff[2]) + 1] = 2
    dense = pred.fill_tags_packed(utf8, boff, ooff, lab2, tagger=tagger)
    g2 = int(ooff[2]) + 2
    assert (dense[g2:g2 + 4] == -1).all() and (dense[g2 - 1] != -1).any()   # (texts[2] is "AB09"; texts[1], "A", keeps its rule tag)
    # an empty batch; no rules at all
    assert pred.tokenize([], tagged=True, tagger=tagger) == []
    e_text, e_off = pred.write_tokenized_packed(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(0, np.uint8), tagged=True,
                                                tagger=tagger)
    assert len(e_text) == 0 and list(e_off) == [0]
    none = api.PatternMatchTagger({})
    assert none.n_tags(pred) == 0 and none.info(pred)["n_keys"] == 0
    plain, _ = oracle(pred, texts, ooff, labels, None)
    text, toff = pred.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, tagger=none)
    assert lines_of(text, toff) == plain
    _, lines = device_calls(pred, none, utf8, boff, ooff, labels)
    assert lines == plain


def run_sentences(n_sent, total_chars):
    """The sentences of a front-end run for a batch of this shape (tag_run_sentences, kernels_tags.hip): about 2048 chars, 1 .. 256 sentences."""
    return min(max((2048 * n_sent + total_chars // 2) // max(total_chars, 1), 1), 256)


def check_full_runs():
    """Batches of many very short sentences: the front-end runs hold 256 sentences, the most there is -- every one of them, the last of a run
    and the last of the batch included, gets its rule tags."""
    pred = predictor_of(tagged_model())
    rules = {"AB": ["short"], "A": ["one", None, "x"], "漢": [None, "k"], "あい": ["never", "二"]}
    rng = random.Random(13)
    for n in (256, 257, 600):
        texts = [rng.choice(["AB", "A", "漢", "あい", "う", "B", "09"]) for _ in range(n)]
        assert run_sentences(n, sum(len(t) for t in texts)) == 256
        labels = np.zeros(sum(len(t) - 1 for t in texts), np.uint8)   # every sentence one token
        want = check_all(pred, texts, rules, labels=labels)
        for t, w in zip(texts, want):
            assert w == {"AB": b"AB/short", "A": b"A/one//x", "漢": "漢//k".encode(), "あい": "あい/x/二".encode()}.get(t, w), (t, w)
            assert t != "B" or w == b"B"
    check_all(pred, ["AB"] * 600, {"AB": ["short"]})   # (on the labels predict gives, through the one-call pipeline)


def check_fullwidth():
    """Case 6: the surfaces are those of the text as fill_tags sees it."""
    pred = predictor_of(tagged_model())
    rules = {"ＡＢ": ["full"]}
    texts = ["AB", "あAB", "ＡＢ"]
    utf8, boff, ooff = pack(texts)
    labels = np.array([0, 1, 0, 0], np.uint8)
    tagger = api.PatternMatchTagger(rules)
    for fw, want in ((True, [b"AB/full", "あ AB/full".encode(), "ＡＢ/full".encode()]), (False, [b"AB", "あ AB".encode(), "ＡＢ/full".encode()])):
        assert oracle(pred, texts, ooff, labels, tagger, fw)[0] == want
        text, toff = pred.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, fullwidth=fw, tagger=tagger)
        assert lines_of(text, toff) == want
        _, lines = device_calls(pred, tagger, utf8, boff, ooff, labels, fw)
        assert lines == want
    check_all(pred, docs(6, 100), {"ＡＢ": ["full"], "０９": [None, "digits"], "漢字": ["k", "k", "k"]}, fullwidth=True)


def check_no_tag_models():
    """Case 7: n_tags == 0: the filter changes nothing (the reference's loop runs over the token's n_tags slots); predict_tags == 0: the existing error."""
    pred = predictor_of(tagged_model(with_tags=False))
    assert pred.n_tags() == 0
    texts = docs(7, 60)
    tagger = api.PatternMatchTagger({"漢字": ["a"], "A": ["b", "c"]})
    utf8, boff, ooff = pack(texts)
    _, labels, _ = pred.predict_packed(utf8, boff)
    untagged, uoff = pred.write_tokenized_packed(utf8, boff, ooff, labels)
    text, toff = pred.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, tagger=tagger)
    assert bytes(text) == bytes(untagged) and np.array_equal(toff, uoff)
    assert [t.encode() for t in pred.tokenize(texts, tagged=True, tagger=tagger)] == lines_of(untagged, uoff)
    _, lines = device_calls(pred, tagger, utf8, boff, ooff, labels)
    assert lines == lines_of(untagged, uoff)
    off = predictor_of(tagged_model(), predict_tags=False)
    t2 = api.PatternMatchTagger({"漢字": ["a"]})
    for call in (lambda: off.tokenize(texts, tagged=True, tagger=t2), lambda: off.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, tagger=t2),
                 lambda: off.fill_tags_packed(utf8, boff, ooff, labels, tagger=t2)):
        with pytest.raises(api.VaporettoError, match="created with predict_tags = false"):
            call()


def check_golden_pipeline():
    """Case 8 on the golden model: the record order through the writer of the device calls and the one-call pipeline, numbers and symbols tagged."""
    pred = golden_predictor()
    rng = random.Random(8)
    alpha = list("まぁ社長は火星猫だ良いろう人地球12,。")
    texts = ["まぁ社長は火星猫だ", "火星猫12", "まぁ良いだろう。"] + ["".join(rng.choice(alpha) for _ in range(rng.randint(1, 40))) for _ in range(250)]
    rules = {"1": ["数詞", "イチ"], "2": ["数詞"], "12": ["数詞", "ジューニ"], "。": ["補助記号"], ",": [None, "カンマ"], "人": ["名詞", "ヒト"], "は": ["never", "never"]}
    want = check_all(pred, texts, rules)
    assert b"never" not in b" ".join(want)


def check_listing():
    """Case 9: the listing with --scores on: a rule-tagged token prints its tags in T; it has no candidates in the tag block."""
    pred = golden_predictor()
    tagger = api.PatternMatchTagger({"12": ["数詞", "ジューニ"], "人": ["名詞"]})
    texts = ["火星猫12だ", "人は12"]
    utf8, boff, ooff = pack(texts)
    scores, labels, _ = pred.predict_packed(utf8, boff)
    S, nb = len(texts), len(labels)
    total_c = nb + S
    want_t, _ = oracle(pred, texts, ooff, labels, tagger)
    for listing in (_lib.VPT_LISTING_SCORES | _lib.VPT_LISTING_TAGGED, _lib.VPT_LISTING_SCORES | _lib.VPT_LISTING_TAG_SCORES | _lib.VPT_LISTING_TAGGED):
        outs = []
        for tg in (tagger, None):
            cap = pred.listing_capacity(len(utf8), total_c, S, listing) + total_c * tagger.max_tag_suffix(pred)
            d_text, d_boff, d_ooff = devmem.put(np.concatenate([utf8, np.zeros(32, np.uint8)])), devmem.put(boff), devmem.put(ooff)
            d_sc, d_lab = devmem.put(np.concatenate([scores, np.zeros(4, np.int32)])), devmem.put(np.concatenate([labels, np.zeros(16, np.uint8)]))
            d_out, d_off = devmem.zeros(cap + 16, np.uint8), devmem.zeros(S + 1, np.uint64)
            batch = api.DeviceBatch(pred)
            batch.set_pattern_tagger(tg)
            batch.predict_listing(d_text.ptr, d_boff.ptr, d_ooff.ptr, S, nb, len(utf8), d_sc.ptr, d_lab.ptr, listing, d_out.ptr, cap, d_off.ptr, devmem.stream())
            batch.sync()
            off = d_off.get()
            outs.append(lines_of(d_out.get(int(off[S])), off))
        with_rules, without = outs
        plain_t, _ = oracle(pred, texts, ooff, labels, None)
        for i in range(S):
            assert with_rules[i].startswith(want_t[i] + b"\n") and without[i].startswith(plain_t[i] + b"\n")
            # everything behind T -- the scores block, the tag block -- is the same with and without the rules: no candidate scores for rule tags
            assert with_rules[i][len(want_t[i]):] == without[i][len(plain_t[i]):]
        assert want_t != plain_t and "/数詞".encode() in b"".join(with_rules) and "/数詞".encode() not in b"".join(without)


def _create(pred, surfaces, lists):
    """vpt_pattern_tagger_create from raw bytes (surfaces: bytes; lists: per rule a list of bytes or None) -> status"""
    utf8, off = api.pack_texts(list(surfaces))
    counts = np.array([len(v) for v in lists], np.uint32)
    present = np.array([0 if t is None else 1 for v in lists for t in v] + [0], np.uint8)
    tb, toff = api.pack_texts([t or b"" for v in lists for t in v] + [b""])
    utf8 = np.concatenate([utf8, np.zeros(1, np.uint8)])
    h = _lib.C.c_void_p()
    st = _lib.load().vpt_pattern_tagger_create(pred.handle, utf8.ctypes.data, off.ctypes.data, len(surfaces), counts.ctypes.data, present.ctypes.data,
                                               tb.ctypes.data, toff.ctypes.data, _lib.C.byref(h))
    if st == _lib.VPT_OK:
        _lib.load().vpt_pattern_tagger_destroy(h)
    return st


def check_errors():
    """Case 10, by message."""
    pred = predictor_of(tagged_model())
    ok = ("あ".encode(), [b"t"])
    for bad, msg in (((b"\xe3\x81", [b"t"]), "a surface is not valid UTF-8 (rule 1)"), ((b"\xed\xa0\x80", [b"t"]), "a surface is not valid UTF-8 (rule 1)"),
                     ((b"", [b"t"]), "a surface must contain at least one character (rule 1)"), ((b"a\0b", [b"t"]), "a surface must not contain NULL (rule 1)"),
                     ((b"ab", [None, b"t\0", b"u"]), "a tag must not contain NULL (rule 1)"), ((b"ab", [None, None, None, None, b"\0"]), "a tag must not contain NULL (rule 1)")):
        st = _create(pred, [ok[0], bad[0]], [ok[1], bad[1]])
        assert st == _lib.VPT_INVALID_ARGUMENT and _lib.last_error() == "InvalidArgumentError: rules: " + msg, _lib.last_error()
    assert _create(pred, [ok[0]], [ok[1]]) == _lib.VPT_OK
    with pytest.raises(api.VaporettoError, match="a surface must contain at least one character \\(rule 0\\)"):
        api.PatternMatchTagger({"": ["x"]}).handle(pred)
    # a tagger belongs to its predictor
    other = predictor_of(tagged_model(seed=12))
    tagger = api.PatternMatchTagger({"A": ["x"]})
    batch = api.DeviceBatch(other)
    st = _lib.load().vpt_batch_set_pattern_tagger(batch._h, tagger.handle(pred))
    assert st == _lib.VPT_INVALID_ARGUMENT and "tagger: does not belong" in _lib.last_error()
    utf8, boff, ooff = pack(["A"])
    out, offs = np.zeros(64, np.uint8), np.zeros(2, np.uint64)
    st = _lib.load().vpt_tokenize_batch_rules(other.handle, utf8.ctypes.data, boff.ctypes.data, 1, 0, 1, out.ctypes.data, 64, offs.ctypes.data, tagger.handle(pred))
    assert st == _lib.VPT_INVALID_ARGUMENT and "tagger: does not belong" in _lib.last_error()
    # records made under another setting of the workspace are not the writer's
    b2 = api.DeviceBatch(pred)
    d_text, d_boff, d_ooff = devmem.put(np.concatenate([utf8, np.zeros(32, np.uint8)])), devmem.put(boff), devmem.put(ooff)
    d_out, d_off, d_lab = devmem.zeros(256, np.uint8), devmem.zeros(2, np.uint64), devmem.zeros(16, np.uint8)
    b2.fill_tags(d_text.ptr, d_boff.ptr, d_ooff.ptr, 1, 0, d_lab.ptr, 0, devmem.stream())
    b2.set_pattern_tagger(tagger)
    with pytest.raises(api.VaporettoError, match="call vpt_fill_tags_batch_device on this workspace"):
        b2.write_tagged(d_text.ptr, d_boff.ptr, d_ooff.ptr, 1, 0, d_lab.ptr, 0, d_out.ptr, 200, d_off.ptr, devmem.stream())
    b2.sync()


def check_python_mirror():
    """Sentence.tags() resolves the rule tags through the tagger; Predictor.write_tokenized_batch takes it."""
    pred = predictor_of(tagged_model())
    tagger = api.PatternMatchTagger({"漢字": ["RULE0", "RULE1"], "AB": ["ab"]})
    texts = docs(9, 40)
    sents = [api.Sentence.from_raw(t) for t in texts]
    pred.predict_batch(sents)
    ref = [api.Sentence.from_raw(t) for t in texts]
    for r, s in zip(ref, sents):
        r._boundaries = s._boundaries.copy()
    pred.fill_tags_batch(ref)
    for r in ref:
        tagger.filter(r)
    pred.fill_tags_batch(sents, tagger=tagger)
    assert [s.tags() for s in sents] == [r.tags() for r in ref]
    assert pred.write_tokenized_batch(sents, tagged=True, tagger=tagger) == [r.write_tokenized_text() for r in ref]
