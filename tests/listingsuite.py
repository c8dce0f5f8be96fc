"""The checks of the predict CLI's listings (vpt_predict_listing_batch[_device], api.Predictor.predict_listing) against the restatement of
tests/listingref.py on the CPU oracle's numbers, run on the CPU emulator by tests/test_listing_emu.py and on the MI355X by
tests/test_listing_gpu.py.  Every comparison is exact."""
import itertools
import os
import random
import re

import numpy as np
import pytest

from tests import devmem, kat, listingref, randmodel
from vaporetto_amd import _lib, api, modelfmt
from vaporetto_amd.modelfmt import ModelData, NgramData, TagModel, TagNgramData, TagWeight

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_MODEL = open(os.path.join(HERE, "golden", "model.bin"), "rb").read()
KAT_TEXT = "この人は地球人だ"
KAT_SCORES = b"0:\xe3\x81\x93\xe3\x81\xae -22\n1:\xe3\x81\xae\xe4\xba\xba 54\n2:\xe4\xba\xba\xe3\x81\xaf 58\n3:\xe3\x81\xaf\xe5\x9c\xb0 43\n" \
             b"4:\xe5\x9c\xb0\xe7\x90\x83 -54\n5:\xe7\x90\x83\xe4\xba\xba 68\n6:\xe4\xba\xba\xe3\x81\xa0 48\n\n"
assert KAT_SCORES.decode() == "0:この -22\n1:の人 54\n2:人は 58\n3:は地 43\n4:地球 -54\n5:球人 68\n6:人だ 48\n\n"
COMBOS = list(itertools.product([False, True], repeat=4))   # scores, tag_scores, tagged, no_norm_order


def predictor(raw, tags):
    return api.Predictor(api.Model.read_slice(raw)[0], tags, device=0)


def compare(raw, pred, texts, **kw):
    want = listingref.listing_lines(raw, texts, **kw)
    kw2 = dict(kw)
    ws = kw2.pop("wsconst", "")
    got = pred.predict_listing(texts, wsconst=[c if c == "G" else listingref.tokenref.WSCONST[c] for c in ws], **kw2)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (kw, i, texts[i][:40], g[:200], w[:200])
    return got


def check_kat():
    raw = api.Model(kat.predictor_test_model()).to_vec()
    pred = predictor(raw, True)
    got = pred.predict_listing([KAT_TEXT], scores=True, fullwidth=False)[0]
    assert got == "この 人 は 地球 人 だ\n".encode() + KAT_SCORES
    got = pred.predict_listing([KAT_TEXT], scores=True, fullwidth=False, no_norm_order=True)[0]
    assert got == "この 人 は 地球 人 だ".encode() + KAT_SCORES + b"\n"
    # predictor.rs:861-903: the tags the reference expects; the candidates' scores are the oracle's
    got = pred.predict_listing([KAT_TEXT], tag_scores=True, tagged=True, fullwidth=False)[0].decode()
    assert got.startswith("この 人/名詞/ヒト は 地球/名詞/チキュー 人/接尾辞/ジン だ\n")
    block = got.split("\n", 1)[1]
    assert re.sub(r":-?\d+", ":#", block) == ("この\n人\t名詞:#,接尾辞:#\tジン:#,ヒト:#\nは\n地球\t名詞:#\tマンホーム:#,チキュー:#\n"
                                              "人\t名詞:#,接尾辞:#\tジン:#,ヒト:#\nだ\n\n")
    assert "地球\t名詞:0\t" in block
    for sc, ts, tg, nn in COMBOS:
        compare(raw, pred, [KAT_TEXT], scores=sc, tag_scores=ts, tagged=tg, no_norm_order=nn, fullwidth=not nn)
    graw, gpred = GOLDEN_MODEL, predictor(GOLDEN_MODEL, True)
    for sc, ts, tg, nn in COMBOS:
        compare(graw, gpred, ["まぁ社長は火星猫だ", "まぁ良いだろう"], scores=sc, tag_scores=ts, tagged=tg, no_norm_order=nn, fullwidth=not nn)


I32_MIN, I32_MAX = -2147483648, 2147483647


def edge_model(seed=3, big=True):
    """A random boundary model (weights up to 2e9 with `big`: the sums wrap, scores of 10 digits and a sign) with hand-made tag models: tags
    with ':' ',' ' ' '/' '\\', a slot with one candidate, a slot with none, a repeated surface (the last wins), a surface that needs escaping,
    a surface that only the normalised text has."""
    m = randmodel.rand_model(seed, alphabet=list("あいうカ漢字09AZaz、 /\\１Ａ"), wc=3, wt=2, big=big)
    def tm(tok, tags, bias, ngram=True):
        return TagModel(token=tok, tags=tags,
                        char_ngram_model=[TagNgramData(tok[-1], [TagWeight(0, list(range(1, len(bias) + 1)))])] if bias and ngram else [],
                        type_ngram_model=[], bias=bias)
    m.tag_models = [
        tm("あ", [["early", "loses"]], [9, 8]),
        tm("カ", [["x:y", "a,b"], ["only"]], [5, -7]),
        tm("い", [["first"]], []),
        tm("う", [[], ["p q", "r/s", "t\\u"]], [I32_MAX, I32_MIN, -1], ngram=False),
        tm("あ", [["later", "wins"], ["z"]], [0, -1]),
        tm("a /", [["sp ace", "sl/ash"]], [1, 2]),
        tm("Ａ", [["full", "width"]], [3, 4]),
    ]
    return api.Model(m).to_vec()


def edge_texts(seed=4):
    rng = random.Random(seed)
    alpha = list("あいうカ漢字09AZaz、 /\\１Ａ") + ["é", "ß", "𠮷", "🤌", "ｱ"]
    texts = ["あ", "a", "🤌", "é", "漢", "あいう", "a / あ", "A0aあ/い\\う 漢", "ＡA１1"]
    texts += ["".join(rng.choice(alpha) for _ in range(n)) for n in (1, 2, 3, 5, 9, 15, 16, 17, 31, 33, 64, 100, 1100, 2500)]
    # 1- to 4-byte chars at every alignment of a 16-byte piece
    for k in range(20):
        texts.append("a" * k + "é" + "あ" + "𠮷" + "b" * (k % 3) + "🤌あ")
    return texts


def has_all(data: bytes, markers):
    """Every marker is in the bytes: a fixture that stops exercising a case fails the check that relies on it."""
    missing = [mk for mk in markers if (mk if isinstance(mk, bytes) else mk.encode()) not in data]
    assert not missing, missing


def check_edges():
    raw = edge_model()
    pred = predictor(raw, True)
    texts = edge_texts()
    got = compare(raw, pred, texts, scores=True, tag_scores=True, tagged=True, fullwidth=True)
    # (compare: got IS the oracle-built bytes) the cases are there: the index crosses 9/10, 99/100, 999/1000 and 1-4 digits are listed, scores
    # of 10 digits with and without a sign, one-char sentences, chars the filter changes (normalised in the listing, as given in T)
    joined = b"".join(got)
    has_all(joined, ["\n9:", "\n10:", "\n99:", "\n100:", "\n999:", "\n1000:", "\n2498:"])
    assert re.search(rb" -[12]\d{9}\n", joined) and re.search(rb" [12]\d{9}\n", joined)
    assert re.fullmatch(r"あ/\w+/z\n\nあ\tlater:-?\d+,wins:-?\d+\tz:0\n\n", got[texts.index("あ")].decode()) and got[texts.index("漢")] == "漢\n\n漢\n\n".encode()   # (no tag model: the surface alone)
    assert got[texts.index("🤌")] == "🤌\n\n🤌\n\n".encode()
    fw = got[texts.index("ＡA１1")].decode()
    assert fw.split("\n")[0].replace(" ", "").startswith("Ａ") and "A" in fw.split("\n")[0] and "0:ＡＡ " in fw and "2:１１ " in fw
    compare(raw, pred, texts, scores=True, tag_scores=True, tagged=True, fullwidth=False, no_norm_order=True)
    compare(raw, pred, texts, scores=True, tag_scores=False, tagged=False, fullwidth=True)
    plain = predictor(raw, False)
    compare(raw, plain, texts, scores=True, fullwidth=True)
    for ws in ("D", "R", "H", "T", "K", "O", "G", "DRHTKO", "OG"):
        compare(raw, pred, texts, scores=True, tag_scores=True, tagged=True, fullwidth=True, wsconst=ws)
    lb = ["a\nb", "あ\r\nい", "\n", "x\n\ny"]
    compare(raw, pred, lb, scores=True, tag_scores=True, tagged=True, fullwidth=True, split_linebreaks=True)


def check_forced_tokens():
    """The tag block's edge cases with the tokens FORCED by labels of the caller (the oracle's scores beside them), so that every case is
    listed whatever the random boundary model would have cut: tags with ':' ',' ' ' '/' '\\', a slot with one candidate, a slot with none,
    a token without a tag model, a repeated surface (the last model wins), a three-char surface with ' ' and '/' (escaped in T, raw in the
    tag block), a surface that only the normalised text has, INT32_MIN and INT32_MAX among the tag scores."""
    raw = edge_model()
    pred = predictor(raw, True)
    listing = _lib.VPT_LISTING_SCORES | _lib.VPT_LISTING_TAG_SCORES | _lib.VPT_LISTING_TAGGED
    cases = [(False, ["a /あ", "xa /", "a /", "あカいう漢", "\\ /"], [0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1],
              ["a /\tsp ace:", ",sl/ash:", "\na\\ \\//s", "あ\tlater:", ",wins:", "\tz:0\n", "カ\tx:y:", ",a,b:", "\tonly:0\n", "い\tfirst:0\n",
               "う\t\tp q:2147483647,r/s:-2147483648,t\\u:-1\n", "\n漢\n\n", "\nx\n", "\n\\\n \n/\n\n", "\n\\\\ \\  \\/"]),
             (True, ["AあA", "a /"], [1, 1, 0, 0],
              ["A/", "Ａ\tfull:", ",width:", "0:Ａあ ", "1:あＡ ", "\nａ ／\n\n"])]
    for fullwidth, texts, lab, markers in cases:
        lab = np.array(lab, dtype=np.uint8)
        sc, ooff = listingref.oracle_scores(raw, texts, fullwidth=fullwidth)
        assert len(lab) == int(ooff[-1])
        utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
        for nn in (False, True):
            want = listingref.listing_lines(raw, texts, scores=True, tag_scores=True, tagged=True, fullwidth=fullwidth, no_norm_order=nn,
                                            labels_override=lab)
            has_all(b"\n" + b"".join(want), markers)
            assert b"early" not in b"".join(want) and b"loses" not in b"".join(want)
            out, offs = pred.predict_listing_packed(utf8, boff, listing | (_lib.VPT_LISTING_NO_NORM_ORDER if nn else 0),
                                                    flags=_lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0, scores=sc, labels=lab)
            assert bytes(out) == b"".join(want), (fullwidth, nn, bytes(out), b"".join(want))
            assert [int(x) for x in offs] == list(np.cumsum([0] + [len(w) for w in want]))


def extreme_model():
    """Boundary scores of exactly INT32_MIN, INT32_MAX, -1 and 0: rand_model's frame (big) with nothing drawn, bias 0 and three unigrams with
    one weight each, every one between chars that weigh nothing."""
    m = randmodel.rand_model(11, alphabet=list("あいう漢"), wc=1, wt=1, n_char=0, n_type=0, n_dict=0, big=True)
    m.bias = 0
    m.char_ngram_model = [NgramData("あ", [I32_MIN, 0]), NgramData("い", [I32_MAX, 0]), NgramData("う", [-1, 0])]
    return api.Model(m).to_vec()


def check_extreme_scores():
    """INT32_MIN, INT32_MAX, 0 and -1 as boundary scores: computed (a model made for them, against the oracle) and as the caller's scores,
    which are listed as they are (labels given)."""
    raw = extreme_model()
    for nn in (False, True):
        got = compare(raw, predictor(raw, False), ["漢あ漢漢い漢漢う漢漢", "あ漢", "漢あ"], scores=True, fullwidth=not nn, no_norm_order=nn)
        has_all(b"".join(got), [" -2147483648\n", " 2147483647\n", " -1\n", " 0\n"])
    raw = edge_model()
    pred = predictor(raw, False)
    text = "あいうカ漢"
    utf8, boff = api.pack_texts([text.encode("utf-8")])
    sc = np.array([I32_MIN, I32_MAX, 0, -1], dtype=np.int32)
    lab = np.array([0, 1, 0, 1], dtype=np.uint8)
    out, offs = pred.predict_listing_packed(utf8, boff, _lib.VPT_LISTING_SCORES, scores=sc, labels=lab)
    assert bytes(out) == "あい うカ 漢\n0:あい -2147483648\n1:いう 2147483647\n2:うカ 0\n3:カ漢 -1\n\n".encode()
    assert int(offs[1]) == len(out)


def synth_batch(seed, n, lo=8, hi=512):
    rng = random.Random(seed)
    alpha = list("あいうえおカキク漢字日本09AZaz、。") + ["𠮷", "é"]
    return ["".join(rng.choice(alpha) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def tagged_model(seed=21):
    m = randmodel.rand_model(seed, alphabet=list("あいうえおカキク漢字日本09AZaz、。"), wc=3, wt=3, n_tag_models=12)
    return api.Model(m).to_vec()


def check_batches(n=300):
    raw = tagged_model()
    pred = predictor(raw, True)
    texts = synth_batch(7, n)
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    for sc, ts, tg, nn in COMBOS:
        got = compare(raw, pred, texts, scores=sc, tag_scores=ts, tagged=tg, no_norm_order=nn, fullwidth=not nn)
        again = pred.predict_listing(texts, scores=sc, tag_scores=ts, tagged=tg, no_norm_order=nn, fullwidth=not nn)
        assert again == got
        # the device variant: the same bytes from scores and labels that stay on the device, and the same again
        listing = (1 if sc else 0) | (2 if ts else 0) | (4 if tg else 0) | (8 if nn else 0)
        for _ in range(2):
            dev, doff = device_listing(pred, utf8, boff, listing, fullwidth=not nn)
            assert dev == b"".join(got)
            assert [int(x) for x in doff] == list(np.cumsum([0] + [len(g) for g in got]))


GUARD = 4096   # bytes of 0xA5 behind every array the device variant is given: checked after every call, a failing one included


def guarded(payload: np.ndarray):
    raw = np.full(payload.nbytes + GUARD, 0xA5, np.uint8)
    raw[:payload.nbytes] = payload.view(np.uint8)
    return devmem.put(raw), payload.nbytes


def device_listing(pred, utf8, boff, listing, fullwidth, capacity=None, ooff=None, labels=None):
    """vpt_predict_listing_batch_device after vpt_predict_batch_device on the same workspace.  The output, its offsets, the scores and the
    labels each have GUARD canary bytes behind them; whether the call succeeds or vpt_batch_sync reports an error, the canaries must be
    intact and the scores and labels unchanged -- checked in a `finally`, so an error case verifies them too."""
    S = len(boff) - 1
    true_ooff = api.count_boundaries(utf8, boff)
    nb = int(true_ooff[-1])
    d_text, d_boff, d_true = devmem.put(np.concatenate([utf8, np.zeros(32, np.uint8)])), devmem.put(boff), devmem.put(true_ooff)
    d_ooff = d_true if ooff is None else devmem.put(ooff)
    (d_scores, n_scores), (d_labels, n_labels) = guarded(np.zeros(nb + 16, np.int32)), guarded(np.zeros(nb + 16, np.uint8))
    cap = pred.listing_capacity(len(utf8), nb + S, S, listing) if capacity is None else capacity
    (d_out, n_out), (d_off, n_off) = guarded(np.full(cap, 0xA5, np.uint8)), guarded(np.zeros(S + 1, np.uint64))
    batch = api.DeviceBatch(pred)
    batch.set_flags(_lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0)
    max_bytes = int(np.max(np.diff(boff.astype(np.int64))))
    batch.predict(d_text.ptr, d_boff.ptr, d_true.ptr, S, nb, max_bytes, d_scores.ptr, d_labels.ptr, devmem.stream())
    batch.sync()
    if labels is not None:
        d_labels.set(labels)
    before = d_scores.get().copy(), d_labels.get().copy()
    try:
        batch.predict_listing(d_text.ptr, d_boff.ptr, d_ooff.ptr, S, nb, len(utf8), d_scores.ptr, d_labels.ptr, listing, d_out.ptr, cap, d_off.ptr,
                              devmem.stream())
        batch.sync()
    finally:
        for name, buf, n in (("out", d_out, n_out), ("listing offsets", d_off, n_off), ("scores", d_scores, n_scores), ("labels", d_labels, n_labels)):
            tail = buf.get()[n:]
            assert len(tail) == GUARD and np.all(tail == 0xA5), "written behind the caller's %s" % name
        assert np.array_equal(d_scores.get(), before[0]) and np.array_equal(d_labels.get(), before[1]), "the scores or labels were changed"
    off = d_off.get()[:n_off].view(np.uint64)
    return d_out.get()[:int(off[S])].tobytes(), off


def check_errors():
    L = _lib.load()
    raw = tagged_model()
    pred, plain = predictor(raw, True), predictor(raw, False)
    texts = synth_batch(9, 40, 8, 64)
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    S = len(texts)
    listing = _lib.VPT_LISTING_SCORES | _lib.VPT_LISTING_TAG_SCORES | _lib.VPT_LISTING_TAGGED
    out, offs = pred.predict_listing_packed(utf8, boff, listing, flags=_lib.VPT_FLAG_KYTEA_FULLWIDTH)
    need = len(out)
    # capacity one byte short: the status, and the canaries behind the buffer are intact (host and device variants)
    buf = np.full(need + 64, 0xA5, np.uint8)
    o2 = np.zeros(S + 1, np.uint64)
    st = L.vpt_predict_listing_batch(pred.handle, utf8.ctypes.data, boff.ctypes.data, S, _lib.VPT_FLAG_KYTEA_FULLWIDTH, listing, None, None,
                                     buf.ctypes.data, need - 1, o2.ctypes.data)
    assert st == _lib.VPT_INVALID_ARGUMENT and "text_capacity" in _lib.last_error(), _lib.last_error()
    assert np.all(buf[need - 1:] == 0xA5)
    st = L.vpt_predict_listing_batch(pred.handle, utf8.ctypes.data, boff.ctypes.data, S, _lib.VPT_FLAG_KYTEA_FULLWIDTH, listing, None, None,
                                     buf.ctypes.data, need, o2.ctypes.data)
    assert st == _lib.VPT_OK and bytes(buf[:need]) == bytes(out) and np.all(buf[need:] == 0xA5)
    with pytest.raises(api.VaporettoError, match="text_capacity"):
        device_listing(pred, utf8, boff, listing, True, capacity=need - 1)
    dev, _ = device_listing(pred, utf8, boff, listing, True, capacity=need)
    assert dev == bytes(out)
    # the tag block on a predictor created without predict_tags
    for bit in (_lib.VPT_LISTING_TAG_SCORES, _lib.VPT_LISTING_TAGGED):
        with pytest.raises(api.VaporettoError, match="predict_tags = false"):
            plain.predict_listing_packed(utf8, boff, bit)
    with pytest.raises(api.VaporettoError, match="predict_tags = false"):
        device_listing(plain, utf8, boff, _lib.VPT_LISTING_TAG_SCORES, True)
    # an Unknown label
    ooff = api.count_boundaries(utf8, boff)
    lab = np.ones(int(ooff[-1]), np.uint8)
    lab[5] = 2
    with pytest.raises(api.VaporettoError, match="labels"):
        pred.predict_listing_packed(utf8, boff, listing, scores=np.zeros(len(lab), np.int32), labels=lab)
    # an empty sentence stays an error of the batch entry point
    e_utf8, e_boff = api.pack_texts([b"a", b"", b"b"])
    with pytest.raises(api.VaporettoError, match="at least one character"):
        pred.predict_listing_packed(e_utf8, e_boff, listing)
    # out_offsets that do not match the text (device variant)
    for wrong in (np.concatenate([ooff[:1], ooff[1:] + 1]), np.concatenate([ooff[:3], ooff[3:] - 1])):
        with pytest.raises(api.VaporettoError, match="out_offsets"):
            device_listing(pred, utf8, boff, listing, True, ooff=wrong.astype(np.uint64))


def check_bad_offsets_across_runs():
    """ADVICE.md's kind of input: several front-end runs of fill_tags, every char the end of a tagged token, and an offset that DECREASES at a run
    boundary: an error, and nothing outside the arrays is touched: device_listing checks the canaries behind the output, its offsets, the scores and
    the labels after the failing call as after the good one."""
    m = randmodel.rand_model(5, alphabet=list("うあ"), wc=2, wt=2)
    m.tag_models = [TagModel(token="う", tags=[["a", "b"], ["c"]], char_ngram_model=[TagNgramData("う", [TagWeight(0, [1, 2])])], type_ngram_model=[], bias=[1, 2])]
    raw = api.Model(m).to_vec()
    pred = predictor(raw, True)
    texts = ["う" * 1500] * 4
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    ooff = api.count_boundaries(utf8, boff)
    labels = np.ones(int(ooff[-1]), np.uint8)
    listing = _lib.VPT_LISTING_SCORES | _lib.VPT_LISTING_TAG_SCORES | _lib.VPT_LISTING_TAGGED
    good, _ = device_listing(pred, utf8, boff, listing, False, labels=labels)
    assert good.count(b"\ta:") == 6000
    wrong = np.array([0, 4400, 100, 4500, 5996], dtype=np.uint64)
    with pytest.raises(api.VaporettoError, match="out_offsets"):
        device_listing(pred, utf8, boff, listing, False, ooff=wrong, labels=labels)
