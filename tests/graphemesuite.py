"""The checks of ConcatGraphemeClustersFilter on the device (VPT_FLAG_CONCAT_GRAPHEMES, vpt_concat_graphemes_batch[_device];
vaporetto_amd/csrc/kernels_graphemes.hip), run on the CPU emulator by tests/test_graphemes_emu.py and on the MI355X by
tests/test_graphemes_gpu.py.  The oracle everywhere is the host filter, api.ConcatGraphemeClustersFilter.filter_packed (the `regex` module's
\\X), over the KyteaFullwidthFilter image of the text when the fullwidth flag is set and over the text itself otherwise; every comparison is
exact equality of label arrays or of output bytes.  Nothing here has a tolerance."""
import functools
import os
import random

import numpy as np
import pytest

from tests import devmem, tokenref, tokensuite
from vaporetto_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_MODEL = open(os.path.join(HERE, "golden", "model.bin"), "rb").read()
G = _lib.VPT_FLAG_CONCAT_GRAPHEMES
FW = _lib.VPT_FLAG_KYTEA_FULLWIDTH

EP, EXT, ZWJ, RI, CONS, LINK, PREP, HL, HV, HT = "\U0001f468", "́", "‍", "\U0001f1ef", "क", "्", "؀", "ᄀ", "ᅡ", "ᆨ"


def tile() -> int:
    """The kernel's tile in chars (kGraphemeTile), as the library says it."""
    n = _lib.C.c_uint32(0)
    assert _lib.load().vpt_concat_graphemes_tile(_lib.C.byref(n)) == _lib.VPT_OK
    return int(n.value)


def oracle(texts, ooff, labels, fullwidth):
    want = np.array(labels, dtype=np.uint8, copy=True)
    norm = api.KyteaFullwidthFilter()
    api.ConcatGraphemeClustersFilter().filter_packed([norm.filter(t) for t in texts] if fullwidth else list(texts), ooff, want)
    return want


def pack(texts):
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    return utf8, boff, api.count_boundaries(utf8, boff)


def device_filter(pred, utf8, boff, ooff, labels, fullwidth):
    """vpt_concat_graphemes_batch_device on buffers of the caller's: a guard behind the labels stays as it is."""
    guard = 64
    d_text, d_boff, d_ooff = devmem.put(np.concatenate([utf8, np.zeros(32, np.uint8)])), devmem.put(boff), devmem.put(ooff)
    d_lab = devmem.put(np.concatenate([labels, np.full(guard, 0xA5, np.uint8)]))
    batch = api.DeviceBatch(pred)
    batch.set_flags(FW if fullwidth else 0)
    batch.concat_graphemes(d_text.ptr, d_boff.ptr, d_ooff.ptr, len(boff) - 1, len(labels), d_lab.ptr, devmem.stream())
    batch.sync()
    out = d_lab.get()
    assert np.all(out[len(labels):] == 0xA5)
    return out[:len(labels)]


def check_both_entry_points(pred, texts, labels=None, fullwidth=False, seed=1):
    utf8, boff, ooff = pack(texts)
    nb = int(ooff[-1])
    if labels is None:
        labels = np.random.default_rng(seed).integers(0, 3, nb).astype(np.uint8)
    want = oracle(texts, ooff, labels, fullwidth)
    got = pred.concat_graphemes_packed(utf8, boff, ooff, labels, fullwidth=fullwidth)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, ("host buffers", fullwidth, bad[:8], int(np.searchsorted(ooff, bad[0], side="right")) - 1)
    got_d = device_filter(pred, utf8, boff, ooff, labels, fullwidth)
    assert np.array_equal(got_d, want), ("device buffers", fullwidth)
    # only labels inside clusters change, and only to NotWordBoundary
    changed = got != labels
    assert (got[changed] == 0).all()
    return utf8, boff, ooff, labels, want


def labels_of_tokenized(tok: str) -> np.ndarray:
    """The boundaries of Sentence::from_tokenized for a line without escapes."""
    out, i = [], 0
    while i < len(tok) - 1:
        if tok[i + 1] == " ":
            out.append(1)
            i += 2
        else:
            out.append(0)
            i += 1
    return np.array(out, dtype=np.uint8)


# concat_grapheme_clusters.rs:43-88: (tokenized in, tokenized out)
REFERENCE_KAT = [("‍", "‍"),
                 ("\U0001f468 ‍ \U0001f469 ‍ \U0001f466", "\U0001f468‍\U0001f469‍\U0001f466"),
                 ("\U0001f44f \U0001f3fd", "\U0001f44f\U0001f3fd"),
                 ("これ は 手 \U0001f44f \U0001f3fd で す", "これ は 手 \U0001f44f\U0001f3fd で す")]


def check_reference_kat():
    raw, pred = tokensuite.predictor_for(7, 3, 3)
    texts = [a.replace(" ", "") for a, _ in REFERENCE_KAT]
    utf8, boff, ooff = pack(texts)
    labels = np.concatenate([labels_of_tokenized(a) for a, _ in REFERENCE_KAT])
    want = np.concatenate([labels_of_tokenized(b) for _, b in REFERENCE_KAT])
    assert np.array_equal(pred.concat_graphemes_packed(utf8, boff, ooff, labels), want)
    assert np.array_equal(device_filter(pred, utf8, boff, ooff, labels, False), want)
    # every label set first: what is left are the cluster edges
    ones = np.ones(len(labels), np.uint8)
    got = pred.concat_graphemes_packed(utf8, boff, ooff, ones)
    assert np.array_equal(got, oracle(texts, ooff, ones, False))
    assert [int(x) for x in got] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1]
    # through predict with the flag, on a random model
    for fw in (False, True):
        _, plain, _ = pred.predict_packed(utf8, boff, fullwidth=fw)
        _, flagged, _ = pred.predict_packed(utf8, boff, fullwidth=fw, wsconst=("G",))
        assert np.array_equal(flagged, oracle(texts, ooff, plain, fw))


@functools.lru_cache(maxsize=None)
def class_pool():
    """Members of every GCB, ExtPict and InCB property (the construction of test_cpp_mirror_segments_like_the_regex_module), with members of
    plane 1 (ExtPict, Regional_Indicator) and plane 14 (Extend, Control) among them."""
    import regex
    rng = np.random.default_rng(29)
    pool = []
    props = ["GCB=CR", "GCB=LF", "GCB=Control", "GCB=Extend", "GCB=ZWJ", "GCB=Regional_Indicator", "GCB=Prepend", "GCB=SpacingMark", "GCB=L", "GCB=V",
             "GCB=T", "GCB=LV", "GCB=LVT", "Extended_Pictographic", "InCB=Consonant", "InCB=Linker", "InCB=Extend"]
    every = "".join(chr(c) for c in range(0x110000) if not 0xD800 <= c <= 0xDFFF and c != 0)
    for pr in props:
        members = [m.group() for m in regex.finditer(r"\p{%s}" % pr, every)]
        pool += [members[int(k)] for k in rng.integers(0, len(members), 12)] + members[:2] + members[-2:]
    pool += list("aあ漢 1") + ["\U0001f468", "\U0001f469", "\U0001f466", "\U0001f3fd", "‍", "क", "्", "ष", "؀", "ᄀ", "ᅡ",
                             "ᆨ", "가", "각", "\U000e0100", "\U000e0001", "\U0001f1ef", "\U0001f1f5"]
    assert any(0x10000 <= ord(c) < 0x20000 for c in pool) and any(0xE0000 <= ord(c) < 0xF0000 for c in pool)
    return tuple(pool)


def random_documents(seed, n=300):
    rng = np.random.default_rng(seed)
    pool = class_pool()
    docs = ["".join(pool[int(k)] for k in rng.integers(0, len(pool), int(m))) for m in rng.integers(1, 41, n)]
    # one-char sentences, and state that must not leak across a sentence edge: ZWJ | ExtPict, RI | RI, Consonant Linker | Consonant
    docs += [ZWJ, EP, "a", RI, EXT, EP + ZWJ, EP, EP + EXT + ZWJ, EP + "x", RI, RI, RI + RI + RI, RI, CONS + LINK, CONS, CONS + EXT + LINK + EXT, CONS + LINK + CONS,
             PREP, "a", "\r", "\n", HL, HV]
    return docs


def check_random(seed=5, n=300):
    raw, pred = tokensuite.predictor_for(seed, 3, 3)
    docs = random_documents(seed, n)
    for fw in (False, True):
        check_both_entry_points(pred, docs, fullwidth=fw, seed=seed)
    utf8, boff, ooff = pack(docs)
    ones = np.ones(int(ooff[-1]), np.uint8)
    check_both_entry_points(pred, docs, labels=ones)
    # the leak cases by hand: the first boundary of the sentence behind an open state stays
    for a, b in ((EP + ZWJ, EP + "x"), (RI, RI + "x"), (CONS + LINK, CONS + "x")):
        u, bo, oo = pack([a, b])
        got = pred.concat_graphemes_packed(u, bo, oo, np.ones(int(oo[-1]), np.uint8))
        assert got[int(oo[1])] == 1, (a, b)
        u, bo, oo = pack([a + b])
        got = pred.concat_graphemes_packed(u, bo, oo, np.ones(int(oo[-1]), np.uint8))
        assert got[len(a) - 1] == 0, (a, b)


def run_lengths(full: bool):
    t = tile()
    return [1, 2, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 2 * t + 1, 3 * t + 2] if full else [1, 2, 65, t - 1, t, t + 1, 2 * t + 1]


def edge_patterns(n):
    a = (n - 1) // 2
    return {"pict_joins": EP + EXT * n + ZWJ + EP, "pict_breaks": EP + EXT * n + ZWJ + EXT + EP,
            "ri": RI * n, "ri_behind_extend": EXT + RI * n,
            "conjunct_joins": CONS + EXT * a + LINK + EXT * (n - 1 - a) + CONS, "conjunct_breaks": CONS + EXT * n + CONS,
            "extend": EXT * n, "prepend": PREP * n + "a", "hangul": HL * n + HV + HT * n, "crlf": "\r\n" * n}


def edge_documents(full: bool):
    t = tile()
    docs = []
    for n in run_lengths(full):
        for name, pat in edge_patterns(n).items():
            for off in (0, 1, t - 2):
                docs.append("か" * off + pat + "かな")
    return docs


def check_edges(full: bool, seed=3):
    """One document per pattern, run length and place behind plain kana, all in one batch: the documents start anywhere in their tiles, the
    patterns straddle the cuts at 0, 1 and T - 2 chars into a document as well."""
    raw, pred = tokensuite.predictor_for(seed, 2, 2)
    docs = edge_documents(full)
    utf8, boff, ooff = pack(docs)
    ones = np.ones(int(ooff[-1]), np.uint8)
    _, _, _, _, want = check_both_entry_points(pred, docs, labels=ones)
    # what the patterns are there to show, on the oracle's answer (so that the cases stay what they are called)
    k = 0
    for n in run_lengths(full):
        for name, pat in edge_patterns(n).items():
            for off in (0, 1, tile() - 2):
                lab = want[int(ooff[k]):int(ooff[k + 1])]
                body = lab[off:off + len(pat) - 1]
                if name in ("pict_joins", "conjunct_joins", "extend"):
                    assert not body.any(), (name, n, off)
                elif name in ("pict_breaks", "conjunct_breaks"):
                    assert body[-1] == 1 and not body[:-1].any(), (name, n, off)
                elif name == "ri":
                    assert [int(x) for x in body] == [0 if j % 2 == 0 else 1 for j in range(n - 1)], (name, n, off)
                elif name == "crlf":
                    assert [int(x) for x in body] == [0 if j % 2 == 0 else 1 for j in range(2 * n - 1)], (name, n, off)
                k += 1
    check_both_entry_points(pred, docs, seed=seed)
    # ... and behind the scoring launch, the documents in another order
    order = list(range(len(docs)))
    random.Random(seed).shuffle(order)
    docs2 = [docs[i] for i in order[:len(order) // 2]]
    u, bo, oo = pack(docs2)
    _, plain, _ = pred.predict_packed(u, bo, fullwidth=True, wsconst=(4,))
    _, flagged, _ = pred.predict_packed(u, bo, fullwidth=True, wsconst=(4, "G"))
    assert np.array_equal(flagged, oracle(docs2, oo, plain, True))


FULLWIDTH_LINES = ["abc ｶﾞｷﾞｸﾞ ﾊﾟﾋﾟ 123", "ｶﾞ", "ﾞﾟ", "ＡＢＣ１２３　ｱｲｳ", "áｶﾞ\U0001f44f\U0001f3fdﾊﾟ!", "\U0001f468‍\U0001f469ﾞx", "ｶ゙ｷ゛", "x\r\ny ﾞ", "～ｰ-ﾞ",
                   "\U0001f1ef\U0001f1f5ﾟ\U0001f1ef", "(ﾟДﾟ)", "ﾊﾞｲｵﾘﾝ\U0001f3bb️"]


def check_fullwidth(seed=9):
    raw, pred = tokensuite.predictor_for(seed, 3, 2)
    rng = random.Random(seed)
    alpha = list("abcXYZ019 ｱｲｶｷﾊﾋﾞﾟＡｂ１あカ漢ー") + ["\U0001f44f", "\U0001f3fd", "\U0001f468", ZWJ, EXT, "゙", "️", RI]
    lines = FULLWIDTH_LINES + ["".join(rng.choice(alpha) for _ in range(rng.randint(1, 30))) for _ in range(200)]
    utf8, boff, ooff = pack(lines)
    ones = np.ones(int(ooff[-1]), np.uint8)
    for fw in (False, True):
        check_both_entry_points(pred, lines, fullwidth=fw, seed=seed)
        check_both_entry_points(pred, lines, labels=ones, fullwidth=fw)
        _, plain, _ = pred.predict_packed(utf8, boff, fullwidth=fw)
        _, flagged, _ = pred.predict_packed(utf8, boff, fullwidth=fw, wsconst=("G",))
        assert np.array_equal(flagged, oracle(lines, ooff, plain, fw)), fw


def pipeline_documents(seed):
    docs = [d for d in random_documents(seed, 200)]
    return docs + ["a\r\nb", "x\n\ny", "\r\n", "あ\r\n\r\nい", "123456円\U0001f90c\U0001f3ff", "1\r\n2 3\n\n4"]


def check_pipelines(seed, wc, wt):
    """One call with the flag against the composition of the existing calls around the host filter."""
    raw, pred = tokensuite.predictor_for(seed, wc, wt)
    docs = pipeline_documents(seed)
    utf8, boff, ooff = pack(docs)
    # tokenize
    for fw in (True, False):
        _, labels, _ = pred.predict_packed(utf8, boff, fullwidth=fw, wsconst=(5,), split_linebreaks=True)
        labels = oracle(docs, ooff, labels, fw)
        text, toff = pred.write_tokenized_packed(utf8, boff, ooff, labels)
        want = [bytes(text)[int(toff[i]):int(toff[i + 1])].decode("utf-8") for i in range(len(docs))]
        assert pred.tokenize(docs, wsconst=("G", 5), split_linebreaks=True, fullwidth=fw) == want, fw
    # the token stream: "G" anywhere in the string, empty documents in the batch
    with_empty = ["", ""] + docs[:50] + [""] + docs[50:] + [""]
    e_utf8, e_boff = api.pack_texts([t.encode("utf-8") for t in with_empty])
    _, labels, _ = pred.predict_packed(utf8, boff, fullwidth=True, wsconst=(1,), split_linebreaks=True, linebreaks_first=True)
    labels = oracle(docs, ooff, labels, True)
    k_toff, k_ends = pred.token_spans_packed(utf8, boff, ooff, labels)
    counts = np.zeros(len(with_empty), np.uint64)
    counts[[i for i, t in enumerate(with_empty) if t]] = np.diff(k_toff)
    want_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    for ws in ("GD", "DG"):
        toff, ends = pred.token_stream_packed(e_utf8, e_boff, ws)
        assert np.array_equal(toff, want_off) and np.array_equal(ends, k_ends), ws
    want_tokens = [tokenref.tokens_from_ends(t, e) for t, e in zip(with_empty, tokenref.ends_batch(raw, with_empty, "DG"))]
    tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "GD", device=0)
    assert [[list(t._key()) for t in d] for d in tok.token_stream_batch(with_empty)] == want_tokens
    # the listing with scores
    sc, labels, _ = pred.predict_packed(utf8, boff, fullwidth=True)
    labels = oracle(docs, ooff, labels, True)
    out, offs = pred.predict_listing_packed(utf8, boff, _lib.VPT_LISTING_SCORES, flags=FW, scores=sc, labels=labels)
    want = [bytes(out)[int(offs[i]):int(offs[i + 1])] for i in range(len(docs))]
    assert pred.predict_listing(docs, scores=True, wsconst=("G",)) == want


def check_evaluate(seed=4):
    """evaluate(.., wsconst=("G",)): the counters of the one call against parse, predict, the host filter and the compare, call by call."""
    raw, pred = tokensuite.predictor_for(seed, 3, 3)
    rng = random.Random(seed)
    docs = [d for d in random_documents(seed, 150) if not any(c in d for c in " \\/\r\n") and not any(api.KyteaFullwidthFilter().filter(c) in " \\/" for c in d)]
    lines = []
    for d in docs:   # a tokenization of the document at random places
        lines.append("".join(c + (" " if i + 1 < len(d) and rng.random() < 0.4 else "") for i, c in enumerate(d)))
    for no_norm in (False, True):
        got = pred.evaluate(lines, wsconst=("G",), no_norm=no_norm)
        h = api.parse_tokenized_host([ln.encode("utf-8") for ln in lines])
        texts = [bytes(h["raw"][int(h["raw_offsets"][i]):int(h["raw_offsets"][i + 1])]).decode("utf-8") for i in range(len(lines))]
        assert texts == docs
        _, sys_l, ooff = pred.predict_packed(h["raw"], h["raw_offsets"], fullwidth=not no_norm)
        assert np.array_equal(ooff, h["out_offsets"])
        sys_l = oracle(texts, ooff, sys_l, not no_norm)
        pad = lambda a: np.concatenate([a, np.zeros(8, a.dtype)])
        d = {k: devmem.put(pad(v)) for k, v in h.items()}
        d_sys, d_counts = devmem.put(pad(sys_l)), devmem.zeros(8, np.uint64)
        batch = api.DeviceBatch(pred)
        mode = _lib.VPT_EVAL_TAGS_GOLD if no_norm else _lib.VPT_EVAL_TAGS_NONE
        st = _lib.load().vpt_evaluate_labels_batch_device(pred.handle, batch._h, d["out_offsets"].ptr, len(lines), d["labels"].ptr, d["n_tags"].ptr, d["tag_index"].ptr,
                                                          d["span_offsets"].ptr, d["tag_bytes"].ptr, d_sys.ptr, mode, d_counts.ptr, devmem.stream())
        assert st == _lib.VPT_OK, _lib.last_error()
        batch.sync()
        want = api.evaluation_result(d_counts.get())
        keys = ("tp", "tn", "fp", "fn", "n_sys", "n_ref", "n_cor", "n_sentences")
        assert [got[k] for k in keys] == [want[k] for k in keys], no_norm
        plain = pred.evaluate(lines, no_norm=no_norm)
        assert plain["n_sys"] > got["n_sys"]   # (the filter joined something)


def check_tagged(seed=6):
    """On the fixture's tag models: fill_tags sees the filtered labels."""
    pred = api.Predictor(api.Model.read_slice(GOLDEN_MODEL)[0], True, device=0)
    assert pred.n_tags() > 0
    rng = random.Random(seed)
    alpha = list("まぁ社長は火星猫だ良いろう人地球") + [EXT, ZWJ, "\U0001f44f", "\U0001f3fd", "゙", RI]
    docs = ["まぁ社長は火星猫だ", "火星゙猫", "まぁ́良いだろう", "火星猫\U0001f44f\U0001f3fdだ"] + ["".join(rng.choice(alpha) for _ in range(rng.randint(1, 40))) for _ in range(150)]
    utf8, boff, ooff = pack(docs)
    for fw in (True, False):
        _, labels, _ = pred.predict_packed(utf8, boff, fullwidth=fw, wsconst=(5,), split_linebreaks=True)
        filtered = oracle(docs, ooff, labels, fw)
        assert not np.array_equal(filtered, labels)
        text, toff = pred.write_tokenized_packed(utf8, boff, ooff, filtered, tagged=True, fullwidth=fw)
        want = [bytes(text)[int(toff[i]):int(toff[i + 1])].decode("utf-8") for i in range(len(docs))]
        got = pred.tokenize(docs, wsconst=("G", 5), split_linebreaks=True, tagged=True, fullwidth=fw)
        assert got == want, fw
        assert any("/" in g for g in got)


G_KAT = [c for c in tokensuite.KAT["cases"] if "G" in c["wsconst"]]


def check_kat_cabi(case):
    """The adapter's known answers with "G", through vpt_token_stream_batch."""
    pred = api.Predictor(api.Model.read_slice(tokensuite.KAT_MODEL)[0], False, device=0)
    utf8, boff = api.pack_texts([case["text"].encode("utf-8")])
    toff, ends = pred.token_stream_packed(utf8, boff, case["wsconst"])
    assert tokenref.tokens_from_ends(case["text"], [int(e) for e in ends]) == case["tokens"]
    assert int(toff[1]) == len(case["tokens"])


def _expect(status, text):
    assert status == _lib.VPT_INVALID_ARGUMENT, status
    assert text in _lib.last_error(), _lib.last_error()


def check_errors(seed=5):
    L = _lib.load()
    raw, pred = tokensuite.predictor_for(seed, 3, 3)
    texts = ["あい́a", "漢\U0001f44f\U0001f3fd", "09"]
    utf8, boff, ooff = pack(texts)
    nb = int(ooff[-1])
    scores, labels = np.zeros(nb, np.int32), np.zeros(nb, np.uint8)
    bad = 1 << 10
    h = pred.handle
    a = (utf8.ctypes.data, boff.ctypes.data, len(texts))
    out, offs = np.zeros(4096, np.uint8), np.zeros(len(texts) + 1, np.uint64)
    ends = np.zeros(64, np.uint32)
    counts = np.zeros(8, np.uint64)
    handles = (_lib.C.c_void_p * 1)(h)
    for flags in (bad, bad | G):
        _expect(L.vpt_predict_batch_flags(h, *a, scores.ctypes.data, labels.ctypes.data, ooff.ctypes.data, flags), "flags: unknown bit")
        _expect(L.vpt_tokenize_batch(h, *a, flags, 0, out.ctypes.data, len(out), offs.ctypes.data), "flags: unknown bit")
        _expect(L.vpt_predict_listing_batch(h, *a, flags, 1, None, None, out.ctypes.data, len(out), offs.ctypes.data), "flags: unknown bit")
        _expect(L.vpt_evaluate_batch(h, *a, flags, 0, counts.ctypes.data), "flags: unknown bits")
        _expect(L.vpt_predict_batch_sharded(handles, 1, utf8.ctypes.data, boff.ctypes.data, len(texts), scores.ctypes.data, labels.ctypes.data, ooff.ctypes.data, flags),
                "flags: unknown bit")
        _expect(L.vpt_token_stream_batch(h, *a, flags, offs.ctypes.data, ends.ctypes.data, 64), "Could not parse a wsconst value")
        batch = api.DeviceBatch(pred)
        with pytest.raises(api.VaporettoError, match="flags: unknown bit"):
            batch.set_flags(flags)
        batch.set_flags(G | FW | _lib.VPT_FLAG_LINEBREAKS_FIRST | _lib.VPT_FLAG_SPLIT_LINEBREAKS)
    _expect(L.vpt_token_stream_batch(h, *a, 1 << 7, offs.ctypes.data, ends.ctypes.data, 64), "Could not parse a wsconst value")
    _expect(L.vpt_token_stream_batch(h, *a, G | (1 << 8), offs.ctypes.data, ends.ctypes.data, 64), "Could not parse a wsconst value")
    # the caller-labels entry point
    for flags in (G, 1 << 7, 2, bad):
        _expect(L.vpt_concat_graphemes_batch(h, *a, ooff.ctypes.data, flags, labels.ctypes.data), "flags: unknown bit")
    _expect(L.vpt_concat_graphemes_batch(None, *a, ooff.ctypes.data, 0, labels.ctypes.data), "predictor: must not be NULL")
    _expect(L.vpt_concat_graphemes_batch(h, None, boff.ctypes.data, len(texts), ooff.ctypes.data, 0, labels.ctypes.data), "NULL argument")
    _expect(L.vpt_concat_graphemes_batch(h, utf8.ctypes.data, None, len(texts), ooff.ctypes.data, 0, labels.ctypes.data), "NULL argument")
    _expect(L.vpt_concat_graphemes_batch(h, *a, None, 0, labels.ctypes.data), "NULL argument")
    _expect(L.vpt_concat_graphemes_batch(h, *a, ooff.ctypes.data, 0, None), "labels: must not be NULL")
    nul_utf8, nul_boff = api.pack_texts(["あ́".encode(), "x\0ý".encode()])
    nul_ooff = np.array([0, 1, 4], np.uint64)   # (vpt_count_boundaries rejects the text itself: the offsets by hand)
    with pytest.raises(api.VaporettoError, match="must not contain NULL"):
        pred.concat_graphemes_packed(nul_utf8, nul_boff, nul_ooff, np.ones(4, np.uint8))
    wrong = ooff.copy()
    wrong[1] += 1
    with pytest.raises(api.VaporettoError, match="out_offsets"):
        pred.concat_graphemes_packed(utf8, boff, wrong, np.ones(int(wrong[-1]) + 4, np.uint8))
    batch = api.DeviceBatch(pred)
    other = tokensuite.predictor_for(seed + 1, 2, 2)[1]
    _expect(L.vpt_concat_graphemes_batch_device(other.handle, batch._h, 1, 1, 1, 1, 1, 1, 0), "batch: does not belong to this predictor")
    _expect(L.vpt_concat_graphemes_batch_device(h, batch._h, None, 1, 1, 1, 1, 1, 0), "NULL device pointer")
    # the flag clear: the labels are the parent's -- the sign of the oracle's scores and the other label filters, nothing else
    docs = random_documents(seed, 100)
    want = tokenref.ends_batch(raw, docs, "D")
    u, bo = api.pack_texts([t.encode("utf-8") for t in docs])
    toff, got = pred.token_stream_packed(u, bo, "D")
    w_off, w_ends = tokenref.csr(want)
    assert np.array_equal(toff, w_off) and np.array_equal(got, w_ends)
    want_g = tokenref.csr(tokenref.ends_batch(raw, docs, "DG"))[1]
    assert not np.array_equal(w_ends, want_g)   # (and the documents are such that the flag matters)
