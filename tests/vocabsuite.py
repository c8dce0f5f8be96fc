"""The checks of the vocabulary ids of the token stream (vpt_vocab_*, vpt_token_ids_batch_device, vpt_token_stream_ids_batch; kernels_vocab.hip)
against the restatement of tests/vocabref.py, run on the CPU emulator by tests/test_vocab_emu.py and on the MI355X by tests/test_vocab_gpu.py;
every comparison is exact.

    python -m tests.vocabsuite --emu-hostile      the hostile CSRs on the emulator, in a child process (hipemu checks its red zones when the
                                                  workspace goes)

The id pass takes vpt_vocab_tile tokens a workgroup, a lane per token; the CSRs built below put tokens, document edges and runs of empty documents
on each side of those edges."""
import os
import random
import sys

import numpy as np

from tests import devmem, patterntagsuite, tagoffsetsuite, tokentagsuite, vocabref
from vaporetto_amd import _lib, api

SENTINEL = 0x5A5A5A5A
FW = _lib.VPT_FLAG_KYTEA_FULLWIDTH
G = tagoffsetsuite.Guarded
CSR_ERROR = "token_offsets / token_starts / token_ends"
# 1-, 2-, 3- and 4-byte chars; halfwidth and fullwidth forms of the same words; "う" has a tag model (the stop filter drops it)
WORDS = ["漢字", "あい", "う", "09", "０９", "AB", "ＡＢ", "é", "ñoé", "𠮷野", "a𠮷", "🤌", "B0", "カ", "A", "い"]

_PRED = []


def predictor():
    if not _PRED:
        _PRED.append(patterntagsuite.predictor_of(patterntagsuite.tagged_model()))
    return _PRED[0]


def csr_of(token_lists):
    """documents as lists of tokens -> (the documents' bytes, token_offsets, starts, ends)"""
    raws, toff, starts, ends = [], [0], [], []
    for toks in token_lists:
        at = 0
        for t in toks:
            starts.append(at)
            at += len(t.encode("utf-8"))
            ends.append(at)
        raws.append("".join(toks).encode("utf-8"))
        toff.append(len(ends))
    return raws, np.array(toff, np.uint64), np.array(starts, np.uint32), np.array(ends, np.uint32)


def run_ids(vocab, raws, toff, starts, ends, flags=0, cap_in=None, batch=None, pred=None):
    """vpt_token_ids_batch_device on guarded arrays of exactly the sizes the call is told -> the ids [capacity_in] or the sync's message"""
    pred = pred or predictor()
    batch = batch or api.DeviceBatch(pred)
    utf8, boff = api.pack_texts(raws)
    cap = len(ends) if cap_in is None else cap_in
    I = {"text": G(utf8 if len(utf8) else np.zeros(1, np.uint8)), "boff": G(boff), "toff": G(np.asarray(toff, np.uint64)),
         "ends": G(np.asarray(ends, np.uint32)[:max(cap, 1)] if len(ends) else np.zeros(1, np.uint32))}
    if starts is not None:
        I["starts"] = G(np.asarray(starts, np.uint32)[:max(cap, 1)] if len(starts) else np.zeros(1, np.uint32))
    out = G(np.full(max(cap, 1), SENTINEL, np.int32))
    batch.token_ids(vocab, I["text"].ptr, I["boff"].ptr, len(raws), I["toff"].ptr, I["starts"].ptr if starts is not None else 0, I["ends"].ptr, cap,
                    out.ptr, flags, devmem.stream())
    try:
        batch.sync()
        raised = None
    except api.VaporettoError as e:
        raised = str(e)
    assert not [k for k, a in I.items() if not a.guards_intact()] and out.guards_intact(), "guard words overwritten"
    got = out.get()
    n = min(int(np.asarray(toff)[-1]), cap) if raised is None else cap
    assert (got[max(n, 0):] == SENTINEL).all() if raised is None else True   # nothing behind the batch's tokens
    return raised if raised is not None else got[:n]


def check_csr(keys, token_lists, unk=-1, flags=0, both=True, batch=None):
    """ids of a hand-built CSR against the restatement, through starts == NULL and through explicit starts; twice"""
    pred = predictor()
    vocab = api.Vocabulary(pred, keys, unk)
    table = {s: k for k, s in enumerate(keys)}
    raws, toff, starts, ends = csr_of(token_lists)
    want = vocabref.ids_from_csr(raws, toff, None, ends, table, unk, flags == FW)
    for st in ((None, starts) if both else (None,)):
        got = run_ids(vocab, raws, toff, st, ends, flags, batch=batch)
        assert isinstance(got, np.ndarray), got
        assert np.array_equal(got, want), (st is None, [k for k in range(len(want)) if got[k] != want[k]][:8])
        again = run_ids(vocab, raws, toff, st, ends, flags, batch=batch)
        assert again.tobytes() == got.tobytes()
    return want


def check_random(seed, fullwidth):
    """~200 documents of 1-12 tokens through the real span kernel (starts == NULL) and the real stop filter; the vocabulary a random half of
    the distinct tokens."""
    pred = predictor()
    rng = random.Random(seed)
    docs = [[rng.choice(WORDS) for _ in range(rng.randint(1, 12))] for _ in range(200)]
    docs[3], docs[77], docs[199] = ["う"], ["う", "う"], ["う"]   # documents the stop filter leaves without a token
    distinct = sorted({t for d in docs for t in d})
    keys = rng.sample(distinct, len(distinct) // 2)
    unk, flags = -3, FW if fullwidth else 0
    table = {s: k for k, s in enumerate(keys)}
    vocab = api.Vocabulary(pred, keys, unk)
    texts, labels = tokentagsuite.labels_of(docs)
    raws = [t.encode("utf-8") for t in texts]
    A = tokentagsuite.Arrays(pred, texts, labels)
    batch = api.DeviceBatch(pred)
    A.fill(batch)
    A.spans(batch)
    ids = G(np.full(A.cap, SENTINEL, np.int32))
    batch.token_ids(vocab, A.d_text.ptr, A.d_boff.ptr, A.S, A.d_toff.ptr, 0, A.d_ends.ptr, A.cap, ids.ptr, flags, devmem.stream())
    # ... and on what the stop filter leaves: "う"'s tag models give p or q in slot 0
    stop = api.TagStopFilter(pred, [(0, "p"), (0, "q")])
    O = {"offsets": G(np.full(A.S + 1, 7, np.uint64)), "starts": G(np.full(A.cap, SENTINEL, np.uint32)), "ends": G(np.full(A.cap, SENTINEL, np.uint32)),
         "positions": G(np.full(A.cap, SENTINEL, np.uint32)), "tags": G(np.full(A.cap * max(A.nt, 1), SENTINEL, np.int32))}
    batch.token_filter(stop, A.d_toff.ptr, A.d_ends.ptr, A.d_tags.ptr, A.S, A.n_tok, O["offsets"].ptr, O["starts"].ptr, O["ends"].ptr, O["positions"].ptr,
                       O["tags"].ptr, A.cap, devmem.stream())
    fids = G(np.full(A.cap, SENTINEL, np.int32))
    batch.token_ids(vocab, A.d_text.ptr, A.d_boff.ptr, A.S, O["offsets"].ptr, O["starts"].ptr, O["ends"].ptr, A.cap, fids.ptr, flags, devmem.stream())
    batch.sync()
    assert ids.guards_intact() and fids.guards_intact() and A.guards_intact()
    toff, ends = A.d_toff.get(A.S + 1), A.d_ends.get(A.n_tok)
    flat = [t for d in docs for t in d]
    norm = api.KyteaFullwidthFilter()
    want = np.array([table.get(norm.filter(t) if fullwidth else t, unk) for t in flat], np.int32)
    assert np.array_equal(vocabref.ids_from_csr(raws, toff, None, ends, table, unk, fullwidth), want)   # (the restatement is the dict lookup)
    assert np.array_equal(ids.get(A.n_tok), want)
    assert (want != unk).any() and (want == unk).any()
    if fullwidth:   # a halfwidth token found under its fullwidth key, and a halfwidth key that no longer matches
        assert any(t == "AB" and "ＡＢ" in table and w == table["ＡＢ"] for t, w in zip(flat, want)) or "ＡＢ" not in table
    f_off, kept = O["offsets"].get(), int(O["offsets"].get()[-1])
    f_starts, f_ends = O["starts"].get(kept), O["ends"].get(kept)
    assert 0 < kept < A.n_tok and any(f_off[i] == f_off[i + 1] for i in range(A.S))
    assert np.array_equal(fids.get(kept), vocabref.ids_from_csr(raws, f_off, f_starts, f_ends, table, unk, fullwidth))
    assert np.array_equal(fids.get(kept), want[np.array([t != "う" for t in flat])])
    assert (fids.get()[kept:] == SENTINEL).all()


def check_edges():
    """Tokens, document edges and runs of 0, 1 and 3 empty documents on both sides of every multiple of the tile, up to 3 tiles; batches of
    exactly 1, tile and tile + 1 tokens; a first and a last document that are empty."""
    tile = api.Vocabulary.tile()
    assert tile >= 64
    keys = ["漢字", "う", "ＡＢ", "𠮷野", "é", "A"]
    n = 3 * tile + 2
    flat = [WORDS[(7 * k + k // 5) % len(WORDS)] for k in range(n)]
    batch = api.DeviceBatch(predictor())
    for empties in (0, 1, 3):
        cuts = sorted({m * tile + d for m in (1, 2, 3) for d in (-1, 0, 1)})
        docs, a = [[]] * empties, 0   # (a first document that is empty)
        for c in cuts + [n]:
            docs.append(flat[a:c])
            docs += [[]] * empties
            a = c
        assert sum(len(d) for d in docs) == n and (empties == 0 or (docs[0] == [] and docs[-1] == []))
        check_csr(keys, docs, batch=batch)
    # one long document over all the tiles; a document per token: more owners than the tile's slice holds in LDS
    check_csr(keys, [flat], batch=batch)
    check_csr(keys, [[t] for t in flat] + [[], []], batch=batch)
    check_csr(keys, [[]] + [[t] for t in flat[:tile]] + [[]] * 700 + [[t] for t in flat[tile:2 * tile + 1]], batch=batch)   # a run of empty documents longer than the slice
    for count in (1, tile, tile + 1):
        check_csr(keys, [flat[:count]], batch=batch)
        check_csr(keys, [[], flat[:count - 1], [], [], [], flat[count - 1:count], []], batch=batch)
    check_csr(keys, [[], [], []], batch=batch)   # no token at all


def check_length_bound():
    keys = ["あいうえ", "あいうえお", "AB"]   # max_surface_chars == 5
    pred = predictor()
    assert api.Vocabulary(pred, keys).info()["max_surface_chars"] == 5
    long_token = "あ" * 5000
    docs = [["あいうえ", "あいうえお", "あいうえおか", "AB"], [long_token], ["ABABAB", "A" * 20, "A" * 21, "あいうえお", long_token, "AB"]]
    want = check_csr(keys, docs, unk=-9)
    assert list(want) == [0, 1, -9, 2, -9, -9, -9, -9, 1, -9, 2]


def check_probing():
    """Three keys with one home slot, and a chain that wraps around the table's end (both found by search in the restatement)."""
    for home_slot in (15, 6):
        three = vocabref.find_same_home(8, home_slot, 3)
        keys = three + ["x1", "漢字", "う", "AB", "𠮷"]
        bits, slots, where = vocabref.place(keys)
        assert bits == 4 and [w[0] for w in where[:3]] == [home_slot] * 3 and [w[2] for w in where[:3]] == [1, 2, 3]
        if home_slot == 15:
            assert [w[1] for w in where[:3]] == [15, 0, 1]
        info = api.Vocabulary(predictor(), keys).info()
        assert info == {"n_keys": 8, "n_slots": 16, "max_surface_chars": max(len(k) for k in keys)}
        others = vocabref.find_same_home(8, home_slot, 6, seed=99)   # more surfaces of that home slot: mostly no keys
        want = check_csr(keys, [keys[::-1], others, three + others[:2]])
        assert list(want[:8]) == list(range(7, -1, -1))


def check_verification():
    """A token that is no key but has a key's length, fingerprint and home slot: only the code points tell them apart."""
    twins = vocabref.find_fingerprint_twins(3)
    assert twins is not None
    a, b = twins
    keys = ["x1", a, "漢字", "う"]
    bits, slots, where = vocabref.place(keys)
    assert bits == 3 and vocabref.fingerprint(a) == vocabref.fingerprint(b) and vocabref.home(b, bits) == where[1][0] and len(a) == len(b)
    want = check_csr(keys, [[a, b, "x1"], [b], [b, a]], unk=-5)
    assert list(want) == [1, -5, 0, -5, -5, 1]


def check_handle():
    pred = predictor()
    for unk in (-1, 0, -(1 << 31)):
        want = check_csr(["漢字", "う"], [["う", "A", "漢字", "字"]], unk=unk, both=False)
        assert list(want) == [1, unk, 0, unk]
    assert list(check_csr(["う"], [["う", "A"], ["う"]], both=False)) == [0, -1, 0]
    big = ["w%d" % k for k in range(70000)]
    v = api.Vocabulary(pred, big, -2)
    assert v.info() == {"n_keys": 70000, "n_slots": 1 << 18, "max_surface_chars": 6} and v.unk_id == -2
    for k in (0, 1, 9999, 69999):
        assert v.surface(k) == big[k]
    try:
        v.surface(70000)
        assert False
    except api.VaporettoError as e:
        assert "no such vocabulary entry" in str(e)
    raws, toff, starts, ends = csr_of([["w0", "w69999", "w70000", "w", "w31415"], ["w123", "x"]])
    assert list(run_ids(v, raws, toff, None, ends)) == [0, 69999, -2, -2, 31415, 123, -2]
    small = api.Vocabulary(pred, ["漢字", "é𠮷"])
    assert [small.surface(0), small.surface(1)] == ["漢字", "é𠮷"] and small.info()["n_slots"] == 4


def _expect(fn, pattern):
    import re
    try:
        fn()
    except api.VaporettoError as e:
        assert re.search(pattern, str(e)), str(e)
        return
    assert False, "no error, wanted " + pattern


def check_errors():
    pred = predictor()
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    _expect(lambda: api.Vocabulary(pred, ["a", "", ""]), r"vocab: a surface must contain at least one character \(entry 1\)")
    _expect(lambda: api.Vocabulary(pred, ["a", "b", "a\0b", ""]), r"vocab: a surface must not contain NULL \(entry 2\)")
    _expect(lambda: api.Vocabulary(pred, ["a", "漢字", "b", "漢字", "a"]), r"vocab: a surface must not repeat an earlier entry's \(entry 3\)")
    _expect(lambda: api.Vocabulary(pred, [b"ok", b"\xe3\x81", b"\xff"]), r"vocab: a surface is not valid UTF-8 \(entry 1\)")
    _expect(lambda: api.Vocabulary(pred, [b"ok", b"\xed\xa0\x80"]), r"vocab: a surface is not valid UTF-8 \(entry 1\)")
    vocab = api.Vocabulary(pred, ["漢字"])
    raws, toff, starts, ends = csr_of([["漢字"]])
    _expect(lambda: run_ids(vocab, raws, toff, None, ends, pred=other), "vocab: does not belong to this predictor")
    for bad in (2, FW | 4, 1 << 7):
        _expect(lambda: run_ids(vocab, raws, toff, None, ends, flags=bad), "flags: unknown bit")
    utf8, boff = api.pack_texts(raws)
    _expect(lambda: other.token_ids_packed(utf8, boff, vocab), "vocab: does not belong to this predictor")
    _expect(lambda: pred.token_ids_packed(utf8, boff, None), "vocab: must not be NULL")
    _expect(lambda: pred.token_ids_packed(utf8, boff, vocab, "X"), "Could not parse a wsconst value")
    _expect(lambda: patterntagsuite.predictor_of(patterntagsuite.tagged_model(), predict_tags=False).token_ids_packed(utf8, boff, vocab),
            "vocab: does not belong")
    plain = patterntagsuite.predictor_of(patterntagsuite.tagged_model(), predict_tags=False)
    _expect(lambda: plain.token_ids_packed(utf8, boff, api.Vocabulary(plain, ["漢字"]), tags=True), "predict_tags = false")


def _device_ids(pred, vocab, raws, toff, starts, ends, flags):
    got = run_ids(vocab, raws, toff, starts, ends, flags, pred=pred)
    assert isinstance(got, np.ndarray), got
    return got


def check_pipeline(seed=31):
    """vpt_token_stream_ids_batch against the existing stream calls with the device id pass behind them, step by step; one chunk and several."""
    m = patterntagsuite.tagged_model(seed)
    raw = api.Model(m).to_vec()
    pred = api.Predictor(api.Model.read_slice(raw)[0], True, device=0)
    texts = tokentagsuite.stream_texts(seed) + ["AB０９ＡＢ09", "ＡＢ"]
    raws = [t.encode("utf-8") for t in texts]
    utf8, boff = api.pack_texts(raws)
    toff0, ends0 = pred.token_stream_packed(utf8, boff, "DR")
    surfaces = []
    for i, r in enumerate(raws):
        a = 0
        for k in range(int(toff0[i]), int(toff0[i + 1])):
            surfaces.append(r[a:int(ends0[k])].decode("utf-8"))
            a = int(ends0[k])
    norm = api.KyteaFullwidthFilter()
    distinct = sorted({s for s in surfaces} | {norm.filter(s) for s in surfaces})
    keys = [s for k, s in enumerate(distinct) if k % 2 == 0 and len(s) <= 12]
    table = {s: k for k, s in enumerate(keys)}
    vocab = api.Vocabulary(pred, keys, -4)
    tagger = api.PatternMatchTagger(tokentagsuite.STREAM_RULES)
    stop = api.TagStopFilter(pred, tokentagsuite.STOP_SETS["both"], tagger)
    results = {}
    for normalize in (True, False):
        flags = FW if normalize else 0
        # the untagged route: vpt_token_stream_batch's arrays, trivial starts and positions, no tags
        toff, starts, ends, pos, tags, ids = pred.token_ids_packed(utf8, boff, vocab, "DR", normalize)
        assert tags is None and np.array_equal(toff, toff0) and np.array_equal(ends, ends0)
        for i in range(len(texts)):
            a, b = int(toff[i]), int(toff[i + 1])
            assert list(pos[a:b]) == list(range(b - a)) and list(starts[a:b]) == ([0] + list(ends[a:b - 1]) if b > a else [])
        assert np.array_equal(ids, _device_ids(pred, vocab, raws, toff, None, ends, flags))
        assert np.array_equal(ids, vocabref.ids_from_csr(raws, toff, starts, ends, table, -4, normalize))
        assert (ids != -4).any() and (ids == -4).any()
        results[("plain", normalize)] = (toff, starts, ends, pos, ids)
        # the tagged route, with the tagger and the stop set
        want5 = pred.token_stream_tagged_packed(utf8, boff, "DR", tagger, stop)
        got = pred.token_ids_packed(utf8, boff, vocab, "DR", normalize, tagger, stop)
        assert all(np.array_equal(x, y) for x, y in zip(got[:5], want5))
        assert np.array_equal(got[5], _device_ids(pred, vocab, raws, want5[0], want5[1], want5[2], flags))
        assert np.array_equal(got[5], vocabref.ids_from_csr(raws, want5[0], want5[1], want5[2], table, -4, normalize))
        assert len(got[5]) < len(ids)
        results[("tagged", normalize)] = got
        # tags asked for, nothing stopped
        want5 = pred.token_stream_tagged_packed(utf8, boff, "DR")
        got = pred.token_ids_packed(utf8, boff, vocab, "DR", normalize, tags=True)
        assert all(np.array_equal(x, y) for x, y in zip(got[:5], want5)) and np.array_equal(got[5], ids)
    assert not np.array_equal(results[("plain", True)][4], results[("plain", False)][4])   # halfwidth tokens change their id
    # the result does not depend on the chunks: at least three
    os.environ["VPT_TOKENIZE_CHUNK_BYTES"] = str(max(len(utf8) // 4, 1))
    try:
        cut = api.Predictor(api.Model.read_slice(raw)[0], True, device=0)
    finally:
        os.environ.pop("VPT_TOKENIZE_CHUNK_BYTES", None)
    vocab2, tg2 = api.Vocabulary(cut, keys, -4), api.PatternMatchTagger(tokentagsuite.STREAM_RULES)
    many = cut.token_ids_packed(utf8, boff, vocab2, "DR", True)
    assert all(np.array_equal(x, y) and x.tobytes() == y.tobytes() for x, y in zip(results[("plain", True)], [many[k] for k in (0, 1, 2, 3, 5)]))
    many = cut.token_ids_packed(utf8, boff, vocab2, "DR", True, tg2, api.TagStopFilter(cut, tokentagsuite.STOP_SETS["both"], tg2))
    assert all(np.array_equal(x, y) and x.tobytes() == y.tobytes() for x, y in zip(results[("tagged", True)], many))
    # the tokenizer class: tokens carry .id; encode_batch gives the ids alone
    tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", vocab=keys)
    assert tok._vocab.unk_id == -1
    some = texts[:120] + texts[-3:]
    stream = tok.token_stream_batch(some)
    assert [[t.id for t in d] for d in stream] == [[table.get(norm.filter(t.text), -1) for t in d] for d in stream]
    assert all(type(t) is api.TantivyToken for d in stream for t in d) and sum(len(d) for d in stream) > 100
    plain = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR").token_stream_batch(some)
    assert [[t._key() for t in d] for d in stream] == [[t._key() for t in d] for d in plain]
    e_off, e_ids = tok.encode_batch(some)
    assert list(e_ids) == [t.id for d in stream for t in d] and [int(e_off[i + 1] - e_off[i]) for i in range(len(some))] == [len(d) for d in stream]
    raw_tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", vocab=api.Vocabulary(pred, keys, 77), _predictor=pred, vocab_normalize=False)
    assert [[t.id for t in d] for d in raw_tok.token_stream_batch(some)] == [[table.get(t.text, 77) for t in d] for d in stream]
    tagged_tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", predict_tags=True, tagger=tagger, stop_tags=tokentagsuite.STOP_SETS["both"],
                                        vocab=keys)
    tagged = tagged_tok.token_stream_batch(some)
    assert all(type(t) is api.TaggedToken and t.id == table.get(norm.filter(t.text), -1) for d in tagged for t in d)


# ---- hostile CSRs: every case is an error at the sync and leaves the guard words alone; none relies on a fault
def hostile_cases():
    docs = [["あい", "う", "漢字"], ["AB", "é", "𠮷野", "う"], [], ["あいう", "A"]]
    raws, toff, starts, ends = csr_of(docs)
    N = len(ends)
    cases = {}

    def case(name, toff_=None, starts_=starts, ends_=None, cap=N):
        cases[name] = (np.array(toff if toff_ is None else toff_, np.uint64), None if starts_ is None else np.array(starts_, np.uint32),
                       np.array(ends if ends_ is None else ends_, np.uint32), cap)

    case("decreasing_offsets", toff_=[0, 5, 3, 3, N])
    case("decreasing_offsets_no_starts", toff_=[0, 5, 3, 3, N], starts_=None)
    case("sawtooth_offsets", toff_=[0, N, 0, N, N])
    case("offsets_past_capacity", toff_=[0, 3, 7, 7, N + 1000])
    case("offsets_past_capacity_small", toff_=toff, cap=N - 2)
    case("huge_offsets", toff_=[0, 1 << 40, 1 << 41, 1 << 62, (1 << 64) - 1])
    e = ends.copy(); e[2] = len(raws[0]) + 5
    case("end_past_document", ends_=e)
    case("end_past_document_no_starts", ends_=e, starts_=None)
    e = ends.copy(); e[N - 1] = 0xFFFFFFFF
    case("end_huge", ends_=e)
    s = starts.copy(); s[4] = ends[4] + 1
    case("start_after_end", starts_=s)
    e = ends.copy(); e[4] = ends[3] - 1   # without starts: the token in front ends behind this one
    case("start_after_end_no_starts", ends_=e, starts_=None)
    s = starts.copy(); s[0] = 1           # inside "あ"
    case("start_on_continuation_byte", starts_=s)
    e = ends.copy(); e[5] = ends[5] - 1   # inside "野": the token's end, and without starts the next token's start
    case("end_on_continuation_byte", ends_=e)
    case("start_on_continuation_byte_no_starts", ends_=e, starts_=None)
    return docs, raws, (toff, starts, ends), cases


N_HOSTILE = 14


def run_hostile():
    docs, raws, true, cases = hostile_cases()
    assert len(cases) == N_HOSTILE
    pred = predictor()
    keys = ["あい", "う", "𠮷野", "A"]
    vocab = api.Vocabulary(pred, keys)
    table = {s: k for k, s in enumerate(keys)}
    batch = api.DeviceBatch(pred)
    want = vocabref.ids_from_csr(raws, true[0], None, true[2], table, -1, False)
    ran = 0
    for name, (toff, starts, ends, cap) in cases.items():
        for flags in (0, FW):
            got = run_ids(vocab, raws, toff, starts, ends, flags, cap_in=cap, batch=batch)
            assert isinstance(got, str) and CSR_ERROR in got, (name, got)
        # the true arrays on the same workspace: the verdict was reported once, the ids are the lookup's
        assert np.array_equal(run_ids(vocab, raws, true[0], true[1], true[2], batch=batch), want), name
        ran += 1
    del batch
    return ran


def main(argv):
    assert argv == ["--emu-hostile"], "usage: python -m tests.vocabsuite --emu-hostile"
    import gc
    from tests import emu
    _lib._lib = emu.load()
    devmem.EMULATED = True
    ran = run_hostile()
    _PRED.clear()
    gc.collect()   # batch, vocabulary and predictor destroyed: hipemu has checked the red zones of every allocation it freed
    print("ran %d cases" % ran, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
