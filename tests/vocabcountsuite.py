"""The checks of the vocabulary counter (vpt_vocab_counter_*, vpt_vocab_count_batch_device, vpt_token_stream_count_batch;
kernels_vocab_count.hip, vocab_count.hpp) against the restatement of tests/vocabcountref.py, run on the CPU emulator by
tests/test_vocab_count_emu.py and on the MI355X by tests/test_vocab_count_gpu.py; every comparison is exact.

    python -m tests.vocabcountsuite --emu-hostile     the hostile CSRs on the emulator, in a child process (hipemu checks its red zones when
                                                      the workspace goes)

A count call takes vpt_vocab_tile tokens a workgroup, a lane per token; the CSRs built below put tokens, document edges and runs of empty
documents on each side of those edges."""
import os
import random
import sys

import numpy as np

from tests import devmem, patterntagsuite, tagoffsetsuite, tokentagsuite, vocabcountref, vocabref, vocabsuite
from vaporetto_amd import _lib, api

FW = vocabsuite.FW
G = tagoffsetsuite.Guarded
WORDS = vocabsuite.WORDS
CSR_ERROR = vocabsuite.CSR_ERROR
FULL_ERROR = r"vocab counter: full \(max_keys / arena_chars\)"
SENTINEL = vocabsuite.SENTINEL
predictor = vocabsuite.predictor


def csr_of(token_lists):
    """documents as lists of tokens (str or bytes) -> (the documents' bytes, token_offsets, starts, ends)"""
    raws, toff, starts, ends = [], [0], [], []
    for toks in token_lists:
        at, doc = 0, b""
        for t in toks:
            t = t.encode("utf-8") if isinstance(t, str) else t
            starts.append(at)
            at += len(t)
            ends.append(at)
            doc += t
        raws.append(doc)
        toff.append(len(ends))
    return raws, np.array(toff, np.uint64), np.array(starts, np.uint32), np.array(ends, np.uint32)


def run_count(counter, raws, toff, starts, ends, flags=0, cap_in=None, batch=None, pred=None, text_guard=None):
    """vpt_vocab_count_batch_device on guarded arrays of exactly the sizes the call is told -> None, or the message of the call or of its sync"""
    pred = pred or predictor()
    batch = batch or api.DeviceBatch(pred)
    utf8, boff = api.pack_texts(raws)
    cap = len(ends) if cap_in is None else cap_in
    I = {"text": text_guard or G(utf8 if len(utf8) else np.zeros(1, np.uint8)), "boff": G(boff), "toff": G(np.asarray(toff, np.uint64)),
         "ends": G(np.asarray(ends, np.uint32)[:max(cap, 1)] if len(ends) else np.zeros(1, np.uint32))}
    if starts is not None:
        I["starts"] = G(np.asarray(starts, np.uint32)[:max(cap, 1)] if len(starts) else np.zeros(1, np.uint32))
    raised = None
    try:
        batch.count_tokens(counter, I["text"].ptr, I["boff"].ptr, len(raws), I["toff"].ptr, I["starts"].ptr if starts is not None else 0, I["ends"].ptr,
                           cap, flags, devmem.stream())
    except api.VaporettoError as e:
        raised = str(e)
    try:
        batch.sync()
    except api.VaporettoError as e:
        raised = raised or str(e)
    assert not [k for k, a in I.items() if not a.guards_intact()], "guard words overwritten"
    return raised


def same_as_ref(counter, ref, also=()):
    """counts, n_counted, n_skipped and the finish bytes of `counter` (and of every counter of `also`) are the restatement's"""
    want_s, want_c = ref.finish()
    want_raw = ref.finish_raw()
    for c in (counter,) + tuple(also):
        got_s, got_c = c.finish()
        assert got_s == want_s, ([x for x in zip(got_s, want_s) if x[0] != x[1]][:5], len(got_s), len(want_s))
        assert got_c.dtype == np.uint64 and np.array_equal(got_c, want_c), [(s, int(a), int(b)) for s, a, b in zip(want_s, got_c, want_c) if a != b][:8]
        raw = c.finish_raw()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(raw, want_raw))
        info = c.info()
        assert (info["n_keys"], info["n_counted"], info["n_skipped"], info["full"]) == (len(ref.counts), ref.n_counted, ref.n_skipped, False), info


def count_lists(counter, ref, token_lists, flags=0, explicit_starts=True, batch=None):
    raws, toff, starts, ends = csr_of(token_lists)
    got = run_count(counter, raws, toff, starts if explicit_starts else None, ends, flags, batch=batch)
    assert got is None, got
    ref.add_csr(raws, toff, None, ends, flags == FW)


def check_random(seed, fullwidth):
    """~200 documents of 1-12 tokens through the real span kernel (starts == NULL) and the real stop filter, into one counter; a second counter
    fed the same calls gives identical finish bytes."""
    pred = predictor()
    rng = random.Random(seed)
    docs = [[rng.choice(WORDS) for _ in range(rng.randint(1, 12))] for _ in range(200)]
    docs[3], docs[77], docs[199] = ["う"], ["う", "う"], ["う"]   # documents the stop filter leaves without a token
    flags = FW if fullwidth else 0
    texts, labels = tokentagsuite.labels_of(docs)
    raws = [t.encode("utf-8") for t in texts]
    A = tokentagsuite.Arrays(pred, texts, labels)
    batch = api.DeviceBatch(pred)
    A.fill(batch)
    A.spans(batch)
    stop = api.TagStopFilter(pred, [(0, "p"), (0, "q")])
    O = {"offsets": G(np.full(A.S + 1, 7, np.uint64)), "starts": G(np.full(A.cap, SENTINEL, np.uint32)), "ends": G(np.full(A.cap, SENTINEL, np.uint32)),
         "positions": G(np.full(A.cap, SENTINEL, np.uint32)), "tags": G(np.full(A.cap * max(A.nt, 1), SENTINEL, np.int32))}
    batch.token_filter(stop, A.d_toff.ptr, A.d_ends.ptr, A.d_tags.ptr, A.S, A.n_tok, O["offsets"].ptr, O["starts"].ptr, O["ends"].ptr, O["positions"].ptr,
                       O["tags"].ptr, A.cap, devmem.stream())
    one, two = api.VocabularyCounter(pred, 64), api.VocabularyCounter(pred, 64)
    for c in (one, two):
        batch.count_tokens(c, A.d_text.ptr, A.d_boff.ptr, A.S, A.d_toff.ptr, 0, A.d_ends.ptr, A.cap, flags, devmem.stream())
        batch.count_tokens(c, A.d_text.ptr, A.d_boff.ptr, A.S, O["offsets"].ptr, O["starts"].ptr, O["ends"].ptr, A.cap, flags, devmem.stream())
    batch.sync()
    assert A.guards_intact() and all(a.guards_intact() for a in O.values())
    ref = vocabcountref.Ref()
    flat = [t for d in docs for t in d]
    ref.add_tokens([t.encode("utf-8") for t in flat], fullwidth)
    ref.add_tokens([t.encode("utf-8") for t in flat if t != "う"], fullwidth)
    kept = int(O["offsets"].get()[-1])
    assert 0 < kept < A.n_tok and ref.n_counted == A.n_tok + kept and ref.n_skipped == 0
    # (the restatement over the device's CSRs is the Counter over the token lists)
    again = vocabcountref.Ref()
    again.add_csr(raws, A.d_toff.get(A.S + 1), None, A.d_ends.get(A.n_tok), fullwidth)
    again.add_csr(raws, O["offsets"].get(), O["starts"].get(kept), O["ends"].get(kept), fullwidth)
    assert again.counts == ref.counts
    same_as_ref(one, ref, also=(two,))
    assert one.finish_raw()[0].tobytes() == two.finish_raw()[0].tobytes()
    if fullwidth:
        assert "AB" not in ref.counts and "ＡＢ" in ref.counts
    else:
        assert "AB" in ref.counts and "ＡＢ" in ref.counts


def check_accumulation():
    """Three calls: a key of call 1 seen again in calls 2 and 3 (the committed-key compare), a key new in call 2 whose home slot a committed key
    holds, a key new in call 3; the totals are those of one call over the concatenation."""
    pred = predictor()
    a, b = [s for s in vocabref.find_same_home(8, 5, 6) if s not in ("う", "漢字", "🤌")][:2]   # 16 slots: both at home in slot 5
    calls = [[[a, "漢字", a], ["う"]], [[b, a, b], ["漢字", a]], [["🤌", a, b, "🤌"], [], ["う", "🤌"]]]
    assert vocabref.home(a, 4) == vocabref.home(b, 4) == 5
    for flags in (0, FW):
        c, ref, batch = api.VocabularyCounter(pred, 8), vocabcountref.Ref(), api.DeviceBatch(pred)
        assert c.info()["n_slots"] == 16
        for k, docs in enumerate(calls):
            count_lists(c, ref, docs, flags, explicit_starts=(k != 1), batch=batch)
            same_as_ref(c, ref)   # (a finish between the calls: a snapshot, counting goes on)
        whole, ref1 = api.VocabularyCounter(pred, 8), vocabcountref.Ref()
        count_lists(whole, ref1, [d for docs in calls for d in docs], flags, batch=batch)
        image = api.KyteaFullwidthFilter().filter if flags == FW else (lambda s: s)
        assert ref1.counts == ref.counts and ref.counts[image(a)] == 5 and ref.counts[image(b)] == 3
        same_as_ref(whole, ref, also=(c,))


def check_contention():
    """One surface fills three whole tiles -- every lane of every wave goes for one slot --, then two surfaces alternate."""
    tile = api.Vocabulary.tile()
    pred = predictor()
    c, ref, batch = api.VocabularyCounter(pred, 4), vocabcountref.Ref(), api.DeviceBatch(pred)
    count_lists(c, ref, [["漢字"] * (3 * tile)], batch=batch)
    same_as_ref(c, ref)
    assert c.finish()[1].tolist() == [3 * tile]
    count_lists(c, ref, [["漢字", "う"] * tile, ["う", "漢字"] * (tile // 2)], explicit_starts=False, batch=batch)
    same_as_ref(c, ref)
    assert ref.counts == {"漢字": 3 * tile + tile + tile // 2, "う": tile + tile // 2}


def check_probing():
    """max_keys = 4: 8 slots.  Three surfaces share one home slot and a chain wraps past the last slot; once with the colliding keys over two calls."""
    pred = predictor()
    for home_slot in (7, 6, 2):
        three = vocabref.find_same_home(4, home_slot, 3)
        assert vocabref.table_bits(4) == 3 and all(vocabref.home(s, 3) == home_slot for s in three)
        docs = [[three[0], three[1], three[0]], [three[2], three[1], three[2], three[2]]]
        c, ref = api.VocabularyCounter(pred, 4), vocabcountref.Ref()
        assert c.info()["n_slots"] == 8
        count_lists(c, ref, docs)
        same_as_ref(c, ref)
        split, ref2, batch = api.VocabularyCounter(pred, 4), vocabcountref.Ref(), api.DeviceBatch(pred)
        count_lists(split, ref2, [[three[0], three[0]], [three[1]]], batch=batch)
        count_lists(split, ref2, [[three[2], three[1], three[2]], [three[0], three[2]]], batch=batch)
        same_as_ref(split, ref2)
        assert ref2.counts == {three[0]: 3, three[1]: 2, three[2]: 3}


def check_twins():
    """Two surfaces of equal chars and equal fingerprint are two keys: within one call (the representative compare) and across two calls (the
    committed-key compare)."""
    twins = vocabref.find_fingerprint_twins(3)
    assert twins is not None
    a, b = twins
    assert vocabref.fingerprint(a) == vocabref.fingerprint(b) and vocabref.home(a, 3) == vocabref.home(b, 3) and len(a) == len(b) and a != b
    pred = predictor()
    c, ref = api.VocabularyCounter(pred, 4), vocabcountref.Ref()
    count_lists(c, ref, [[a, b, a], [b], [b, a, b]])
    same_as_ref(c, ref)
    assert ref.counts == {a: 3, b: 4}
    c2, ref2, batch = api.VocabularyCounter(pred, 4), vocabcountref.Ref(), api.DeviceBatch(pred)
    count_lists(c2, ref2, [[a, a]], batch=batch)
    count_lists(c2, ref2, [[b, a], [b]], batch=batch)
    same_as_ref(c2, ref2)
    assert ref2.counts == {a: 3, b: 2}


def check_skip_rules():
    """Empty, invalid and long tokens are skipped and counted as skipped; the length bound is exact; a token of more than 4 * max_surface_chars
    bytes is not read: it is a span that the arrays allow but whose bytes lie behind the guarded text."""
    pred = predictor()
    m = 5
    bad = [b"\xff", b"\xc0\x80", b"\xed\xa0\x80", b"\xe3\x81", b"A\xf0\x9f\xa4"]   # FF, an overlong form, a surrogate, truncated at the end (twice)
    for flags in (0, FW):
        c, ref = api.VocabularyCounter(pred, 16, max_surface_chars=m), vocabcountref.Ref(m)
        docs = [["A", b"", "A", b""], [b""], [x for t in bad for x in (t, "い")], ["あ" * m, "あ" * (m + 1), "a" * m, "a" * (m + 1), "𠮷" * m, "𠮷" * (m + 1)],
                ["a" * (4 * m), "a" * (4 * m + 1), "あ" * 40, "A"]]
        count_lists(c, ref, docs, flags)
        same_as_ref(c, ref)
        assert ref.n_skipped == 3 + len(bad) + 3 + 3 and ref.counts["い"] == len(bad) and ("あ" * m) in ref.counts and ("𠮷" * m) in ref.counts
    # a long token whose span reaches far behind the text the call may read: byte_offsets say the document is that long, the guarded
    # allocation is not (the bytes are never read, so nothing faults and the guards stay)
    c, ref = api.VocabularyCounter(pred, 16, max_surface_chars=m), vocabcountref.Ref(m)
    raws = [b"AB", b"x" * 100000]
    utf8, boff = api.pack_texts(raws)
    short = G(np.frombuffer(b"ABxx", np.uint8).copy())
    toff, ends = np.array([0, 1, 2], np.uint64), np.array([2, 100000], np.uint32)
    batch = api.DeviceBatch(pred)
    I = {"boff": G(boff), "toff": G(toff), "ends": G(ends)}
    batch.count_tokens(c, short.ptr, I["boff"].ptr, 2, I["toff"].ptr, 0, I["ends"].ptr, 2, 0, devmem.stream())
    batch.sync()
    assert short.guards_intact() and all(a.guards_intact() for a in I.values())
    ref.add_tokens([b"AB", b"x" * 100000], False)
    same_as_ref(c, ref)
    assert ref.n_skipped == 1 and ref.counts == {"AB": 1}


def check_fullwidth():
    pred = predictor()
    docs = [["AB", "ＡＢ", "AB"], ["09", "０９"], ["カ"]]
    c, ref = api.VocabularyCounter(pred, 8), vocabcountref.Ref()
    count_lists(c, ref, docs, FW)
    same_as_ref(c, ref)
    got = dict(zip(*c.finish()))
    assert got == {"ＡＢ": 3, "０９": 2, "カ": 1}   # the surface handed out is the image
    c, ref = api.VocabularyCounter(pred, 8), vocabcountref.Ref()
    count_lists(c, ref, docs, 0)
    same_as_ref(c, ref)
    assert dict(zip(*c.finish())) == {"AB": 2, "ＡＢ": 1, "09": 1, "０９": 1, "カ": 1}


def check_edges():
    """Tokens, document ends and runs of 0, 1 and 3 empty documents on both sides of every tile edge up to 3 tiles: with starts == NULL and with
    explicit starts."""
    tile = api.Vocabulary.tile()
    pred = predictor()
    n = 3 * tile + 2
    flat = [WORDS[(7 * k + k // 5) % len(WORDS)] for k in range(n)]
    batch = api.DeviceBatch(pred)
    for explicit in (False, True):
        c, ref = api.VocabularyCounter(pred, 32), vocabcountref.Ref()
        for empties in (0, 1, 3):
            cuts = sorted({m * tile + d for m in (1, 2, 3) for d in (-1, 0, 1)})
            docs, a = [[]] * empties, 0
            for cut in cuts + [n]:
                docs.append(flat[a:cut])
                docs += [[]] * empties
                a = cut
            assert sum(len(d) for d in docs) == n
            count_lists(c, ref, docs, explicit_starts=explicit, batch=batch)
        count_lists(c, ref, [flat], explicit_starts=explicit, batch=batch)
        count_lists(c, ref, [[]] + [[t] for t in flat[:tile]] + [[]] * 700 + [[t] for t in flat[tile:2 * tile + 1]], explicit_starts=explicit, batch=batch)
        for count in (1, tile, tile + 1):
            count_lists(c, ref, [[], flat[:count - 1], [], [], [], flat[count - 1:count], []], explicit_starts=explicit, batch=batch)
        count_lists(c, ref, [[], [], []], explicit_starts=explicit, batch=batch)   # no token at all
        same_as_ref(c, ref)


def _expect(fn, pattern):
    import re
    try:
        fn()
    except api.VaporettoError as e:
        assert re.search(pattern, str(e)), str(e)
        return
    assert False, "no error, wanted " + pattern


def check_full():
    """More keys than max_keys, more distinct surfaces in one call than slots, more chars than the arena: the message at the sync, sticky for
    count and finish, gone after reset.  Every step returns: no kernel waits."""
    import re
    pred = predictor()
    nine = ["k%d" % k for k in range(9)]
    cases = [(dict(max_keys=4), [nine[:5]]), (dict(max_keys=4), [nine]), (dict(max_keys=4, arena_chars=6), [["あいう", "AB", "漢字"]]),
             (dict(max_keys=4), [nine[:3], nine[3:6]])]   # (the last: full in a second call, on top of committed keys)
    for kw, calls in cases:
        c, batch = api.VocabularyCounter(pred, **kw), api.DeviceBatch(pred)
        got = None
        for docs in calls:
            raws, toff, starts, ends = csr_of([docs])
            got = run_count(c, raws, toff, starts, ends, batch=batch)
        assert got is not None and re.search(FULL_ERROR, got), (kw, got)
        raws, toff, starts, ends = csr_of([["AB"]])
        for _ in range(2):   # sticky: at the sync while the host has not looked, at the call once it has
            again = run_count(c, raws, toff, starts, ends, batch=batch)
            assert again is not None and re.search(FULL_ERROR, again), again
            assert c.info()["full"]
        _expect(c.finish, FULL_ERROR)
        c.reset()
        assert c.info() == {"n_keys": 0, "n_counted": 0, "n_skipped": 0, "n_slots": 8, "full": False}
        ref = vocabcountref.Ref()
        count_lists(c, ref, [["AB", "漢", "AB"], ["う", "漢"]], batch=batch)
        same_as_ref(c, ref)
    # exactly max_keys keys and exactly arena_chars chars are no error
    c, ref = api.VocabularyCounter(pred, 4, arena_chars=7), vocabcountref.Ref()
    count_lists(c, ref, [["あいう", "AB", "漢", "う", "AB"]])
    same_as_ref(c, ref)


def check_finish():
    pred = predictor()
    c, ref = api.VocabularyCounter(pred, 32), vocabcountref.Ref()
    assert c.finish()[0] == [] and len(c.finish()[1]) == 0   # an empty counter: no entry, offsets [0]
    s, o, n = c.finish_raw()
    assert len(s) == 0 and o.tolist() == [0] and len(n) == 0
    # ties in count: 3 x {い, あ, 漢字, 漢}, 2 x {b, a, ab, 𠮷}, 1 x {é, z}
    toks = ["い", "あ", "漢字", "漢"] * 3 + ["b", "a", "ab", "𠮷"] * 2 + ["é", "z"]
    random.Random(5).shuffle(toks)
    count_lists(c, ref, [toks[:9], toks[9:]])
    same_as_ref(c, ref)
    assert c.finish()[0] == ["あ", "い", "漢", "漢字", "a", "ab", "b", "𠮷", "z", "é"]
    for min_count, max_entries in ((1, None), (1, 0), (2, None), (3, None), (4, None), (1, 1), (1, 5), (2, 6), (2, 100), (3, 2)):
        got_s, got_c = c.finish(min_count, max_entries)
        want_s, want_c = ref.finish(min_count, max_entries)
        assert got_s == want_s and np.array_equal(got_c, want_c), (min_count, max_entries, got_s)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(c.finish_raw(min_count, max_entries), ref.finish_raw(min_count, max_entries)))
        again = c.finish(min_count, max_entries)
        assert again[0] == got_s and again[1].tobytes() == got_c.tobytes()
    assert len(c.finish(1, 0)[0]) == 10 and len(c.finish(4)[0]) == 0


def check_round_trip():
    """build_vocab over a small corpus, with specials, then encode_batch of the same corpus: the bincount of the ids is the counts, id for id;
    unk_id counts what min_count / max_size cut."""
    m = patterntagsuite.tagged_model(31)
    raw = api.Model(m).to_vec()
    texts = tokentagsuite.stream_texts(31)[:150] + ["AB０９ＡＢ09", "ＡＢ"]
    batches = [texts[:60], texts[60:61], texts[61:]]
    for min_count, max_size in ((1, None), (2, None), (1, 7), (2, 4)):
        tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR")
        counter = api.VocabularyCounter(tok.predictor, 1 << 12)
        for b in batches:
            tok.count_batch(b, counter)
        all_s, all_c = counter.finish()
        info = counter.info()
        assert info["n_counted"] == int(all_c.sum()) > 100 and len(all_s) > 10
        kept_s, kept_c = counter.finish(min_count, max_size)
        specials = ["<pad>"] + kept_s[:1] + ["<s>"]   # (one special occurs in the corpus)
        assert len(kept_s) >= 2
        vocab = tok.build_vocab(batches, min_count, max_size, specials=specials, unk_id=-7, max_keys=1 << 12)
        order = specials + [s for s in kept_s if s not in specials]
        assert [vocab.surface(k) for k in range(len(order))] == order and vocab.info()["n_keys"] == len(order) and vocab.unk_id == -7
        tok.set_vocab(vocab)
        toff, ids = tok.encode_batch(texts)
        assert len(ids) == info["n_counted"] + info["n_skipped"] and int(toff[-1]) == len(ids)
        counts = dict(zip(kept_s, (int(x) for x in kept_c)))
        got = np.bincount(ids[ids >= 0], minlength=len(order))
        assert got.tolist() == [counts.get(s, 0) for s in order]
        assert int((ids == -7).sum()) == info["n_skipped"] + int(all_c.sum()) - int(kept_c.sum())
        stream = [t for d in tok.token_stream_batch(texts[:40]) for t in d]
        assert all((vocab.surface(t.id) == api.KyteaFullwidthFilter().filter(t.text)) if t.id >= 0 else True for t in stream)


def check_pipeline(seed=31):
    """vpt_token_stream_count_batch against the existing stream calls with the device count call behind them, step by step: untagged, tagged
    with a stop set; unchanged under three values of VPT_TOKENIZE_CHUNK_BYTES."""
    m = patterntagsuite.tagged_model(seed)
    raw = api.Model(m).to_vec()
    texts = tokentagsuite.stream_texts(seed) + ["AB０９ＡＢ09", "ＡＢ"]
    raws = [t.encode("utf-8") for t in texts]
    utf8, boff = api.pack_texts(raws)
    results = {}
    for chunk in (None, max(len(utf8) // 4, 1), max(len(utf8) // 9, 1), max(len(utf8) // 30, 1)):
        if chunk is not None:
            os.environ["VPT_TOKENIZE_CHUNK_BYTES"] = str(chunk)
        try:
            pred = api.Predictor(api.Model.read_slice(raw)[0], True, device=0)
        finally:
            os.environ.pop("VPT_TOKENIZE_CHUNK_BYTES", None)
        tagger = api.PatternMatchTagger(tokentagsuite.STREAM_RULES)
        stop = api.TagStopFilter(pred, tokentagsuite.STOP_SETS["both"], tagger)
        for route in ("plain", "tagged"):
            for normalize in (True, False):
                c = api.VocabularyCounter(pred, 1 << 12)
                if route == "plain":
                    pred.count_tokens_packed(utf8, boff, c, "DR", normalize)
                else:
                    pred.count_tokens_packed(utf8, boff, c, "DR", normalize, tagger, stop)
                pred.count_tokens_packed(utf8[:0], boff[:1], c, "DR", normalize)   # no document: nothing happens
                got = tuple(x.tobytes() for x in c.finish_raw()) + (c.info()["n_counted"], c.info()["n_skipped"])
                if chunk is None:   # the steps: the stream's arrays, then the device count call over them
                    if route == "plain":
                        toff, ends = pred.token_stream_packed(utf8, boff, "DR")
                        starts = None
                    else:
                        toff, starts, ends = pred.token_stream_tagged_packed(utf8, boff, "DR", tagger, stop)[:3]
                    step, ref = api.VocabularyCounter(pred, 1 << 12), vocabcountref.Ref()
                    assert run_count(step, raws, toff, starts, ends, FW if normalize else 0, pred=pred) is None
                    ref.add_csr(raws, toff, starts, ends, normalize)
                    same_as_ref(step, ref, also=(c,))
                    assert ref.n_counted + ref.n_skipped == int(toff[-1]) and ref.n_counted > 100
                    results[(route, normalize)] = got
                else:
                    assert got == results[(route, normalize)], (chunk, route, normalize)
    assert results[("plain", True)] != results[("plain", False)] and results[("plain", True)][3] > results[("tagged", True)][3]


def check_errors():
    pred = predictor()
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    _expect(lambda: api.VocabularyCounter(pred, 0), "max_keys: must be between 1 and 2\\^24")
    _expect(lambda: api.VocabularyCounter(pred, (1 << 24) + 1), "max_keys: must be between 1 and 2\\^24")
    _expect(lambda: api.VocabularyCounter(pred, 4, max_surface_chars=0), "max_surface_chars: must be between")
    c = api.VocabularyCounter(pred, 4)
    raws, toff, starts, ends = csr_of([["漢字"]])
    for bad in (2, FW | 4, 1 << 7):
        assert "flags: unknown bit" in run_count(c, raws, toff, None, ends, flags=bad)
    assert "counter: must not be NULL" in run_count(None, raws, toff, None, ends)
    assert "counter: does not belong to this predictor" in run_count(c, raws, toff, None, ends, pred=other)
    utf8, boff = api.pack_texts(raws)
    _expect(lambda: other.count_tokens_packed(utf8, boff, c), "counter: does not belong to this predictor")
    _expect(lambda: pred.count_tokens_packed(utf8, boff, None), "counter: must not be NULL")
    _expect(lambda: pred.count_tokens_packed(utf8, boff, c, "X"), "Could not parse a wsconst value")
    assert c.info() == {"n_keys": 0, "n_counted": 0, "n_skipped": 0, "n_slots": 8, "full": False}   # none of these touched it


# ---- hostile CSRs: every case is an error at the sync, leaves the guard words alone and the counter usable after reset
def run_hostile():
    docs, raws, true, cases = vocabsuite.hostile_cases()
    assert len(cases) == vocabsuite.N_HOSTILE
    pred = predictor()
    batch = api.DeviceBatch(pred)
    c = api.VocabularyCounter(pred, 16)
    want = vocabcountref.Ref()
    want.add_csr(raws, true[0], None, true[2], False)
    ran = 0
    for name, (toff, starts, ends, cap) in cases.items():
        for flags in (0, FW):
            got = run_count(c, raws, toff, starts, ends, flags, cap_in=cap, batch=batch)
            assert isinstance(got, str) and CSR_ERROR in got, (name, got)
            c.reset()
            assert run_count(c, raws, true[0], true[1], true[2], batch=batch) is None, name
            same_as_ref(c, want)
            c.reset()
        ran += 1
    del batch
    return ran


def main(argv):
    assert argv == ["--emu-hostile"], "usage: python -m tests.vocabcountsuite --emu-hostile"
    import gc
    from tests import emu
    _lib._lib = emu.load()
    devmem.EMULATED = True
    ran = run_hostile()
    vocabsuite._PRED.clear()
    gc.collect()   # batch, counter and predictor destroyed: hipemu has checked the red zones of every allocation it freed
    print("ran %d cases" % ran, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
