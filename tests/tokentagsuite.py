"""The checks of tags in the token stream against the restatement of tests/tokentagref.py, run on the CPU emulator by
tests/test_token_tags_emu.py and on the MI355X by tests/test_token_tags_gpu.py; every comparison is exact:
  * the tag vocabulary (vpt_predictor_n_tag_strings / vpt_predictor_tag_string);
  * the tagged spans (vpt_token_tags_batch_device; kernels_tokens.hip, token_spans_kernel<true>);
  * the stop filter (vpt_tag_stop_*, vpt_token_filter_batch_device; kernels_token_filter.hip), through the device entry on labels of the
    caller's -- kept and dropped tokens on both sides of every edge -- and with hostile token_offsets and capacities;
  * the one host call (vpt_token_stream_tagged_batch) and the tokenizer class.

    python -m tests.tokentagsuite --emu-hostile BATCH VARIANT    the hostile out_offsets of tests/tagoffsetsuite.py through the span entry
    python -m tests.tokentagsuite --emu-filter                   hostile token_offsets / capacities through the filter entry
(on the emulator, in a child process: hipemu checks its red zones when the workspace goes)

The span kernel walks a run in pieces of PIECE bytes, sixteen bytes a thread, a wave WAVE bytes; the filter takes vpt_token_filter_tile tokens a
workgroup; the documents built below put tokens on each side of those edges, of a span-run edge and of a fill_tags run edge."""
import os
import random
import sys

import numpy as np
import pytest

from tests import devmem, patterntagsuite, tagoffsetsuite, tokentagref
from vaporetto_amd import _lib, api

PIECE, WAVE = 4096, 1024   # kernels_tokens.hip: kSpanPiece = kEmitThreads * 16, a wave's share of it
GUARD = 0x5A5A5A5A
RULES = {"AB": ["rA", "rB", "rC"], "あい": [None, "rule", "長いタグ/ "], "字漢": ["名"], "B0": [None, None, "rZ"], "09": ["d"]}


def vocabulary_checks(m, pred):
    want = tokentagref.walk_vocabulary(m)
    assert pred.tag_strings() == want
    again = api.Predictor.load_compiled(pred.save_compiled(), device=0)
    assert again.tag_strings() == want
    return want


def check_vocabulary():
    m = patterntagsuite.tagged_model()
    # strings shared between slots and models get one id; bytes the writer escapes come back raw; the empty string is a tag
    from vaporetto_amd.modelfmt import TagModel
    m.tag_models += [TagModel("AB", [["名", "x", "a/b c\\d"], ["", "カ"]], bias=[1, 2, 3, 4, 5])]
    want = vocabulary_checks(m, patterntagsuite.predictor_of(m))
    assert want == ["名", "動", "カ", "x", "p", "q", "r", "s", "t", "a/b c\\d", ""]
    # none without predict_tags, none without tag models
    assert patterntagsuite.predictor_of(m, predict_tags=False).tag_strings() == []
    assert patterntagsuite.predictor_of(patterntagsuite.tagged_model(with_tags=False)).tag_strings() == []
    L = _lib.load()
    import ctypes as C
    ptr, n = C.c_void_p(), C.c_size_t()
    pred = patterntagsuite.predictor_of(m)
    assert L.vpt_predictor_tag_string(pred.handle, len(want), C.byref(ptr), C.byref(n)) == _lib.VPT_INVALID_ARGUMENT
    assert "no such tag string" in _lib.last_error()


class Arrays:
    """The batch on the device with guard words behind every output array."""

    def __init__(self, pred, texts, labels, capacity=None):
        self.utf8, self.boff, self.ooff = patterntagsuite.pack(texts)
        self.S, self.nb, self.nt = len(texts), len(labels), pred.n_tags()
        assert self.nb == int(self.ooff[-1])
        self.n_tok = int(np.count_nonzero(labels == 1)) + self.S
        self.cap = self.n_tok if capacity is None else capacity
        self.d_text = devmem.put(np.concatenate([self.utf8, np.zeros(32, np.uint8)]))
        self.d_boff, self.d_ooff = devmem.put(self.boff), devmem.put(self.ooff)
        self.d_lab = devmem.put(np.concatenate([labels, np.zeros(16, np.uint8)]))
        self.d_toff = devmem.put(np.full(self.S + 1 + 8, GUARD, np.uint64))
        self.d_ends = devmem.put(np.full(self.cap + 64, GUARD, np.uint32))
        self.d_tags = devmem.put(np.full(self.cap * max(self.nt, 1) + 64, GUARD, np.int32))

    def fill(self, batch):
        batch.fill_tags(self.d_text.ptr, self.d_boff.ptr, self.d_ooff.ptr, self.S, self.nb, self.d_lab.ptr, 0, devmem.stream())

    def spans(self, batch):
        batch.token_tags(self.d_text.ptr, self.d_boff.ptr, self.d_ooff.ptr, self.S, self.nb, self.d_lab.ptr, self.d_toff.ptr, self.d_ends.ptr,
                         self.d_tags.ptr, self.cap, devmem.stream())

    def guards_intact(self):
        return bool((self.d_toff.get()[self.S + 1:] == GUARD).all() and (self.d_ends.get()[self.cap:] == GUARD).all()
                    and (self.d_tags.get()[self.cap * self.nt:] == GUARD).all())


def device_tokens(pred, tagger, texts, labels, fullwidth=False, per_block=None):
    """fill_tags + the tagged spans on a workspace of the caller's -> (per document [from, to, position, tag strings], raw tags, plan)."""
    A = Arrays(pred, texts, labels)
    if per_block:   # (a workspace reads VPT_EMIT_PER_BLOCK when it is made: documents a workgroup of the span kernel takes)
        os.environ["VPT_EMIT_PER_BLOCK"] = str(per_block)
    try:
        batch = api.DeviceBatch(pred)
    finally:
        os.environ.pop("VPT_EMIT_PER_BLOCK", None)
    batch.set_flags(patterntagsuite.FW if fullwidth else 0)
    batch.set_pattern_tagger(tagger)
    A.fill(batch)
    A.spans(batch)
    batch.sync()
    assert A.guards_intact()
    toff, ends, tags = A.d_toff.get(A.S + 1), A.d_ends.get(A.n_tok), A.d_tags.get(A.n_tok * A.nt).reshape(A.n_tok, A.nt)
    assert int(toff[0]) == 0 and int(toff[-1]) == A.n_tok
    vocab = pred.tag_strings()
    rule = [tagger.tag(pred, k) for k in range(tagger.n_tags(pred))] if tagger is not None and A.nt else []
    assert (tags >= -1 - len(rule)).all() and (tags < max(len(vocab), 1)).all() if A.nt else True

    def name(v):
        return None if v == -1 else vocab[v] if v >= 0 else rule[-2 - v]

    docs = []
    for i in range(A.S):
        a, b = int(toff[i]), int(toff[i + 1])
        docs.append([[int(ends[k - 1]) if k > a else 0, int(ends[k]), k - a, tuple(name(int(v)) for v in tags[k])] for k in range(a, b)])
    return docs, tags, batch.last_plan()


def check_against_restatement(pred, texts, labels, rules=None, fullwidth=False, expect_rule_ids=None):
    tagger = api.PatternMatchTagger(rules) if rules is not None else None
    _, _, ooff = patterntagsuite.pack(texts)
    want = tokentagref.token_tags(pred, texts, ooff, labels, tagger, fullwidth)
    got, tags, plan = device_tokens(pred, tagger, texts, labels, fullwidth)
    bad = [i for i in range(len(texts)) if got[i] != want[i]]
    assert not bad, (bad[:4], got[bad[0]][:6], want[bad[0]][:6])
    got2, tags2, _ = device_tokens(pred, tagger, texts, labels, fullwidth)   # two runs give identical arrays
    assert np.array_equal(tags, tags2) and got2 == got
    if expect_rule_ids is not None:
        assert bool((tags <= -2).any()) == expect_rule_ids
    return got, tags, plan


def labels_of(token_lists):
    """-> (texts, labels): every document a list of tokens"""
    texts, labels = [], []
    for toks in token_lists:
        texts.append("".join(toks))
        lab = []
        for t in toks:
            lab += [0] * (len(t) - 1) + [1]
        labels += lab[:-1]
    return texts, np.array(labels, np.uint8)


def random_token_docs(seed, n, lo=1, hi=12, extra=()):
    rng = random.Random(seed)
    words = ["漢字", "あい", "う", "09", "AB", "字漢", "B0", "A", "0", "い"] + list(extra)
    return [[rng.choice(words) for _ in range(rng.randint(lo, hi))] for _ in range(n)]


def check_random(seed, n_tags):
    """Random documents of whole words on a model with n_tags 3 (slots left None, models with fewer slots) or 1; small, tiny, one long document."""
    m = patterntagsuite.tagged_model(seed)
    if n_tags == 1:
        for tm in m.tag_models:
            del tm.tags[1:]
        m.tag_models[2].bias[:] = [1, 2]
    pred = patterntagsuite.predictor_of(m)
    assert pred.n_tags() == n_tags
    vocabulary_checks(m, pred)
    small = random_token_docs(seed, 180)
    tiny = random_token_docs(seed + 1, 3000, 1, 2)
    long_doc = [random_token_docs(seed + 2, 1, 12000, 12000)[0]]   # ~20 K chars: several pieces, many fill_tags runs
    for docs in (small, tiny, long_doc):
        texts, labels = labels_of(docs)
        check_against_restatement(pred, texts, labels)
        check_against_restatement(pred, texts, labels, RULES, expect_rule_ids=True)
    # labels that are not whole words, fullwidth
    texts = patterntagsuite.docs(seed + 3, 300)
    _, _, ooff = patterntagsuite.pack(texts)
    labels = np.random.default_rng(seed).integers(0, 2, int(ooff[-1])).astype(np.uint8)
    check_against_restatement(pred, texts, labels, RULES)
    # under KyteaFullwidthFilter tags and rules see the normalised text (ASCII -> fullwidth), the spans count the caller's bytes
    fw = ["AB漢字09あい", "う" * 5 + "A", "AB"]
    fw_rules = dict(RULES, **{"ＡＢ": ["fA", "fB"], "０９": [None, "fD"]})
    _, _, ooff = patterntagsuite.pack(fw)
    check_against_restatement(pred, fw, np.ones(int(ooff[-1]), np.uint8), fw_rules, fullwidth=True)
    labels = np.zeros(int(ooff[-1]), np.uint8)
    labels[[1, 3, 5]] = 1
    check_against_restatement(pred, fw, labels, fw_rules, fullwidth=True, expect_rule_ids=True)


def check_edges():
    """A tagged token's last char on each side of a piece edge, a wave edge, a span-run edge and a fill_tags run edge; a tagged token as the last
    of one document and the first of the next; three span runs at least."""
    pred = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    # "う" (3 bytes, a model that tags fully) ends a token; fillers of one byte shift it byte by byte over the edge
    docs = []
    for edge in (PIECE, WAVE, 2 * PIECE, PIECE + WAVE):
        for shift in (-3, -2, -1, 0, 1):
            # one document whose second token "う" ends `shift` bytes from `edge`, counted from the document's start; it begins and ends with a
            # tagged token, and documents this long are fill_tags runs (and, below, span runs) of their own: tagged tokens on both sides of those edges
            docs.append(["う"] + ["A"] * (edge + shift - 8) + ["AB", "う", "う", "漢字", "あい", "う"])
    # documents that end and begin with a tagged token, one-char documents among them
    docs += [["う"], ["う"], ["漢字"], ["う", "A", "う"], ["あい"], ["う"]] * 40
    texts, labels = labels_of(docs)
    for rules in (None, RULES):
        got, tags, plan = check_against_restatement(pred, texts, labels, rules)
        assert plan["tag_runs"] >= 3, plan
    # the same with every document a span run of its own and with span runs of 3 and 7 documents: run edges between any two documents, span runs
    # that start inside a fill_tags run (their records begin further on in the slice)
    tagger = api.PatternMatchTagger(RULES)
    _, _, ooff = patterntagsuite.pack(texts)
    want = tokentagref.token_tags(pred, texts, ooff, labels, tagger)
    for per_block in (1, 3, 7):
        got, _, plan = device_tokens(pred, tagger, texts, labels, per_block=per_block)
        assert got == want, per_block
        assert plan["tag_run_sent"] > 1 or per_block == 1, plan


def check_no_record_and_every_record():
    pred = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    texts, labels = labels_of([["A", "B0", "字漢", "0"] * 30] * 50)          # no token has a record
    got, tags, _ = check_against_restatement(pred, texts, labels)
    assert (tags == -1).all()
    texts, labels = labels_of([["う", "漢字", "あい", "う"] * 30] * 50)      # every token has one
    got, tags, _ = check_against_restatement(pred, texts, labels)
    assert (tags[:, 0] >= 0).all()
    # a model without tag models: the untagged spans, no tag entry touched; a tagger over it changes nothing
    plain = patterntagsuite.predictor_of(patterntagsuite.tagged_model(with_tags=False))
    assert plain.n_tags() == 0
    for rules in (None, RULES):
        got, tags, _ = check_against_restatement(plain, texts, labels, rules)
        assert tags.shape[1] == 0


def _expect(fn, text):
    with pytest.raises(api.VaporettoError, match=text):
        fn()


def check_errors():
    m = patterntagsuite.tagged_model()
    pred = patterntagsuite.predictor_of(m)
    texts, labels = labels_of(random_token_docs(3, 40))
    # predict_tags == 0
    untagged = patterntagsuite.predictor_of(m, predict_tags=False)
    A = Arrays(untagged, texts, labels)
    _expect(lambda: A.spans(api.DeviceBatch(untagged)), "predict_tags = false")
    # no fill_tags on the workspace for this batch
    A = Arrays(pred, texts, labels)
    _expect(lambda: A.spans(api.DeviceBatch(pred)), "call vpt_fill_tags_batch_device on this workspace")
    # a workspace of another predictor
    other = patterntagsuite.predictor_of(m)
    batch = api.DeviceBatch(other)
    L = _lib.load()
    st = L.vpt_token_tags_batch_device(pred.handle, batch._h, A.d_text.ptr, A.d_boff.ptr, A.d_ooff.ptr, A.S, A.nb, A.d_lab.ptr, A.d_toff.ptr, A.d_ends.ptr,
                                       A.d_tags.ptr, A.cap, devmem.stream())
    assert st == _lib.VPT_INVALID_ARGUMENT and "does not belong to this predictor" in _lib.last_error()
    # capacity one token too small: the verdict at the sync, the guard words behind every output array intact; then the true capacity
    short = Arrays(pred, texts, labels, capacity=A.n_tok - 1)
    batch = api.DeviceBatch(pred)
    short.fill(batch)
    short.spans(batch)
    _expect(batch.sync, "text_capacity")
    assert short.guards_intact()
    A.fill(batch)
    A.spans(batch)
    batch.sync()
    assert A.guards_intact()
    # labels edited between fill_tags and the span call: a record whose token no longer ends there
    texts, labels = labels_of([["A", "う", "A", "漢字", "B0"]] * 20)
    A = Arrays(pred, texts, labels)
    batch = api.DeviceBatch(pred)
    A.fill(batch)
    batch.sync()
    edited = labels.copy()
    edited[1] = 0   # "う" is no token any more: "うA"
    A.d_lab.set(np.concatenate([edited, np.zeros(16, np.uint8)]))
    B = Arrays(pred, texts, edited)
    batch.token_tags(A.d_text.ptr, A.d_boff.ptr, A.d_ooff.ptr, A.S, A.nb, A.d_lab.ptr, B.d_toff.ptr, B.d_ends.ptr, B.d_tags.ptr, B.cap, devmem.stream())
    _expect(batch.sync, "do not match the text")
    assert B.guards_intact()


def run_hostile_case(env, name):
    """One corruption of tests/tagoffsetsuite.py: fill_tags and the tagged spans on the bad offsets, the verdict at the sync, guard words intact;
    then the true offsets on the same workspace give the restatement's tokens."""
    S, nb, nt = env.S, env.nb, env.nt
    st = devmem.stream()
    batch = api.DeviceBatch(env.pred)
    batch.set_pattern_tagger(env.tagger)
    d_text = devmem.put(np.concatenate([env.utf8, np.zeros(32, np.uint8)]))
    d_boff = devmem.put(env.boff.astype(np.uint64))
    if env.run_sent is None:
        d_o, d_l = devmem.put(env.ooff), devmem.put(np.ones(nb + 16, np.uint8))
        batch.fill_tags(d_text.ptr, d_boff.ptr, d_o.ptr, S, nb, d_l.ptr, 0, st)
        batch.sync()
        env.check_geometry(batch.last_plan())
    bad, tb = tagoffsetsuite.corrupt(env, name)
    rewritten = name == "rewritten_behind_fill_tags"
    cap = max(tb, nb) + S
    G = tagoffsetsuite.Guarded
    A = {"offsets": G(env.ooff if rewritten else bad), "labels": G(np.ones(max(tb, nb, 1), np.uint8)), "toff": G(np.zeros(S + 1, np.uint64)),
         "ends": G(np.full(cap, GUARD, np.uint32)), "tags": G(np.full(cap * nt, GUARD, np.int32))}

    def calls(total_boundaries):
        batch.fill_tags(d_text.ptr, d_boff.ptr, A["offsets"].ptr, S, total_boundaries, A["labels"].ptr, 0, st)
        return lambda: batch.token_tags(d_text.ptr, d_boff.ptr, A["offsets"].ptr, S, total_boundaries, A["labels"].ptr, A["toff"].ptr, A["ends"].ptr,
                                        A["tags"].ptr, cap, st)

    spans = calls(tb)
    if rewritten:
        A["offsets"].set(bad)   # in stream order behind fill_tags, in front of the span kernel
    try:
        spans()
    except api.VaporettoError:
        pass
    try:
        batch.sync()
        raised = None
    except api.VaporettoError as e:
        raised = str(e)
    if name in tagoffsetsuite.UPPER_BOUND_IS_VALID:
        assert raised is None, (name, raised)
    else:
        assert raised is not None and tagoffsetsuite.MESSAGE in raised, (name, raised)
    broken = [k for k, a in A.items() if not a.guards_intact()]
    assert not broken, (name, "guard words overwritten around", broken)
    # ---- the workspace stays usable: the true offsets
    A["offsets"].set(env.ooff)
    calls(nb)()
    batch.sync()
    n_tok = nb + S   # labels all 1: every char a token
    vocab = env.pred.tag_strings()
    by_token = {tm.token: tm.tags for tm in env.model.tag_models}
    flat = "".join(env.texts)
    want = np.array([[vocab.index(by_token[c][j][int(v)]) for j, v in enumerate(row)] for c, row in zip(flat, env.want_tags)], np.int32)
    assert np.array_equal(A["tags"].get(n_tok * nt).reshape(n_tok, nt), want), name
    assert np.array_equal(A["ends"].get(n_tok), np.full(n_tok, 3, np.uint32) * (np.arange(n_tok) - np.repeat(env.ooff[:-1].astype(np.int64) + np.arange(S), [len(t) for t in env.texts]) + 1).astype(np.uint32)), name
    broken = [k for k, a in A.items() if not a.guards_intact()]
    assert not broken, (name, "guard words overwritten around", broken)
    del batch


def run_hostile_group(batch, variant, log=None):
    env = tagoffsetsuite.Env(batch, variant)
    env.model = tagoffsetsuite.tag_model_data()
    ran = 0
    for name in tagoffsetsuite.names_for(batch):
        if log:
            log("case %s %s %s" % (batch, variant, name))
        run_hostile_case(env, name)
        ran += 1
    assert ran == tagoffsetsuite.CASES_PER_BATCH[batch]
    return ran


# ---- the one host call (vpt_token_stream_tagged_batch), the stop filter (vpt_tag_stop_*, vpt_token_filter_batch_device) and the tokenizer class
STREAM_RULES = {"ＡＢ": ["rA", "rB", "rC"], "Ｂ０": [None, None, "rZ"], "字漢": ["名"], "０": ["rA"]}   # (the rules see the normalised text)
STOP_SETS = {
    "nothing": [(0, "動詞なし")],                                  # a string in neither vocabulary
    "model_only": [(0, "p"), (0, "名"), (2, "カ")],
    "rule_only": [(0, "rA"), (2, "rZ")],
    "both": [(0, "名"), (0, "rA"), (1, "r"), (0, "x")],
    "everything": None,                                            # filled in: every string of both vocabularies in every slot
}


def _want_arrays(raw, pred, texts, ws, tagger, pairs):
    (off, starts, ends, pos, tags), counts = tokentagref.token_stream_tagged(raw, pred, texts, ws, tagger, pairs)
    return off, starts, ends, pos, tags, counts


def _got_arrays(pred, tagger, texts, ws, stop):
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    toff, starts, ends, pos, tags = pred.token_stream_tagged_packed(utf8, boff, ws, tagger, stop)
    vocab = pred.tag_strings()
    rule = [tagger.tag(pred, k) for k in range(tagger.n_tags(pred))] if tagger is not None and tags.shape[1] else []
    names = [tuple(None if v == -1 else vocab[v] if v >= 0 else rule[-2 - v] for v in (int(x) for x in row)) for row in tags]
    return [int(x) for x in toff], [int(x) for x in starts], [int(x) for x in ends], [int(x) for x in pos], names, (toff, starts, ends, pos, tags)


def stream_texts(seed, n=260):
    filt = vpt_filter_tile()
    t = patterntagsuite.docs(seed, n, lo=1, hi=40)
    # empty documents, a document of several filter blocks and pieces (its tokens cross the filter's block edge), documents of stopped tokens only
    return ["", ""] + t[:n // 2] + ["", "う" * (3 * filt + 5), "漢字" * 9, "う"] + t[n // 2:] + ["あいう" * (PIECE // 9 + 7), ""]


def vpt_filter_tile():
    import ctypes as C
    v = C.c_uint32()
    assert _lib.load().vpt_token_filter_tile(C.byref(v)) == _lib.VPT_OK and v.value >= 64
    return int(v.value)


def check_stream(seed=31):
    m = patterntagsuite.tagged_model(seed)
    raw = api.Model(m).to_vec()
    pred = api.Predictor(api.Model.read_slice(raw)[0], True, device=0)
    tagger = api.PatternMatchTagger(STREAM_RULES)
    texts = stream_texts(seed)
    every = [(j, s) for j in range(3) for s in pred.tag_strings() + [tagger.tag(pred, k) for k in range(tagger.n_tags(pred))]]
    for ws in ("", "DR"):
        for tg in (None, tagger):
            # tags alone: starts and positions are the trivial ones
            off, starts, ends, pos, tags, counts = _want_arrays(raw, pred, texts, ws, tg, None)
            got = _got_arrays(pred, tg, texts, ws, None)
            assert list(got[:5]) == [off, starts, ends, pos, tags], (ws, tg is not None)
            for i in range(len(texts)):
                a, b = off[i], off[i + 1]
                assert got[3][a:b] == list(range(b - a)) and got[1][a:b] == ([0] + got[2][a:b - 1] if b > a else [])
    # the stop sets, with the tagger
    hit = {}
    for name, pairs in STOP_SETS.items():
        pairs = every if pairs is None else pairs
        stop = api.TagStopFilter(pred, pairs, tagger)
        off, starts, ends, pos, tags, counts = _want_arrays(raw, pred, texts, "", tagger, pairs)
        got = _got_arrays(pred, tagger, texts, "", stop)
        assert list(got[:5]) == [off, starts, ends, pos, tags], name
        again = _got_arrays(pred, tagger, texts, "", stop)[5]
        assert all(np.array_equal(x, y) and x.tobytes() == y.tobytes() for x, y in zip(got[5], again)), name   # two runs byte-identical
        hit[name] = sum(counts) - len(ends)
        lost = [i for i in range(len(texts)) if texts[i] and off[i] == off[i + 1]]
        if name in ("both", "everything"):
            assert lost, name                     # documents that lose all their tokens
    assert hit["nothing"] == 0 and hit["model_only"] > 0 and hit["rule_only"] > 0 and hit["everything"] > hit["both"] > 0
    # a stop set made WITHOUT the tagger stops no rule tag; model tags still
    off, starts, ends, pos, tags, _ = _want_arrays(raw, pred, texts, "", tagger, STOP_SETS["model_only"])
    assert list(_got_arrays(pred, tagger, texts, "", api.TagStopFilter(pred, STOP_SETS["model_only"] + STOP_SETS["rule_only"]))[:5]) == [off, starts, ends, pos, tags]
    # the whole batch stopped
    all_stopped = ["う", "ううう", "う" * 700]
    got = _got_arrays(pred, None, all_stopped, "", api.TagStopFilter(pred, [(0, s) for s in pred.tag_strings()]))
    want = _want_arrays(raw, pred, all_stopped, "", None, [(0, s) for s in pred.tag_strings()])
    assert list(got[:5]) == list(want[:5])
    # the result does not depend on the chunks: at least three
    os.environ["VPT_TOKENIZE_CHUNK_BYTES"] = str(max(sum(len(t.encode("utf-8")) for t in texts) // 4, 1))
    try:
        cut = api.Predictor(api.Model.read_slice(raw)[0], True, device=0)
    finally:
        os.environ.pop("VPT_TOKENIZE_CHUNK_BYTES", None)
    pairs = STOP_SETS["both"]
    tg2 = api.PatternMatchTagger(STREAM_RULES)
    one = _got_arrays(pred, tagger, texts, "DR", api.TagStopFilter(pred, pairs, tagger))[5]
    many = _got_arrays(cut, tg2, texts, "DR", api.TagStopFilter(cut, pairs, tg2))[5]
    assert all(np.array_equal(x, y) for x, y in zip(one, many))
    return raw, pred


def check_tokenizer(seed=31):
    m = patterntagsuite.tagged_model(seed)
    raw = api.Model(m).to_vec()
    texts = stream_texts(seed, 60)
    pairs = STOP_SETS["both"]
    tagger = api.PatternMatchTagger(STREAM_RULES)
    tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", predict_tags=True, tagger=tagger, stop_tags=pairs)
    (off, starts, ends, pos, tags), counts = tokentagref.token_stream_tagged(raw, tok.predictor, texts, "DR", tagger, pairs)
    want = [[(t.encode("utf-8")[starts[k]:ends[k]].decode("utf-8"), starts[k], ends[k], pos[k], counts[i], tags[k]) for k in range(off[i], off[i + 1])]
            for i, t in enumerate(texts)]
    got = tok.token_stream_batch(texts)
    assert [[t._key() + (t.tags,) for t in d] for d in got] == want
    again = api.VaporettoTokenizer.deserialize(tok.predictor.save_compiled(), "DR", predict_tags=True, tagger=tagger, stop_tags=pairs)
    assert again.token_stream_batch(texts) == got
    # without predict_tags: today's class, token for token
    plain = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR")
    untagged = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", predict_tags=True)
    a, b = plain.token_stream_batch(texts), untagged.token_stream_batch(texts)
    assert all(type(t) is api.TantivyToken for d in a for t in d)
    assert [[t._key() for t in d] for d in a] == [[t._key() for t in d] for d in b]


def check_stop_errors():
    m = patterntagsuite.tagged_model()
    pred, other = patterntagsuite.predictor_of(m), patterntagsuite.predictor_of(m)
    _expect(lambda: api.TagStopFilter(pred, [(0, "名"), (3, "名")]), r"slot must be smaller than the predictor's n_tags \(entry 1\)")
    _expect(lambda: api.TagStopFilter(pred, [(0, "a\0b")]), r"a tag must not contain NULL \(entry 0\)")
    tagger = api.PatternMatchTagger(RULES)
    tagger.handle(other)
    L = _lib.load()
    import ctypes as C
    h = C.c_void_p()
    slots, off = np.zeros(1, np.uint32), np.zeros(2, np.uint64)
    st = L.vpt_tag_stop_create(pred.handle, tagger.handle(other), slots.ctypes.data, slots.ctypes.data, off.ctypes.data, 0, C.byref(h))
    assert st == _lib.VPT_INVALID_ARGUMENT and "tagger: does not belong to this predictor" in _lib.last_error()
    utf8, boff = api.pack_texts(["あい".encode("utf-8")])
    _expect(lambda: other.token_stream_tagged_packed(utf8, boff, "", None, api.TagStopFilter(pred, [(0, "名")])), "stop: does not belong to this predictor")
    _expect(lambda: other.token_stream_tagged_packed(utf8, boff, "", _Foreign(tagger, pred), None), "tagger: does not belong")
    _expect(lambda: patterntagsuite.predictor_of(m, predict_tags=False).token_stream_tagged_packed(utf8, boff), "predict_tags = false")
    _expect(lambda: pred.token_stream_tagged_packed(utf8, boff, "X"), "Could not parse a wsconst value")
    bad, bo = api.pack_texts(["あ\0い".encode("utf-8")])
    _expect(lambda: pred.token_stream_tagged_packed(bad, bo), "must not contain NULL")


class _Foreign:
    """A tagger handle of another predictor, whatever predictor asks."""

    def __init__(self, tagger, pred):
        self._h = tagger.handle(pred)

    def handle(self, _):
        return self._h


# ---- the filter through its device entry: labels of the caller's, so that the tokens on every edge are chosen
def device_filtered(pred, tagger, texts, labels, stop, per_block=None, capacity=None):
    """fill_tags, the tagged spans and the filter on a workspace of the caller's -> ((offsets, starts, ends, positions, tag strings), the arrays)."""
    A = Arrays(pred, texts, labels)
    if per_block:
        os.environ["VPT_EMIT_PER_BLOCK"] = str(per_block)
    try:
        batch = api.DeviceBatch(pred)
    finally:
        os.environ.pop("VPT_EMIT_PER_BLOCK", None)
    batch.set_pattern_tagger(tagger)
    cap = A.n_tok if capacity is None else capacity
    G = tagoffsetsuite.Guarded
    O = {"offsets": G(np.full(A.S + 1, 7, np.uint64)), "starts": G(np.full(cap, GUARD, np.uint32)), "ends": G(np.full(cap, GUARD, np.uint32)),
         "positions": G(np.full(cap, GUARD, np.uint32)), "tags": G(np.full(cap * max(A.nt, 1), GUARD, np.int32))}
    A.fill(batch)
    A.spans(batch)
    batch.token_filter(stop, A.d_toff.ptr, A.d_ends.ptr, A.d_tags.ptr, A.S, A.n_tok, O["offsets"].ptr, O["starts"].ptr, O["ends"].ptr,
                       O["positions"].ptr, O["tags"].ptr, cap, devmem.stream())
    try:
        batch.sync()
        raised = None
    except api.VaporettoError as e:
        raised = str(e)
    assert not [k for k, a in O.items() if not a.guards_intact()]
    if raised:
        return raised, O
    off = [int(x) for x in O["offsets"].get()]
    n = off[-1]
    vocab = pred.tag_strings()
    rule = [tagger.tag(pred, k) for k in range(tagger.n_tags(pred))] if tagger is not None and A.nt else []
    tags = O["tags"].get(n * A.nt).reshape(n, A.nt)
    names = [tuple(None if v == -1 else vocab[v] if v >= 0 else rule[-2 - v] for v in (int(x) for x in row)) for row in tags]
    return (off, [int(x) for x in O["starts"].get(n)], [int(x) for x in O["ends"].get(n)], [int(x) for x in O["positions"].get(n)], names), O


def check_filter_edges():
    """Kept and dropped tokens on both sides of the piece, wave, span-run and fill_tags-run edges and of the filter's block edge; a whole span run
    that loses every token; the capacity one short."""
    pred = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    tile = vpt_filter_tile()
    # token number tile - 1 of the batch is "う", number tile is "AB" (a rule's tag): under DROP_U the edge has a dropped token in front and a kept one behind, under
    # DROP_REST the other way round; the same again two blocks on
    docs = [["A"] * (tile - 1) + ["う", "AB"] + ["AB"] * (2 * tile - 2) + ["う", "漢字"]]
    for edge in (PIECE, WAVE, 2 * PIECE):
        for shift in (-3, -1, 0, 1):
            docs.append(["う"] + ["A"] * (edge + shift - 8) + ["AB", "う", "漢字", "う", "あい", "う"])
    docs += [["う"], ["う"], ["漢字"], ["う", "A", "う"], ["あい"], ["う"]] * 30     # under DROP_U and runs of one or three documents: whole span runs without a token
    texts, labels = labels_of(docs)
    flat = [t for d in docs for t in d]
    assert flat[tile - 1] == "う" and flat[tile] == "AB" and flat[3 * tile - 1] == "う" and flat[3 * tile] == "漢字"
    tagger = api.PatternMatchTagger(RULES)
    drop_u = [(0, "p"), (0, "q")]
    drop_rest = [(0, "名"), (0, "動"), (0, "x"), (0, "rA"), (1, "rule"), (0, "d")]
    _, _, ooff = patterntagsuite.pack(texts)
    unfiltered = tokentagref.token_tags(pred, texts, ooff, labels, tagger)
    for pairs in (drop_u, drop_rest, None):
        want = tokentagref.five_arrays(unfiltered, pairs)
        kept = [not (pairs and tokentagref.stopped(t[3], pairs)) for d in unfiltered for t in d]
        if pairs:
            assert kept[tile - 1] != kept[tile] and kept[3 * tile - 1] != kept[3 * tile]   # the filter's block edge
            assert any(a == b for a, b in zip(want[0], want[0][1:]))   # documents -- with runs of one document whole span runs -- that keep no token
        stop = api.TagStopFilter(pred, pairs, tagger) if pairs else None
        for per_block in (None, 1, 3):
            got, _ = device_filtered(pred, tagger, texts, labels, stop, per_block)
            assert list(got) == list(want), (pairs, per_block)
    # capacity one token too small: the verdict at the sync, nothing behind any of the five arrays; the exact capacity is enough
    want = tokentagref.five_arrays(unfiltered, drop_u)
    stop = api.TagStopFilter(pred, drop_u, tagger)
    raised, _ = device_filtered(pred, tagger, texts, labels, stop, capacity=len(want[2]) - 1)
    assert isinstance(raised, str) and "text_capacity" in raised
    got, _ = device_filtered(pred, tagger, texts, labels, stop, capacity=len(want[2]))
    assert list(got) == list(want)


def run_filter_hostile():
    """token_offsets that are no offsets and capacities that do not hold the CSR, through vpt_token_filter_batch_device alone: never a write outside
    the five arrays (guard words; the emulator's red zones) and never a read outside the inputs (red zones; exact-size inputs); then the true
    arrays on the same workspace give the plain compaction.  -> the cases run"""
    pred = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    nt, S = pred.n_tags(), 40
    rng = random.Random(7)
    counts = [rng.randint(0, 30) for _ in range(S)]   # empty documents among them
    true_off = np.zeros(S + 1, np.uint64)
    true_off[1:] = np.cumsum(counts)
    N = int(true_off[-1])
    ends = np.arange(1, N + 1, dtype=np.uint32)
    vocab = pred.tag_strings()
    tags = np.array([[rng.choice([-1, 0, 1, len(vocab) - 1, -2, -3, 999999, -999999]) for _ in range(nt)] for _ in range(N)], np.int32)
    stop = api.TagStopFilter(pred, [(0, vocab[0]), (1, vocab[1]), (2, vocab[-1])])
    G = tagoffsetsuite.Guarded
    batch = api.DeviceBatch(pred)
    st = devmem.stream()

    def run(off, cap_in, cap_out, expect_error=None):
        I = {"off": G(off), "ends": G(ends[:max(cap_in, 1)]), "tags": G(tags[:max(cap_in, 1)].reshape(-1))}
        O = {"offsets": G(np.full(S + 1, 7, np.uint64)), "starts": G(np.full(max(cap_out, 1), GUARD, np.uint32)), "ends": G(np.full(max(cap_out, 1), GUARD, np.uint32)),
             "positions": G(np.full(max(cap_out, 1), GUARD, np.uint32)), "tags": G(np.full(max(cap_out, 1) * nt, GUARD, np.int32))}
        batch.token_filter(stop, I["off"].ptr, I["ends"].ptr, I["tags"].ptr, S, cap_in, O["offsets"].ptr, O["starts"].ptr, O["ends"].ptr, O["positions"].ptr,
                           O["tags"].ptr, cap_out, st)
        try:
            batch.sync()
            raised = None
        except api.VaporettoError as e:
            raised = str(e)
        assert not [k for k, a in list(I.items()) + list(O.items()) if not a.guards_intact()], "guard words overwritten"
        if expect_error is not None:
            assert (raised is not None) == expect_error, raised
        for k in ("starts", "ends", "positions"):   # (an array of max(cap_out, 1) entries: with cap_out == 0 its one entry is untouched too)
            assert (O[k].get()[cap_out:] == GUARD).all(), k
        return raised, O

    def stopped(row):
        return (row[0] == 0) or (nt > 1 and row[1] == 1) or (nt > 2 and row[2] == len(vocab) - 1)

    keep = [not stopped(r) for r in tags]
    K = sum(keep)
    ran = 0
    hostile = {
        "all_zero": np.zeros(S + 1, np.uint64), "all_total": np.full(S + 1, N, np.uint64), "huge": np.full(S + 1, 1 << 63, np.uint64),
        "max": np.full(S + 1, (1 << 64) - 1, np.uint64), "sawtooth": np.array([N - i if i & 1 else i for i in range(S + 1)], np.uint64),
        "decreasing": true_off[::-1].copy(), "last_larger": np.concatenate([true_off[:-1], [N + 1000]]).astype(np.uint64),
        "one_huge": np.concatenate([true_off[:5], [1 << 40], true_off[6:]]).astype(np.uint64),
    }
    for name, off in hostile.items():
        for cap_in, cap_out in ((N, N), (N // 2, N), (N, 3), (0, 0)):
            run(off, cap_in, cap_out)
            ran += 1
    # capacity_in smaller than token_offsets[n] on true offsets: only the first capacity_in tokens are looked at
    run(true_off, N // 2, N)
    run(true_off, N, K - 1, expect_error=True)   # one kept token too many for the output
    ran += 2
    raised, O = run(true_off, N, K, expect_error=False)
    ran += 1
    want_off, want_pos, want_start = [0], [], []
    for d in range(S):
        a, b = int(true_off[d]), int(true_off[d + 1])
        for k in range(a, b):
            if keep[k]:
                want_pos.append(k - a)
                want_start.append(int(ends[k - 1]) if k > a else 0)
        want_off.append(len(want_pos))
    assert [int(x) for x in O["offsets"].get()] == want_off
    assert [int(x) for x in O["positions"].get(K)] == want_pos and [int(x) for x in O["starts"].get(K)] == want_start
    assert np.array_equal(O["ends"].get(K), ends[np.array(keep)]) and np.array_equal(O["tags"].get(K * nt).reshape(K, nt), tags[np.array(keep)])
    del batch
    return ran


def main(argv):
    usage = "usage: python -m tests.tokentagsuite --emu-hostile BATCH VARIANT | --emu-filter"
    assert argv and argv[0] in ("--emu-hostile", "--emu-filter"), usage
    import gc
    from tests import emu
    _lib._lib = emu.load()
    devmem.EMULATED = True
    if argv[0] == "--emu-filter":
        ran = run_filter_hostile()
    else:
        assert len(argv) == 3, usage
        ran = run_hostile_group(argv[1], argv[2], lambda line: print(line, flush=True))
    gc.collect()   # batch and predictor destroyed: hipemu has checked the red zones of every allocation it freed
    print("ran %d cases" % ran, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
