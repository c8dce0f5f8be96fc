"""TEST INFRASTRUCTURE: the device-resident add calls of the trainer (vpt_trainer_add_batch_device, vpt_trainer_add_tagged_batch_device)
as a device caller meets them -- the checks tests/test_train_device_emu.py runs on the CPU emulator and tests/test_train_device_gpu.py
on the MI355X.  Every comparison is exact (integers, keys, model bytes): against the restatements of tests/trainref.py and
tests/tagtrainref.py, and against a trainer fed the same sentences through the host calls (the header promises byte-identical models
for the same examples and arguments).

`ctx` is (lib, predictor handle, workspace handle) as in tests/partialsuite.py: the two device parsers need them.  Device buffers come
from tests/devmem.py; `stream` is a raw HIP stream (0: the default one)."""
import functools

import numpy as np
import pytest

from tests import devmem, partialsuite, tagtrainref, tagtrainsuite, trainref, trainsuite
from vaporetto_amd import _lib, api

KEYS, DTYPES = partialsuite.KEYS, partialsuite.DTYPES
FILLER = 0xE3            # the lead byte of a 3-byte char: a read outside the text decodes it into a wrong char
EPS, COST = 0.01, 1.0
M_START = "InvalidArgumentError: out_offsets: must start at 0"
M_TOTAL = "InvalidArgumentError: total_boundaries: must equal out_offsets[n_sentences]"
M_LABEL = "InvalidArgumentError: labels: must be 0, 1 or 2"


# ---------------------------------------------------------------------------------------------------- corpora and references
def params_of(case):
    seed, charw, charn, typew, typen, dictn, with_dict = case
    return charw, charn, typew, typen, dictn


@functools.lru_cache(maxsize=None)
def corpus(case, n_sent=60, unknown=0.1):
    """(sentences, dictionary words) of a trainsuite case; tokenized text has no mark for Unknown, so the parser's corpus has none"""
    sents = trainsuite.corpus(case[0], n_sent, unknown=unknown)
    return sents, (trainsuite.dictionary(sents, case[0]) if case[6] else [])


def make_trainer(case, words, **kw):
    charw, charn, typew, typen, dictn = params_of(case)
    return api.Trainer(charw, charn, typew, typen, words, dictn if words else 0, **kw)


def reference(case, words, sents):
    """(keys, row_ptr, cols, counts) of RefTrainer.matrix()"""
    charw, charn, typew, typen, dictn = params_of(case)
    r = trainref.RefTrainer(charw, charn, typew, typen, words, dictn)
    for text, lab in sents:
        r.add_example(text, lab)
    return r.matrix()[:4]


@functools.lru_cache(maxsize=None)
def corpus_reference(case, n_sent=60, unknown=0.1, first=None):
    sents, words = corpus(case, n_sent, unknown)
    return reference(case, words, sents[:first])


def host_trainer(case, words, sents, **kw):
    t = make_trainer(case, words, **kw)
    t.add_packed(*api.pack_texts([s.encode("utf-8") for s, _ in sents]), np.concatenate([lab for _, lab in sents]))
    return t


def assert_matrix(t, ref, keys_too=False):
    keys, ptr, cols, cnt = ref
    assert t.n_features() == len(keys)
    gptr, gcols, gcnt = t.csr()
    assert np.array_equal(gptr.astype(np.int64), ptr)
    assert np.array_equal(gcols.astype(np.int64), cols)
    assert np.array_equal(gcnt.astype(np.float64), cnt)
    if keys_too:   # the keys come back with the weights
        t.train_bytes(EPS, COST, 2)
        assert t.weights()[2] == keys


def tokenized_line(text, lab):
    def esc(tok):
        return "".join("\\" + c if c in " \\/" else c for c in tok)
    cuts = [0] + [i + 1 for i, b in enumerate(lab) if b == 1] + [len(text)]
    return " ".join(esc(text[a:b]) for a, b in zip(cuts, cuts[1:]))


# ---------------------------------------------------------------------------------------------------- buffers
class Placed:
    """A batch in device buffers.  The text lies inside a larger buffer of FILLER bytes: `lead` of them in front, of which d_utf8 skips k
    (so the offsets start at lead - k), and the last sentence's last byte directly in front of `tail` more -- no zero padding."""

    def __init__(self, sents, k=0, lead=0, tail=0, labels=None, ooff=None):
        self.n = len(sents)
        utf8, boff = api.pack_texts([s.encode("utf-8") for s, _ in sents])
        self.ooff = api.count_boundaries(utf8, boff) if ooff is None else ooff
        self.total = int(api.count_boundaries(utf8, boff)[-1]) if self.n else 0
        lab = np.concatenate([np.asarray(lab, np.uint8) for _, lab in sents] + [np.zeros(0, np.uint8)]) if labels is None else labels
        fill = np.full(1, FILLER, np.uint8)
        self.text = devmem.put(np.concatenate([fill.repeat(lead), utf8, fill.repeat(tail), np.zeros(0 if lead + len(utf8) + tail else 1, np.uint8)]))
        self.d_utf8 = self.text.ptr + k
        self.boff = devmem.put(boff + np.uint64(lead - k))
        self.d_ooff = devmem.put(self.ooff)
        self.labels = devmem.put(lab if len(lab) else np.zeros(1, np.uint8))
        self.d_labels = self.labels.ptr if len(lab) else 0

    def args(self, total=None):
        return self.d_utf8, self.boff.ptr, self.d_ooff.ptr, self.n, self.total if total is None else total, self.d_labels

    def scribble(self):
        """0xFF over everything the caller owns: the trainer must have kept nothing that points into it"""
        for b in (self.text, self.boff, self.d_ooff, self.labels):
            a = b.get()
            b.set(np.full(len(a), 0xFF, a.dtype))


def tag_buffers(arrays):
    """(n_tags, tag_index, span_offsets, tag_bytes) of tagtrainsuite.pack in device buffers -> (buffers, the call's tag arguments)"""
    n_tags, tindex, so, tb = (np.array(a) for a in arrays)   # (copies: pack_texts' bytes are read-only)
    bufs = [devmem.put(n_tags if len(n_tags) else np.zeros(1, np.uint32)), devmem.put(tindex), devmem.put(so),
            devmem.put(tb if len(tb) else np.zeros(1, np.uint8))]
    return bufs, (bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr if len(tb) else 0, len(so) - 1, len(tb))


def device_parse(ctx, lines, kind, stream):
    """Enqueues vpt_parse_<kind>_batch_device on `stream` and returns its buffers WITHOUT a synchronisation of any sort."""
    lib, pred, batch = ctx
    utf8, boff = api.pack_texts([ln.encode("utf-8") for ln in lines])
    S, cap = len(lines), len(utf8)
    _, bufs = partialsuite.parse_buffers(S, cap, 0xAB)
    bufs["_in"] = (devmem.put(np.concatenate([utf8, np.zeros(16, np.uint8)])), devmem.put(boff))
    st = getattr(lib, "vpt_parse_%s_batch_device" % kind)(pred, batch, bufs["_in"][0].ptr, bufs["_in"][1].ptr, S, cap, *[bufs[k].ptr for k in KEYS], stream)
    assert st == 0, lib.vpt_last_error()
    return bufs


def parse_ok(ctx):
    lib, _, batch = ctx
    assert lib.vpt_batch_sync(batch) == 0, lib.vpt_last_error()


def host_total(sents):
    """total_boundaries as a caller computes it: vpt_count_boundaries over the raw text, on the host"""
    return int(api.count_boundaries(*api.pack_texts([s[0].encode("utf-8") for s in sents]))[-1])


# ---------------------------------------------------------------------------------------------------- (a) parser into trainer
def check_parser_into_trainer(ctx, case, stream=0):
    sents, words = corpus(case, unknown=0.0)
    lines = [tokenized_line(*s) for s in sents]
    t = make_trainer(case, words)
    p = device_parse(ctx, lines, "tokenized", stream)
    t.add_device(p["raw"].ptr, p["raw_offsets"].ptr, p["out_offsets"].ptr, len(sents), host_total(sents), p["labels"].ptr, 0, stream)
    parse_ok(ctx)
    assert_matrix(t, corpus_reference(case, unknown=0.0), keys_too=True)
    assert t.train_bytes(EPS, COST, 2) == host_trainer(case, words, sents).train_bytes(EPS, COST, 2)


# ---------------------------------------------------------------------------------------------------- (b) placement
def check_placement(case, stream=0):
    sents, words = corpus(case)
    sents = sents[:20]
    ref = corpus_reference(case, first=20)
    assert any(len(s) == 1 for s, _ in sents)
    for k in range(16):
        t = make_trainer(case, words)
        b = Placed(sents, k=k, lead=16 + 21, tail=48)
        assert int(b.boff.get()[0]) == 37 - k != 0
        t.add_device(*b.args(), 0, stream)
        assert_matrix(t, ref)


# ---------------------------------------------------------------------------------------------------- (c) shapes
SHAPE_CASE = (0, 3, 3, 2, 2, 3, True)
SHAPE_WORDS = ["あい", "い", "あいう", "\U00020B9F\U0002000B", "ａ", "１２", "アｱ"]


def _short_sentences(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.integers(1, 4))
        out.append(("".join("あいう\U00020B9Fa1"[j] for j in rng.integers(0, 6, ln)), rng.integers(0, 3, ln - 1).astype(np.uint8)))
    return out


def shapes():
    """name -> (sentences, fullwidth)"""
    nb = "\U00020B9F\U0002000B"
    lone = [("あ", np.zeros(0, np.uint8)), ("いあい", np.array([1, 0], np.uint8)), ("う", np.zeros(0, np.uint8)),
            ("あいう漢", np.array([0, 1, 2], np.uint8)), ("字", np.zeros(0, np.uint8))]
    return {
        "300_short": (_short_sentences(300, 5), False),          # launch_decode_chars cuts two runs (at most 256 sentences a workgroup)
        "one_char_first_middle_last": (lone, False),
        "four_byte_chars_only": ([(nb + nb[::-1] + nb, np.array([1, 0, 0, 1, 0], np.uint8)), ("あい", np.array([0], np.uint8))], False),
        "fullwidth_mix": ([("aａ1１2２ｱアｶﾞ-ー", np.array([0, 1, 0, 1, 0, 1, 0, 1, 2, 0, 1], np.uint8)), ("12あい１２", np.array([1, 0, 1, 0, 1], np.uint8))], True),
    }


def check_shape(name, stream=0):
    sents, fw = shapes()[name]
    if name == "300_short":
        assert len(sents) > 256 and all(1 <= len(s) <= 3 for s, _ in sents) and any(len(s) == 1 for s, _ in sents)
    t = make_trainer(SHAPE_CASE, SHAPE_WORDS)
    b = Placed(sents, tail=16)
    t.add_device(*b.args(), _lib.VPT_FLAG_KYTEA_FULLWIDTH if fw else 0, stream)
    seen = [(api.KyteaFullwidthFilter().filter(s) if fw else s, lab) for s, lab in sents]
    if fw:
        assert any(a != s for (a, _), (s, _) in zip(seen, sents))
    assert_matrix(t, reference(SHAPE_CASE, SHAPE_WORDS, seen), keys_too=True)


def check_no_boundary_batches(stream=0):
    """a batch of one-char sentences only (no boundary, d_labels NULL) and a batch of no sentence (NULL pointers): VPT_OK, no row"""
    sents, _ = shapes()["one_char_first_middle_last"]
    t = make_trainer(SHAPE_CASE, SHAPE_WORDS)
    t.add_device(*Placed(sents, tail=16).args(), 0, stream)
    ref = reference(SHAPE_CASE, SHAPE_WORDS, sents)
    for fresh in (False, True):
        u = make_trainer(SHAPE_CASE, SHAPE_WORDS) if fresh else t
        ones = Placed([("あ", []), ("\U00020B9F", []), ("a", [])], tail=16)
        assert ones.total == 0 and ones.d_labels == 0
        u.add_device(*ones.args(), 0, stream)
        u.add_device(0, 0, 0, 0, 0, 0, 0, stream)
        if not fresh:
            assert_matrix(u, ref)
    assert_matrix(t, ref, keys_too=True)
    tagged = make_trainer(SHAPE_CASE, SHAPE_WORDS, train_tags=True)
    tagged.add_tagged_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, stream)


# ---------------------------------------------------------------------------------------------------- (d) append order
def check_append_order(case, stream=0):
    sents, words = corpus(case)
    parts = [sents[12 * i:12 * (i + 1)] for i in range(5)]
    t = make_trainer(case, words)
    held = []
    for i, part in enumerate(parts):
        if i % 2 == 0:
            b = Placed(part, k=3 * i + 1, lead=32, tail=16)
            t.add_device(*b.args(), 0, stream)
            b.scribble()
            held.append(b)   # the buffers stay allocated, overwritten
        else:
            t.add_packed(*api.pack_texts([s.encode("utf-8") for s, _ in part]), np.concatenate([lab for _, lab in part]))
    assert len(held) == 3
    assert_matrix(t, corpus_reference(case), keys_too=True)
    assert t.train_bytes(EPS, COST, 2) == host_trainer(case, words, sents).train_bytes(EPS, COST, 2)


# ---------------------------------------------------------------------------------------------------- (e) tagged
TAG_PARAMS = tagtrainsuite.CASES["small"]


def tag_trainer(**kw):
    _, _, _, charw, charn, typew, typen = TAG_PARAMS
    return api.Trainer(charw, charn, typew, typen, train_tags=True, tag_dictionary=tagtrainsuite.TAG_DICTIONARY, **kw)


def as_written(sent):
    """The sentence a tokenized line carries: its slots are those of its widest token (a char's trailing Nones are not written)"""
    text, bounds, nt, tags = sent
    ends = [i for i, b in enumerate(bounds) if b == 1] + [len(text) - 1]
    width = 0
    for e in ends:
        row = list(tags[e * nt:(e + 1) * nt])
        while row and row[-1] is None:
            row.pop()
        width = max(width, len(row))
    return text, bounds, width, [tags[c * nt + j] for c in range(len(text)) for j in range(width)]


@functools.lru_cache(maxsize=None)
def tagged_corpus(kind):
    """kind "tokenized": (sentences as the lines carry them, lines).  kind "partial": Unknown boundaries, tags on chars that end no
    token, and chars that end in empty tags (None, but counted in n_tags); the sentences are the restatement's reading of the lines."""
    seed, n_sent, n_fill = TAG_PARAMS[:3]
    if kind == "tokenized":
        sents = [as_written(s) for s in tagtrainsuite.corpus(seed, n_sent, n_fill, unknown=0.0)]
        return sents, tagtrainsuite.tokenized_lines(sents)
    lines = []
    for i, (text, bounds, nt, tags) in enumerate(tagtrainsuite.corpus(seed, n_sent, n_fill)):
        tags = list(tags)
        if nt and len(text) > 2 and i % 4 == 0:
            tags[1 * nt] = "mid"   # the second char, wherever the tokens end
        s = api.Sentence.from_raw(text)
        s._boundaries, s._tags, s._n_tags = np.asarray(bounds, np.uint8), tags, nt
        lines.append(s.write_partial_annotation_text() + ("//" if i % 7 == 3 else ""))
    sents = []
    for ln in lines:
        s = api.Sentence.from_partial_annotation(ln)
        sents.append((s.as_raw_text(), np.asarray(s.boundaries(), np.uint8), s.n_tags(), list(s.tags())))
    assert any(2 in b for _, b, _, _ in sents) and any("/mid" in ln for ln in lines)
    assert any(ln.endswith("//") and nt > 1 and tg[-2:] == [None, None] for (_, _, nt, tg), ln in zip(sents, lines))
    return sents, lines


@functools.lru_cache(maxsize=None)
def tagged_reference(kind, first=None):
    """(the tag problems of tagtrainref, the boundary matrix of trainref)"""
    _, _, _, charw, charn, typew, typen = TAG_PARAMS
    sents = tagged_corpus(kind)[0][:first]
    r = tagtrainref.RefTagTrainer(charn, typen, tagtrainsuite.TAG_DICTIONARY)
    b = trainref.RefTrainer(charw, charn, typew, typen)
    for s in sents:
        r.add_example(*s)
        b.add_example(s[0], s[1])
    models = r.models()
    return [(m["token"], p) for m in models for p in m["problems"]], len(models), b.matrix()[:4]


def assert_tag_problems(t, kind, first=None):
    ref, n_models, boundary = tagged_reference(kind, first)
    got = t.tag_problems()
    assert t.n_tag_models() == n_models
    assert [(g["surface"], g["slot"]) for g in got] == [(tok, p["slot"]) for tok, p in ref]
    assert len(ref) > 3
    for g, (tok, p) in zip(got, ref):
        assert g["candidates"] == p["candidates"]
        assert g["n_rows"] == len(p["y"])
        assert g["keys"] == p["keys"]
        assert np.array_equal(g["row_ptr"].astype(np.int64), p["row_ptr"])
        assert np.array_equal(g["cols"].astype(np.int64), p["cols"])
        assert np.array_equal(g["y"].astype(np.int64), p["y"])
    assert_matrix(t, boundary)


def host_tag_trainer(sents, **kw):
    t = tag_trainer(**kw)
    t.add_packed_tagged(*tagtrainsuite.pack(sents))
    return t


def check_tagged_from_parser(ctx, kind, stream=0, l1=False):
    """the parser's eight arrays into add_tagged_device; the caller knows the totals from the host (the host parser's span counts: the
    partial parser writes a char's trailing empty tags too)"""
    sents, lines = tagged_corpus(kind)
    host = (api.parse_tokenized_host if kind == "tokenized" else api.parse_partial_host)([ln.encode("utf-8") for ln in lines])
    n_spans, n_tag_bytes = len(host["span_offsets"]) - 1, len(host["tag_bytes"])
    total = host_total(sents)
    p = device_parse(ctx, lines, kind, stream)
    a = [p["raw"].ptr, p["raw_offsets"].ptr, p["out_offsets"].ptr, len(sents), total, p["labels"].ptr]
    kw = dict(l1r=True, l1r_tags=True) if l1 else {}
    t = tag_trainer(**kw)
    t.add_tagged_device(*a, p["n_tags"].ptr, p["tag_index"].ptr, p["span_offsets"].ptr, p["tag_bytes"].ptr, n_spans, n_tag_bytes, 0, stream)
    parse_ok(ctx)
    partialsuite.assert_same(api._trim_parsed({k: p[k].get() for k in KEYS}, len(sents)), host, kind)
    assert_tag_problems(t, kind)
    # the untagged call on the same buffers: the same boundary matrix
    _, _, _, charw, charn, typew, typen = TAG_PARAMS
    plain = api.Trainer(charw, charn, typew, typen)
    plain.add_device(*a, 0, stream)
    for x, y in zip(plain.csr(), t.csr()):
        assert np.array_equal(x, y)
    solver = 5 if l1 else 2
    assert t.train_bytes(EPS, COST, solver) == host_tag_trainer(sents, **kw).train_bytes(EPS, COST, solver)


def check_tagged_placement(stream=0):
    sents = tagged_corpus("partial")[0][:40]
    arrays = tagtrainsuite.pack(sents)
    for k in (0, 5, 15):
        t = tag_trainer()
        b = Placed([(s[0], s[1]) for s in sents], k=k, lead=16 + 21, tail=48)
        bufs, targs = tag_buffers(arrays[3:])
        t.add_tagged_device(*b.args(), *targs, 0, stream)
        assert_tag_problems(t, "partial", 40)


# ---------------------------------------------------------------------------------------------------- (f) refusals
def _state(t, tagged):
    return t.n_features(), t.csr(), t.tag_problems() if tagged else None


def _same_state(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)
    if a[2] is not None:
        assert len(a[2]) == len(b[2])
        for p, q in zip(a[2], b[2]):
            assert p.keys() == q.keys()
            for key in p:
                if key not in ("path",):
                    assert np.array_equal(p[key], q[key]) if isinstance(p[key], np.ndarray) else p[key] == q[key], key


REFUSALS = ("total_plus_1", "total_minus_1", "total_plus_10000", "offsets_start_at_1", "label_3", "label_255_last")
TAG_REFUSALS = REFUSALS + ("tag_index_decreases",)


def _bad_call(name, sents, arrays):
    """-> (Placed, total_boundaries, tag arrays, the message): the good batch with one thing wrong"""
    utf8, boff = api.pack_texts([s[0].encode("utf-8") for s in sents])
    true = int(api.count_boundaries(utf8, boff)[-1])
    pairs = [(s[0], s[1]) for s in sents]
    lab = np.concatenate([np.asarray(s[1], np.uint8) for s in sents] + [np.zeros(16, np.uint8)])   # room behind for the shifted offsets
    kw, total, msg = {"labels": lab}, true, M_TOTAL
    if name == "total_plus_1":
        total = true + 1
    elif name == "total_minus_1":
        total = true - 1
    elif name == "total_plus_10000":
        total = true + 10000
    elif name == "offsets_start_at_1":
        kw["ooff"], total, msg = api.count_boundaries(utf8, boff) + np.uint64(1), true + 1, M_START
    elif name == "label_3":
        lab[true // 2], msg = 3, M_LABEL
    elif name == "label_255_last":
        lab[true - 1], msg = 255, M_LABEL
    elif name == "tag_index_decreases":
        tindex = arrays[1].copy()
        k = int(np.flatnonzero(np.diff(tindex.astype(np.int64)) > 0)[0])
        tindex[k], tindex[k + 1] = tindex[k + 1], tindex[k]
        arrays, msg = (arrays[0], tindex, arrays[2], arrays[3]), "InvalidArgumentError: tag_index: "
    return Placed(pairs, k=2, lead=18, tail=16, **kw), total, arrays, msg


def check_refusal(name, tagged, stream=0):
    """On a trainer that holds one good batch: the refusal's status and message, the state as it was, and after a good add the model of a
    trainer that never saw the bad call."""
    if tagged:
        sents = tagged_corpus("partial")[0]
        first, second = sents[:30], sents[30:60]
        new = tag_trainer
    else:
        case = trainsuite.CASES[0]
        sents, words = corpus(case)
        first, second = sents[:20], sents[20:40]
        new = lambda: make_trainer(case, words)   # noqa: E731

    def add(t, part, bad=None):
        arrays = tagtrainsuite.pack(part)[3:] if tagged else None
        if bad:
            b, total, arrays, msg = _bad_call(bad, part, arrays)
        else:
            b, total, msg = Placed([(s[0], s[1]) for s in part], tail=16), None, None
        a = b.args(total)
        if tagged:
            bufs, targs = tag_buffers(arrays)
            call = lambda: t.add_tagged_device(*a, *targs, 0, stream)   # noqa: E731
        else:
            call = lambda: t.add_device(*a, 0, stream)   # noqa: E731
        if not bad:
            return call()
        with pytest.raises(api.VaporettoError) as e:
            call()
        assert e.value.kind == "InvalidArgument"
        assert str(e.value).startswith(msg) if msg.endswith(": ") else str(e.value) == msg, str(e.value)

    t = new()
    add(t, first)
    before = _state(t, tagged)
    add(t, second, bad=name)
    _same_state(before, _state(t, tagged))
    add(t, second)
    assert t.train_bytes(EPS, COST, 2) == clean_model(tagged)


@functools.lru_cache(maxsize=None)
def clean_model(tagged):
    """the two good batches through the host calls, on a trainer that saw nothing else"""
    if tagged:
        sents = tagged_corpus("partial")[0]
        t = tag_trainer()
        t.add_packed_tagged(*tagtrainsuite.pack(sents[:30]))
        t.add_packed_tagged(*tagtrainsuite.pack(sents[30:60]))
    else:
        case = trainsuite.CASES[0]
        sents, words = corpus(case)
        t = host_trainer(case, words, sents[:20])
        t.add_packed(*api.pack_texts([s.encode("utf-8") for s, _ in sents[20:40]]), np.concatenate([lab for _, lab in sents[20:40]]))
    return t.train_bytes(EPS, COST, 2)
