"""The checks of the postings pass (vpt_postings_batch_device, vpt_token_stream_postings_batch; kernels_postings.hip) against the definition
of tests/postingsref.py, run on the CPU emulator by tests/test_postings_emu.py and on the MI355X by tests/test_postings_gpu.py; every
comparison is exact integer equality.

    python -m tests.postingssuite --emu-hostile     the hostile CSRs on the emulator, in a child process (hipemu checks its red zones when
                                                    the workspace goes)

Every array handed to the device call has exactly the size the call is told and guard words on both sides, checked after the sync; outputs
are filled with SENTINEL first, so an entry the call must not write is seen to be left alone.  The sort's tile is T = vpt_postings_tile
(4096), the key pass's vpt_vocab_tile (256); no case has more than 3 T + 1 tokens.  check_doc_base runs the pass at the two HIGH_BASES too: a
batch that straddles document 2^31 and one whose last document is 0xFFFFFFFF (high_base; the search, phrase and merge suites use the same two)."""
import os
import random
import re
import sys

import numpy as np

from tests import devmem, kat, patterntagsuite, postingsref, tagoffsetsuite, tokentagsuite, vocabsuite
from vaporetto_amd import _lib, api

G = tagoffsetsuite.Guarded
SENTINEL = vocabsuite.SENTINEL
CSR_ERROR = vocabsuite.CSR_ERROR
SMALL_ERROR = "capacity: smaller than the number of postings"
predictor = vocabsuite.predictor
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def tile():
    return api.DeviceBatch.postings_tile()


HIGH_BASES = ("2^31-3", "2^32-n")   # the names the parametrised tests carry


def high_base(name, n_docs):
    """the doc_base of n_docs documents that straddle the sign bit of the document word / whose last document is 0xFFFFFFFF"""
    return {"2^31-3": (1 << 31) - 3, "2^32-n": (1 << 32) - n_docs}[name]


class Result:
    """what one call left: the error of the call or of its sync (or None), the five output arrays whole, the two counts"""

    def same_bytes(self, other):
        return self.error == other.error and all(getattr(self, k).tobytes() == getattr(other, k).tobytes()
                                                 for k in ("term", "docs", "tfs", "first", "order", "counts"))


def run(toff, ids, n_terms, doc_base=0, positions=True, cap_in=None, cap_out=None, batch=None, pred=None, n_docs=None):
    """vpt_postings_batch_device on guarded arrays of exactly the sizes the call is told"""
    pred = pred or predictor()
    batch = batch or api.DeviceBatch(pred)
    toff, ids = np.asarray(toff, np.uint64), np.asarray(ids, np.int32)
    cap_in = len(ids) if cap_in is None else cap_in
    cap_out = cap_in if cap_out is None else cap_out
    n_docs = len(toff) - 1 if n_docs is None else n_docs
    I = {"toff": G(toff), "ids": G(ids[:cap_in] if cap_in else np.zeros(1, np.int32))}
    O = {"term": G(np.full(n_terms + 1, SENTINEL, np.uint64)), "docs": G(np.full(max(cap_out, 1), SENTINEL, np.uint32)),
         "tfs": G(np.full(max(cap_out, 1), SENTINEL, np.uint32)), "counts": G(np.full(2, SENTINEL, np.uint64))}
    if positions:
        O["first"] = G(np.full(cap_out + 1, SENTINEL, np.uint64))
        O["order"] = G(np.full(max(cap_in, 1), SENTINEL, np.uint32))
    r = Result()
    r.error = None
    try:
        batch.postings(I["toff"].ptr, n_docs, I["ids"].ptr, cap_in, n_terms, doc_base, O["term"].ptr, O["docs"].ptr, O["tfs"].ptr, cap_out,
                       O["first"].ptr if positions else 0, O["order"].ptr if positions else 0, O["counts"].ptr, devmem.stream())
    except api.VaporettoError as e:
        r.error = str(e)
    try:
        batch.sync()
    except api.VaporettoError as e:
        r.error = r.error or str(e)
    bad = [k for k, a in list(I.items()) + list(O.items()) if not a.guards_intact()]
    assert not bad, ("guard words overwritten", bad)
    assert all(np.array_equal(a.get(), a.sent) for a in I.values()), "an input was written"
    r.cap_in, r.cap_out = cap_in, cap_out
    for k in ("term", "docs", "tfs", "counts"):
        setattr(r, k, O[k].get())
    r.first = O["first"].get() if positions else np.zeros(0, np.uint64)
    r.order = O["order"].get() if positions else np.zeros(0, np.uint32)
    r.positions = positions
    return r


def same_as_ref(r, ref):
    """every output of a call that succeeded is the definition's, and nothing behind what it had to write was touched"""
    assert r.error is None, r.error
    term, docs, tfs, first, order = ref.arrays()
    n_post, n_idx = len(docs), len(order)
    assert r.counts.tolist() == [n_post, ref.n_dropped], (r.counts.tolist(), n_post, ref.n_dropped)
    assert np.array_equal(r.term, term), [(k, int(a), int(b)) for k, (a, b) in enumerate(zip(r.term, term)) if a != b][:8]
    assert int(r.term[0]) == 0 and int(r.term[-1]) == n_post
    assert np.array_equal(r.docs[:n_post], docs) and np.array_equal(r.tfs[:n_post], tfs)
    assert (r.docs[n_post:r.cap_out] == SENTINEL).all() and (r.tfs[n_post:r.cap_out] == SENTINEL).all()
    if r.positions:
        assert np.array_equal(r.first[:n_post + 1], first) and (r.first[n_post + 1:] == SENTINEL).all()
        assert np.array_equal(r.order[:n_idx], order) and (r.order[n_idx:r.cap_in] == SENTINEL).all()


def check(toff, ids, n_terms, doc_base=0, batch=None, both=True):
    """one CSR against the definition, with the optional pair and (both) without"""
    ref = postingsref.Ref(toff, ids, n_terms, doc_base)
    for positions in ((True, False) if both else (True,)):
        same_as_ref(run(toff, ids, n_terms, doc_base, positions, batch=batch), ref)
    return ref


def csr(doc_ids):
    """documents as lists of ids -> (token_offsets, ids)"""
    toff, ids = [0], []
    for d in doc_ids:
        ids += list(d)
        toff.append(len(ids))
    return np.array(toff, np.uint64), np.array(ids, np.int64).astype(np.int32)


def zipf(rng, n_terms):
    return min(int(n_terms * (rng.random() ** 4)), n_terms - 1)


# ---- 1
def check_random(seed):
    """1-40 documents of 0-300 tokens; ids uniform and Zipf-like over n_terms; a share of dropped values"""
    rng = random.Random(seed)
    batch = api.DeviceBatch(predictor())
    for n_terms, skew in ((1, False), (7, True), (300, False), (300, True), (70000, True)):
        docs = []
        for _ in range(rng.randint(1, 40)):
            n = rng.choice([0, 0, 1, 2]) if rng.random() < 0.2 else rng.randint(0, 300)
            d = [zipf(rng, n_terms) if skew else rng.randrange(n_terms) for _ in range(n)]
            docs.append([rng.choice([-1, n_terms, n_terms + 5, INT32_MIN, INT32_MAX]) if rng.random() < 0.1 else x for x in d])
        toff, ids = csr(docs)
        ref = check(toff, ids, n_terms, batch=batch)
        assert len(ids) <= 3 * tile() + 1 and (len(ids) == 0 or ref.n_dropped > 0 or len(ids) < 10)


# ---- 2
def token_count(name):
    """"65", "T-1", "2T+1", ... -> the number (T is read from the library, so the parametrised tests name their sizes)"""
    m = re.fullmatch(r"(\d*)(T?)([+-]\d+)?", name)
    return (int(m.group(1) or 1) * (tile() if m.group(2) else 1)) + int(m.group(3) or 0)


def check_token_counts(n):
    """n tokens as one document and as many"""
    rng = random.Random(n)
    batch = api.DeviceBatch(predictor())
    ids = [zipf(rng, 50) if k % 11 else -1 for k in range(n)]
    check(*csr([ids]), 50, batch=batch, both=False)
    docs, a = [], 0
    while a < n:
        b = min(n, a + rng.choice([0, 1, 1, 2, 5, 40, 300]))
        docs.append(ids[a:b])
        a = b
    check(*csr(docs), 50, batch=batch, both=False)


# ---- 3
N_TERMS_EDGES = [1, 2, 255, 256, 257, 65535, 65536, 65537, 1 << 24]


def check_n_terms(n_terms):
    """ids 0 and n_terms - 1 and a dropped n_terms, on each side of the number of the sort's passes"""
    hi = n_terms - 1
    docs = [[hi, 0, n_terms, hi], [], [0, hi, hi // 2, n_terms, 0], [hi]]
    ref = check(*csr(docs), n_terms, both=False)
    assert ref.n_dropped == 2 and (ref.terms[hi] == {0: 2, 2: 1, 3: 1} if n_terms > 1 else ref.terms == {0: {0: 3, 2: 4, 3: 1}})


# ---- 4
def check_runs():
    T = tile()
    n = 2 * T + 1
    batch = api.DeviceBatch(predictor())
    r = check(*csr([[3] * n]), 5, batch=batch, both=False)            # one posting of tf n
    assert r.terms == {3: {0: n}}
    r = check(*csr([[3]] * n), 5, batch=batch, both=False)            # n postings of tf 1
    assert len(r.terms[3]) == n
    perm = list(range(n))
    random.Random(4).shuffle(perm)
    check(*csr([perm[:100], perm[100:T + 3], perm[T + 3:]]), n, batch=batch, both=False)   # every token a distinct id
    check(*csr([[1, 0] * T + [1]]), 2, batch=batch, both=False)                             # two ids alternating, one document
    check(*csr([[k & 1] * 3 for k in range(n // 3)]), 2, batch=batch, both=False)
    # a (term, document) run that starts one before and ends one after an edge of the SORTED order: the documents come in descending term
    # order, so the sort turns the batch round; terms ascend over the sorted places, a run per term
    for edge in (64, 256, T, 2 * T):
        for length in (2, 3):
            if edge + length > 3 * T + 1:
                continue
            runs = [edge - 1, length, 5]                  # term 0 fills the places below edge - 1; term 1 is the run; term 2 behind it
            docs = [[2] * runs[2], [1] * runs[1], [0] * (runs[0] - 1), [0]]
            ref = check(*csr(docs), 3, batch=batch, both=False)
            assert ref.arrays()[3].tolist() == [0, edge - 2, edge - 1, edge - 1 + length, edge + length + 4]


# ---- 5
def check_empty_documents():
    """runs of 0, 1 and 3 empty documents on both sides of every key-tile edge up to 3 tiles, first and last document empty, and a tile whose
    documents do not fit the LDS slice (600 one-token documents)"""
    kt = api.Vocabulary.tile()
    n = 3 * kt + 2
    flat = [(7 * k + k // 5) % 23 for k in range(n)]
    batch = api.DeviceBatch(predictor())
    for empties in (0, 1, 3):
        cuts = sorted({m * kt + d for m in (1, 2, 3) for d in (-1, 0, 1)})
        docs, a = [[]] * empties, 0
        for cut in cuts + [n]:
            docs.append(flat[a:cut])
            docs += [[]] * empties
            a = cut
        assert sum(len(d) for d in docs) == n
        ref = check(*csr(docs), 23, batch=batch, both=False)
        assert max(d for t in ref.terms.values() for d in t) < len(docs)
    check(*csr([[]] + [[t] for t in flat[:kt]] + [[]] * 700 + [[t] for t in flat[kt:2 * kt + 1]]), 23, batch=batch, both=False)
    check(*csr([[t] for t in flat[:600]]), 23, batch=batch, both=False)
    for count in (1, kt, kt + 1):
        check(*csr([[], flat[:count - 1], [], [], [], flat[count - 1:count], []]), 23, batch=batch, both=False)
    r = run(*csr([[], [], []]), 23, batch=batch)   # no token at all
    same_as_ref(r, postingsref.Ref([0, 0, 0, 0], [], 23))
    assert int(r.first[0]) == 0 and not r.term.any()


# ---- 6
def check_dropped():
    n_terms = 9
    bad = [-1, INT32_MIN, n_terms, INT32_MAX]
    docs = [[4, -1, 4, INT32_MIN], [n_terms, 8, INT32_MAX, 0], bad, []]
    ref = check(*csr(docs), n_terms)
    assert ref.n_dropped == 8 and ref.terms == {4: {0: 2}, 8: {1: 1}, 0: {1: 1}}
    toff, ids = csr([bad * 70, bad, [], bad * 3])   # every token dropped
    r = run(toff, ids, n_terms)
    same_as_ref(r, postingsref.Ref(toff, ids, n_terms))
    assert r.counts.tolist() == [0, len(ids)] and not r.term.any() and int(r.first[0]) == 0
    # the pass sees ids only: an unk_id inside the range is a term like any other
    ref = check(*csr([[2, 2, 1], [2]]), 3)
    assert ref.n_dropped == 0 and ref.terms[2] == {0: 2, 1: 1}


# ---- 7
def check_stability(seed=9):
    rng = random.Random(seed)
    n_terms = 40
    docs = [[zipf(rng, n_terms) if rng.random() < 0.9 else -1 for _ in range(rng.randint(0, 200))] for _ in range(30)]
    toff, ids = csr(docs)
    r = run(toff, ids, n_terms)
    assert r.error is None
    n_post = int(r.counts[0])
    seen = []
    for q in range(n_post):
        toks = r.order[int(r.first[q]):int(r.first[q + 1])].tolist()
        assert toks == sorted(toks) and len(toks) == int(r.tfs[q]) and len(set(toks)) == len(toks)
        d = int(r.docs[q])
        assert all(int(toff[d]) <= t < int(toff[d + 1]) for t in toks) and len({int(ids[t]) for t in toks}) == 1
        seen += toks
    indexed = [t for t in range(len(ids)) if 0 <= ids[t] < n_terms]
    assert sorted(seen) == indexed and len(seen) == int(r.first[n_post]) == len(ids) - int(r.counts[1])


# ---- 8
def check_doc_base():
    docs = [[1, 0, 1], [], [2, 1], [0]]
    toff, ids = csr(docs)
    n = len(docs)
    base = run(toff, ids, 3)
    same_as_ref(base, postingsref.Ref(toff, ids, 3))
    for doc_base in (7, high_base("2^31-3", n), (1 << 32) - n):
        r = run(toff, ids, 3, doc_base)
        same_as_ref(r, postingsref.Ref(toff, ids, 3, doc_base))
        k = int(r.counts[0])
        assert (r.docs[:k].astype(np.uint64) - base.docs[:k].astype(np.uint64) == doc_base).all()
        assert r.term.tobytes() == base.term.tobytes() and r.tfs.tobytes() == base.tfs.tobytes() and r.order.tobytes() == base.order.tobytes()
    r = run(toff, ids, 3, (1 << 32) - n + 1)
    assert r.error is not None and "doc_base: doc_base + n_documents must not exceed 2^32" in r.error
    assert (r.term == SENTINEL).all() and (r.counts == SENTINEL).all()   # refused at the call: nothing ran


# ---- 9
def check_capacity():
    rng = random.Random(2)
    docs = [[zipf(rng, 30) for _ in range(rng.randint(0, 90))] for _ in range(12)]
    toff, ids = csr(docs)
    ref = postingsref.Ref(toff, ids, 30)
    term, rdocs, rtfs, first, order = ref.arrays()
    needed = len(rdocs)
    assert 3 < needed < len(ids)
    batch = api.DeviceBatch(predictor())
    for cap_out in (needed - 1, 0):
        r = run(toff, ids, 30, cap_out=cap_out, batch=batch)
        assert r.error is not None and SMALL_ERROR in r.error, r.error
        assert int(r.counts[0]) == needed and int(r.counts[1]) == ref.n_dropped
        # what fits is the definition's; (guards: run)
        assert np.array_equal(r.docs[:cap_out], rdocs[:cap_out]) and np.array_equal(r.tfs[:cap_out], rtfs[:cap_out])
        assert np.array_equal(r.first[:cap_out], first[:cap_out]) and int(r.first[cap_out]) == SENTINEL
    same_as_ref(run(toff, ids, 30, cap_out=needed, batch=batch), ref)   # exactly enough, on the workspace that reported the error


# ---- 10
def check_determinism(seed=12):
    rng = random.Random(seed)
    T = tile()
    docs = [[zipf(rng, 500) if rng.random() < 0.95 else -3 for _ in range(rng.randint(0, 400))] for _ in range(2 * T // 200)]
    toff, ids = csr(docs)
    pred = predictor()
    one, two = api.DeviceBatch(pred), api.DeviceBatch(pred)
    a = run(toff, ids, 500, batch=one)
    b = run(toff, ids, 500, batch=one)
    run(*csr([[1, 2, 3] * 50]), 4, batch=two)   # (the second workspace's scratch holds something else)
    c = run(toff, ids, 500, batch=two)
    assert a.error is None and a.same_bytes(b) and a.same_bytes(c)
    same_as_ref(a, postingsref.Ref(toff, ids, 500))


# ---- 11
def hostile_cases():
    docs = [[1, 0, 1, 2, 2], [0, 3, 1, 1], [], [2, 0, 0]]
    toff, ids = csr(docs)
    N = len(ids)
    rng = np.random.RandomState(5)
    wild = rng.randint(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32).view(np.int32)
    cases = {   # name -> (token_offsets, ids, capacity_in, an error is expected)
        "decreasing_offsets": ([0, 5, 3, 3, N], ids, N, True),
        "sawtooth_offsets": ([0, N, 0, N, N], ids, N, True),
        "offsets_past_capacity": ([0, 3, 7, 7, N + 1000], ids, N, True),
        "offsets_past_capacity_small": (toff, ids, N - 2, True),
        "first_offset_above_zero": ([2, 5, 9, 9, N], ids, N, True),
        "last_offset_far_beyond": ([0, 5, 9, 9, 1 << 62], ids, N, True),
        "huge_offsets": ([0, 1 << 40, 1 << 41, 1 << 62, (1 << 64) - 1], ids, N, True),
        "random_ids": (toff, wild, N, False),
    }
    return toff, ids, cases


N_HOSTILE = 8


def run_hostile():
    toff, ids, cases = hostile_cases()
    assert len(cases) == N_HOSTILE
    batch = api.DeviceBatch(predictor())
    want = postingsref.Ref(toff, ids, 4)
    ran = 0
    for name, (h_toff, h_ids, cap, is_error) in cases.items():
        for positions in (True, False):
            r = run(h_toff, h_ids, 4, positions=positions, cap_in=cap, cap_out=len(ids), batch=batch)
            if is_error:
                assert r.error is not None and CSR_ERROR in r.error, (name, r.error)
            else:
                same_as_ref(r, postingsref.Ref(h_toff, h_ids, 4))
            # the true arrays on the same workspace: the verdict was reported once, the result is the definition's
            same_as_ref(run(toff, ids, 4, positions=positions, batch=batch), want)
        ran += 1
    del batch
    return ran


# ---- 12
def check_errors():
    pred = predictor()
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    toff, ids = csr([[1, 0], [1]])
    assert "n_terms: must be between 1 and 2^24" in run(toff, ids, 0).error
    assert "n_terms: must be between 1 and 2^24" in run(toff[:1], ids[:0], (1 << 24) + 1, cap_out=1).error
    assert "fewer than 2^32 tokens" in run(toff, ids, 2, positions=False, cap_in=1 << 32, cap_out=4).error
    assert "doc_base: doc_base + n_documents must not exceed 2^32" in run(toff, ids, 2, doc_base=(1 << 32) - 1).error
    assert "doc_base: doc_base + n_documents must not exceed 2^32" in run(toff, ids, 2, doc_base=1 << 33).error
    # a NULL mandatory pointer, each in turn; only one of the optional pair; p and b that do not match
    batch = api.DeviceBatch(pred)
    A = {k: devmem.zeros(8, dt) for k, dt in (("toff", np.uint64), ("ids", np.int32), ("term", np.uint64), ("docs", np.uint32), ("tfs", np.uint32),
                                             ("first", np.uint64), ("order", np.uint32), ("counts", np.uint64))}

    def call(**null):
        p = {k: (0 if k in null else a.ptr) for k, a in A.items()}
        batch.postings(p["toff"], 2, p["ids"], 3, 2, 0, p["term"], p["docs"], p["tfs"], 3, p["first"], p["order"], p["counts"], devmem.stream())

    for k in ("toff", "ids", "term", "docs", "tfs", "counts"):
        _expect(lambda: call(**{k: 1}), "NULL device pointer")
    _expect(lambda: call(first=1), "post_first / token_order: both or neither")
    _expect(lambda: call(order=1), "post_first / token_order: both or neither")
    for p_h, b_h in ((other.handle, batch._h), (pred.handle, api.DeviceBatch(other)._h), (None, batch._h), (pred.handle, None)):
        st = _lib.load().vpt_postings_batch_device(p_h, b_h, A["toff"].ptr, 2, A["ids"].ptr, 3, 2, 0, A["term"].ptr, A["docs"].ptr, A["tfs"].ptr, 3, None, None,
                                                   A["counts"].ptr, devmem.stream())
        assert st == _lib.VPT_INVALID_ARGUMENT
        _expect(lambda: api._raise(st), "batch: does not belong to this predictor")
    call(first=1, order=1)
    call()
    batch.sync()
    assert A["term"].get(3).tolist() == [0, 0, 0] and A["counts"].get(2).tolist() == [0, 0]
    # the host call
    vocab = api.Vocabulary(pred, ["漢字", "う"])
    utf8, boff = api.pack_texts(["漢字う".encode("utf-8")])
    _expect(lambda: pred.token_postings_packed(utf8, boff, None), "vocab: must not be NULL")
    _expect(lambda: other.token_postings_packed(utf8, boff, vocab), "vocab: does not belong to this predictor")
    _expect(lambda: pred.token_postings_packed(utf8, boff, vocab, "X"), "Could not parse a wsconst value")
    _expect(lambda: pred.token_postings_packed(utf8, boff, vocab, doc_base=1 << 32), "doc_base: doc_base \\+ n_documents must not exceed 2\\^32")
    tok = api.VaporettoTokenizer(None, "", _predictor=pred)
    _expect(lambda: tok.index_batch(["漢字"]), "index_batch: the tokenizer has no vocab")


def _expect(fn, pattern):
    try:
        fn()
    except api.VaporettoError as e:
        assert re.search(pattern, str(e)), str(e)
        return e
    assert False, "no error, wanted " + pattern


# ---- 13
def packed_steps(pred, toff, ids, n_terms, doc_base=0):
    """the second of the two steps: Predictor.postings_packed on the GPU; on the emulator, whose device pointers are host pointers and where
    that method's torch upload cannot run, the same device call over the same arrays"""
    if not devmem.EMULATED:
        return pred.postings_packed(toff, ids, n_terms, doc_base)
    r = run(toff, ids, n_terms, doc_base, positions=False, pred=pred)
    assert r.error is None, r.error
    k = int(r.counts[0])
    return api.Postings(r.term, r.docs[:k], r.tfs[:k], None, None, int(r.counts[1]))


def check_postings_packed(seed=3):
    """Predictor.postings_packed (host arrays in, api.Postings out; the GPU only: it uploads with torch) and the accessors of api.Postings"""
    rng = random.Random(seed)
    docs = [[zipf(rng, 60) if rng.random() < 0.9 else -1 for _ in range(rng.randint(0, 120))] for _ in range(25)]
    toff, ids = csr(docs)
    pred = predictor()
    for doc_base in (0, 9):
        ref = postingsref.Ref(toff, ids, 60, doc_base)
        term, rdocs, rtfs, first, order = ref.arrays()
        p = pred.postings_packed(toff, ids, 60, doc_base, positions=True)
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip((p.term_offsets, p.docs, p.tfs, p.first, p.order), ref.arrays()))
        assert p.n_dropped == ref.n_dropped and len(p) == len(rdocs) and np.array_equal(p.df(), np.diff(term))
        q = 0
        for k in range(60):
            d, tf = p.postings(k)
            assert dict(zip(d.tolist(), tf.tolist())) == dict(ref.terms.get(k, {}))
            for doc in d.tolist():
                assert p.tokens(q).tolist() == ref.tokens[(k, doc)]
                q += 1
        bare = pred.postings_packed(toff, ids, 60, doc_base)
        assert bare.first is None and bare.order is None and same_postings(bare, p)
        _expect(lambda: bare.tokens(0), "made without positions")
    none = pred.postings_packed(np.zeros(1, np.uint64), np.zeros(0, np.int32), 5, positions=True)
    assert len(none) == 0 and none.term_offsets.tolist() == [0] * 6 and none.first.tolist() == [0] and len(none.order) == 0


def fixture_corpus():
    lines = [l for l in open(os.path.join(kat.GOLDEN, "docs.tok"), encoding="utf-8").read().split("\n") if l]
    surfaces = ["".join(t.split("/")[0] for t in l.split(" ")) for l in lines]
    assert surfaces == ["まぁ社長は火星猫だ", "まぁ良いだろう"]
    more = ["東京特許許可局", "１２３４５６円🤌🏿", "AB09ＡＢ０９", "火星猫は東京だ"]
    rng = random.Random(17)
    texts = []
    for k in range(90):
        texts.append("" if k % 13 == 5 else "".join(rng.choice(surfaces + more) for _ in range(rng.randint(1, 4))))
    return ["", ""] + texts + [""]   # (empty documents: in front, inside, behind)


def same_postings(a, b):
    return (a.term_offsets.tobytes() == b.term_offsets.tobytes() and a.docs.tobytes() == b.docs.tobytes() and a.tfs.tobytes() == b.tfs.tobytes()
            and a.n_dropped == b.n_dropped and a.docs.dtype == b.docs.dtype == np.uint32 and a.term_offsets.dtype == np.uint64)


def check_pipeline():
    """vpt_token_stream_postings_batch = vpt_token_stream_ids_batch, then the device call = the definition over the token strings of
    token_stream_batch; under three values of VPT_TOKENIZE_CHUNK_BYTES; with a stop set; empty documents in the batch."""
    raw, _ = kat.load_fixture("tantivy_model.bin")
    texts = fixture_corpus()
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    norm = api.KyteaFullwidthFilter()
    results = {}
    for chunk in (None, max(len(utf8) // 3, 1), max(len(utf8) // 8, 1), max(len(utf8) // 25, 1)):
        if chunk is not None:
            os.environ["VPT_TOKENIZE_CHUNK_BYTES"] = str(chunk)
        try:
            pred = api.Predictor(api.Model.read_slice(raw)[0], True, device=0)
        finally:
            os.environ.pop("VPT_TOKENIZE_CHUNK_BYTES", None)
        tok = api.VaporettoTokenizer(None, "DR", _predictor=pred)
        stream = tok.token_stream_batch(texts)
        distinct = sorted({norm.filter(t.text) for d in stream for t in d})
        keys = [s for k, s in enumerate(distinct) if k % 3 != 1]
        table = {s: k for k, s in enumerate(keys)}
        vocab = api.Vocabulary(pred, keys, -4)
        tagger = api.PatternMatchTagger({"東京": ["地名"], "だ": ["助動詞"]})
        routes = {"plain": (None, None)}
        if pred.n_tags():
            routes["stop"] = (tagger, api.TagStopFilter(pred, [(0, "助動詞")], tagger))
        for route, (tg, stop) in routes.items():
            for doc_base in (0, 1000):
                got = pred.token_postings_packed(utf8, boff, vocab, "DR", True, tg, stop, doc_base)
                assert got.first is None and got.order is None
                if chunk is None:
                    toff, _s, _e, _p, _t, ids = pred.token_ids_packed(utf8, boff, vocab, "DR", True, tg, stop)
                    assert same_postings(got, packed_steps(pred, toff, ids, len(keys), doc_base)), (route, doc_base)
                    ref = postingsref.Ref(toff, ids, len(keys), doc_base)
                    term, docs, tfs, _f, _o = ref.arrays()
                    assert same_postings(got, api.Postings(term, docs, tfs, None, None, ref.n_dropped))
                    if route == "plain":   # the definition over the token STRINGS
                        sref = postingsref.from_token_strings([[norm.filter(t.text) for t in d] for d in stream], table, -4, doc_base)
                        assert sref.terms == ref.terms and sref.n_dropped == ref.n_dropped and ref.n_dropped > 0 and len(docs) > 20
                        assert int(toff[1]) == int(toff[2]) == 0 and int(toff[-1]) == int(toff[-2])
                    results[(route, doc_base)] = got
                else:
                    assert same_postings(got, results[(route, doc_base)]), (chunk, route, doc_base)
        if chunk is None:
            # too small a capacity: the existing kind of error, with the number needed
            needed = len(results[("plain", 0)].docs)
            e = _expect(lambda: pred.token_postings_packed(utf8, boff, vocab, "DR", capacity=needed - 1), SMALL_ERROR)
            assert e.n_postings == needed
            assert same_postings(pred.token_postings_packed(utf8, boff, vocab, "DR", capacity=needed), results[("plain", 0)])
            none = pred.token_postings_packed(utf8[:0], boff[:1], vocab, "DR")
            assert len(none.docs) == 0 and not none.term_offsets.any() and none.n_dropped == 0
    return results


def check_pipeline_stop_set(seed=31):
    """the same equalities on a model with tag models, a tagger and a stop set (tests/patterntagsuite.py's model), one chunk and several"""
    m = patterntagsuite.tagged_model(seed)
    raw = api.Model(m).to_vec()
    texts = [""] + tokentagsuite.stream_texts(seed)[:120] + ["", "AB０９ＡＢ09", ""]
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    keep = keys = None
    norm = api.KyteaFullwidthFilter()
    for chunk in (None, max(len(utf8) // 5, 1), max(len(utf8) // 17, 1)):
        if chunk is not None:
            os.environ["VPT_TOKENIZE_CHUNK_BYTES"] = str(chunk)
        try:
            pred = api.Predictor(api.Model.read_slice(raw)[0], True, device=0)
        finally:
            os.environ.pop("VPT_TOKENIZE_CHUNK_BYTES", None)
        tagger = api.PatternMatchTagger(tokentagsuite.STREAM_RULES)
        stop = api.TagStopFilter(pred, tokentagsuite.STOP_SETS["both"], tagger)
        if keys is None:   # two thirds of the surfaces the unfiltered stream has
            toff0, ends0 = pred.token_stream_packed(utf8, boff, "DR")
            surfaces = set()
            for i, t in enumerate(texts):
                r, a = t.encode("utf-8"), 0
                for k in range(int(toff0[i]), int(toff0[i + 1])):
                    surfaces.add(norm.filter(r[a:int(ends0[k])].decode("utf-8")))
                    a = int(ends0[k])
            keys = [x for k, x in enumerate(sorted(surfaces)) if k % 3 != 1]
        vocab = api.Vocabulary(pred, keys, -1)
        got = pred.token_postings_packed(utf8, boff, vocab, "DR", True, tagger, stop, 5)
        if chunk is None:
            toff, _s, _e, _p, _t, ids = pred.token_ids_packed(utf8, boff, vocab, "DR", True, tagger, stop)
            plain = pred.token_ids_packed(utf8, boff, vocab, "DR", True)
            assert len(ids) < len(plain[5])   # the stop set dropped tokens
            ref = postingsref.Ref(toff, ids, len(keys), 5)
            term, docs, tfs, _f, _o = ref.arrays()
            assert same_postings(got, api.Postings(term, docs, tfs, None, None, ref.n_dropped)) and len(docs) > 20 and ref.n_dropped > 0
            assert same_postings(got, packed_steps(pred, toff, ids, len(keys), 5))
            keep = got
        else:
            assert same_postings(got, keep), chunk


# ---- 14
def check_three_features_agree(seed=31):
    """build_vocab on a corpus, set_vocab, index_batch on the same corpus: per term the sum of its tfs is the counter's count of that surface;
    n_dropped is what the counter skipped plus the tokens of surfaces below min_count"""
    m = patterntagsuite.tagged_model(seed)
    raw = api.Model(m).to_vec()
    texts = tokentagsuite.stream_texts(seed)[:150] + ["AB０９ＡＢ09", "ＡＢ", ""]
    for min_count in (1, 2):
        tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR")
        _expect(lambda: tok.index_batch(texts), "index_batch: the tokenizer has no vocab")
        counter = api.VocabularyCounter(tok.predictor, 1 << 12)
        tok.count_batch(texts, counter)
        all_s, all_c = counter.finish()
        kept_s, kept_c = counter.finish(min_count)
        info = counter.info()
        vocab = tok.build_vocab([texts], min_count, max_keys=1 << 12)
        assert [vocab.surface(k) for k in range(len(kept_s))] == kept_s and vocab.info()["n_keys"] == len(kept_s)
        tok.set_vocab(vocab)
        post = tok.index_batch(texts, doc_base=11)
        assert len(post.term_offsets) == len(kept_s) + 1 and len(post) == int(post.term_offsets[-1]) > (50 if min_count == 1 else 0)
        sums = [int(post.postings(k)[1].sum()) for k in range(len(kept_s))]
        assert sums == [int(c) for c in kept_c]
        assert post.n_dropped == info["n_skipped"] + int(all_c.sum()) - int(kept_c.sum())
        assert (min_count == 1) == (post.n_dropped == info["n_skipped"])
        assert post.df().tolist() == [len(post.postings(k)[0]) for k in range(len(kept_s))] and (post.df() >= 1).all()
        assert all(11 <= int(d) < 11 + len(texts) for d in post.docs)


def main(argv):
    assert argv == ["--emu-hostile"], "usage: python -m tests.postingssuite --emu-hostile"
    import gc
    from tests import emu
    _lib._lib = emu.load()
    devmem.EMULATED = True
    ran = run_hostile()
    vocabsuite._PRED.clear()
    gc.collect()   # batch and predictor destroyed: hipemu has checked the red zones of every allocation it freed
    print("ran %d cases" % ran, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
