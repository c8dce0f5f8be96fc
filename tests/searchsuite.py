"""The checks of the BM25 top-k search (vpt_postings_search_device, vpt_postings_search, vpt_okapi_idf; kernels_postings_search.hip) against the
definition of tests/searchref.py, run on the CPU emulator by tests/test_postings_search_emu.py and on the MI355X by
tests/test_postings_search_gpu.py; every comparison of documents, counts and score BITS is exact equality with searchref, never with another
device call.

    python -m tests.searchsuite --emu-hostile     the hostile inputs on the emulator, in a child process (hipemu checks its red zones when the
                                                  workspace goes)

Every array handed to the device call has exactly the size the call is told and guard words on both sides, checked after the sync with the
inputs unwritten; the outputs are filled with SENTINEL first (the scores are handed over as their uint32 bits), so an entry the call must not
write is seen to be left alone.  T = vpt_postings_tile (4096); no case has more than 3 T + 1 candidates.

    python -m tests.searchsuite --emu-hostile-high     the hostile postings at the top of the document range, in the same way

check_high_documents runs the random and the ties corpus at the two bases of postingssuite.HIGH_BASES (documents on both sides of 2^31, the
last document 0xFFFFFFFF) with two hostile postings at the upper one; check_tile_edge_ties cuts a group of n equal scores (n = T, T + 1,
2 T + 1 candidates, the largest it uses) with k on both sides of T and puts a query's last candidate on records T - 2, T - 1 and T."""
import math
import random
import sys

import numpy as np

from tests import devmem, patterntagsuite, postingsmergesuite, postingssuite, searchref, vocabsuite
from vaporetto_amd import _lib, api

G = postingssuite.G
SENTINEL = postingssuite.SENTINEL
SEG_ERROR = postingsmergesuite.SEG_ERROR
QCSR_ERROR = "query_offsets: do not describe the queries' slots"
WEIGHT_ERROR = "weights: negative or not finite"
LONG_ERROR = "query: more than 1024 slots"
CAND_ERROR = "capacity_candidates: smaller than the number of candidates"
predictor = postingssuite.predictor
tile = postingssuite.tile
csr = postingssuite.csr
zipf = postingssuite.zipf
_expect = postingssuite._expect
Seg = postingsmergesuite.Seg
seg_of = postingsmergesuite.seg_of
F = np.float32
OUTPUTS = ("hd", "hs", "hc", "mc")


class Result:
    def same_bytes(self, other):
        return self.error == other.error and all(getattr(self, k).tobytes() == getattr(other, k).tobytes() for k in OUTPUTS + ("counts",))

    def untouched(self):
        return all((getattr(self, k) == SENTINEL).all() for k in ("hd", "hs", "hc")) and (self.mc == np.uint64(SENTINEL)).all()


def avgdl_of(dl):
    return F(float(sum(int(x) for x in dl)) / float(len(dl)))


def run(seg, doc_base, dl, queries, k, k1=1.2, b=0.75, avgdl=None, cap_slots=None, cap_cand=None, batch=None, pred=None, qoff=None, n_docs=None):
    """vpt_postings_search_device on guarded arrays of exactly the sizes the call is told.  queries: lists of (term, weight)."""
    pred = pred or predictor()
    batch = batch or api.DeviceBatch(pred)
    flat = [x for q in queries for x in q]
    cap_slots = len(flat) if cap_slots is None else cap_slots
    offsets = np.array([0] + list(np.cumsum([len(q) for q in queries])), np.uint64) if qoff is None else np.asarray(qoff, np.uint64)
    spare = max(cap_slots - len(flat), 0)   # places behind the slots: a term in range and a weight that is an error if it is looked at
    terms = np.array([t for t, _ in flat] + [0] * spare, np.int64).astype(np.int32)[:cap_slots]
    weights = np.array([w for _, w in flat] + [np.nan] * spare, np.float32)[:cap_slots]
    dl = np.asarray(dl, np.uint32)
    avgdl = avgdl_of(dl) if avgdl is None else avgdl
    if cap_cand is None:
        n_terms = seg.n_terms
        cap_cand = sum(int(seg.term[t + 1]) - int(seg.term[t]) for t, _ in flat if 0 <= t < n_terms and int(seg.term[t + 1]) >= int(seg.term[t]))
    n_q = len(queries)
    I = {"term": G(seg.term), "docs": G(seg.docs), "tfs": G(seg.tfs), "dl": G(dl), "qoff": G(offsets), "qterms": G(terms), "qweights": G(weights)}
    O = {"hd": G(np.full(n_q * k, SENTINEL, np.uint32)), "hs": G(np.full(n_q * k, SENTINEL, np.uint32)), "hc": G(np.full(n_q, SENTINEL, np.uint32)),
         "mc": G(np.full(n_q, SENTINEL, np.uint64)), "counts": G(np.full(3, SENTINEL, np.uint64))}
    r = Result()
    r.error = None
    try:
        batch.search_postings(I["term"].ptr, I["docs"].ptr, I["tfs"].ptr, seg.n_terms, seg.cap, doc_base, len(dl) if n_docs is None else n_docs, I["dl"].ptr,
                              I["qoff"].ptr, I["qterms"].ptr, I["qweights"].ptr, n_q, cap_slots, k1, b, avgdl, k, cap_cand, O["hd"].ptr, O["hs"].ptr,
                              O["hc"].ptr, O["mc"].ptr, O["counts"].ptr, devmem.stream())
    except api.VaporettoError as e:
        r.error = str(e)
    try:
        batch.sync()
    except api.VaporettoError as e:
        r.error = r.error or str(e)
    bad = [name for name, a in list(I.items()) + list(O.items()) if not a.guards_intact()]
    assert not bad, ("guard words overwritten", bad)
    assert all(a.get().tobytes() == a.sent.tobytes() for a in I.values()), "an input was written"
    r.k, r.n_q = k, n_q
    for name in OUTPUTS + ("counts",):
        setattr(r, name, O[name].get())
    return r


def same_as(r, ref):
    """every output of a call that succeeded is the definition's, bits included, and nothing behind a query's hit count was touched"""
    assert r.error is None, r.error
    assert r.counts.tolist() == ref.counts, (r.counts.tolist(), ref.counts)
    assert r.mc.tolist() == ref.match_counts, (r.mc.tolist(), ref.match_counts)
    assert r.hc.tolist() == [min(r.k, m) for m in ref.match_counts]
    for q, hits in enumerate(ref.hits):
        a = q * r.k
        got = list(zip(r.hd[a:a + len(hits)].tolist(), r.hs[a:a + len(hits)].tolist()))
        want = [(d, searchref.bits(s)) for d, s in hits]
        assert got == want, (q, [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w][:4])
        assert (r.hd[a + len(hits):a + r.k] == SENTINEL).all() and (r.hs[a + len(hits):a + r.k] == SENTINEL).all(), q


def check(seg, doc_base, dl, queries, k, k1=1.2, b=0.75, batch=None):
    ref = searchref.SearchRef(seg.term, seg.docs, seg.tfs, doc_base, dl, queries, k, k1, b)
    same_as(run(seg, doc_base, dl, queries, k, k1, b, batch=batch), ref)
    return ref


def idf_of(n_docs, df):
    """vpt_okapi_idf, checked against the definition on the way: every (N, df) the suite uses passes here"""
    got, want = api.bm25_idf(n_docs, df), searchref.idf(n_docs, df)
    assert type(got) is np.float32 and searchref.bits(got) == searchref.bits(want), (n_docs, df, got, want)
    return got


def with_idf(seg, n_docs, query_terms):
    df = np.diff(seg.term.astype(np.int64))
    return [[(t, idf_of(n_docs, int(df[t])) if 0 <= t < seg.n_terms else F(1.5)) for t in q] for q in query_terms]


# ---- 1, 2
def random_input(seed, doc_base, batch):
    """a few dozen documents over 20 terms through the device's postings pass; 17 queries of 1-5 slots"""
    rng = random.Random(seed)
    n_terms = 20
    docs = []
    for _ in range(37):
        n = 0 if rng.random() < 0.1 else rng.randint(1, 40)
        docs.append([rng.choice([-1, n_terms]) if rng.random() < 0.05 else zipf(rng, n_terms) for _ in range(n)])
    toff, ids = csr(docs)
    seg = postingsmergesuite.device_segment(toff, ids, n_terms, doc_base, batch)
    dl = np.diff(toff.astype(np.int64)).astype(np.uint32)
    query_terms = [[zipf(rng, n_terms) if rng.random() < 0.7 else rng.randrange(n_terms) for _ in range(rng.randint(1, 5))] for _ in range(17)]
    return seg, dl, with_idf(seg, len(docs), query_terms)


def check_random(seed=3):
    batch = api.DeviceBatch(predictor())
    for doc_base in (0, 1000):
        seg, dl, queries = random_input(seed, doc_base, batch)
        big = None
        for k in (1, 3, 64):
            ref = check(seg, doc_base, dl, queries, k, batch=batch)
            big = ref
        assert max(big.match_counts) < 64 and max(big.match_counts) > 3 and big.counts[0] > 100
        # the addition order is visible in this input: some (query, document) sums to other bits under another order of its slots
        assert big.order_matters(), "the input does not show the order of the additions"


# ---- 3
def check_ties():
    batch = api.DeviceBatch(predictor())
    same = [1, 2, 2, 5]
    docs = [[3, 3], same, [0], same, same, [1, 1, 1, 1], same, same, [2]]
    toff, ids = csr(docs)
    for doc_base in (0, 7):
        seg = postingsmergesuite.device_segment(toff, ids, 6, doc_base, batch)
        dl = np.diff(toff.astype(np.int64)).astype(np.uint32)
        queries = with_idf(seg, len(docs), [[1, 2], [5], [2, 1, 5]])
        for k in (2, 3, 5, 9):   # 2, 3: inside the group of five equal scores
            ref = check(seg, doc_base, dl, queries, k, batch=batch)
            group = [doc_base + d for d in (1, 3, 4, 6, 7)]
            assert [d for d, _ in ref.hits[1]] == group[:k] and len({searchref.bits(s) for _, s in ref.hits[1]}) == 1
            assert ref.match_counts[1] == 5


# ---- 4
def check_slots():
    limit = api.DeviceBatch.postings_search_limit()
    assert limit == 1024
    batch = api.DeviceBatch(predictor())
    seg = seg_of({0: {0: 1, 2: 3}, 1: {1: 2, 2: 1, 4: 7}, 2: {3: 1}, 3: {0: 2, 4: 1}, 5: {2: 2, 3: 9}}, 6, extra=3)   # term 4: df 0
    dl = [3, 2, 6, 10, 8]
    w = [idf_of(5, int(x)) for x in np.diff(seg.term.astype(np.int64))]
    rng = random.Random(9)
    longest = [(t, F(w[t] * F(1 + (j % 7) / 8))) for j, t in enumerate(rng.randrange(6) for _ in range(limit))]
    queries = [[], [], [(1, w[1]), (1, w[1]), (0, w[0]), (1, w[1])], [], [(4, w[4])], [], [], [(-1, F(2)), (6, F(2)), (2, w[2]), (-(1 << 31), F(1)), ((1 << 31) - 1, F(1))],
               longest, [(3, w[3])], []]
    ref = check(seg, 0, dl, queries, 4, batch=batch)
    assert ref.counts[2] == 4 and ref.match_counts[4] == 0 and ref.match_counts[2] == 4 and len(ref.contributions[2][2]) == 4
    assert max(len(c) for c in ref.contributions[8].values()) > 300 and ref.order_matters()
    # one slot more: an error at the sync, the outputs left alone; the workspace takes the sound batch afterwards
    r = run(seg, 0, dl, queries[:8] + [longest + [(0, w[0])]] + queries[9:], 4, batch=batch)
    assert r.error is not None and LONG_ERROR in r.error and r.untouched(), r.error
    check(seg, 0, dl, queries, 4, batch=batch)
    # capacity_slots above the slots, no slot at all, and a single empty query
    same_as(run(seg, 0, dl, queries, 4, cap_slots=sum(len(q) for q in queries) + 300, batch=batch), ref)
    none = searchref.SearchRef(seg.term, seg.docs, seg.tfs, 0, dl, [[], []], 2)
    same_as(run(seg, 0, dl, [[], []], 2, batch=batch), none)
    assert none.counts == [0, 0, 0]


# ---- 5
def check_candidates(n):
    """n candidates and n matches in one query of one slot; n candidates of two slots whose lists overlap in 5 documents"""
    batch = api.DeviceBatch(predictor())
    a = n - n // 3
    seg = seg_of({0: {d: 1 + d % 3 for d in range(n)}, 1: {d: 1 + d % 2 for d in range(a)}, 3: {d: 2 for d in range(a - 5, n - 5)}}, 4, extra=2)
    dl = [1 + (7 * d) % 50 for d in range(n)]
    k = n + 2
    ref = check(seg, 0, dl, [[(0, idf_of(n, n))]], k, batch=batch)
    assert ref.counts == [n, n, 0]
    ref = check(seg, 0, dl, [[(1, idf_of(n, a)), (3, idf_of(n, n - a))]], k, batch=batch)
    assert ref.counts == [n, n - 5, 0]


# ---- 6
def fixture_tokenizer():
    from tests import kat
    raw, _ = kat.load_fixture("tantivy_model.bin")
    texts = postingssuite.fixture_corpus()
    norm = api.KyteaFullwidthFilter()
    plain = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR")
    distinct = sorted({norm.filter(t.text) for d in plain.token_stream_batch(texts) for t in d})
    return api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", vocab=[s for j, s in enumerate(distinct) if j % 3 != 1]), texts


QUERY_TEXTS = ["火星猫", "東京特許許可局", "", "まぁ良いだろう火星猫は東京だ", "１２３４５６円", "だだだ"]


def check_merged_segment():
    """index_batches of three batches searched = index_batch of the concatenation searched = the definition; VaporettoTokenizer.search"""
    tok, texts = fixture_tokenizer()
    toff, ids = tok.encode_batch(texts)
    dl = np.diff(toff.astype(np.int64)).astype(np.uint32)
    qoff, qids = tok.encode_batch(QUERY_TEXTS)
    for doc_base in (0, 1000):
        whole = tok.index_batch(texts, doc_base)
        parts = tok.index_batches([texts[:30], texts[30:31], texts[31:]], doc_base)
        assert postingssuite.same_postings(whole, parts)
        assert whole.doc_base == parts.doc_base == doc_base and np.array_equal(whole.doc_lens, dl) and np.array_equal(parts.doc_lens, dl)
        assert whole.doc_lens.dtype == np.uint32 and int(dl.sum()) > len(whole)
        df = whole.df()
        n_terms = len(df)
        queries = [[(int(t), idf_of(len(texts), int(df[t])) if 0 <= t < n_terms else F(0)) for t in qids[int(qoff[i]):int(qoff[i + 1])]]
                   for i in range(len(QUERY_TEXTS))]
        assert any(not 0 <= t < n_terms for q in queries for t, _ in q) and any(len(q) > 3 for q in queries)
        for k in (1, 10):
            ref = searchref.SearchRef(whole.term_offsets, whole.docs, whole.tfs, doc_base, dl, queries, k)
            assert max(ref.match_counts) > 10 and ref.match_counts[2] == 0
            for post in (whole, parts):
                hits, mc = tok.search(post, QUERY_TEXTS, k)
                assert mc.tolist() == ref.match_counts and mc.dtype == np.uint64
                assert [[(d, searchref.bits(s)) for d, s in h] for h in hits] == [[(d, searchref.bits(s)) for d, s in h] for h in ref.hits]
                assert post.last_search_counts.tolist() == ref.counts
    merged = api.Postings.merge([whole, whole], predictor=tok.predictor)   # a general merge: the caller says what the documents are
    assert merged.doc_lens is None and merged.doc_base is None
    _expect(lambda: merged.search([[0]]), "search: the postings carry no doc_lens / doc_base")


# ---- 7
def check_weights_and_parameters():
    batch = api.DeviceBatch(predictor())
    seg = seg_of({0: {0: 1, 1: 3, 3: 2}, 1: {1: 1, 2: 40, 3: 2}, 2: {2: 1}}, 3)
    dl = [4, 0, 41, 9]   # document 1 has postings and length 0: dl is the caller's
    terms = [[0, 1], [1], [2, 0, 1]]
    idf = with_idf(seg, 4, terms)
    ref = check(seg, 0, dl, [[(t, F(0)) for t in q] for q in terms], 4, batch=batch)
    assert all(searchref.bits(s) == 0 for h in ref.hits for _, s in h) and [d for d, _ in ref.hits[0]] == [0, 1, 2, 3]
    for k1, b in ((0.0, 0.75), (1.2, 0.0), (1.2, 1.0), (2.0, 0.5), (65536.0, 1.0)):
        ref = check(seg, 0, dl, idf, 4, k1, b, batch=batch)
        assert all(len(h) == m for h, m in zip(ref.hits, ref.match_counts))
    # k1 = 0: every contribution is the slot's weight
    ref = searchref.SearchRef(seg.term, seg.docs, seg.tfs, 0, dl, idf, 4, 0.0, 0.75)
    assert {searchref.bits(s) for _, s in ref.hits[1]} == {searchref.bits(idf[1][0][1])}
    # a sum that reaches +inf sorts first, ties by document
    huge = [[(0, F(3e38)), (1, F(3e38))]]
    ref = check(seg, 0, dl, huge, 4, batch=batch)
    assert [math.isinf(float(s)) for _, s in ref.hits[0]].count(True) >= 1 and math.isinf(float(ref.hits[0][0][1]))


# ---- 8
def check_idf():
    for n, df in ((1, 0), (1, 1), (10, 3), (37, 37), (93, 1), (1 << 32, 12345), ((1 << 53) + 1, 1), (1000003, 999)):
        idf_of(n, df)
    _expect(lambda: api.bm25_idf(3, 4), "df: above n_documents")


# ---- 9
def check_capacity(seed=3):
    batch = api.DeviceBatch(predictor())
    seg, dl, queries = random_input(seed, 5, batch)
    ref = searchref.SearchRef(seg.term, seg.docs, seg.tfs, 5, dl, queries, 3)
    need = ref.counts[0]
    for cap in (need - 1, 0):
        r = run(seg, 5, dl, queries, 3, cap_cand=cap, batch=batch)
        assert r.error is not None and CAND_ERROR in r.error, r.error
        assert int(r.counts[0]) == need and r.untouched()
    same_as(run(seg, 5, dl, queries, 3, cap_cand=need, batch=batch), ref)
    same_as(run(seg, 5, dl, queries, 3, cap_cand=need + tile() + 1, batch=batch), ref)


# ---- 10
def check_errors():
    pred = predictor()
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    batch = api.DeviceBatch(pred)
    names = ("term", "docs", "tfs", "dl", "qoff", "qterms", "qweights", "hd", "hs", "hc", "mc", "counts")
    A = {n: devmem.zeros(8, np.uint64) for n in names}

    def call(b=batch, n_terms=2, cap_post=2, doc_base=0, n_docs=2, n_q=1, cap_slots=1, k1=1.2, bb=0.75, avgdl=1.0, k=2, cap_cand=2, **null):
        p = {n: (0 if n in null else a.ptr) for n, a in A.items()}
        b.search_postings(p["term"], p["docs"], p["tfs"], n_terms, cap_post, doc_base, n_docs, p["dl"], p["qoff"], p["qterms"], p["qweights"], n_q, cap_slots,
                          k1, bb, avgdl, k, cap_cand, p["hd"], p["hs"], p["hc"], p["mc"], p["counts"], devmem.stream())

    for n in names:
        _expect(lambda: call(**{n: 1}), "NULL device pointer")
    for v in (0, (1 << 24) + 1):
        _expect(lambda: call(n_terms=v), "n_terms: must be between 1 and 2\\^24")
        _expect(lambda: call(n_q=v), "n_queries: must be between 1 and 2\\^24")
    _expect(lambda: call(k=0), "k: must be at least 1")
    _expect(lambda: call(n_q=1 << 16, k=1 << 16), "n_queries \\* k below 2\\^32")
    _expect(lambda: call(cap_slots=1 << 32), "fewer than 2\\^32 slots and candidates")
    _expect(lambda: call(cap_cand=1 << 32), "fewer than 2\\^32 slots and candidates")
    _expect(lambda: call(doc_base=(1 << 32) - 1, n_docs=2), "doc_base \\+ n_documents must not exceed 2\\^32")
    _expect(lambda: call(doc_base=(1 << 32) + 1, n_docs=0), "doc_base \\+ n_documents must not exceed 2\\^32")
    for v in (-1.0, 65537.0, float("nan"), float("inf")):
        _expect(lambda: call(k1=v), "k1: must be between 0 and 65536")
    for v in (-0.1, 1.5, float("nan")):
        _expect(lambda: call(bb=v), "b: must be between 0 and 1")
    for v in (0.0, 2.0 ** -33, 2.0 ** 33, float("nan"), -1.0):
        _expect(lambda: call(avgdl=v), "avgdl: must be between 2\\^-32 and 2\\^32")
    p = {n: a.ptr for n, a in A.items()}
    for p_h, b_h in ((other.handle, batch._h), (pred.handle, api.DeviceBatch(other)._h), (None, batch._h), (pred.handle, None)):
        st = _lib.load().vpt_postings_search_device(p_h, b_h, p["term"], p["docs"], p["tfs"], 2, 2, 0, 2, p["dl"], p["qoff"], p["qterms"], p["qweights"], 1, 1,
                                                    1.2, 0.75, 1.0, 2, 2, p["hd"], p["hs"], p["hc"], p["mc"], p["counts"], devmem.stream())
        assert st == _lib.VPT_INVALID_ARGUMENT
        _expect(lambda: api._raise(st), "batch: does not belong to this predictor")
    st = _lib.load().vpt_postings_search_limits(None)
    assert st == _lib.VPT_INVALID_ARGUMENT
    batch.sync()
    call(k1=65536.0, bb=1.0, avgdl=2.0 ** 32)   # the ends of the ranges are inside; all-zero arrays: one query without a slot
    batch.sync()
    assert A["counts"].get(3).tolist() == [0, 0, 0] and int(A["mc"].get(1)[0]) == 0


# ---- 11
def hostile_cases():
    """name -> (segment, queries, query_offsets or None, cap_slots or None, the message)"""
    def base():
        return seg_of({0: {11: 1, 13: 2}, 1: {12: 1}, 3: {10: 1, 11: 1, 14: 4}}, 4, extra=2)   # term 0 2 3 3 6; cap 8; documents 10 .. 14
    w = F(1.25)
    sound = [[(0, w), (3, w)], [], [(1, w), (3, F(0.5))]]
    cases = {}

    def seg_case(name, fn):
        s = base()
        fn(s)
        cases[name] = (s, sound, None, None, SEG_ERROR)
    seg_case("descending_term_offsets", lambda s: s.term.__setitem__(3, 7))                   # term 3: [7, 6)
    seg_case("bound_above_capacity", lambda s: s.term.__setitem__(4, 9))
    seg_case("huge_offsets", lambda s: s.term.__setitem__(slice(1, 5), [1 << 40, 1 << 41, 1 << 62, (1 << 64) - 1]))
    seg_case("document_below_doc_base", lambda s: s.docs.__setitem__(0, 9))
    seg_case("document_at_the_end", lambda s: s.docs.__setitem__(5, 15))
    seg_case("document_far_outside", lambda s: s.docs.__setitem__(5, 0xFFFFFFFF))
    seg_case("zero_tf", lambda s: s.tfs.__setitem__(4, 0))
    cases["descending_query_offsets"] = (base(), sound, [0, 2, 1, 4], None, QCSR_ERROR)
    cases["query_offsets_end_above_capacity_slots"] = (base(), sound, [0, 2, 2, 5], None, QCSR_ERROR)
    cases["query_offsets_far_above"] = (base(), sound, [0, 2, 1 << 63, (1 << 64) - 1], None, QCSR_ERROR)
    for name, bad in (("nan_weight", F("nan")), ("negative_weight", F(-1.0)), ("negative_zero_weight", F(-0.0)), ("infinite_weight", F("inf"))):
        cases[name] = (base(), [[(0, w), (3, bad)], [], [(1, w), (3, F(0.5))]], None, None, WEIGHT_ERROR)
    return base(), sound, cases


N_HOSTILE = 14


def run_hostile():
    sound_seg, sound, cases = hostile_cases()
    assert len(cases) == N_HOSTILE
    dl = [3, 5, 2, 9, 4]
    batch = api.DeviceBatch(predictor())
    ran = 0
    for name, (seg, queries, qoff, cap_slots, message) in cases.items():
        r = run(seg, 10, dl, queries, 3, cap_slots=cap_slots, cap_cand=16, qoff=qoff, batch=batch)
        assert r.error is not None and message in r.error, (name, r.error)
        assert r.untouched(), name
        check(sound_seg, 10, dl, sound, 3, batch=batch)   # the sound ones on the same workspace
        ran += 1
    del batch
    return ran


# ---- 12
def check_determinism(seed=12):
    rng = random.Random(seed)
    T = tile()
    pred = predictor()
    one, two = api.DeviceBatch(pred), api.DeviceBatch(pred)
    n_docs, n_terms = 700, 40
    terms = {}
    for _ in range(2 * T):
        terms.setdefault(zipf(rng, n_terms), {})[rng.randrange(n_docs)] = rng.randint(1, 9)
    seg = seg_of(terms, n_terms)
    dl = [rng.randint(0, 90) for _ in range(n_docs)]
    queries = with_idf(seg, n_docs, [[rng.randrange(n_terms) for _ in range(rng.randint(0, 6))] for _ in range(23)])
    a = run(seg, 0, dl, queries, 10, batch=one)
    b = run(seg, 0, dl, queries, 10, batch=one)
    run(seg_of({1: {2: 3}}, 4), 0, [1, 1, 1], [[(1, F(1))]], 1, batch=two)   # (the second workspace's scratch holds something else)
    c = run(seg, 0, dl, queries, 10, batch=two)
    assert a.error is None and a.same_bytes(b) and a.same_bytes(c)
    ref = searchref.SearchRef(seg.term, seg.docs, seg.tfs, 0, dl, queries, 10)
    assert T < ref.counts[0] <= 3 * T + 1
    same_as(a, ref)


# ---- 13
def check_host_call(seed=5):
    """vpt_postings_search through Postings.search: host arrays in and out, the default weights and the caller's"""
    rng = random.Random(seed)
    pred = predictor()
    terms = {}
    for _ in range(300):
        terms.setdefault(zipf(rng, 30), {})[100 + rng.randrange(50)] = rng.randint(1, 5)
    seg = seg_of(terms, 30)
    term, docs, tfs = seg.triple()
    post = api.Postings(term, docs.copy(), tfs.copy(), None, None, 0)
    dl = np.array([rng.randint(1, 60) for _ in range(50)], np.uint32)
    ids = [[rng.randrange(30) for _ in range(rng.randint(1, 4))] for _ in range(9)] + [[], [-1, 30, 2]]
    df = np.diff(term.astype(np.int64))
    queries = [[(t, idf_of(50, int(df[t])) if 0 <= t < 30 else F(0)) for t in q] for q in ids]
    for k in (1, 5, 60):
        ref = searchref.SearchRef(term, docs, tfs, 100, dl, queries, k)
        hits, mc = post.search(ids, k, dl, 100, predictor=pred)
        assert [[(d, searchref.bits(s)) for d, s in h] for h in hits] == [[(d, searchref.bits(s)) for d, s in h] for h in ref.hits]
        assert all(type(s) is np.float32 for h in hits for _, s in h) and mc.tolist() == ref.match_counts and post.last_search_counts.tolist() == ref.counts
    mine = [[(t, F(0.25 + j)) for j, t in enumerate(q)] for q in ids]
    ref = searchref.SearchRef(term, docs, tfs, 100, dl, mine, 4, 0.9, 0.4)
    hits, mc = post.search(ids, 4, dl, 100, 0.9, 0.4, weights=[[w for _, w in q] for q in mine], predictor=pred)
    assert [[(d, searchref.bits(s)) for d, s in h] for h in hits] == [[(d, searchref.bits(s)) for d, s in h] for h in ref.hits]
    _expect(lambda: post.search(ids, 4, dl, 100), "search: no predictor")
    _expect(lambda: post.search(ids, 4, predictor=pred), "search: the postings carry no doc_lens / doc_base")
    _expect(lambda: post.search(ids, 0, dl, 100, predictor=pred), "k: must be at least 1")
    _expect(lambda: post.search(ids, 4, dl, 100, weights=[[F(-1)] * len(q) for q in ids], predictor=pred), WEIGHT_ERROR)
    _expect(lambda: post.search(ids, 4, dl[:10], 100, weights=[[F(1)] * len(q) for q in ids], predictor=pred), SEG_ERROR)   # documents outside the lengths given
    _expect(lambda: post.search(ids, 4, dl[:10], 100, predictor=pred), "df: above n_documents")
    assert post.search([], 4, dl, 100, predictor=pred)[0] == []


# ---- 14
def hits_of(ref):
    return {d for h in ref.hits for d, _ in h}


def check_high_documents(name, hostile=True):
    """the random input and the ties corpus at a doc_base of postingssuite.HIGH_BASES: documents on both sides of 2^31, or the last document
    0xFFFFFFFF; at the upper base the two hostile postings too (hostile=False where they run in a process of their own)"""
    batch = api.DeviceBatch(predictor())
    doc_base = postingssuite.high_base(name, 37)
    seg, dl, queries = random_input(3, doc_base, batch)
    last = doc_base + 36
    for k in (1, 3, 64):
        ref = check(seg, doc_base, dl, queries, k, batch=batch)
    assert max(ref.match_counts) < 64 and {doc_base, last} <= hits_of(ref) and last >= 1 << 31   # (k = 64: every match is a hit)
    assert (doc_base < 1 << 31) == (name == "2^31-3") and (last == 0xFFFFFFFF) == (name == "2^32-n")
    same = [1, 2, 2, 5]
    docs = [[3, 3], same, [0], same, same, [1, 1, 1, 1], same, same, [2]]
    toff, ids = csr(docs)
    doc_base = postingssuite.high_base(name, len(docs))
    tseg = postingsmergesuite.device_segment(toff, ids, 6, doc_base, batch)
    tdl = np.diff(toff.astype(np.int64)).astype(np.uint32)
    tqueries = with_idf(tseg, len(docs), [[1, 2], [5], [2, 1, 5]])
    for k in (2, 5):   # 2: inside the group of five equal scores, which stands on both sides of 2^31 at the lower base
        ref = check(tseg, doc_base, tdl, tqueries, k, batch=batch)
        group = [doc_base + d for d in (1, 3, 4, 6, 7)]
        assert [d for d, _ in ref.hits[1]] == group[:k] and len({searchref.bits(s) for _, s in ref.hits[1]}) == 1 and ref.match_counts[1] == 5
    # (k = 5: the whole group is hits; the last document matches and is below the best five)
    assert group[-1] in hits_of(ref) and group[-1] >= 1 << 31 and (group[0] < 1 << 31) == (name == "2^31-3") and doc_base + 8 in ref.scores[0]
    if hostile and name == "2^32-n":
        assert run_hostile_high(batch) == N_HOSTILE_HIGH


HIGH_HOSTILE_BASE = (1 << 32) - 5


def high_hostile_cases():
    """hostile_cases' segment on the documents 2^32 - 5 .. 2^32 - 1; name -> the segment with one posting outside them"""
    B = HIGH_HOSTILE_BASE

    def base():
        return seg_of({0: {B + 1: 1, B + 3: 2}, 1: {B + 2: 1}, 3: {B: 1, B + 1: 1, B + 4: 4}}, 4, extra=2)   # term 0 2 3 3 6; cap 8
    cases = {}

    def seg_case(name, fn):
        s = base()
        fn(s)
        cases[name] = s
    # both are the first posting of term 0's list, so the list's own order is sound: only the range check can see them
    seg_case("document_below_doc_base", lambda s: s.docs.__setitem__(0, B - 1))
    seg_case("document_at_the_end_wrapped_to_zero", lambda s: s.docs.__setitem__(0, (B + 5 - 1 + 1) & 0xFFFFFFFF))
    return base(), cases


N_HOSTILE_HIGH = 2


def run_hostile_high(batch=None):
    B = HIGH_HOSTILE_BASE
    sound_seg, cases = high_hostile_cases()
    assert len(cases) == N_HOSTILE_HIGH and cases["document_at_the_end_wrapped_to_zero"].docs[0] == 0
    _s, sound, _c = hostile_cases()
    dl = [3, 5, 2, 9, 4]
    batch = batch or api.DeviceBatch(predictor())
    ran = 0
    for name, seg in cases.items():
        r = run(seg, B, dl, sound, 3, cap_cand=16, batch=batch)
        assert r.error is not None and SEG_ERROR in r.error, (name, r.error)
        assert r.untouched(), name
        ref = check(sound_seg, B, dl, sound, 3, batch=batch)   # the sound ones on the same workspace
        assert 0xFFFFFFFF in hits_of(ref)
        ran += 1
    return ran


# ---- 15
def cut(ref, k):
    """the definition for a smaller k: the same ranking, its first k of every query (the reference is computed once and left as it is)"""
    import copy
    out = copy.copy(ref)
    out.k, out.hits = k, [h[:k] for h in ref.hits]
    return out


def candidate_records(seg, queries):
    """the candidates in the order the first sort leaves them, by the definition alone: (query, document, slot)"""
    out = []
    for q, query in enumerate(queries):
        for s, (t, _w) in enumerate(query):
            if 0 <= t < seg.n_terms:
                out += [(q, int(seg.docs[at]), s) for at in range(int(seg.term[t]), int(seg.term[t + 1]))]
    return sorted(out)


def check_tile_edge_ties(n):
    """n documents of one length that all hold term 0 once: one query of that slot has n equal scores, a tie group over the records 0 .. n - 1
    that k cuts at 1, T - 1, T and n.  Then two queries: the first has T - 1, T and T + 1 candidates (terms 2, 3 and 4 add up to them), so the
    second one's group of 7 equal scores (term 1, another tf) starts on record T - 1, T and T + 1."""
    T = tile()
    assert n >= T
    batch = api.DeviceBatch(predictor())
    doc_base = 5
    seven = [doc_base + (j * (n - 1)) // 6 for j in range(7)]   # the first and the last document among them
    terms = {0: {doc_base + d: 1 for d in range(n)}, 1: {d: 3 for d in seven}, 2: {doc_base + d: 1 for d in range(T - 1)}, 3: {doc_base + T - 1: 1},
             4: {doc_base: 1}}
    seg = seg_of(terms, 5, extra=1)
    dl = [4] * n
    w = [idf_of(n, len(terms[t])) for t in range(5)]
    # what the input has to be, by the definition alone and before any device call
    whole = searchref.SearchRef(seg.term, seg.docs, seg.tfs, doc_base, dl, [[(0, w[0])]], n)
    assert whole.match_counts == [n] and len(whole.hits[0]) == n and len({searchref.bits(s) for _, s in whole.hits[0]}) == 1
    assert len(set(seven)) == 7 and len({searchref.bits(searchref.contribution(w[0], tf, 4, 1.2, 0.75, whole.avgdl)) for tf in (1, 3)}) == 2
    pairs = []
    for c, slots in ((T - 1, [2]), (T, [2, 3]), (T + 1, [2, 3, 4])):
        queries = [[(t, w[2]) for t in slots], [(1, w[1])]]   # (one weight for the three terms: their documents tie)
        records = candidate_records(seg, queries)
        assert [r[0] for r in records] == [0] * c + [1] * 7, c   # the query changes on record c
        pairs.append((c, queries))
    for k in (1, T - 1, T, n):
        r = run(seg, doc_base, dl, [[(0, w[0])]], k, batch=batch)
        same_as(r, cut(whole, k))
        m = min(k, n)
        assert r.hd[:m].tolist() == list(range(doc_base, doc_base + m)) and len(set(r.hs[:m].tolist())) == 1
        assert r.mc.tolist() == [n] and r.counts.tolist() == [n, n, 0]
    for c, queries in pairs:
        ref = searchref.SearchRef(seg.term, seg.docs, seg.tfs, doc_base, dl, queries, 9)
        r = run(seg, doc_base, dl, queries, 9, batch=batch)
        same_as(r, ref)
        assert int(r.counts[0]) == c + 7 and r.mc.tolist() == [min(c, T), 7] and r.hd[9:16].tolist() == seven
        # (T + 1 candidates: the first document holds two of them, so it leads with a score of its own)
        assert len(set(r.hs[:9].tolist())) == (2 if c == T + 1 else 1) and len(set(r.hs[1:9].tolist())) == 1 and len(set(r.hs[9:16].tolist())) == 1
        assert r.hd[:9].tolist() == list(range(doc_base, doc_base + 9))


def example_lines(post, dl, doc_base, queries, k):
    """the lines examples/token_stream.cpp --postings --search prints for these hits"""
    ref = searchref.SearchRef(post.term_offsets, post.docs, post.tfs, doc_base, dl, queries, k)
    return ["%d\t%08x\t%.9g" % (d, searchref.bits(s), float(s)) for d, s in ref.hits[0]], ref


def main(argv):
    assert argv in (["--emu-hostile"], ["--emu-hostile-high"]), "usage: python -m tests.searchsuite --emu-hostile | --emu-hostile-high"
    import gc
    from tests import emu
    _lib._lib = emu.load()
    devmem.EMULATED = True
    ran = run_hostile() if argv == ["--emu-hostile"] else run_hostile_high()
    vocabsuite._PRED.clear()
    gc.collect()   # batch and predictor destroyed: hipemu has checked the red zones of every allocation it freed
    print("ran %d cases" % ran, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
