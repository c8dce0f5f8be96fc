"""The checks of the BM25 top-k search with MUST / SHOULD / MUST_NOT slots (vpt_postings_boolean_search_device, vpt_postings_boolean_search;
kernels_postings_boolean.hip) against the definition of tests/boolref.py, run on the CPU emulator by tests/test_postings_boolean_emu.py and on
the MI355X by tests/test_postings_boolean_gpu.py; every comparison of documents, counts and score BITS is exact equality.

    python -m tests.boolsuite --emu-hostile     the hostile inputs on the emulator, in a child process (hipemu checks its red zones when the
                                                workspace goes)

Every array handed to the device call has exactly the size the call is told and guard words on both sides, checked after the sync with the
inputs unwritten; the outputs are filled with SENTINEL first, so an entry the call must not write is seen to be left alone (searchsuite's
arrangement, with the occurs beside the weights).  T = vpt_postings_tile (4096); no case has more than 3 T + 1 places."""
import random
import sys

import numpy as np

from tests import boolref, devmem, patterntagsuite, postingsmergesuite, postingssuite, searchref, searchsuite, vocabsuite
from vaporetto_amd import _lib, api

G = postingssuite.G
SENTINEL = postingssuite.SENTINEL
SEG_ERROR = searchsuite.SEG_ERROR
QCSR_ERROR = searchsuite.QCSR_ERROR
WEIGHT_ERROR = searchsuite.WEIGHT_ERROR
LONG_ERROR = searchsuite.LONG_ERROR
CAND_ERROR = searchsuite.CAND_ERROR
OCCUR_ERROR = "occurs: a value above 2"
predictor = postingssuite.predictor
tile = postingssuite.tile
csr = postingssuite.csr
_expect = postingssuite._expect
seg_of = postingsmergesuite.seg_of
idf_of = searchsuite.idf_of
same_as = searchsuite.same_as
F = np.float32
S, M, N = boolref.SHOULD, boolref.MUST, boolref.MUST_NOT
OUTPUTS = searchsuite.OUTPUTS


def places_of(seg, queries):
    """the places by the header's rule, from the segment's bounds alone (boolref counts them from the lists)"""
    n = 0
    for q in queries:
        df = [int(seg.term[t + 1]) - int(seg.term[t]) if 0 <= t < seg.n_terms and int(seg.term[t + 1]) >= int(seg.term[t]) else 0 for t, _o, _w in q]
        must = [df[j] for j, x in enumerate(q) if x[1] == M]
        n += (0 if 0 in must else min(must)) if must else sum(df[j] for j, x in enumerate(q) if x[1] == S)
    return n


def run(seg, doc_base, dl, queries, k, k1=1.2, b=0.75, avgdl=None, cap_slots=None, cap_places=None, batch=None, pred=None, qoff=None, n_docs=None):
    """vpt_postings_boolean_search_device on guarded arrays of exactly the sizes the call is told.  queries: lists of (term, occur, weight)."""
    pred = pred or predictor()
    batch = batch or api.DeviceBatch(pred)
    flat = [x for q in queries for x in q]
    cap_slots = len(flat) if cap_slots is None else cap_slots
    offsets = np.array([0] + list(np.cumsum([len(q) for q in queries])), np.uint64) if qoff is None else np.asarray(qoff, np.uint64)
    spare = max(cap_slots - len(flat), 0)   # places behind the slots: a term in range, a weight and an occur that are errors if they are looked at
    terms = np.array([t for t, _o, _w in flat] + [0] * spare, np.int64).astype(np.int32)[:cap_slots]
    weights = np.array([w for _t, _o, w in flat] + [np.nan] * spare, np.float32)[:cap_slots]
    occurs = np.array([o for _t, o, _w in flat] + [77] * spare, np.uint8)[:cap_slots]
    dl = np.asarray(dl, np.uint32)
    avgdl = searchsuite.avgdl_of(dl) if avgdl is None else avgdl
    cap_places = places_of(seg, queries) if cap_places is None else cap_places
    n_q = len(queries)
    I = {"term": G(seg.term), "docs": G(seg.docs), "tfs": G(seg.tfs), "dl": G(dl), "qoff": G(offsets), "qterms": G(terms), "qweights": G(weights),
         "qoccurs": G(occurs)}
    O = {"hd": G(np.full(n_q * k, SENTINEL, np.uint32)), "hs": G(np.full(n_q * k, SENTINEL, np.uint32)), "hc": G(np.full(n_q, SENTINEL, np.uint32)),
         "mc": G(np.full(n_q, SENTINEL, np.uint64)), "counts": G(np.full(3, SENTINEL, np.uint64))}
    r = searchsuite.Result()
    r.error = None
    try:
        batch.boolean_search_postings(I["term"].ptr, I["docs"].ptr, I["tfs"].ptr, seg.n_terms, seg.cap, doc_base, len(dl) if n_docs is None else n_docs,
                                      I["dl"].ptr, I["qoff"].ptr, I["qterms"].ptr, I["qweights"].ptr, I["qoccurs"].ptr, n_q, cap_slots, k1, b, avgdl, k,
                                      cap_places, O["hd"].ptr, O["hs"].ptr, O["hc"].ptr, O["mc"].ptr, O["counts"].ptr, devmem.stream())
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


def ref_of(seg, doc_base, dl, queries, k, k1=1.2, b=0.75):
    ref = boolref.BoolRef(seg.term, seg.docs, seg.tfs, doc_base, dl, queries, k, k1, b)
    assert ref.counts[0] == places_of(seg, queries)
    return ref


def check(seg, doc_base, dl, queries, k, k1=1.2, b=0.75, batch=None, ref=None):
    ref = ref or ref_of(seg, doc_base, dl, queries, k, k1, b)
    same_as(run(seg, doc_base, dl, queries, k, k1, b, batch=batch), ref)
    return ref


def with_occurs(queries, occurs):
    """searchsuite's (term, weight) queries with an occur per slot: a constant, or a function of (query, slot)"""
    return [[(t, occurs(q, j) if callable(occurs) else occurs, w) for j, (t, w) in enumerate(query)] for q, query in enumerate(queries)]


# ---- 1
def check_all_should_is_the_or_search(seed=3):
    """all-SHOULD queries: the four outputs and the counts of vpt_postings_search_device on the same inputs, byte for byte, and searchref's"""
    batch = api.DeviceBatch(predictor())
    for doc_base in (0, 1000):
        seg, dl, queries = searchsuite.random_input(seed, doc_base, batch)
        for k in (1, 3, 64):
            ref = searchref.SearchRef(seg.term, seg.docs, seg.tfs, doc_base, dl, queries, k)
            mine = run(seg, doc_base, dl, with_occurs(queries, S), k, batch=batch)
            theirs = searchsuite.run(seg, doc_base, dl, queries, k, batch=batch)
            assert theirs.error is None and mine.same_bytes(theirs)
            same_as(mine, ref)
        assert ref.counts[0] > 100 and ref.order_matters()
    # the slot-limit query, empty queries and skipped slots of searchsuite.check_slots
    seg = seg_of({0: {0: 1, 2: 3}, 1: {1: 2, 2: 1, 4: 7}, 2: {3: 1}, 3: {0: 2, 4: 1}, 5: {2: 2, 3: 9}}, 6, extra=3)
    dl = [3, 2, 6, 10, 8]
    queries = [[], [(1, F(1.5)), (1, F(1.5)), (0, F(0.25))], [], [(4, F(1))], [(-1, F(2)), (6, F(2)), (2, F(3))]]
    mine = run(seg, 0, dl, with_occurs(queries, S), 4, batch=batch)
    assert mine.same_bytes(searchsuite.run(seg, 0, dl, queries, 4, batch=batch))
    same_as(mine, searchref.SearchRef(seg.term, seg.docs, seg.tfs, 0, dl, queries, 4))


# ---- 2
def mixed_input(seed, doc_base, batch):
    seg, dl, queries = searchsuite.random_input(seed, doc_base, batch)
    rng = random.Random(seed + 100)
    return seg, dl, with_occurs(queries, lambda q, j: rng.choice([S, S, M, M, N]))


def check_random(seed=3):
    batch = api.DeviceBatch(predictor())
    for doc_base in (0, 1000):
        seg, dl, queries = mixed_input(seed, doc_base, batch)
        refs = {k: ref_of(seg, doc_base, dl, queries, k) for k in (1, 3, 64)}
        big = refs[64]
        # what the input has to hold, by the definition alone and before any device call
        assert any(m > 0 for m in big.match_counts) and any(m == 0 for m in big.match_counts) and max(big.match_counts) > 3
        assert big.vetoes["must"] >= 1 and big.vetoes["must_not"] >= 1
        assert any(a is not None for a in big.anchors) and any(a is None and m > 0 for a, m in zip(big.anchors, big.match_counts))
        assert any(o == N for q in queries for _t, o, _w in q if not any(x[1] == M for x in q))   # a MUST_NOT on the unanchored route
        for k, ref in refs.items():
            check(seg, doc_base, dl, queries, k, batch=batch, ref=ref)


# ---- 3
def check_addition_order():
    """four scoring slots on the anchored route, the anchor (term 0, the rarest MUST) in the first, a middle and the last slot"""
    rng = random.Random(21)
    n = 24
    docs = range(7, 7 + n)
    terms = {0: {d: rng.randint(1, 5) for d in docs[::3]}, 1: {d: rng.randint(1, 9) for d in docs}, 2: {d: rng.randint(1, 9) for d in docs},
             3: {d: rng.randint(1, 9) for d in docs if d != 12}}
    seg = seg_of(terms, 4, extra=2)
    dl = [rng.randint(3, 70) for _ in range(n)]
    w = [F(0.3), F(1.7), F(0.9), F(2.9)]
    queries = [[(0, M, w[0]), (1, S, w[1]), (2, S, w[2]), (3, M, w[3])],
               [(1, S, w[1]), (0, M, w[0]), (2, M, w[2]), (3, S, w[3])],
               [(1, M, w[1]), (2, S, w[2]), (3, S, w[3]), (0, M, w[0])]]
    ref = ref_of(seg, 7, dl, queries, n)
    assert ref.anchors == [0, 1, 3] and all(m == len(terms[0]) for m in ref.match_counts) and ref.counts[0] == 3 * len(terms[0])
    for q in range(3):
        assert ref.order_matters(q), "query %d does not show the order of the additions" % q
        assert all(len(cs) == 4 for cs in ref.contributions[q].values())
    check(seg, 7, dl, queries, n, batch=None, ref=ref)


# ---- 4
def check_anchor_choice():
    batch = api.DeviceBatch(predictor())
    # term 0: df 2; term 1: df 2 (a tie with 0); term 2: df 4; term 3: df 0; term 4: df 1; term 5: df 3
    seg = seg_of({0: {1: 2, 3: 1}, 1: {1: 1, 4: 2}, 2: {0: 1, 1: 3, 3: 1, 4: 1}, 4: {3: 5}, 5: {0: 2, 1: 1, 2: 2}}, 6, extra=3)
    dl = [3, 2, 6, 10, 8]
    w = [idf_of(5, int(x)) for x in np.diff(seg.term.astype(np.int64))]

    def one(query, k=5):
        return check(seg, 0, dl, [query], k, batch=batch)
    # a df tie: the first MUST slot of the smallest df is the anchor; the places are one df, not the sum
    ref = one([(2, M, w[2]), (1, M, w[1]), (0, M, w[0])])
    assert ref.anchors == [1] and ref.counts == [2, 1, 0] and [d for d, _ in ref.hits[0]] == [1]
    ref = one([(0, M, w[0]), (1, M, w[1])])
    assert ref.anchors == [0] and ref.counts == [2, 1, 0]
    # a MUST of df 0 and a MUST out of range: no matches, the skipped slots counted, no place
    ref = one([(2, M, w[2]), (3, M, w[3]), (0, S, w[0])])
    assert ref.counts == [0, 0, 0]
    ref = one([(2, M, w[2]), (6, M, F(1)), (-1, S, F(1)), (7, N, F(0))])
    assert ref.counts == [0, 0, 3]
    ref = one([(2, M, w[2]), (-1, S, F(1)), (7, N, F(0))])   # out of range SHOULD / MUST_NOT: ignored
    assert ref.counts == [4, 4, 2]
    # only MUST_NOT slots; SHOULD with a MUST_NOT; the same term as MUST and MUST_NOT; a MUST repeated (scored twice)
    assert one([(2, N, F(0)), (0, N, F(0))]).counts == [0, 0, 0]
    ref = one([(2, S, w[2]), (5, S, w[5]), (0, N, F(0))])
    assert ref.counts == [7, 3, 0] and sorted(ref.scores[0]) == [0, 2, 4]
    assert one([(2, M, w[2]), (5, S, w[5]), (2, N, F(0))]).counts == [4, 0, 0]
    ref = one([(0, M, w[0]), (2, S, w[2]), (0, M, w[0])])
    assert ref.counts == [2, 2, 0] and all(len(cs) == 3 and searchref.bits(cs[0]) == searchref.bits(cs[2]) for cs in ref.contributions[0].values())
    # an empty query between non-empty ones, in one call with the above
    queries = [[(2, M, w[2]), (0, M, w[0])], [], [(5, S, w[5]), (2, N, F(0))], [], [], [(4, M, w[4]), (2, S, w[2])], []]
    ref = check(seg, 0, dl, queries, 2, batch=batch)
    assert ref.match_counts == [2, 0, 1, 0, 0, 1, 0] and ref.counts == [2 + 3 + 1, 4, 0]
    none = check(seg, 0, dl, [[], []], 2, batch=batch)
    assert none.counts == [0, 0, 0]
    # capacity_slots above the slots: the places behind them are not looked at
    same_as(run(seg, 0, dl, queries, 2, cap_slots=sum(len(q) for q in queries) + 300, batch=batch), ref)


def check_slot_limit():
    """1024 slots over short lists on both routes; one more is kErrQueryTooLong with the outputs left alone"""
    limit = api.DeviceBatch.postings_search_limit()
    assert limit == 1024
    batch = api.DeviceBatch(predictor())
    seg = seg_of({0: {0: 1, 2: 3}, 1: {1: 2, 2: 1, 4: 7}, 2: {3: 1}, 3: {0: 2, 2: 1, 4: 1}, 5: {2: 2, 3: 9}}, 6, extra=3)   # term 4: df 0
    dl = [3, 2, 6, 10, 8]
    rng = random.Random(9)
    body = [(t, F(0.3 + ((j * 37) % 101) / 97)) for j, t in enumerate(rng.choice([0, 1, 3, 5]) for _ in range(limit))]
    anchored = [(t, M if t == 0 and j % 50 == 0 else S, w) for j, (t, w) in enumerate(body[:-1])] + [(0, M, F(1.25))]
    loose = [(t, N if j == 700 else S, w) for j, (t, w) in enumerate(body[:699])] + [(2, N, F(0))] + [(t, S, w) for t, w in body[700:]]
    assert len(anchored) == limit and len(loose) == limit
    queries = [[(3, S, F(1))], anchored, [], loose]
    ref = check(seg, 0, dl, queries, 4, batch=batch)
    assert ref.anchors[1] is not None and ref.match_counts[1] >= 1 and ref.match_counts[3] >= 3 and 3 not in ref.scores[3]
    assert max(len(c) for c in ref.contributions[1].values()) > 300   # (the order of the additions: check_addition_order)
    for q, extra in ((1, (0, M, F(1))), (3, (0, S, F(1)))):
        longer = [x + [extra] if i == q else x for i, x in enumerate(queries)]
        r = run(seg, 0, dl, longer, 4, batch=batch)
        assert r.error is not None and LONG_ERROR in r.error and r.untouched(), r.error
    check(seg, 0, dl, queries, 4, batch=batch, ref=ref)   # the workspace takes the sound batch afterwards


# ---- 5
def check_bisection_edges():
    """the anchor's documents are below the first, the first, inside, in a gap of, the last and above the last of the bisected list; a list of
    length 1 as the anchor and as the bisected list"""
    batch = api.DeviceBatch(predictor())
    B = 40
    anchor = {B + d: 1 + d % 3 for d in (2, 5, 9, 20, 30)}
    wide = {B + d: 2 for d in (5, 6, 7, 9, 11, 30)}            # 2 below its first, 5 its first, 9 inside, 20 in a gap, 30 its last
    low = {B + d: 1 for d in range(3, 20)}                     # 2 below its first, 20 and 30 above its last
    single = {B + 9: 4}
    other = {B + 9: 1}
    seg = seg_of({0: anchor, 1: wide, 2: low, 3: single, 4: other, 5: {B + 31: 1}}, 6, extra=1)
    dl = [1 + (5 * d) % 23 for d in range(32)]
    w = [idf_of(32, int(x)) for x in np.diff(seg.term.astype(np.int64))]
    queries = []
    for t in (1, 2):
        for o in (M, S, N):
            queries.append([(0, M, w[0]), (t, o, w[t])])
            queries.append([(t, o, w[t]), (0, M, w[0])])
    queries += [[(3, M, w[3]), (1, M, w[1])], [(3, M, w[3]), (4, M, w[4])], [(4, M, w[4]), (3, N, F(0))], [(0, M, w[0]), (3, N, w[3])], [(0, M, w[0]), (5, N, F(0))],
                [(1, S, w[1]), (3, N, F(0))], [(2, S, w[2]), (0, S, w[0]), (1, N, F(0))]]
    ref = check(seg, B, dl, queries, 32, batch=batch)
    assert sorted(ref.scores[0]) == [B + 5, B + 9, B + 30] and sorted(ref.scores[4]) == [B + 2, B + 20] and sorted(ref.scores[6]) == [B + 5, B + 9]
    assert sorted(ref.scores[10]) == [B + 2, B + 20, B + 30] and ref.match_counts[12:15] == [1, 1, 0] and ref.anchors[13] == 0
    assert ref.match_counts[16] == 5 and B + 9 not in ref.scores[17] and len(ref.scores[17]) == 5


# ---- 6
def check_places(n):
    """n places on the anchored route (the anchor's df) and on the other one (two SHOULD lists that add up to n, and a MUST_NOT); every matching
    document scores the same where k cuts"""
    batch = api.DeviceBatch(predictor())
    a = n - n // 3
    seg = seg_of({0: {d: 1 for d in range(n)}, 1: {d: 1 + d % 2 for d in range(a)}, 2: {d: 1 for d in range(0, n + 9, 2)}, 3: {d: 2 for d in range(a - 5, n - 5)},
                  4: {d: 1 for d in range(0, 2 * n) if d % 5}}, 5, extra=2)
    dl = [7] * (2 * n)
    w = [idf_of(2 * n, int(x)) for x in np.diff(seg.term.astype(np.int64))]
    # anchored: term 0 (df n) is rarer than term 4 (df 1.6 n); even documents hold the forbidden term 2, multiples of 5 lack term 4
    queries = [[(4, M, w[4]), (0, M, w[0]), (2, N, F(0))]]
    ref = ref_of(seg, 0, dl, queries, n + 2)
    want = [d for d in range(n) if d % 2 and d % 5]
    assert ref.counts == [n, len(want), 0] and ref.anchors == [1] and [d for d, _ in ref.hits[0]] == want   # one score: by document
    assert len({searchref.bits(s) for _, s in ref.hits[0]}) == 1
    check(seg, 0, dl, queries, n + 2, batch=batch, ref=ref)
    for k in (1, len(want) - 1):   # k cuts the group of equal scores
        same_as(run(seg, 0, dl, queries, k, batch=batch), searchsuite.cut(ref, k))
    # unanchored: n places of two slots whose lists overlap in 5 documents
    queries = [[(1, S, w[1]), (3, S, w[3]), (2, N, F(0))]]
    ref = check(seg, 0, dl, queries, n + 2, batch=batch)
    assert ref.counts[0] == n and ref.counts[1] == len([d for d in range(n - 5) if d % 2]) and ref.anchors == [None]


# ---- 7
def check_high_documents(name):
    batch = api.DeviceBatch(predictor())
    doc_base = postingssuite.high_base(name, 37)
    seg, dl, queries = mixed_input(3, doc_base, batch)
    last = doc_base + 36
    for k in (1, 64):
        ref = check(seg, doc_base, dl, queries, k, batch=batch)
    hits = {d for h in ref.hits for d, _ in h}
    anchored = {d for h, a in zip(ref.hits, ref.anchors) if a is not None for d, _ in h}
    loose = {d for h, a in zip(ref.hits, ref.anchors) if a is None for d, _ in h}
    assert any(d >= 1 << 31 for d in anchored) and any(d >= 1 << 31 for d in loose) and last >= 1 << 31 and last in hits   # (k = 64: every match is a hit)
    assert (doc_base < 1 << 31) == (name == "2^31-3") and (last == 0xFFFFFFFF) == (name == "2^32-n")
    if name == "2^31-3":
        assert any(d < 1 << 31 for d in hits)
    # the last document of the word on both routes, required, forbidden and merely wanted
    B = postingssuite.high_base(name, 5)
    seg = seg_of({0: {B: 1, B + 2: 1, B + 4: 3}, 1: {B + 1: 1, B + 3: 2, B + 4: 1}, 2: {B + 4: 1}}, 3, extra=1)
    q = [[(0, M, F(1)), (1, M, F(2))], [(0, S, F(1)), (2, N, F(0))], [(1, M, F(1)), (2, S, F(3))], [(0, S, F(1)), (1, S, F(1))]]
    ref = check(seg, B, [2, 2, 2, 2, 5], q, 5, batch=batch)
    assert ref.match_counts == [1, 2, 3, 5] and ref.hits[0][0][0] == B + 4 and ref.hits[2][0][0] == B + 4


def check_merged_segment():
    """index_batches of three batches searched = index_batch of the concatenation searched = the definition; VaporettoTokenizer.boolean_search
    and its clause syntax"""
    tok, texts = searchsuite.fixture_tokenizer()
    toff, ids = tok.encode_batch(texts)
    dl = np.diff(toff.astype(np.int64)).astype(np.uint32)
    texts_q = ["+猫 東京特許許可局", "東京特許許可局 -猫", "", "+", "- +  ", "まぁ +だろう  -東京特許許可局", "-だ", "+１２３４５６円 +猫", "+猫 +まぁ", "猫 は -火星"]
    clauses = [[("猫", M), ("東京特許許可局", S)], [("東京特許許可局", S), ("猫", N)], [], [], [], [("まぁ", S), ("だろう", M), ("東京特許許可局", N)],
               [("だ", N)], [("１２３４５６円", M), ("猫", M)], [("猫", M), ("まぁ", M)], [("猫", S), ("は", S), ("火星", N)]]
    for doc_base in (0, 1000):
        whole = tok.index_batch(texts, doc_base)
        parts = tok.index_batches([texts[:30], texts[30:31], texts[31:]], doc_base)
        assert postingssuite.same_postings(whole, parts)
        df = whole.df()
        n_terms = len(df)
        queries = []
        for cl in clauses:
            query = []
            for text, occur in cl:
                coff, cids = tok.encode_batch([text])
                query += [(int(t), occur, (idf_of(len(texts), int(df[t])) if 0 <= t < n_terms else F(0)) if occur != N else F(0)) for t in cids]
            queries.append(query)
        assert any(len([x for x in q if x[1] == M]) > 1 for q in queries)   # a MUST clause of several tokens: every token a MUST slot
        for k in (1, 10):
            ref = boolref.BoolRef(whole.term_offsets, whole.docs, whole.tfs, doc_base, dl, queries, k)
            assert ref.match_counts[2:5] == [0, 0, 0] and ref.match_counts[6:8] == [0, 0] and max(ref.match_counts) > 10 and ref.counts[2] >= 4
            assert ref.vetoes["must"] >= 1 and ref.vetoes["must_not"] >= 1 and sum(1 for m in ref.match_counts if m) >= 4
            for post in (whole, parts):
                hits, mc = tok.boolean_search(post, texts_q, k)
                assert mc.tolist() == ref.match_counts and mc.dtype == np.uint64
                assert [[(d, searchref.bits(s)) for d, s in h] for h in hits] == [[(d, searchref.bits(s)) for d, s in h] for h in ref.hits]
                assert post.last_search_counts.tolist() == ref.counts
                hits2, _ = post.boolean_search([[(t, api.Occur(o)) for t, o, _w in q] for q in queries], k)   # the default weights
                assert [[(d, searchref.bits(s)) for d, s in h] for h in hits2] == [[(d, searchref.bits(s)) for d, s in h] for h in ref.hits]


def check_weights_and_parameters():
    batch = api.DeviceBatch(predictor())
    seg = seg_of({0: {0: 1, 1: 3, 3: 2}, 1: {1: 1, 2: 40, 3: 2}, 2: {2: 1}}, 3)
    dl = [4, 0, 41, 9]   # document 1 has postings and length 0: dl is the caller's
    shapes = [[(0, M), (1, S)], [(1, S), (2, N)], [(2, S), (0, M), (1, M)], [(1, M), (0, N)]]
    idf = searchsuite.with_idf(seg, 4, [[t for t, _ in q] for q in shapes])
    queries = [[(t, o, w) for (t, o), (_t, w) in zip(q, ws)] for q, ws in zip(shapes, idf)]
    ref = check(seg, 0, dl, [[(t, o, F(0)) for t, o, _w in q] for q in queries], 4, batch=batch)
    assert all(searchref.bits(s) == 0 for h in ref.hits for _, s in h) and [d for d, _ in ref.hits[0]] == [0, 1, 3]
    for k1, b in ((0.0, 0.75), (1.2, 0.0), (1.2, 1.0), (2.0, 0.5), (65536.0, 1.0)):
        ref = check(seg, 0, dl, queries, 4, k1, b, batch=batch)
        assert ref.match_counts == [3, 2, 2, 1] and 1 in ref.scores[0] and 1 in ref.scores[2]   # the document of length 0 on the anchored route
    ref = boolref.BoolRef(seg.term, seg.docs, seg.tfs, 0, dl, queries, 4, 0.0, 0.75)   # k1 = 0: every contribution is the slot's weight
    assert {searchref.bits(s) for _, s in ref.hits[3]} == {searchref.bits(queries[3][0][2])}
    # a MUST_NOT slot's weight is checked like the rest
    r = run(seg, 0, dl, [[(0, M, F(1)), (2, N, F(-1.0))]], 2, batch=batch)
    assert r.error is not None and WEIGHT_ERROR in r.error and r.untouched()


# ---- 8
def check_capacity(seed=3):
    batch = api.DeviceBatch(predictor())
    seg, dl, queries = mixed_input(seed, 5, batch)
    ref = ref_of(seg, 5, dl, queries, 3)
    need = ref.counts[0]
    candidates = searchref.SearchRef(seg.term, seg.docs, seg.tfs, 5, dl, [[(t, w) for t, _o, w in q] for q in queries], 3).counts[0]
    assert 0 < need < candidates   # the places are fewer than the OR search's candidates
    for cap in (need - 1, 0):
        r = run(seg, 5, dl, queries, 3, cap_places=cap, batch=batch)
        assert r.error is not None and CAND_ERROR in r.error, r.error
        assert int(r.counts[0]) == need and r.untouched()
    same_as(run(seg, 5, dl, queries, 3, cap_places=need, batch=batch), ref)
    same_as(run(seg, 5, dl, queries, 3, cap_places=candidates + tile() + 1, batch=batch), ref)


def check_errors():
    pred = predictor()
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    batch = api.DeviceBatch(pred)
    names = ("term", "docs", "tfs", "dl", "qoff", "qterms", "qweights", "qoccurs", "hd", "hs", "hc", "mc", "counts")
    A = {n: devmem.zeros(8, np.uint64) for n in names}

    def call(b=batch, n_terms=2, cap_post=2, doc_base=0, n_docs=2, n_q=1, cap_slots=1, k1=1.2, bb=0.75, avgdl=1.0, k=2, cap_cand=2, **null):
        p = {n: (0 if n in null else a.ptr) for n, a in A.items()}
        b.boolean_search_postings(p["term"], p["docs"], p["tfs"], n_terms, cap_post, doc_base, n_docs, p["dl"], p["qoff"], p["qterms"], p["qweights"],
                                  p["qoccurs"], n_q, cap_slots, k1, bb, avgdl, k, cap_cand, p["hd"], p["hs"], p["hc"], p["mc"], p["counts"], devmem.stream())

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
        st = _lib.load().vpt_postings_boolean_search_device(p_h, b_h, p["term"], p["docs"], p["tfs"], 2, 2, 0, 2, p["dl"], p["qoff"], p["qterms"], p["qweights"],
                                                            p["qoccurs"], 1, 1, 1.2, 0.75, 1.0, 2, 2, p["hd"], p["hs"], p["hc"], p["mc"], p["counts"],
                                                            devmem.stream())
        assert st == _lib.VPT_INVALID_ARGUMENT
        _expect(lambda: api._raise(st), "batch: does not belong to this predictor")
    batch.sync()
    call(k1=65536.0, bb=1.0, avgdl=2.0 ** 32)   # the ends of the ranges are inside; all-zero arrays: one query without a slot
    batch.sync()
    assert A["counts"].get(3).tolist() == [0, 0, 0] and int(A["mc"].get(1)[0]) == 0


def check_bad_occurs():
    """an occur of 3 or 255, on either route and in a query that is dead anyway: an error at the sync, the outputs left alone"""
    batch = api.DeviceBatch(predictor())
    seg = seg_of({0: {11: 1, 13: 2}, 1: {12: 1}, 3: {10: 1, 11: 1, 14: 4}}, 4, extra=2)
    dl = [3, 5, 2, 9, 4]
    w = F(1.25)
    sound = [[(0, M, w), (3, S, w)], [], [(1, S, w), (3, N, F(0))]]
    for bad in (3, 255):
        for q, j in ((0, 0), (0, 1), (2, 0), (2, 1)):
            queries = [[(t, bad if (i, s) == (q, j) else o, x) for s, (t, o, x) in enumerate(query)] for i, query in enumerate(sound)]
            r = run(seg, 10, dl, queries, 3, cap_places=16, batch=batch)
            assert r.error is not None and OCCUR_ERROR in r.error and r.untouched(), (bad, q, j, r.error)
            check(seg, 10, dl, sound, 3, batch=batch)   # the sound ones on the same workspace
        r = run(seg, 10, dl, [[(2, M, w), (0, bad, w)]], 3, cap_places=16, batch=batch)   # (term 2: df 0)
        assert r.error is not None and OCCUR_ERROR in r.error and r.untouched()
    r = run(seg, 10, dl, sound, 3, cap_slots=3, cap_places=16, batch=batch)   # capacity_slots cuts a slot off: the CSR ends above it
    assert r.error is not None and QCSR_ERROR in r.error and r.untouched()


def hostile_cases():
    """name -> (segment, queries, query_offsets or None, the message, or None where the call has to succeed)"""
    def base():
        return seg_of({0: {11: 1, 13: 2}, 1: {12: 1}, 3: {10: 1, 11: 1, 14: 4}}, 4, extra=2)   # term 0 2 3 3 6; cap 8; documents 10 .. 14
    w = F(1.25)
    sound = [[(0, M, w), (3, S, w)], [], [(1, S, w), (3, N, F(0.5))], [(3, M, w), (0, N, w)]]
    cases = {}

    def seg_case(name, fn, queries=sound, message=SEG_ERROR):
        s = base()
        fn(s)
        cases[name] = (s, queries, None, message)
    seg_case("descending_term_offsets", lambda s: s.term.__setitem__(3, 7))                   # term 3: [7, 6), a bisected list's bounds too
    seg_case("bound_above_capacity", lambda s: s.term.__setitem__(4, 9))
    seg_case("huge_offsets", lambda s: s.term.__setitem__(slice(1, 5), [1 << 40, 1 << 41, 1 << 62, (1 << 64) - 1]))
    seg_case("bisected_bounds_far_outside", lambda s: s.term.__setitem__(slice(3, 5), [(1 << 64) - 8, (1 << 64) - 1]))
    seg_case("anchor_document_below_doc_base", lambda s: s.docs.__setitem__(0, 9))
    seg_case("anchor_document_at_the_end", lambda s: s.docs.__setitem__(1, 15))
    seg_case("should_document_far_outside", lambda s: s.docs.__setitem__(2, 0xFFFFFFFF))
    seg_case("anchor_zero_tf", lambda s: s.tfs.__setitem__(1, 0))
    seg_case("bisected_zero_tf", lambda s: s.tfs.__setitem__(4, 0))                           # term 3's posting of document 11, found from term 0's
    seg_case("anchor_list_descends", lambda s: s.docs.__setitem__(slice(0, 2), [13, 11]))
    # only the list that deals out places is checked for ascent: a bisected one that descends is followed inside its bounds and not reported;
    # with the tie of the two dfs this also shows WHICH slot is the anchor (the first)
    tie = [[(0, M, w), (1, M, w)]]
    both = lambda s: (s.term.__setitem__(slice(1, 5), [2, 4, 4, 6]), s.docs.__setitem__(slice(0, 6), [11, 13, 13, 11, 10, 14]))   # term 1: 13, 11
    seg_case("bisected_list_descends_unreported", both, tie, None)
    seg_case("tie_second_order_the_descending_list_is_the_anchor", both, [[(1, M, w), (0, M, w)]])
    seg_case("bisected_documents_outside_the_range_unreported", lambda s: s.docs.__setitem__(slice(3, 6), [0, 5, 0xFFFFFFFF]), [[(0, M, w), (3, N, w)]], None)
    cases["descending_query_offsets"] = (base(), sound, [0, 2, 1, 4, 6], QCSR_ERROR)
    cases["query_offsets_end_above_capacity_slots"] = (base(), sound, [0, 2, 2, 4, 7], QCSR_ERROR)
    cases["query_offsets_far_above"] = (base(), sound, [0, 2, 1 << 63, (1 << 64) - 1, (1 << 64) - 1], QCSR_ERROR)
    for name, bad in (("nan_weight", F("nan")), ("negative_weight", F(-1.0)), ("negative_zero_weight", F(-0.0)), ("infinite_weight", F("inf"))):
        cases[name] = (base(), [[(0, M, w), (3, S, bad)], [], [(1, S, w), (3, N, F(0.5))]], None, WEIGHT_ERROR)
        cases[name + "_must_not"] = (base(), [[(0, M, w), (3, S, w)], [], [(1, S, w), (3, N, bad)]], None, WEIGHT_ERROR)
    for bad in (3, 128, 255):
        cases["occur_%d" % bad] = (base(), [[(0, M, w), (3, bad, w)], [], [(1, bad, w), (3, N, F(0.5))]], None, OCCUR_ERROR)
    return base(), sound, cases


N_HOSTILE = 27


def run_hostile():
    sound_seg, sound, cases = hostile_cases()
    assert len(cases) == N_HOSTILE, len(cases)
    dl = [3, 5, 2, 9, 4]
    batch = api.DeviceBatch(predictor())
    ran = 0
    for name, (seg, queries, qoff, message) in cases.items():
        r = run(seg, 10, dl, queries, 3, cap_places=16, qoff=qoff, batch=batch)
        if message is None:
            assert r.error is None and not r.untouched(), (name, r.error)
        else:
            assert r.error is not None and message in r.error, (name, r.error)
            assert r.untouched(), name
        check(sound_seg, 10, dl, sound, 3, batch=batch)   # the sound ones on the same workspace
        ran += 1
    del batch
    return ran


def check_determinism(seed=12):
    rng = random.Random(seed)
    T = tile()
    pred = predictor()
    one, two = api.DeviceBatch(pred), api.DeviceBatch(pred)
    n_docs, n_terms = 700, 40
    terms = {}
    for _ in range(4 * T):
        terms.setdefault(postingssuite.zipf(rng, n_terms), {})[rng.randrange(n_docs)] = rng.randint(1, 9)
    seg = seg_of(terms, n_terms)
    dl = [rng.randint(0, 90) for _ in range(n_docs)]
    plain = searchsuite.with_idf(seg, n_docs, [[rng.randrange(n_terms) for _ in range(rng.randint(0, 6))] for _ in range(23)])
    queries = with_occurs(plain, lambda q, j: rng.choice([S, S, S, M, N]))
    a = run(seg, 0, dl, queries, 10, batch=one)
    b = run(seg, 0, dl, queries, 10, batch=one)
    run(seg_of({1: {2: 3}}, 4), 0, [1, 1, 1], [[(1, M, F(1))]], 1, batch=two)   # (the second workspace's scratch holds something else)
    c = run(seg, 0, dl, queries, 10, batch=two)
    assert a.error is None and a.same_bytes(b) and a.same_bytes(c)
    ref = ref_of(seg, 0, dl, queries, 10)
    assert T < ref.counts[0] <= 3 * T + 1 and ref.vetoes["must"] and ref.vetoes["must_not"]
    same_as(a, ref)


def check_scratch_reuse(seed=17):
    """one workspace through the five drivers that lay out its postings scratch, each in a layout of its own over the same bytes -- a postings
    pass with positions, a positional general merge of two segments, a phrase search with 2 T + 1 probes, an OR search with T + 1 candidates
    and a boolean search with a MUST, a SHOULD and a MUST_NOT slot and T - 1 places, in this order: every result is, byte for byte, that of
    the same call on a workspace of its own"""
    from tests import phrasesuite, positionsmergesuite
    rng = random.Random(seed)
    T = tile()
    pred = predictor()
    docs = positionsmergesuite.random_docs(rng, 30, 6)
    toff, ids = csr(docs)
    owner = [[rng.randrange(2) for _ in d] for d in docs]
    segs = [positionsmergesuite.pseg_of(d, 6, 0, p) for d, p in positionsmergesuite.deal(docs, None, owner, 2)]
    n = 2 * T + 1
    phrase_docs = [[0, 1, 2] * min(3, n - a) for a in range(0, n, 3)]   # 2 T + 1 tokens of each term
    phrase_seg = phrasesuite.pseg_of(phrase_docs, 3)
    wide = seg_of({0: {d: 1 + d % 3 for d in range(T + 1)}, 1: {d: 2 for d in range(0, T - 1, 2)}, 2: {d: 1 for d in range(T - 1)},
                   3: {d: 1 for d in range(5, T - 1, 7)}}, 4, extra=2)
    dl = [1 + (7 * d) % 50 for d in range(T + 1)]
    steps = [
        ("postings", None, lambda b: postingssuite.run(toff, ids, 6, batch=b)),
        ("merge", None, lambda b: positionsmergesuite.run(segs, 6, False, batch=b)),
        ("phrase", n, lambda b: phrasesuite.run(phrase_seg, 0, [len(d) for d in phrase_docs], [[0, 1]], [F(1.5)], 7, batch=b)),
        ("search", T + 1, lambda b: searchsuite.run(wide, 0, dl, [[(0, F(0.75))]], 7, batch=b)),
        ("boolean", T - 1, lambda b: run(wide, 0, dl, [[(2, M, F(1.25)), (1, S, F(0.5)), (3, N, F(0))]], 7, batch=b)),
    ]
    shared = api.DeviceBatch(pred)
    for name, places, step in steps:
        got, want = step(shared), step(api.DeviceBatch(pred))
        assert got.error is None and want.error is None, (name, got.error, want.error)
        assert got.same_bytes(want), name
        assert places is None or int(got.counts[0]) == places, (name, got.counts.tolist())
    assert int(got.mc[0]) == len([d for d in range(T - 1) if (d - 5) % 7])   # (the last step: the MUST list without the forbidden documents)


# ---- 9
def check_host_call(seed=5):
    """vpt_postings_boolean_search through Postings.boolean_search: host arrays in and out, the default weights and the caller's"""
    rng = random.Random(seed)
    pred = predictor()
    terms = {}
    for _ in range(300):
        terms.setdefault(postingssuite.zipf(rng, 30), {})[100 + rng.randrange(50)] = rng.randint(1, 5)
    seg = seg_of(terms, 30)
    term, docs, tfs = seg.triple()
    post = api.Postings(term, docs.copy(), tfs.copy(), None, None, 0)
    dl = np.array([rng.randint(1, 60) for _ in range(50)], np.uint32)
    shapes = [[(rng.randrange(30), rng.choice([S, S, M, N])) for _ in range(rng.randint(1, 4))] for _ in range(12)] + [[], [(-1, S), (30, N), (2, M)], [(30, M), (2, S)],
                                                                                                                       [(1, M), (2, M), (0, S)], [(2, M), (1, N)]]
    df = np.diff(term.astype(np.int64))
    queries = [[(t, o, idf_of(50, int(df[t])) if 0 <= t < 30 and o != N else F(0)) for t, o in q] for q in shapes]
    for k in (1, 5, 60):
        ref = boolref.BoolRef(term, docs, tfs, 100, dl, queries, k)
        hits, mc = post.boolean_search([[(t, api.Occur(o)) for t, o in q] for q in shapes], k, dl, 100, predictor=pred)
        assert [[(d, searchref.bits(s)) for d, s in h] for h in hits] == [[(d, searchref.bits(s)) for d, s in h] for h in ref.hits]
        assert all(type(s) is np.float32 for h in hits for _, s in h) and mc.tolist() == ref.match_counts and post.last_search_counts.tolist() == ref.counts
    assert ref.vetoes["must"] and ref.vetoes["must_not"] and sum(1 for m in ref.match_counts if m) > 3 and ref.counts[2] == 3
    mine = [[(t, o, F(0.25 + j)) for j, (t, o) in enumerate(q)] for q in shapes]
    ref = boolref.BoolRef(term, docs, tfs, 100, dl, mine, 4, 0.9, 0.4)
    hits, mc = post.boolean_search(mine, 4, dl, 100, 0.9, 0.4, predictor=pred)
    assert [[(d, searchref.bits(s)) for d, s in h] for h in hits] == [[(d, searchref.bits(s)) for d, s in h] for h in ref.hits]
    # all SHOULD: Postings.search's hits
    ids = [[t for t, _o in q] for q in shapes]
    a, amc = post.boolean_search([[(t, api.Occur.SHOULD) for t in q] for q in ids], 5, dl, 100, predictor=pred)
    b, bmc = post.search(ids, 5, dl, 100, predictor=pred)
    assert [[(d, searchref.bits(s)) for d, s in h] for h in a] == [[(d, searchref.bits(s)) for d, s in h] for h in b] and amc.tolist() == bmc.tolist()
    _expect(lambda: post.boolean_search(mine, 4, dl, 100), "boolean_search: no predictor")
    _expect(lambda: post.boolean_search(mine, 4, predictor=pred), "boolean_search: the postings carry no doc_lens / doc_base")
    _expect(lambda: post.boolean_search(mine, 0, dl, 100, predictor=pred), "k: must be at least 1")
    _expect(lambda: post.boolean_search([[(1, 3)]], 4, dl, 100, predictor=pred), OCCUR_ERROR)
    _expect(lambda: post.boolean_search([[(1, 300)]], 4, dl, 100, predictor=pred), OCCUR_ERROR)
    _expect(lambda: post.boolean_search([[(1,)]], 4, dl, 100, predictor=pred), "a slot is \\(term, occur\\) or \\(term, occur, weight\\)")
    _expect(lambda: post.boolean_search([[(1, M, F(-1))]], 4, dl, 100, predictor=pred), WEIGHT_ERROR)
    assert post.boolean_search([], 4, dl, 100, predictor=pred)[0] == []
    assert [int(x) for x in api.Occur] == [0, 1, 2] and api.Occur.MUST_NOT == N


def example_lines(post, dl, doc_base, query, k):
    """the lines examples/token_stream.cpp --postings --boolean prints for these hits"""
    ref = boolref.BoolRef(post.term_offsets, post.docs, post.tfs, doc_base, dl, [query], k)
    return ["%d\t%08x\t%.9g" % (d, searchref.bits(s), float(s)) for d, s in ref.hits[0]], ref


def main(argv):
    assert argv == ["--emu-hostile"], "usage: python -m tests.boolsuite --emu-hostile"
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
