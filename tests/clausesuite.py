"""The checks of the phrase lists and of the clause search (vpt_postings_phrase_lists_device, vpt_postings_clause_search_device,
vpt_postings_phrase_lists, vpt_postings_clause_search; kernels_postings_phrase.hip, kernels_postings_boolean.hip) against the definition of
tests/clauseref.py and against the calls they are made of, run on the CPU emulator by tests/test_postings_clause_emu.py and on the MI355X by
tests/test_postings_clause_gpu.py; every comparison of documents, counts, frequencies and score BITS is exact equality.

    python -m tests.clausesuite --emu-hostile     the hostile inputs on the emulator, in a child process (hipemu checks its red zones when
                                                  the workspace goes)

Every array handed to a device call has exactly the size the call is told and guard words on both sides, checked after the sync with the
inputs unwritten; the outputs are filled with SENTINEL first, so an entry a call must not write is seen to be left alone (boolsuite's
arrangement).  T = vpt_postings_tile (4096); no case has more than 3 T + 1 probes or list entries, or 6 T + 3 places."""
import random
import sys

import numpy as np

from tests import boolref, boolsuite, clauseref, devmem, patterntagsuite, phraseref, phrasesuite, postingssuite, searchref, searchsuite, vocabsuite
from vaporetto_amd import _lib, api

G = postingssuite.G
SENTINEL = postingssuite.SENTINEL
SEG_ERROR = searchsuite.SEG_ERROR
QCSR_ERROR = searchsuite.QCSR_ERROR
CAND_ERROR = searchsuite.CAND_ERROR
LONG_ERROR = phrasesuite.LONG_ERROR
PROBES_ERROR = phrasesuite.PROBES_ERROR
LISTS_ERROR = "capacity_lists: smaller than the number of list entries"
predictor = postingssuite.predictor
tile = postingssuite.tile
csr = postingssuite.csr
_expect = postingssuite._expect
pseg_of = phrasesuite.pseg_of
idf_of = searchsuite.idf_of
same_as = searchsuite.same_as
bits = searchref.bits
F = np.float32
S, M, N = boolref.SHOULD, boolref.MUST, boolref.MUST_NOT
OUTPUTS = searchsuite.OUTPUTS
LISTS = ("loff", "ldocs", "ltfs")


class Result(searchsuite.Result):
    def same_bytes(self, other):
        return searchsuite.Result.same_bytes(self, other) and all(getattr(self, n).tobytes() == getattr(other, n).tobytes() for n in LISTS + ("lcounts",))

    def lists_untouched(self):
        return (self.loff == np.uint64(SENTINEL)).all() and (self.ldocs == SENTINEL).all() and (self.ltfs == SENTINEL).all()


def list_bound(seg, phrases):
    """what always suffices as capacity_lists, from the segment's bounds alone: per phrase the smallest df among its terms"""
    df = lambda t: int(seg.term[t + 1]) - int(seg.term[t])
    return sum(min(df(t) for t in ph) if ph and len(ph) <= 64 and all(0 <= t < seg.n_terms for t in ph) else 0 for ph in phrases)


def place_bound(seg, phrases, queries):
    """boolsuite.places_of with every list counted as its bound"""
    n = 0
    for q in queries:
        df = []
        for t, _o, _w in q:
            if 0 <= t < seg.n_terms:
                df.append(max(int(seg.term[t + 1]) - int(seg.term[t]), 0))
            else:
                df.append(list_bound(seg, [phrases[t - seg.n_terms]]) if seg.n_terms <= t < seg.n_terms + len(phrases) else 0)
        must = [df[j] for j, x in enumerate(q) if x[1] == M]
        n += (0 if 0 in must else min(must)) if must else sum(df[j] for j, x in enumerate(q) if x[1] == S)
    return n


def run(seg, doc_base, dl, phrases, queries, k, k1=1.2, b=0.75, cap_probes=None, cap_lists=None, cap_places=None, batch=None, sync_between=False,
        lists=None, poff=None, n_lists=None, search=True):
    """vpt_postings_phrase_lists_device over `phrases` (None: no lists call; `lists` = (offsets, docs, tfs) are then the derived segment), then
    vpt_postings_clause_search_device over `queries` of slots (term, occur, weight) on the same stream -- with no sync between the two unless
    sync_between -- on guarded arrays of exactly the sizes the calls are told."""
    batch = batch or api.DeviceBatch(predictor())
    dl = np.asarray(dl, np.uint32)
    avgdl = searchsuite.avgdl_of(dl)
    I = {"term": G(seg.term), "docs": G(seg.docs), "tfs": G(seg.tfs), "first": G(seg.first), "ppos": G(seg.ppos), "dl": G(dl)}
    O = {}
    r = Result()
    r.error = r.lists_error = None
    if phrases is not None:
        pflat = [t for ph in phrases for t in ph]
        cap_probes = phrasesuite.probes_of(seg, [ph for ph in phrases if len(ph) <= 64]) if cap_probes is None else cap_probes
        cap_lists = list_bound(seg, phrases) if cap_lists is None else cap_lists
        I["poff"] = G(np.array([0] + list(np.cumsum([len(ph) for ph in phrases])), np.uint64) if poff is None else np.asarray(poff, np.uint64))
        I["pterms"] = G(np.array(pflat + [0], np.int64).astype(np.int32)[:max(len(pflat), 1)])
        n_l = len(phrases)
        O.update({"loff": G(np.full(n_l + 1, SENTINEL, np.uint64)), "ldocs": G(np.full(max(cap_lists, 1), SENTINEL, np.uint32)),
                  "ltfs": G(np.full(max(cap_lists, 1), SENTINEL, np.uint32)), "lcounts": G(np.full(3, SENTINEL, np.uint64))})
        try:
            batch.phrase_lists_postings(I["term"].ptr, I["docs"].ptr, I["tfs"].ptr, I["first"].ptr, I["ppos"].ptr, seg.n_terms, seg.cap, seg.cap_pos,
                                        doc_base, len(dl), I["poff"].ptr, I["pterms"].ptr, n_l, len(pflat), cap_probes, O["loff"].ptr, O["ldocs"].ptr,
                                        O["ltfs"].ptr, cap_lists, O["lcounts"].ptr, devmem.stream())
            if sync_between:
                batch.sync()
        except api.VaporettoError as e:
            r.error = r.lists_error = str(e)
        L = O
    elif lists is None:   # no derived segment at all: n_lists = 0 and three NULL pointers
        class _Null:
            ptr = 0
        n_l, cap_lists, L = 0, 0, {n: _Null for n in LISTS}
    else:
        offsets, ldocs, ltfs = lists
        n_l, cap_lists = len(offsets) - 1, (len(ldocs) if cap_lists is None else cap_lists)
        L = {"loff": G(np.asarray(offsets, np.uint64)), "ldocs": G(np.array(list(ldocs) + [SENTINEL], np.uint32)[:max(cap_lists, 1)]),
             "ltfs": G(np.array(list(ltfs) + [SENTINEL], np.uint32)[:max(cap_lists, 1)])}
        I.update({"in_" + n: a for n, a in L.items()})
    n_l = n_l if n_lists is None else n_lists
    if search:
        flat = [x for q in queries for x in q]
        n_q, n_s = len(queries), len(flat)
        I["qoff"] = G(np.array([0] + list(np.cumsum([len(q) for q in queries])), np.uint64))
        I["qterms"] = G(np.array([t for t, _o, _w in flat] + [0], np.int64).astype(np.int32)[:max(n_s, 1)])
        I["qweights"] = G(np.array([w for _t, _o, w in flat] + [0], np.float32)[:max(n_s, 1)])
        I["qoccurs"] = G(np.array([o for _t, o, _w in flat] + [0], np.uint8)[:max(n_s, 1)])
        cap_places = place_bound(seg, phrases or [[]] * n_l, queries) if cap_places is None else cap_places
        O.update({"hd": G(np.full(n_q * k, SENTINEL, np.uint32)), "hs": G(np.full(n_q * k, SENTINEL, np.uint32)), "hc": G(np.full(n_q, SENTINEL, np.uint32)),
                  "mc": G(np.full(n_q, SENTINEL, np.uint64)), "counts": G(np.full(3, SENTINEL, np.uint64))})
        try:
            if r.error is None or not sync_between:
                batch.clause_search_postings(I["term"].ptr, I["docs"].ptr, I["tfs"].ptr, seg.n_terms, seg.cap, L["loff"].ptr, L["ldocs"].ptr, L["ltfs"].ptr,
                                             n_l, cap_lists, doc_base, len(dl), I["dl"].ptr, I["qoff"].ptr, I["qterms"].ptr, I["qweights"].ptr,
                                             I["qoccurs"].ptr, n_q, n_s, k1, b, avgdl, k, cap_places, O["hd"].ptr, O["hs"].ptr, O["hc"].ptr, O["mc"].ptr,
                                             O["counts"].ptr, devmem.stream())
        except api.VaporettoError as e:
            r.error = r.error or str(e)
        r.k, r.n_q = k, n_q
    try:
        batch.sync()
    except api.VaporettoError as e:
        r.error = r.error or str(e)
    bad = [name for name, a in list(I.items()) + list(O.items()) if not a.guards_intact()]
    assert not bad, ("guard words overwritten", bad)
    assert all(a.get().tobytes() == a.sent.tobytes() for a in I.values()), "an input was written"
    for name, a in O.items():
        setattr(r, name, a.get())
    return r


def lists_same_as(r, ref):
    """the three list arrays and the counts are the definition's, and nothing behind the entries was written"""
    assert r.error is None, r.error
    assert r.lcounts.tolist() == ref.counts, (r.lcounts.tolist(), ref.counts)
    n = ref.counts[1]
    assert r.loff.tolist() == ref.offsets and r.ldocs[:n].tolist() == ref.docs and r.ltfs[:n].tolist() == ref.tfs
    assert (r.ldocs[n:] == SENTINEL).all() and (r.ltfs[n:] == SENTINEL).all()


def check(docs, n_terms, doc_base, phrases, queries, k, positions=None, batch=None, extra=0, seg=None, **kw):
    """lists, then the clause search with no sync between them, against ListsRef and ClauseRef"""
    seg = seg or pseg_of(docs, n_terms, doc_base, positions, extra)
    lref = clauseref.ListsRef(docs, n_terms, doc_base, phrases, positions)
    ref = clauseref.ClauseRef(docs, n_terms, doc_base, lref.lists, queries, k)
    r = run(seg, doc_base, [len(d) for d in docs], phrases, queries, k, batch=batch, **kw)
    lists_same_as(r, lref)
    same_as(r, ref)
    return ref, lref, r


def device_pseg(docs, n_terms, doc_base, batch):
    """a positional segment as the device's postings pass and positions call leave it: capacity = the tokens, SENTINEL behind what it holds"""
    toff, ids = csr(docs)
    n = len(ids)
    A = {"toff": G(toff), "ids": G(ids)}
    O = {"term": G(np.full(n_terms + 1, SENTINEL, np.uint64)), "docs": G(np.full(n, SENTINEL, np.uint32)), "tfs": G(np.full(n, SENTINEL, np.uint32)),
         "counts": G(np.full(2, SENTINEL, np.uint64)), "first": G(np.full(n + 1, SENTINEL, np.uint64)), "order": G(np.full(n, SENTINEL, np.uint32)),
         "ppos": G(np.full(n, SENTINEL, np.uint32))}
    batch.postings(A["toff"].ptr, len(docs), A["ids"].ptr, n, n_terms, doc_base, O["term"].ptr, O["docs"].ptr, O["tfs"].ptr, n, O["first"].ptr, O["order"].ptr,
                   O["counts"].ptr, devmem.stream())
    batch.postings_positions(A["toff"].ptr, len(docs), n, 0, O["term"].ptr, n_terms, O["first"].ptr, n, O["order"].ptr, O["ppos"].ptr, devmem.stream())
    batch.sync()
    n_post = int(O["counts"].get()[0])
    seg = phrasesuite.PSeg(O["term"].get(), O["docs"].get()[:n_post], O["tfs"].get()[:n_post], O["first"].get()[:n_post + 1],
                           O["ppos"].get()[:int(O["first"].get()[n_post])])
    want = pseg_of(docs, n_terms, doc_base)
    assert all(getattr(seg, a).tobytes() == getattr(want, a).tobytes() for a in ("term", "docs", "tfs", "first", "ppos"))
    seg = phrasesuite.PSeg(seg.term, seg.docs, seg.tfs, seg.first, seg.ppos, extra=n - n_post)   # (the capacity the pass was given)
    return seg


def random_queries(rng, n_terms, phrases, n=17):
    """slots over the terms and the lists of `phrases` under all three occurs; the weights are idf-like and differ per slot"""
    out = []
    for _ in range(n):
        q = []
        for _ in range(rng.randint(1, 4)):
            t = rng.randrange(n_terms) if rng.random() < 0.45 else n_terms + rng.randrange(len(phrases))
            o = rng.choice([S, S, M, M, N])
            q.append((t, o, F(0) if o == N else F(0.25 + rng.randrange(300) / 97)))
        out.append(q)
    return out


PHRASES = [[0, 1], [1, 0, 2], [2, 2], [0], [1, 1, 1, 1, 1, 1, 1], [], [2, 7], [0, 1, 2, 0], [1, 2]]


# ---- 1
def check_no_lists_is_the_boolean_search(seed=3):
    """n_lists = 0: vpt_postings_boolean_search_device's four outputs and counts, byte for byte -- with NULL list pointers too"""
    batch = api.DeviceBatch(predictor())
    for doc_base in (0, 1000):
        docs = phrasesuite.random_docs(seed, alphabet=5)
        seg, dl = pseg_of(docs, 5, doc_base, extra=2), [len(d) for d in docs]
        queries = random_queries(random.Random(seed), 5, [[]], 17)
        queries = [[(t if t < 5 else 9, o, w) for t, o, w in q] for q in queries]   # (9: out of range in both calls)
        for k in (1, 3, 64):
            theirs = boolsuite.run(seg, doc_base, dl, queries, k, batch=batch)
            mine = run(seg, doc_base, dl, None, queries, k, lists=([0], [], []), cap_lists=0, cap_places=boolsuite.places_of(seg, queries), batch=batch)
            assert theirs.error is None and searchsuite.Result.same_bytes(mine, theirs)
            null = run(seg, doc_base, dl, None, queries, k, cap_places=boolsuite.places_of(seg, queries), batch=batch)
            assert searchsuite.Result.same_bytes(null, theirs)
            same_as(mine, boolref.BoolRef(seg.term, seg.docs, seg.tfs, doc_base, dl, queries, k))
        assert int(theirs.counts[1]) > 20 and int(theirs.counts[2]) >= 1


# ---- 2
def check_one_term_phrases_are_the_terms_lists(seed=3):
    batch = api.DeviceBatch(predictor())
    n_terms = 5
    docs = phrasesuite.random_docs(seed, alphabet=n_terms) + [[4, 4, 4]]
    dl = [len(d) for d in docs]
    for doc_base in (0, 1000):
        seg = pseg_of(docs, n_terms, doc_base, extra=2)
        phrases = [[t] for t in range(n_terms)]
        rng = random.Random(seed)
        by_term = random_queries(rng, n_terms, [[]], 17)
        by_term = [[(t if t < n_terms else 0, o, w) for t, o, w in q] for q in by_term]
        by_list = [[(n_terms + t, o, w) for t, o, w in q] for q in by_term]
        for k in (1, 64):
            r = run(seg, doc_base, dl, phrases, by_list, k, batch=batch)
            assert r.error is None
            n = int(seg.term[n_terms])
            assert r.loff.tolist() == seg.term.tolist() and r.ldocs[:n].tobytes() == seg.docs[:n].tobytes() and r.ltfs[:n].tobytes() == seg.tfs[:n].tobytes()
            assert r.lcounts.tolist() == [int(seg.first[n]), n, 0]
            theirs = boolsuite.run(seg, doc_base, dl, by_term, k, batch=batch)
            assert theirs.error is None and searchsuite.Result.same_bytes(r, theirs) and int(theirs.counts[1]) > 20


# ---- 3
def check_one_should_slot_is_the_phrase_search(seed=7):
    """a query of one SHOULD slot naming a phrase's list, under the phrase weight: the phrase search's documents, score bits, hit counts and
    match counts; the list's tfs are its hit_freqs"""
    batch = api.DeviceBatch(predictor())
    docs = phrasesuite.random_docs(seed)
    dl = [len(d) for d in docs]
    phrases = [ph for ph in PHRASES if all(0 <= t < 3 for t in ph)]
    weights = phrasesuite.weights_of(docs, 3, phrases)
    for doc_base in (0, 1000):
        seg = pseg_of(docs, 3, doc_base, extra=1)
        queries = [[(3 + i, S, w)] for i, w in enumerate(weights)]
        for k in (1, 3, 64):
            theirs = phrasesuite.run(seg, doc_base, dl, phrases, weights, k, batch=batch)
            mine = run(seg, doc_base, dl, phrases, queries, k, batch=batch)
            assert theirs.error is None and mine.error is None
            assert all(getattr(mine, n).tobytes() == getattr(theirs, n).tobytes() for n in OUTPUTS), k
            assert mine.lcounts.tolist() == theirs.counts.tolist() and int(mine.counts[1]) == int(theirs.counts[1])
        for q in range(len(phrases)):   # k = 64: every match is a hit
            a, b, n = int(mine.loff[q]), int(mine.loff[q + 1]), int(theirs.hc[q])
            assert b - a == n == int(theirs.mc[q])
            assert sorted(zip(theirs.hd[q * 64:q * 64 + n].tolist(), theirs.hf[q * 64:q * 64 + n].tolist())) == list(zip(mine.ldocs[a:b].tolist(), mine.ltfs[a:b].tolist()))
        assert max(theirs.mc.tolist()) > 10 and max(theirs.hf[theirs.hf != SENTINEL].tolist()) > 1 and 0 in theirs.mc.tolist()


# ---- 4
def check_random(seed=8):
    """random mixed queries over a postings-pass positional segment: term and phrase slots under all three occurs"""
    batch = api.DeviceBatch(predictor())
    docs = phrasesuite.random_docs(seed)
    rng = random.Random(seed + 1)
    queries = random_queries(rng, 3, PHRASES, 23) + [[(3, M, F(1.5)), (-1, S, F(1)), (3 + len(PHRASES), S, F(1)), (40, N, F(0))]]
    lref = clauseref.ListsRef(docs, 3, 0, PHRASES)
    big = clauseref.ClauseRef(docs, 3, 0, lref.lists, queries, 64)
    # what the input has to hold, by the definition alone and before any device call
    kinds = {(("list" if t >= 3 else "term"), o) for q in queries for t, o, _w in q if 0 <= t < 3 + len(PHRASES)}
    assert kinds == {(a, o) for a in ("list", "term") for o in (S, M, N)}
    assert any(m > 3 for m in big.match_counts) and any(m == 0 for m in big.match_counts) and big.vetoes["must"] and big.vetoes["must_not"]
    assert any(a is not None and q[a][0] >= 3 for a, q in zip(big.anchors, queries)) and any(a is None and m for a, m in zip(big.anchors, big.match_counts))
    assert big.counts[2] == 3 and lref.counts[2] == 1 and lref.counts[1] > 50 and max(lref.tfs) > 1
    for doc_base in (0, 1000):
        seg = device_pseg(docs, 3, doc_base, batch)
        for k in (1, 3, 64):
            check(docs, 3, doc_base, PHRASES, queries, k, batch=batch, seg=seg)


# ---- 5
def check_addition_order():
    """four scoring slots on the anchored route; the phrase clause (the rarest MUST, so the anchor) stands first, in the middle and last"""
    rng = random.Random(21)
    n = 24
    docs = []
    for d in range(n):
        body = [rng.choice([1, 2, 3]) for _ in range(rng.randint(3, 30))] + [1, 2, 3]
        if d % 3 == 0:
            at = rng.randrange(len(body))
            body[at:at] = [0, 4] * rng.randint(1, 3)
        docs.append(body)
    w = [F(0.3), F(1.7), F(0.9), F(2.9)]
    P = 5   # the list of phrase [0, 4]
    queries = [[(P, M, w[0]), (1, S, w[1]), (2, S, w[2]), (3, M, w[3])],
               [(1, S, w[1]), (P, M, w[0]), (2, M, w[2]), (3, S, w[3])],
               [(1, M, w[1]), (2, S, w[2]), (3, S, w[3]), (P, M, w[0])]]
    lref = clauseref.ListsRef(docs, 5, 7, [[0, 4]])
    ref = clauseref.ClauseRef(docs, 5, 7, lref.lists, queries, n)
    assert ref.anchors == [0, 1, 3] and all(m == 8 for m in ref.match_counts) and ref.counts[0] == 3 * 8 and max(lref.tfs) > 1
    for q in range(3):
        assert ref.order_matters(q), "query %d does not show the order of the additions" % q
        assert all(len(cs) == 4 for cs in ref.contributions[q].values())
    check(docs, 5, 7, [[0, 4]], queries, n)


# ---- 6
def check_anchor_choice():
    batch = api.DeviceBatch(predictor())
    # term 0: df 3; term 1: df 4; term 2: df 2; term 3: df 0; phrase [0, 1]: df 2 (documents 0, 3); [1, 0]: df 1; [2, 2]: df 1; [0, 0]: df 1 (pf 2)
    docs = [[0, 1, 2, 2, 2], [1, 0, 0, 0], [1, 1], [2, 0, 1, 0, 1], []]
    phrases = [[0, 1], [1, 0], [2, 2], [0, 0], [0, 3], [1, 2, 1]]
    L = lambda i: 4 + i
    w = F(1.25)
    lref = clauseref.ListsRef(docs, 4, 0, phrases)
    assert lref.lists == [[(0, 1), (3, 2)], [(1, 1), (3, 1)], [(0, 2)], [(1, 2)], [], []]   # (`a a`: two starts in 0 0 0; 2 2 2 likewise)

    def one(query, k=5):
        return check(docs, 4, 0, phrases, [query], k, batch=batch)[0]
    ref = one([(1, M, w), (L(0), M, w), (0, S, w)])   # the phrase list is the rarest MUST
    assert ref.anchors == [1] and ref.counts == [2, 2, 0]
    ref = one([(2, M, w), (L(0), M, w)])              # a df tie between a term and a list: the first slot
    assert ref.anchors == [0] and ref.counts == [2, 2, 0]
    ref = one([(L(0), M, w), (2, M, w)])
    assert ref.anchors == [0] and ref.counts == [2, 2, 0]
    assert one([(1, M, w), (L(4), M, w)]).counts == [0, 0, 0]     # a MUST phrase that matches nothing (a term of df 0) kills its query
    assert one([(1, M, w), (L(5), M, w)]).counts == [0, 0, 0]     # ... (no occurrence)
    ref = one([(1, M, w), (L(5), S, w), (L(4), S, w)])            # a SHOULD phrase that matches nothing adds nothing
    assert ref.counts == [4, 4, 0] and all(len(c) == 1 for c in ref.contributions[0].values())
    ref = one([(1, S, w), (L(1), N, F(0))])                       # a MUST_NOT phrase vetoes exactly its documents
    assert sorted(ref.scores[0]) == [0, 2] and ref.counts == [4, 2, 0]
    ref = one([(L(3), M, w), (0, S, w)])                          # the phrase `a a`
    assert sorted(ref.scores[0]) == [1] and len(ref.contributions[0][1]) == 2
    ref = one([(L(2), S, w), (L(3), S, w), (L(0), N, F(0))])      # only lists, no anchor
    assert sorted(ref.scores[0]) == [1] and ref.counts == [2, 1, 0]
    ref = one([(L(6), M, w), (-1, S, w), (1, S, w)])              # a list out of range: as a term out of range
    assert ref.counts == [0, 0, 2]
    queries = [[(L(0), M, w), (1, S, w)], [], [(L(1), S, w), (L(2), S, w), (2, N, F(0))], [(0, M, w), (L(3), N, w)]]
    ref = check(docs, 4, 0, phrases, queries, 2, batch=batch)[0]
    assert ref.match_counts == [2, 0, 1, 2]


def check_phrase_limit():
    """a phrase at the 64-term limit, and one term more: an error at the sync with everything left alone"""
    limit = api.DeviceBatch.postings_phrase_limit()
    assert limit == 64
    batch = api.DeviceBatch(predictor())
    docs = [[0, 1] * 40, [1, 0] * 32 + [1], [0, 1] * 32, [0] * 70, []]
    at_limit = [0, 1] * 32
    w = F(1.25)
    queries = [[(2, M, w), (0, S, w)], [(0, S, w), (2, N, F(0))]]
    ref, lref, _ = check(docs, 2, 0, [at_limit], queries, 5, batch=batch)
    assert lref.lists == [[(0, 9), (1, 1), (2, 1)]] and ref.match_counts == [3, 1]
    r = run(pseg_of(docs, 2), 0, [len(d) for d in docs], [at_limit + [0]], queries, 5, batch=batch)
    assert r.error is not None and LONG_ERROR in r.error and r.untouched() and r.lists_untouched(), r.error
    check(docs, 2, 0, [at_limit], queries, 5, batch=batch)   # the workspace takes the sound batch afterwards


# ---- 7
def check_tile_edges(n):
    """n probes, n list entries and n or 2 n + 1 places: the phrase [0, 1] occurs once in each of n documents; every capacity exactly the need, and
    each in turn one less (an error at the sync, the need in the counts, everything left alone)"""
    batch = api.DeviceBatch(predictor())
    docs = [[0, 1] + [2] * (d % 3) for d in range(n)] + [[1], [2]]
    dl = [len(d) for d in docs]
    seg = pseg_of(docs, 3, 0)
    w = F(1.25)
    queries = [[(3, M, w), (2, S, F(0.5))], [(1, M, w), (3, N, F(0))]]   # (the second: the one document of term 1 outside the list)
    lref = clauseref.ListsRef(docs, 3, 0, [[0, 1]])
    ref = clauseref.ClauseRef(docs, 3, 0, lref.lists, queries, 7)
    assert lref.counts == [n, n, 0] and ref.counts[0] == 2 * n + 1 and ref.match_counts == [n, 1]
    r = run(seg, 0, dl, [[0, 1]], queries, 7, cap_probes=n, cap_lists=n, cap_places=2 * n + 1, batch=batch)
    lists_same_as(r, lref)
    same_as(r, ref)
    r = run(seg, 0, dl, [[0, 1]], queries, 7, cap_probes=n, cap_lists=n - 1, cap_places=2 * n + 1, batch=batch)
    assert r.error is not None and LISTS_ERROR in r.error and int(r.lcounts[1]) == n and int(r.lcounts[0]) == n, r.error
    assert r.untouched() and r.lists_untouched()
    r = run(seg, 0, dl, [[0, 1]], queries, 7, cap_probes=n - 1, cap_lists=n, cap_places=2 * n + 1, batch=batch)
    assert r.error is not None and PROBES_ERROR in r.error and int(r.lcounts[0]) == n and r.untouched() and r.lists_untouched(), r.error
    r = run(seg, 0, dl, [[0, 1]], queries, 7, cap_places=2 * n, batch=batch)
    assert r.error is not None and CAND_ERROR in r.error and int(r.counts[0]) == 2 * n + 1 and r.untouched(), r.error
    lists_same_as(searchless(r), lref)   # (the lists call before it was sound)
    # n places exactly: one MUST slot naming the list
    only = [[(3, M, w)]]
    oref = clauseref.ClauseRef(docs, 3, 0, lref.lists, only, 7)
    assert oref.counts == [n, n, 0]
    same_as(run(seg, 0, dl, [[0, 1]], only, 7, cap_probes=n, cap_lists=n, cap_places=n, batch=batch), oref)
    r = run(seg, 0, dl, [[0, 1]], only, 7, cap_probes=n, cap_lists=n, cap_places=n - 1, batch=batch)
    assert r.error is not None and CAND_ERROR in r.error and int(r.counts[0]) == n and r.untouched(), r.error
    same_as(run(seg, 0, dl, [[0, 1]], queries, 7, batch=batch), ref)


def searchless(r):
    out = Result()
    out.error = None
    for n in LISTS + ("lcounts",):
        setattr(out, n, getattr(r, n))
    return out


# ---- 8
def check_high_documents(name):
    batch = api.DeviceBatch(predictor())
    docs = phrasesuite.random_docs(7, n_docs=37)
    doc_base = postingssuite.high_base(name, len(docs))
    docs[-1] = [0, 1, 0, 2, 2]
    rng = random.Random(8)
    queries = random_queries(rng, 3, PHRASES, 17) + [[(3, M, F(1)), (2, S, F(2))], [(3, S, F(1)), (5, S, F(1))]]
    for k in (1, 64):
        ref, lref, _ = check(docs, 3, doc_base, PHRASES, queries, k, batch=batch)
    last = doc_base + len(docs) - 1
    hits = {d for h in ref.hits for d, _ in h}
    assert last >= 1 << 31 and last in hits and last in lref.docs and any(d >= 1 << 31 for d in lref.docs)
    assert (doc_base < 1 << 31) == (name == "2^31-3") and (last == 0xFFFFFFFF) == (name == "2^32-n")
    if name == "2^31-3":
        assert any(d < 1 << 31 for d in hits) and any(d < 1 << 31 for d in lref.docs)


# ---- 9, 13
CLAUSE_TEXTS = ["+東京特許許可局 猫", "だろう -東京特許許可局", "", "+", "+まぁ -だろう 猫", "-だ", "+猫 +１２３４５６円", "まぁ 東京特許許可局 火星猫は", "+だろう +まぁ",
                "+まぁ +東京特許許可局"]


def check_tokenizer():
    """index_batches(positions=True) searched = index_batch searched = the definition over the encoded ids; Postings.clause_search with the
    default weights and boolean_search(phrases=True); boolean_search() without the keyword is boolean_search's old result"""
    tok, texts = searchsuite.fixture_tokenizer()
    toff, ids = tok.encode_batch(texts)
    docs = [ids[int(toff[i]):int(toff[i + 1])].tolist() for i in range(len(texts))]
    parsed = []
    for text in CLAUSE_TEXTS:
        q = []
        for clause in text.split(" "):
            occur = M if clause[:1] == "+" else N if clause[:1] == "-" else S
            body = clause[1:] if occur != S else clause
            if body:
                q.append((tok.encode_batch([body])[1].tolist(), occur))
        parsed.append(q)
    assert sum(1 for q in parsed for t, _o in q if len(t) > 1) >= 6 and any(len(t) == 1 for q in parsed for t, _o in q)
    for doc_base in (0, 1000):
        whole = tok.index_batch(texts, doc_base, positions=True)
        parts = tok.index_batches([texts[:30], texts[30:31], texts[31:]], doc_base, positions=True)
        assert postingssuite.same_postings(whole, parts) and np.array_equal(whole.positions, parts.positions)
        df, n_terms = whole.df(), len(whole.term_offsets) - 1
        assert any(not 0 <= t < n_terms for q in parsed for ts, _o in q for t in ts)   # an unknown token: the phrase is unmatched
        queries = [[(ts, o, F(0) if o == N else phraseref.phrase_weight(len(texts), df, [t for t in ts if 0 <= t < n_terms])) for ts, o in q] for q in parsed]
        for k in (1, 10):
            ref = clauseref.of_clauses(docs, n_terms, doc_base, queries, k)
            assert ref.match_counts[2:4] == [0, 0] and ref.match_counts[5] == 0 and sum(1 for m in ref.match_counts if m) >= 4
            for post in (whole, parts):
                hits, mc = tok.boolean_search(post, CLAUSE_TEXTS, k, phrases=True)
                assert mc.tolist() == ref.match_counts and mc.dtype == np.uint64
                assert [[(d, bits(s)) for d, s in h] for h in hits] == [[(d, bits(s)) for d, s in h] for h in ref.hits]
                assert post.last_search_counts.tolist() == ref.counts
                hits2, _ = post.clause_search([[(ts, api.Occur(o)) for ts, o in q] for q in parsed], k)   # the default weights
                assert [[(d, bits(s)) for d, s in h] for h in hits2] == [[(d, bits(s)) for d, s in h] for h in ref.hits]
        assert ref.vetoes["must"] >= 1 and ref.vetoes["must_not"] >= 1
        # without the keyword: every token a slot, as before -- boolref over the flattened clauses, and other hits than the phrases give
        flat = [[(t, o, F(0) if o == N or not 0 <= t < n_terms else idf_of(len(texts), int(df[t]))) for ts, o in q for t in ts] for q in parsed]
        old = boolref.BoolRef(whole.term_offsets, whole.docs, whole.tfs, doc_base, [len(d) for d in docs], flat, 10)
        hits, mc = tok.boolean_search(whole, CLAUSE_TEXTS, 10)
        assert mc.tolist() == old.match_counts and [[(d, bits(s)) for d, s in h] for h in hits] == [[(d, bits(s)) for d, s in h] for h in old.hits]
        assert whole.last_search_counts.tolist() == old.counts and old.match_counts != ref.match_counts
        plain = tok.index_batch(texts, doc_base)
        hits3, mc3 = tok.boolean_search(plain, CLAUSE_TEXTS, 10)
        assert mc3.tolist() == mc.tolist() and [[(d, bits(s)) for d, s in h] for h in hits3] == [[(d, bits(s)) for d, s in h] for h in hits]
        _expect(lambda: tok.boolean_search(plain, CLAUSE_TEXTS, 3, phrases=True), "made without positions")


def check_host_call(seed=5):
    """vpt_postings_phrase_lists and vpt_postings_clause_search through ctypes and Postings.clause_search: host arrays in and out"""
    rng = random.Random(seed)
    pred = predictor()
    docs = phrasesuite.random_docs(seed, n_docs=50)
    post = pseg_of(docs, 3, 100).postings()
    dl = np.array([len(d) for d in docs], np.uint32)
    lref = clauseref.ListsRef(docs, 3, 100, PHRASES)
    poff = np.array(lref_offsets(PHRASES), np.uint64)
    pterms = np.array([t for ph in PHRASES for t in ph], np.int32)
    for cap in (lref.counts[1], lref.bound):
        loff, ld, lt, cnt = np.zeros(len(PHRASES) + 1, np.uint64), np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32), np.zeros(3, np.uint64)
        st = _lib.load().vpt_postings_phrase_lists(pred.handle, post.term_offsets.ctypes.data, post.docs.ctypes.data, post.tfs.ctypes.data,
                                                   post.first.ctypes.data, post.positions.ctypes.data, 3, 100, len(docs), poff.ctypes.data,
                                                   pterms.ctypes.data, len(PHRASES), loff.ctypes.data, ld.ctypes.data, lt.ctypes.data, cap, cnt.ctypes.data)
        assert st == _lib.VPT_OK, _lib.last_error()
        n = lref.counts[1]
        assert cnt.tolist() == lref.counts and loff.tolist() == lref.offsets and ld[:n].tolist() == lref.docs and lt[:n].tolist() == lref.tfs
    st = _lib.load().vpt_postings_phrase_lists(pred.handle, post.term_offsets.ctypes.data, post.docs.ctypes.data, post.tfs.ctypes.data,
                                               post.first.ctypes.data, post.positions.ctypes.data, 3, 100, len(docs), poff.ctypes.data, pterms.ctypes.data,
                                               len(PHRASES), loff.ctypes.data, ld.ctypes.data, lt.ctypes.data, n - 1, cnt.ctypes.data)
    assert st == _lib.VPT_INVALID_ARGUMENT and LISTS_ERROR in _lib.last_error() and int(cnt[1]) == n
    shapes = [[(rng.choice(PHRASES + [[0], [1], [2], [5], [-1]]), rng.choice([S, S, M, N])) for _ in range(rng.randint(1, 4))] for _ in range(14)]
    shapes += [[], [([0, 1], M), ([], S)], [([], M), ([0], S)], [([0, 1], M), ([0, 1], N)], [([0, 1], M), ([2, 2], M), ([1], S)]]
    queries = [[(ts, o, F(0.25 + j)) for j, (ts, o) in enumerate(q)] for q in shapes]
    for k in (1, 5, 60):
        ref = clauseref.of_clauses(docs, 3, 100, queries, k, None, dl, 0.9, 0.4)
        hits, mc = post.clause_search(queries, k, dl, 100, 0.9, 0.4, predictor=pred)
        assert [[(d, bits(s)) for d, s in h] for h in hits] == [[(d, bits(s)) for d, s in h] for h in ref.hits]
        assert all(type(s) is np.float32 for h in hits for _, s in h) and mc.tolist() == ref.match_counts and post.last_search_counts.tolist() == ref.counts
    assert ref.vetoes["must"] and ref.vetoes["must_not"] and sum(1 for m in ref.match_counts if m) > 3 and ref.counts[2] >= 2
    _expect(lambda: post.clause_search(queries, 4, dl, 100), "clause_search: no predictor")
    _expect(lambda: post.clause_search([[([1],)]], 4, dl, 100, predictor=pred), "a clause is \\(terms, occur\\) or \\(terms, occur, weight\\)")
    _expect(lambda: post.clause_search([[([1], 3)]], 4, dl, 100, predictor=pred), boolsuite.OCCUR_ERROR)
    _expect(lambda: post.clause_search([[([0] * 65, M)]], 4, dl, 100, predictor=pred), LONG_ERROR)
    assert post.clause_search([], 4, dl, 100, predictor=pred)[0] == []


def lref_offsets(phrases):
    out = [0]
    for ph in phrases:
        out.append(out[-1] + len(ph))
    return out


# ---- 10
def check_chained_errors():
    """lists, then the clause search on one stream with no sync between them: an error raised by the lists call leaves the clause search's
    outputs as they were pre-filled; with the lists call synced first, the same clause search over the same lists is sound"""
    batch = api.DeviceBatch(predictor())
    docs = phrasesuite.random_docs(7)
    dl = [len(d) for d in docs]
    seg = pseg_of(docs, 3, 5)
    phrases = [[0, 1], [2, 2, 1], [1]]
    w = F(1.25)
    queries = [[(3, M, w), (2, S, w)], [(0, S, w), (4, N, F(0))], [(5, M, w)]]   # (the last: a query that no error of the lists call concerns)
    lref = clauseref.ListsRef(docs, 3, 5, phrases)
    ref = clauseref.ClauseRef(docs, 3, 5, lref.lists, queries, 4)
    need_l, need_p = lref.counts[1], lref.counts[0]
    cases = [({"cap_lists": need_l - 1}, LISTS_ERROR), ({"cap_probes": need_p - 1, "cap_lists": need_l}, PROBES_ERROR)]
    if devmem.EMULATED:   # a phrase CSR that descends is no declared capacity or limit error: on the emulator only
        cases.append(({"poff": [0, 2, 1, 6]}, QCSR_ERROR))
    for kw, message in cases:
        r = run(seg, 5, dl, phrases, queries, 4, cap_places=sum(dl), batch=batch, **kw)
        assert r.error is not None and message in r.error and r.untouched() and r.lists_untouched(), (kw, r.error)
        r = run(seg, 5, dl, phrases, queries, 4, batch=batch)   # the sound ones on the same workspace
        lists_same_as(r, lref)
        same_as(r, ref)
    r = run(seg, 5, dl, phrases, queries, 4, batch=batch, sync_between=True)
    lists_same_as(r, lref)
    same_as(r, ref)


# ---- 11
def check_errors():
    pred = predictor()
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    batch = api.DeviceBatch(pred)
    lnames = ("term", "docs", "tfs", "first", "ppos", "poff", "pterms", "loff", "ldocs", "ltfs", "counts")
    cnames = ("term", "docs", "tfs", "loff", "ldocs", "ltfs", "dl", "qoff", "qterms", "qweights", "qoccurs", "hd", "hs", "hc", "mc", "counts")
    A = {n: devmem.zeros(8, np.uint64) for n in set(lnames + cnames)}

    def lists(b=batch, n_terms=2, cap_post=2, cap_pos=2, doc_base=0, n_docs=2, n_ph=1, cap_slots=1, cap_probes=2, cap_lists=2, **null):
        p = {n: (0 if n in null else a.ptr) for n, a in A.items()}
        b.phrase_lists_postings(p["term"], p["docs"], p["tfs"], p["first"], p["ppos"], n_terms, cap_post, cap_pos, doc_base, n_docs, p["poff"], p["pterms"],
                                n_ph, cap_slots, cap_probes, p["loff"], p["ldocs"], p["ltfs"], cap_lists, p["counts"], devmem.stream())

    def clause(b=batch, n_terms=2, cap_post=2, n_lists=1, cap_lists=2, doc_base=0, n_docs=2, n_q=1, cap_slots=1, k1=1.2, bb=0.75, avgdl=1.0, k=2, cap_cand=2,
               **null):
        p = {n: (0 if n in null else a.ptr) for n, a in A.items()}
        b.clause_search_postings(p["term"], p["docs"], p["tfs"], n_terms, cap_post, p["loff"], p["ldocs"], p["ltfs"], n_lists, cap_lists, doc_base, n_docs,
                                 p["dl"], p["qoff"], p["qterms"], p["qweights"], p["qoccurs"], n_q, cap_slots, k1, bb, avgdl, k, cap_cand, p["hd"], p["hs"],
                                 p["hc"], p["mc"], p["counts"], devmem.stream())

    for n in lnames:
        _expect(lambda: lists(**{n: 1}), "NULL device pointer")
    for n in cnames:
        _expect(lambda: clause(**{n: 1}), "NULL device pointer")
    for v in (0, (1 << 24) + 1):
        _expect(lambda: lists(n_terms=v), "n_terms: must be between 1 and 2\\^24")
        _expect(lambda: clause(n_terms=v), "n_terms: must be between 1 and 2\\^24")
        _expect(lambda: lists(n_ph=v), "n_phrases: must be between 1 and 2\\^24")
        _expect(lambda: clause(n_q=v), "n_queries: must be between 1 and 2\\^24")
    _expect(lambda: lists(cap_slots=1 << 32), "fewer than 2\\^32 slots and probes")
    _expect(lambda: lists(cap_probes=1 << 32), "fewer than 2\\^32 slots and probes")
    _expect(lambda: lists(cap_lists=1 << 32), "capacity_lists: must be below 2\\^32")
    _expect(lambda: clause(cap_lists=1 << 32), "capacity_lists: must be below 2\\^32")
    _expect(lambda: clause(n_terms=1 << 24, n_lists=1), "n_terms \\+ n_lists must not exceed 2\\^24")
    _expect(lambda: clause(n_terms=5, n_lists=(1 << 24) - 4), "n_terms \\+ n_lists must not exceed 2\\^24")
    _expect(lambda: clause(k=0), "k: must be at least 1")
    _expect(lambda: clause(cap_slots=1 << 32), "fewer than 2\\^32 slots and candidates")
    _expect(lambda: clause(cap_cand=1 << 32), "fewer than 2\\^32 slots and candidates")
    for call in (lists, clause):
        _expect(lambda: call(doc_base=(1 << 32) - 1, n_docs=2), "doc_base \\+ n_documents must not exceed 2\\^32")
    _expect(lambda: clause(k1=-1.0), "k1: must be between 0 and 65536")
    _expect(lambda: clause(bb=1.5), "b: must be between 0 and 1")
    _expect(lambda: clause(avgdl=0.0), "avgdl: must be between 2\\^-32 and 2\\^32")
    wrong = phrasesuite._MismatchBatch(batch, other)
    _expect(lambda: lists(b=wrong), "batch: does not belong to this predictor")
    _expect(lambda: clause(b=wrong), "batch: does not belong to this predictor")
    batch.sync()
    lists()   # all-zero arrays: one empty phrase, one query without a slot
    clause()
    clause(n_lists=0, loff=1, ldocs=1, ltfs=1)   # no list: the three pointers are not looked at
    batch.sync()
    assert A["counts"].get(3).tolist() == [0, 0, 0] and int(A["mc"].get(1)[0]) == 0


# ---- 12
def check_determinism(seed=12):
    rng = random.Random(seed)
    T = tile()
    pred = predictor()
    one, two = api.DeviceBatch(pred), api.DeviceBatch(pred)
    docs = [[rng.randrange(3) for _ in range(rng.randint(0, 40))] for _ in range(200)]
    dl = [len(d) for d in docs]
    seg = pseg_of(docs, 3, 0)
    queries = random_queries(rng, 3, PHRASES, 23)
    a = run(seg, 0, dl, PHRASES, queries, 10, batch=one)
    b = run(seg, 0, dl, PHRASES, queries, 10, batch=one)
    run(pseg_of([[0, 1, 0]], 3), 0, [3], [[1, 0]], [[(3, M, F(1))]], 1, batch=two)   # (the second workspace's scratch holds something else)
    c = run(seg, 0, dl, PHRASES, queries, 10, batch=two)
    assert a.error is None and a.same_bytes(b) and a.same_bytes(c)
    lref = clauseref.ListsRef(docs, 3, 0, PHRASES)
    ref = clauseref.ClauseRef(docs, 3, 0, lref.lists, queries, 10)
    assert T < lref.counts[0] <= 3 * T + 1 and lref.counts[1] > 500 and ref.counts[0] > 1000   # (entries and places past a tile: check_tile_edges)
    lists_same_as(a, lref)
    same_as(a, ref)


def check_scratch_reuse(seed=17):
    """one workspace alternated with the other postings calls that lay out its postings scratch -- a phrase search, the lists and the clause
    search, an OR search, a boolean search, the lists and the clause search again: every result is, byte for byte, that of the same call on
    a workspace of its own"""
    pred = predictor()
    docs = phrasesuite.random_docs(seed, n_docs=60)
    dl = [len(d) for d in docs]
    seg = pseg_of(docs, 3, 0, extra=2)
    queries = random_queries(random.Random(seed), 3, PHRASES, 9)
    plain = [[(t % 3, o, w) for t, o, w in q] for q in queries]
    clause = lambda b: run(seg, 0, dl, PHRASES, queries, 7, batch=b)
    steps = [("phrase", lambda b: phrasesuite.run(seg, 0, dl, [[0, 1], [2]], [F(1.5), F(1)], 7, batch=b)), ("clause", clause),
             ("search", lambda b: searchsuite.run(seg, 0, dl, [[(t, w) for t, _o, w in q] for q in plain], 7, batch=b)),
             ("boolean", lambda b: boolsuite.run(seg, 0, dl, plain, 7, batch=b)), ("clause again", clause)]
    shared = api.DeviceBatch(pred)
    for name, step in steps:
        got, want = step(shared), step(api.DeviceBatch(pred))
        assert got.error is None and want.error is None, (name, got.error, want.error)
        assert got.same_bytes(want), name
    assert int(got.counts[1]) > 10


# ---- hostile inputs (the emulator only)
def hostile_cases():
    """name -> (offsets, docs, tfs of the derived segment, queries, the message, or None where the call has to succeed).  The segment: documents
    10 .. 14 of phrasesuite.HOSTILE_DOCS; the sound lists: [11, 13], [10, 12, 14]"""
    w = F(1.25)
    sound = ([0, 2, 5], [11, 13, 10, 12, 14], [1, 2, 1, 1, 3])
    queries = [[(4, M, w), (5, S, w)], [], [(0, S, w), (5, N, F(0.5))], [(5, M, w), (4, N, w)], [(4, S, w), (3, S, w)]]
    cases = {}

    def case(name, message, offsets=None, docs=None, tfs=None, q=queries, cap=None):
        cases[name] = (offsets or sound[0], docs or sound[1], tfs or sound[2], q, message, cap)
    case("descending_list_bounds", SEG_ERROR, offsets=[0, 4, 3])
    case("list_offsets_above_capacity_lists", SEG_ERROR, offsets=[0, 2, 6])
    case("huge_list_offsets", SEG_ERROR, offsets=[1 << 62, (1 << 64) - 1, (1 << 64) - 1])
    case("bisected_bounds_far_outside", SEG_ERROR, offsets=[0, (1 << 64) - 8, (1 << 64) - 1], q=[[(0, M, w), (4, S, w)]])
    case("capacity_lists_cuts_a_list_off", SEG_ERROR, cap=4)
    case("list_document_below_doc_base", SEG_ERROR, docs=[9, 13, 10, 12, 14])
    case("list_document_at_the_end", SEG_ERROR, docs=[11, 15, 10, 12, 14])
    case("list_document_far_outside", SEG_ERROR, docs=[11, 13, 10, 12, 0xFFFFFFFF])
    case("anchor_list_descends", SEG_ERROR, docs=[13, 11, 10, 12, 14])
    case("anchor_list_repeats", SEG_ERROR, docs=[11, 11, 10, 12, 14])
    case("anchor_list_tf_zero", SEG_ERROR, tfs=[1, 0, 1, 1, 3])
    case("bisected_list_tf_zero", SEG_ERROR, tfs=[1, 2, 1, 0, 3], q=[[(0, M, w), (5, S, w)]])   # (term 0 has document 12)
    case("bisected_list_descends_unreported", None, docs=[11, 13, 14, 12, 10], q=[[(0, M, w), (5, S, w)]])
    case("bisected_list_documents_outside_unreported", None, docs=[11, 13, 0, 5, 0xFFFFFFFF], q=[[(0, M, w), (5, N, w)]])
    return sound, queries, cases


N_HOSTILE = 14


def run_hostile():
    sound, queries, cases = hostile_cases()
    assert len(cases) == N_HOSTILE, len(cases)
    docs = phrasesuite.HOSTILE_DOCS
    dl = [len(d) for d in docs]
    seg = pseg_of(docs, 4, 10, extra=2)
    assert [sorted(set(10 + i for i, d in enumerate(docs) if 0 in d))] == [[10, 12]]
    batch = api.DeviceBatch(predictor())
    lists = [list(zip(sound[1][a:b], sound[2][a:b])) for a, b in zip(sound[0], sound[0][1:])]
    ref = clauseref.ClauseRef(docs, 4, 10, lists, queries, 3)
    ran = 0
    for name, (offsets, ldocs, ltfs, q, message, cap) in cases.items():
        r = run(seg, 10, dl, None, q, 3, lists=(offsets, ldocs, ltfs), cap_lists=cap, cap_places=16, batch=batch)
        if message is None:
            assert r.error is None and not r.untouched(), (name, r.error)
        else:
            assert r.error is not None and message in r.error, (name, r.error)
            assert r.untouched(), name
        same_as(run(seg, 10, dl, None, queries, 3, lists=sound, cap_places=16, batch=batch), ref)   # the sound ones on the same workspace
        ran += 1
    del batch
    return ran


def main(argv):
    assert argv == ["--emu-hostile"], "usage: python -m tests.clausesuite --emu-hostile"
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
