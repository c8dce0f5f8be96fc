"""The checks of the sloppy phrase search and the sloppy phrase lists (vpt_postings_sloppy_phrase_search_device,
vpt_postings_sloppy_phrase_lists_device, the three host calls, Postings.phrase_search(slop=), clause_search(slop=),
VaporettoTokenizer.phrase_search / boolean_search(slop=); phrase_probe_kernel<true> of kernels_postings_phrase.hip) against the definition of
tests/sloppyref.py, run on the CPU emulator by tests/test_postings_sloppy_emu.py and on the MI355X by tests/test_postings_sloppy_gpu.py; every
comparison of documents, counts, frequencies and score BITS is exact equality with sloppyref.

The device calls are made by tests/phrasesuite.py's and tests/clausesuite.py's runners -- guarded arrays of exactly the stated sizes, SENTINEL
outputs -- through a workspace that adds the slops (SlopBatch); the slops array is guarded in the same way.

    python -m tests.sloppysuite --emu-hostile     the hostile inputs on the emulator, in a child process (hipemu checks its red zones when the
                                                  workspace goes)"""
import random
import sys

import numpy as np

from tests import clauseref, clausesuite, devmem, phrasesuite, postingssuite, searchsuite, sloppyref, vocabsuite
from vaporetto_amd import _lib, api

G = postingssuite.G
SENTINEL = postingssuite.SENTINEL
SLOP_ERROR = "query: a slop above 31"
PROBES_ERROR = phrasesuite.PROBES_ERROR
predictor = postingssuite.predictor
tile = postingssuite.tile
pseg_of = phrasesuite.pseg_of
same_as = phrasesuite.same_as
_expect = postingssuite._expect
bits = sloppyref.bits
F = np.float32
S, M, N = clauseref.SHOULD, clauseref.MUST, clauseref.MUST_NOT
A, B, C, X = 0, 1, 2, 3


class SlopBatch:
    """a workspace whose phrase search and phrase lists calls are the sloppy ones: slops a list (one per query, uploaded with guard words),
    or None for the NULL pointer"""

    def __init__(self, batch, slops):
        self.batch = batch
        self.slops = None if slops is None else G(np.asarray(list(slops) if len(slops) else [0], np.uint32))

    def _ptr(self):
        return 0 if self.slops is None else self.slops.ptr

    def phrase_search_postings(self, *a):
        self.batch.phrase_search_postings(*a, slops=self._ptr())

    def phrase_lists_postings(self, *a):
        self.batch.phrase_lists_postings(*a, slops=self._ptr())

    def clause_search_postings(self, *a):
        self.batch.clause_search_postings(*a)

    def sync(self):
        self.batch.sync()

    def check(self):
        if self.slops is not None:
            assert self.slops.guards_intact() and self.slops.get().tobytes() == self.slops.sent.tobytes(), "the slops were written"


def run(seg, doc_base, dl, phrases, weights, slops, k, batch=None, **kw):
    """vpt_postings_sloppy_phrase_search_device by phrasesuite.run; slops None: the NULL pointer"""
    sb = SlopBatch(batch or api.DeviceBatch(predictor()), slops)
    r = phrasesuite.run(seg, doc_base, dl, phrases, weights, k, batch=sb, **kw)
    sb.check()
    return r


def run_lists(seg, doc_base, dl, phrases, slops, queries=None, k=1, batch=None, **kw):
    """vpt_postings_sloppy_phrase_lists_device (and, with queries of slots, the clause search behind it with no sync) by clausesuite.run"""
    sb = SlopBatch(batch or api.DeviceBatch(predictor()), slops)
    r = clausesuite.run(seg, doc_base, dl, phrases, queries or [], k, batch=sb, search=queries is not None, **kw)
    sb.check()
    return r


def ref_of(docs, n_terms, doc_base, phrases, weights, slops, k, **kw):
    return sloppyref.SloppyRef(docs, n_terms, doc_base, phrases, weights, slops, k, **kw)


def check(docs, n_terms, doc_base, phrases, slops, k, positions=None, batch=None, extra=0, weights=None):
    weights = phrasesuite.weights_of(docs, n_terms, phrases) if weights is None else weights
    seg = pseg_of(docs, n_terms, doc_base, positions, extra)
    ref = ref_of(docs, n_terms, doc_base, phrases, weights, slops, k, positions=positions)
    same_as(run(seg, doc_base, [len(d) for d in docs], phrases, weights, slops, k, batch=batch), ref)
    return ref


def both_forms_agree(docs, n_terms, phrases, slops, positions=None):
    """the literal definition and the enumeration of choices, on the documents of at most 8 tokens"""
    positions = sloppyref.default_positions(docs) if positions is None else positions
    n = 0
    for ids, pos in zip(docs, positions):
        if len(ids) > 8:
            continue
        for ph in phrases:
            if len(ph) > 4 or any(not 0 <= t < n_terms for t in ph):
                continue
            for slop in slops:
                assert sloppyref.occurrences(ids, pos, ph, n_terms, slop) == sloppyref.occurrences_by_tuples(ids, pos, ph, n_terms, slop), (ids, ph, slop)
                n += 1
    return n


def owned(ids, positions, phrase, n_terms, slop, anchor):
    """by the definition alone: how many occurrences each anchor position of the document owns -- an occurrence belongs to the first adjusted
    anchor position at or after it"""
    occ = sloppyref.occurrences(ids, positions, phrase, n_terms, slop)
    anchors = sorted(sloppyref.adjusted(ids, positions, phrase, n_terms)[anchor])
    count = {a: 0 for a in anchors}
    for s in occ:
        first = min(a for a in anchors if a >= s)
        assert first <= s + slop
        count[first] += 1
    return [count[a] for a in anchors]


def anchor_of(docs, n_terms, phrase):
    n = [sum(d.count(t) for d in docs) for t in range(n_terms)]
    return min(range(len(phrase)), key=lambda j: (n[phrase[j]], j))


# ---- 1
DOCUMENTED_DOCS = [[A, X, B, C], [A, B, X, C], [A, X, B, X, C], [B, A], [A]]
DOCUMENTED_PHRASES = [[A, B, C], [A, B], [A, A]]


def check_documented_cases():
    """`A X B C` and `A B X C` match "A B C" at slop 1, `A X B X C` does not; `B A` matches "A B" at slop 2 and not at 1 (the cases of
    tantivy's set_slop documentation); "A A" at slop 1 matches a single A.  At slops 0, 1, 2, with the pf the definition gives."""
    docs, phrases = DOCUMENTED_DOCS, DOCUMENTED_PHRASES
    assert both_forms_agree(docs, 4, phrases, (0, 1, 2, 3)) == len(docs) * len(phrases) * 4
    want = {0: [{}, {1: 1}, {}], 1: [{0: 1, 1: 1}, {0: 1, 1: 1, 2: 1}, {0: 1, 1: 1, 2: 1, 3: 1, 4: 1}],
            2: [{0: 1, 1: 1, 2: 1}, {0: 1, 1: 1, 2: 1, 3: 1}, {0: 1, 1: 1, 2: 1, 3: 1, 4: 1}]}
    batch = api.DeviceBatch(predictor())
    for slop in (0, 1, 2):
        ref = check(docs, 4, 0, phrases, [slop] * 3, 5, batch=batch)
        assert ref.pf == want[slop], (slop, ref.pf)
    ref = check(docs, 4, 0, phrases * 3, [0] * 3 + [1] * 3 + [2] * 3, 5, batch=batch)   # the nine in one batch
    assert ref.pf == want[0] + want[1] + want[2]
    # a pf above 1: two places of "A B" apart by one token each
    ref = check([[A, X, B, A, B, X, X, A, X, B]], 4, 0, [[A, B]], [1], 1, batch=batch)
    assert ref.pf == [{0: 3}]


# ---- 2
def random_phrases(seed=8):
    rng = random.Random(seed)
    return [[rng.randrange(3) for _ in range(rng.randint(1, 5))] for _ in range(20)] + [[0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2], [2, 2, 2, 2, 2, 2, 2, 2]]


def check_slop_zero(seed=7):
    """every slop 0, and the NULL pointer: the exact calls' outputs and counts byte for byte, search and lists, over phrasesuite's random
    segment"""
    docs = phrasesuite.random_docs(seed)
    phrases = random_phrases(seed + 1)
    weights = phrasesuite.weights_of(docs, 3, phrases)
    dl = [len(d) for d in docs]
    batch = api.DeviceBatch(predictor())
    for doc_base in (0, 1000):
        seg = pseg_of(docs, 3, doc_base, extra=3)
        for k in (1, 3, 50):
            exact = phrasesuite.run(seg, doc_base, dl, phrases, weights, k, batch=batch)
            assert exact.error is None and int(exact.counts[1]) > 50
            for slops in ([0] * len(phrases), None):
                assert run(seg, doc_base, dl, phrases, weights, slops, k, batch=batch).same_bytes(exact), (k, slops)
        exact = clausesuite.run(seg, doc_base, dl, phrases, [], 1, batch=batch, search=False)
        assert exact.error is None and int(exact.lcounts[1]) > 50
        for slops in ([0] * len(phrases), None):
            r = run_lists(seg, doc_base, dl, phrases, slops, batch=batch)
            assert r.error is None and all(getattr(r, n).tobytes() == getattr(exact, n).tobytes() for n in clausesuite.LISTS + ("lcounts",))
    same_as(exact_ref_run(docs, phrases, weights, batch), ref_of(docs, 3, 0, phrases, weights, [0] * len(phrases), 3))   # (and the definition's)


def exact_ref_run(docs, phrases, weights, batch):
    return run(pseg_of(docs, 3, 0), 0, [len(d) for d in docs], phrases, weights, [0] * len(phrases), 3, batch=batch)


# ---- 3
def check_anchor_independence(seed=21):
    """phrasesuite's corpus: the same first documents with fillers that make each slot in turn the rarest; pf of the first documents is equal"""
    core = phrasesuite.random_docs(seed, 25, 3, 18)
    phrases = [[0, 1, 2], [2, 1, 0], [1, 1], [0, 2, 2, 1], [1, 0]]
    slops = [2, 1, 1, 3, 31]
    batch = api.DeviceBatch(predictor())
    seen, anchors = [], set()
    fillers = ([], [[0] * 30, [1] * 30 + [0] * 7], [[1] * 30, [2] * 30 + [1] * 7], [[2] * 30, [0] * 30 + [2] * 7], [[0] * 40 + [2] * 39 + [1] * 38])
    for filler in fillers:
        docs = core + filler
        ref = check(docs, 3, 0, phrases, slops, 40, batch=batch)
        seen.append([{d: n for d, n in per.items() if d < len(core)} for per in ref.pf])
        anchors.add(anchor_of(docs, 3, phrases[0]))
    assert all(s == seen[0] for s in seen) and anchors == {0, 1, 2} and all(seen[0])
    assert max(n for per in seen[0] for n in per.values()) > 2
    exact = phrasesuite.phraseref.PhraseRef(core, 3, 0, phrases, [F(1)] * 5, 40)
    assert all(len(s) > len(e) for s, e in zip(seen[0], exact.pf))   # (the slop widens every phrase's matches here)


# ---- 4
def check_one_lane_per_occurrence():
    """anchor positions closer to each other than the slop: a count that double-counts shared windows, or misses windows behind the previous
    anchor position, differs from the definition.  Asserted of the input: some place owns more than 1 occurrence, some owns 32."""
    batch = api.DeviceBatch(predictor())
    most = []
    for make_rare in (A, B):
        filler = [[B if make_rare == A else A] * 250]
        # `A A A A B` with "A B" at slop 3
        docs = [[A, A, A, A, B]] + filler
        assert anchor_of(docs, 2, [A, B]) == (0 if make_rare == A else 1)
        ref = check(docs, 2, 0, [[A, B]], [3], 2, batch=batch)
        assert ref.pf[0][0] == 4
        most.append(max(owned(docs[0], range(5), [A, B], 2, 3, anchor_of(docs, 2, [A, B]))))
        # `A B` x 100 with "A B" at slops 1 and 31, and "B A"
        docs = [[A, B] * 100] + filler
        ref = check(docs, 2, 0, [[A, B], [A, B], [B, A], [B, A], [A, B]], [1, 31, 1, 31, 0], 2, batch=batch)
        assert [per.get(0) for per in ref.pf] == [100, 100, 99, 100, 100], ref.pf   # ("B A": 99 exact places, and s = -1 at slop 31)
        most.append(max(owned(docs[0], range(200), [B, A], 2, 31, anchor_of(docs, 2, [B, A]))))
    assert most[0] == 1 and most[2] == 4, most
    # one A behind forty Bs, "B A" at slop 31: the 32 occurrences 8 .. 39 belong to the one anchor place; at slop 7: 8 of them
    docs = [[B] * 40 + [A], [B, X, X, A] * 3]
    ref = check(docs, 4, 0, [[B, A], [B, A], [A, B]], [31, 7, 31], 2, batch=batch)
    assert anchor_of(docs, 4, [B, A]) == 1 and owned(docs[0], range(41), [B, A], 4, 31, 1) == [32] and owned(docs[0], range(41), [B, A], 4, 7, 1) == [8]
    assert ref.pf == [{0: 32, 1: 5}, {0: 8, 1: 5}, {0: 30, 1: 3}], ref.pf   # ("A B": A at 40 needs s >= 9, a B at s + 1 needs s <= 38)
    # anchor positions 1, 2 and 40 apart under slop 31, the other slot dense: every s is counted once
    ids = [B] * 120
    for p in (3, 4, 6, 46, 47, 90):
        ids[p] = A
    docs = [ids, [B] * 300]
    ref = check(docs, 2, 0, [[A, B], [B, A]], [31, 31], 2, batch=batch)
    own = owned(ids, range(120), [A, B], 2, 31, 0)
    assert sum(own) == ref.pf[0][0] and own == [4, 1, 1, 31, 1, 31], own   # (s = a - 1 is nobody's adjusted position: an A stands there)


# ---- 5
def check_signs_and_the_top_of_the_range():
    batch = api.DeviceBatch(predictor())
    # a transposition at positions 0 and 1: s = -1
    docs = [[B, A], [B, A, A], [X, B, A]]
    ref = check(docs, 4, 0, [[A, B], [A, B], [A, A, B]], [2, 1, 3], 3, batch=batch)
    assert ref.pf[0] == {0: 1, 1: 1, 2: 1} and ref.pf[1] == {} and ref.pf[2][0] == 1
    assert sloppyref.occurrences(docs[0], [0, 1], [A, B], 4, 2) == [-1] and sloppyref.occurrences(docs[0], [0, 1], [A, A, B], 4, 3) == [-2]
    assert both_forms_agree(docs, 4, [[A, B], [A, A, B]], (1, 2, 3)) == 18
    # 64 slots, slop 31, the caller's token_positions up to 2^32 - 1: the document's last token at 2^32 - 1 - t
    top = (1 << 32) - 1
    phrase = list(range(64))
    rng = random.Random(5)
    docs, positions = [], []
    for t, spare in ((0, 31), (1, 32), (2, 0), (3, 17)):   # spare: the gaps between the 64 tokens add up to it
        gaps = [0] * 63
        for _ in range(spare):
            gaps[rng.randrange(63)] += 1
        pos = [top - t]
        for g in reversed(gaps):
            pos.append(pos[-1] - 1 - g)
        docs.append(list(phrase))
        positions.append(pos[::-1])
    docs.append([63, 63, 63, 0])   # slot 0 at 2^32 - 1 and nothing behind it: lo + j lies above every position
    positions.append([top - 30, top - 20, top - 10, top])
    wrap = [0] + [63] * 40   # its anchor is slot 0 (term 0 is the rarer): in the last document a = 2^32 - 1 and lo + j > 2^32 - 1 from j = 32 on
    ref = check(docs, 64, 0, [phrase, phrase, phrase[:2] + phrase[62:], wrap, [0, 63]], [31, 30, 31, 31, 31], 5, positions=positions, batch=batch)
    assert anchor_of(docs, 64, wrap) == 0 and ref.pf[3] == {} and 4 in ref.pf[4]
    assert sorted(ref.pf[0]) == [0, 2, 3] and sorted(ref.pf[1]) == [2, 3] and max(p for d in positions for p in d) == top
    assert all(a < b for d in positions for a, b in zip(d, d[1:]))


# ---- 6
def check_limits():
    assert api.DeviceBatch.postings_sloppy_phrase_limits() == (64, 31) and api.DeviceBatch.postings_phrase_limit() == 64
    assert _lib.load().vpt_postings_sloppy_phrase_limits(None, None) == _lib.VPT_INVALID_ARGUMENT
    batch = api.DeviceBatch(predictor())
    docs = phrasesuite.random_docs(11, 30, 3, 20) + [[A]]
    phrases = [[0, 1], [1, 2, 0], [2, 0], [0, 1, 1]]
    weights = phrasesuite.weights_of(docs, 3, phrases)
    seg, dl = pseg_of(docs, 3, 7), [len(d) for d in docs]
    for slops in ([0, 1, 31, 32], [32, 0, 0, 0], [0, 0, 0, 0xFFFFFFFF]):
        r = run(seg, 7, dl, phrases, weights, slops, 4, batch=batch)
        assert r.error is not None and SLOP_ERROR in r.error and r.untouched(), r.error
        r = run_lists(seg, 7, dl, phrases, slops, batch=batch)
        assert r.error is not None and SLOP_ERROR in r.error and r.lists_untouched(), r.error
    ref = ref_of(docs, 3, 7, phrases[:3], weights[:3], [0, 1, 31], 4)
    same_as(run(seg, 7, dl, phrases[:3], weights[:3], [0, 1, 31], 4, batch=batch), ref)   # the workspace is sound again
    assert len(ref.pf[2]) > len(ref.pf[0]) > 0
    # 64 slots with slop 31 over ordinary positions: tokens dropped in between, one too many in the last document
    phrase = list(range(64))   # (distinct terms: no other token can serve a slot)
    spread = lambda n: [x for j, t in enumerate(phrase) for x in ([t] + ([64] if j in range(5, 5 + n) else []))]
    docs = [spread(0), spread(31), spread(32), [64] + spread(3) + [64] + spread(3)]
    ref = check(docs, 65, 0, [phrase, phrase], [31, 2], 4, batch=batch)
    assert ref.pf == [{0: 1, 1: 1, 3: 2}, {0: 1}], ref.pf
    # a repeated term served by one token
    ref = check([[A], [X, A, X], [B]], 4, 0, [[A, A], [A, A], [A, A, A]], [1, 0, 2], 3, batch=batch)
    assert ref.pf == [{0: 1, 1: 1}, {}, {0: 1, 1: 1}]


# ---- 7
def edge_docs(n):
    """n tokens of term 1, the anchor of [0, 1] and [1, 2] (term 0 and term 2 have more): documents of one to three of them, and a dense
    document of 24 of them, closer to each other than the slop, across place 256 (a workgroup's last lane) and across place T (the sort
    tile), where n reaches that far"""
    rng = random.Random(n)
    T = tile()
    dense_at = [a for a in (256 - 12, T - 12) if a + 24 <= n]
    docs, done = [], 0
    while done < n:
        if dense_at and done == dense_at[0]:
            dense_at.pop(0)
            docs.append([0, 2] + [1, 1, 0, 2, 1] * 8 + [0, 2])
            done += 24
            continue
        limit = min([n - done] + [a - done for a in dense_at])
        m = min(limit, rng.choice([1, 1, 2, 3]))
        d = []
        for _ in range(m):
            d += [0] * rng.randint(1, 2) + [2] * rng.randint(0, 1) + [1] + [2] + [0] * rng.randint(0, 1)
        docs.append(d)
        done += m
    assert sum(d.count(1) for d in docs) == n and all(sum(d.count(t) for d in docs) > n for t in (0, 2))
    return docs


def check_probes(n):
    docs = edge_docs(n)
    T = tile()
    batch = api.DeviceBatch(predictor())
    k = 7
    ref = check(docs, 3, 0, [[0, 1]], [2], k, batch=batch)
    assert ref.counts[0] == n and ref.counts[1] > n // 4
    ref = check(docs, 3, 0, [[1, 2], [], [0, 1, 2]], [3, 0, 2], 5, batch=batch)
    assert ref.counts[0] == 2 * n
    # the dense posting's places and what they own, by the definition
    first = 0
    for d in docs:
        if d.count(1) == 24:
            assert first in (256 - 12, T - 12)
            own = owned(d, range(len(d)), [0, 1], 3, 2, 1)
            assert len(own) == 24 and sum(own) == ref_of([d], 3, 0, [[0, 1]], [F(1)], [2], 1).pf[0][0]
        first += d.count(1)
    assert n < 256 + 12 or any(d.count(1) == 24 for d in docs)


# ---- 8
def check_topk():
    same = [1, 3, 2, 2, 0]
    docs = [[3, 3], same, [0], same, same, [1, 2, 3, 1, 3, 2], same, same, [2]]
    batch = api.DeviceBatch(predictor())
    bases = (0, 7) + tuple(postingssuite.high_base(name, len(docs)) for name in postingssuite.HIGH_BASES)
    for doc_base in bases:
        for k in (2, 3, 5, 9):   # 2, 3: inside the group of five equal scores; 9: above the matches
            ref = check(docs, 4, doc_base, [[1, 2], [2, 2, 0], [3, 3, 3]], [2, 2, 2], k, batch=batch)
            group = [doc_base + d for d in (1, 3, 4, 6, 7)]
            assert [d for d, _, _ in ref.hits[1]] == group[:k] and len({bits(s) for _, s, _ in ref.hits[1]}) == 1
            assert ref.match_counts == [6, 5, 7] and ref.hits[0][0][0] == doc_base + 5 and ref.hits[0][0][2] >= 2
    assert bases[-1] + len(docs) == 1 << 32 and bases[-2] < 1 << 31 < bases[-2] + len(docs)


def check_high_documents(name):
    docs = phrasesuite.random_docs(7)
    phrases = random_phrases()
    doc_base = postingssuite.high_base(name, len(docs))
    batch = api.DeviceBatch(predictor())
    for k in (1, 50):
        ref = check(docs, 3, doc_base, phrases, [2] * len(phrases), k, batch=batch, extra=3)
    last = doc_base + len(docs) - 1
    assert {doc_base, last} <= phrasesuite.hits_of(ref) and last >= 1 << 31


def check_capacity(seed=7):
    docs = phrasesuite.random_docs(seed)
    phrases, slops = [[0, 1], [2], [1, 1, 2], []], [2, 2, 2, 2]
    weights = phrasesuite.weights_of(docs, 3, phrases)
    seg, dl = pseg_of(docs, 3, 5), [len(d) for d in docs]
    ref = ref_of(docs, 3, 5, phrases, weights, slops, 3)
    need = ref.counts[0]
    assert need == phrasesuite.probes_of(seg, phrases) > 50
    batch = api.DeviceBatch(predictor())
    for cap in (need - 1, 0):
        r = run(seg, 5, dl, phrases, weights, slops, 3, cap_probes=cap, batch=batch)
        assert r.error is not None and PROBES_ERROR in r.error, r.error
        assert int(r.counts[0]) == need and r.untouched()
    same_as(run(seg, 5, dl, phrases, weights, slops, 3, cap_probes=need, batch=batch), ref)
    same_as(run(seg, 5, dl, phrases, weights, slops, 3, cap_probes=need + tile() + 1, batch=batch), ref)


def check_errors():
    """the errors at the call are the exact call's; the slops pointer may be NULL"""
    batch = api.DeviceBatch(predictor())
    names = ("term", "docs", "tfs", "first", "ppos", "dl", "qoff", "qterms", "qweights", "hd", "hs", "hf", "hc", "mc", "counts", "slops")
    Z = {n: devmem.zeros(8, np.uint64) for n in names}

    def call(n_terms=2, n_q=1, cap_slots=1, k=2, cap_probes=2, doc_base=0, avgdl=1.0, **null):
        p = {n: (0 if n in null else a.ptr) for n, a in Z.items()}
        batch.phrase_search_postings(p["term"], p["docs"], p["tfs"], p["first"], p["ppos"], n_terms, 2, 2, doc_base, 2, p["dl"], p["qoff"], p["qterms"],
                                     p["qweights"], n_q, cap_slots, 1.2, 0.75, avgdl, k, cap_probes, p["hd"], p["hs"], p["hf"], p["hc"], p["mc"],
                                     p["counts"], devmem.stream(), slops=p["slops"])

    def call_lists(n_phrases=1, cap_lists=2, **null):
        p = {n: (0 if n in null else a.ptr) for n, a in Z.items()}
        batch.phrase_lists_postings(p["term"], p["docs"], p["tfs"], p["first"], p["ppos"], 2, 2, 2, 0, 2, p["qoff"], p["qterms"], n_phrases, 1, 2,
                                    p["hd"], p["hs"], p["hf"], cap_lists, p["counts"], devmem.stream(), slops=p["slops"])

    for n in names:
        if n not in ("hf", "slops"):
            _expect(lambda: call(**{n: 1}), "NULL device pointer")
    for n in ("term", "docs", "tfs", "first", "ppos", "qoff", "qterms", "hd", "hs", "hf", "counts"):
        _expect(lambda: call_lists(**{n: 1}), "NULL device pointer")
    for v in (0, (1 << 24) + 1):
        _expect(lambda: call(n_terms=v), "n_terms: must be between 1 and 2\\^24")
        _expect(lambda: call(n_q=v), "n_queries: must be between 1 and 2\\^24")
        _expect(lambda: call_lists(n_phrases=v), "n_phrases: must be between 1 and 2\\^24")
    _expect(lambda: call(k=0), "k: must be at least 1")
    _expect(lambda: call(cap_slots=1 << 32), "fewer than 2\\^32 slots and probes")
    _expect(lambda: call(cap_probes=1 << 32), "fewer than 2\\^32 slots and probes")
    _expect(lambda: call(doc_base=(1 << 32) - 1), "doc_base \\+ n_documents must not exceed 2\\^32")
    _expect(lambda: call(avgdl=0.0), "avgdl: must be between 2\\^-32 and 2\\^32")
    _expect(lambda: call_lists(cap_lists=1 << 32), "capacity_lists: must be below 2\\^32")
    batch.sync()
    call(hf=1, slops=1)   # all-zero arrays: one query without a slot, the two optional pointers NULL
    call_lists(slops=1)
    call()
    batch.sync()
    assert Z["counts"].get(3).tolist() == [0, 0, 0]


def check_determinism(seed=12):
    rng = random.Random(seed)
    T = tile()
    docs = [[postingssuite.zipf(rng, 6) for _ in range(rng.randint(0, 30))] for _ in range(3 * T // 32)]
    phrases = [[rng.randrange(6) for _ in range(rng.randint(0, 4))] for _ in range(23)]
    slops = [rng.choice([0, 1, 2, 2, 8, 31]) for _ in phrases]
    weights = phrasesuite.weights_of(docs, 6, phrases)
    seg, dl = pseg_of(docs, 6), [len(d) for d in docs]
    pred = predictor()
    one, two = api.DeviceBatch(pred), api.DeviceBatch(pred)
    a = run(seg, 0, dl, phrases, weights, slops, 10, batch=one)
    b = run(seg, 0, dl, phrases, weights, slops, 10, batch=one)
    run(pseg_of([[1, 2, 1]], 4), 0, [3], [[1, 2]], [F(1)], [1], 1, batch=two)   # (the second workspace's scratch holds something else)
    c = run(seg, 0, dl, phrases, weights, slops, 10, batch=two)
    assert a.error is None and a.same_bytes(b) and a.same_bytes(c)
    ref = ref_of(docs, 6, 0, phrases, weights, slops, 10)
    assert T < ref.counts[0] <= 3 * T + 1, ref.counts
    same_as(a, ref)


# ---- 9
def run_hostile():
    """phrasesuite's hostile segments, query CSRs and weights under slop 31: an error at the sync with every output untouched; positions that
    descend inside a posting: no error is required, the call returns and no guard word is touched (phrasesuite.run asserts the guards)"""
    w, cases = phrasesuite.hostile_cases()
    docs, phrases = phrasesuite.HOSTILE_DOCS, phrasesuite.HOSTILE_PHRASES
    dl = [len(d) for d in docs]
    slops = [31, 31, 31, 31]
    sound = pseg_of(docs, 4, 10, extra=2)
    ref = ref_of(docs, 4, 10, phrases, w, slops, 3)
    batch = api.DeviceBatch(predictor())
    ran = 0
    for name, (change, ph, qoff, weights, message) in cases.items():
        seg = pseg_of(docs, 4, 10, extra=2)
        if change:
            change(seg)
        r = run(seg, 10, dl, ph, weights, slops, 3, cap_probes=16, qoff=qoff, batch=batch)
        assert r.error is not None and message in r.error, (name, r.error)
        assert r.untouched(), name
        same_as(run(sound, 10, dl, phrases, w, slops, 3, batch=batch), ref)   # the sound ones on the same workspace
        ran += 1
    for positions in ([[5, 1, 0], [3], [9, 2, 7, 1], [], [4, 0]], [[0xFFFFFFFF, 0xFFFFFFFE, 0], [0], [3, 2, 1, 0], [], [0, 0]],
                      [[7, 7, 7], [7], [7, 7, 7, 7], [], [7, 7]]):
        seg = pseg_of(docs, 4, 10, positions=positions, extra=2)
        for s in (slops, [0, 1, 2, 3]):
            r = run(seg, 10, dl, phrases, w, s, 3, batch=batch)
            assert r.error is None, r.error
            assert all(int(f) <= 32 * 4 for f in r.hf[r.hf != SENTINEL]) and all(int(m) <= len(docs) for m in r.mc)   # a bounded result
            r = run_lists(seg, 10, dl, phrases, s, batch=batch)
            assert r.error is None, r.error
        ran += 1
    same_as(run(sound, 10, dl, phrases, w, slops, 3, batch=batch), ref)
    del batch
    return ran


N_HOSTILE = phrasesuite.N_HOSTILE + 3


# ---- 10
def check_clause_identities(seed=7):
    batch = api.DeviceBatch(predictor())
    docs = phrasesuite.random_docs(seed)
    dl = [len(d) for d in docs]
    phrases = [ph for ph in clausesuite.PHRASES if all(0 <= t < 3 for t in ph)]
    slops = [(2, 1, 31, 5, 0, 3, 8, 2, 1)[i] for i in range(len(phrases))]
    weights = phrasesuite.weights_of(docs, 3, phrases)
    for doc_base in (0, 1000):
        seg = pseg_of(docs, 3, doc_base, extra=1)
        ref = ref_of(docs, 3, doc_base, phrases, weights, slops, 64)
        queries = [[(3 + i, S, w)] for i, w in enumerate(weights)]
        for k in (1, 3, 64):
            theirs = run(seg, doc_base, dl, phrases, weights, slops, k, batch=batch)
            mine = run_lists(seg, doc_base, dl, phrases, slops, queries, k, batch=batch)
            assert theirs.error is None and mine.error is None
            assert all(getattr(mine, n).tobytes() == getattr(theirs, n).tobytes() for n in clausesuite.OUTPUTS), k
            assert mine.lcounts.tolist() == theirs.counts.tolist()
        off, ldocs, ltfs = ref.lists()
        n = off[-1]
        assert mine.loff.tolist() == off and mine.ldocs[:n].tolist() == ldocs and mine.ltfs[:n].tolist() == ltfs and max(ltfs) > 2
        assert (mine.ldocs[n:] == SENTINEL).all()
        # a one-term phrase's sloppy list is the term's own list at any slop
        r = run_lists(seg, doc_base, dl, [[0], [1], [2]], [0, 7, 31], batch=batch)
        n = int(seg.term[3])
        assert r.error is None and r.loff.tolist() == seg.term.tolist() and r.ldocs[:n].tobytes() == seg.docs[:n].tobytes()
        assert r.ltfs[:n].tobytes() == seg.tfs[:n].tobytes()
    # mixed queries over terms and sloppy lists against clauseref with the lists of sloppyref
    rng = random.Random(seed)
    queries = clausesuite.random_queries(rng, 3, phrases, 17)
    lists = [sorted(per.items()) for per in ref_of(docs, 3, 0, phrases, weights, slops, 1).pf]
    cref = clauseref.ClauseRef(docs, 3, 0, lists, queries, 5)
    r = run_lists(pseg_of(docs, 3, 0), 0, dl, phrases, slops, queries, 5, batch=batch)
    clausesuite.same_as(r, cref)
    assert cref.counts[1] > 30


# ---- 11
def of_clauses(docs, n_terms, doc_base, queries, slop, k, dl=None):
    """clauseref.of_clauses with the lists of sloppyref at one slop"""
    phrases, slots, skipped = clauseref.slots_of(n_terms, queries)
    lists = [sorted(per.items()) for per in ref_of(docs, n_terms, doc_base, phrases, [F(0)] * len(phrases), [slop] * len(phrases), 1).pf]
    ref = clauseref.ClauseRef(docs, n_terms, doc_base, lists, slots, k, dl)
    ref.counts[2] += skipped
    return ref


def triples(hits):
    return [[(d, bits(s), f) for d, s, f in h] for h in hits]


def check_host_calls(seed=5):
    """the three host calls through Postings.phrase_search(slop=), the lists entry point and Postings.clause_search(slop=)"""
    docs = phrasesuite.random_docs(seed, 50, 4, 30)
    pred = predictor()
    post = pseg_of(docs, 4, 100).postings()
    dl = np.array([len(d) for d in docs], np.uint32)
    rng = random.Random(seed)
    phrases = [[rng.randrange(4) for _ in range(rng.randint(1, 4))] for _ in range(9)] + [[], [4, 2]]
    weights = [F(0.25 + j) for j in range(len(phrases))]
    per_phrase = [rng.choice([0, 1, 2, 5, 31]) for _ in phrases]
    for slop in (2, per_phrase, np.uint32(1), [0] * len(phrases)):
        slops = [int(slop)] * len(phrases) if not isinstance(slop, list) else slop
        for k in (1, 60):
            ref = ref_of(docs, 4, 100, phrases, weights, slops, k)
            hits, mc = post.phrase_search(phrases, k, dl, 100, weights=weights, predictor=pred, slop=slop)
            assert triples(hits) == triples(ref.hits) and mc.tolist() == ref.match_counts and post.last_search_counts.tolist() == ref.counts
    exact = post.phrase_search(phrases, 5, dl, 100, predictor=pred)
    for zero in (0, [0] * len(phrases)):
        again = post.phrase_search(phrases, 5, dl, 100, predictor=pred, slop=zero)
        assert triples(again[0]) == triples(exact[0]) and again[1].tolist() == exact[1].tolist()
    _expect(lambda: post.phrase_search(phrases, 5, dl, 100, predictor=pred, slop=32), SLOP_ERROR)
    _expect(lambda: post.phrase_search(phrases, 5, dl, 100, predictor=pred, slop=-1), SLOP_ERROR)
    _expect(lambda: post.phrase_search(phrases, 5, dl, 100, predictor=pred, slop=[1, 2]), "slop: an int or one per phrase")
    # the lists call over host arrays
    ref = ref_of(docs, 4, 100, phrases, weights, per_phrase, 1)
    off, ldocs, ltfs = ref.lists()
    qoff = np.array([0] + list(np.cumsum([len(p) for p in phrases])), np.uint64)
    terms = np.array([t for p in phrases for t in p] + [0], np.int32)
    cap = len(ldocs) + 3
    lo, ld, lt, cnt = np.zeros(len(phrases) + 1, np.uint64), np.full(cap, 9, np.uint32), np.full(cap, 9, np.uint32), np.zeros(3, np.uint64)
    sl = np.array(per_phrase, np.uint32)
    st = _lib.load().vpt_postings_sloppy_phrase_lists(pred.handle, post.term_offsets.ctypes.data, post.docs.ctypes.data, post.tfs.ctypes.data,
                                                      post.first.ctypes.data, post.positions.ctypes.data, 4, 100, len(docs), qoff.ctypes.data,
                                                      terms.ctypes.data, sl.ctypes.data, len(phrases), lo.ctypes.data, ld.ctypes.data, lt.ctypes.data, cap,
                                                      cnt.ctypes.data)
    assert st == _lib.VPT_OK, _lib.last_error()
    n = len(ldocs)
    assert lo.tolist() == off and ld[:n].tolist() == ldocs and lt[:n].tolist() == ltfs and (ld[n:] == 9).all() and cnt.tolist() == ref.counts
    # queries of clauses
    queries = [[([0, 1], M), ([2], S)], [([1, 2, 0], S), ([3, 3], S, F(2.5))], [([0], M), ([2, 1], N)], [([1, 4], S), ([0, 2], S)], []]
    dfs = post.df()
    full = [[(t, o, x[0] if x else (F(0) if o == N else sloppyref.phrase_weight(len(docs), dfs, [u for u in t if 0 <= u < 4]))) for t, o, *x in q]
            for q in queries]
    for slop in (0, 2, 31):
        ref = of_clauses(docs, 4, 100, full, slop, 6, dl.tolist())
        hits, mc = post.clause_search(queries, 6, dl, 100, predictor=pred, slop=slop)
        assert [[(d, bits(s)) for d, s in h] for h in hits] == [[(d, bits(s)) for d, s in h] for h in ref.hits], slop
        assert mc.tolist() == ref.match_counts and post.last_search_counts.tolist() == ref.counts
    _expect(lambda: post.clause_search(queries, 6, dl, 100, predictor=pred, slop=32), SLOP_ERROR)


def check_tokenizer():
    """VaporettoTokenizer.phrase_search(slop=1) and boolean_search(phrases=True, slop=2) on the fixture model against the definition over the
    encoded ids; a `~` in a clause stays a character of it"""
    tok, texts = searchsuite.fixture_tokenizer()
    toff, ids = tok.encode_batch(texts)
    docs = [ids[int(toff[i]):int(toff[i + 1])].tolist() for i in range(len(texts))]
    qtexts = phrasesuite.PHRASE_TEXTS + ["火星だ", "猫東京"]
    qoff, qids = tok.encode_batch(qtexts)
    phrases = [qids[int(qoff[i]):int(qoff[i + 1])].tolist() for i in range(len(qtexts))]
    post = tok.index_batch(texts, 1000, positions=True)
    n_terms = len(post.term_offsets) - 1
    df = post.df()
    weights = [sloppyref.phrase_weight(len(texts), df, [t for t in ph if 0 <= t < n_terms]) for ph in phrases]
    widened = 0
    for slop in (1, 3):
        ref = ref_of(docs, n_terms, 1000, phrases, weights, [slop] * len(phrases), 10)
        hits, mc = tok.phrase_search(post, qtexts, 10, slop=slop)
        assert mc.tolist() == ref.match_counts and triples(hits) == triples(ref.hits) and post.last_search_counts.tolist() == ref.counts
        exact = tok.phrase_search(post, qtexts, 10)[1]
        widened += sum(int(a) > int(b) for a, b in zip(mc, exact))
    assert widened >= 1, "no query text gains a match from the slop on this fixture"
    ctexts = clausesuite.CLAUSE_TEXTS + ["+火星だ~2"]
    hits2, mc2 = tok.boolean_search(post, ctexts, 5, phrases=True, slop=2)
    queries = []
    for text in ctexts:
        q = []
        for clause in text.split(" "):
            occur = M if clause[:1] == "+" else N if clause[:1] == "-" else S
            body = clause[1:] if occur != S else clause
            if body:
                o, t = tok.encode_batch([body])
                if len(t):
                    terms = t.tolist()
                    q.append((terms, occur, F(0) if occur == N else sloppyref.phrase_weight(len(texts), df, [u for u in terms if 0 <= u < n_terms])))
        queries.append(q)
    ref = of_clauses(docs, n_terms, 1000, queries, 2, 5)
    assert [[(d, bits(s)) for d, s in h] for h in hits2] == [[(d, bits(s)) for d, s in h] for h in ref.hits] and mc2.tolist() == ref.match_counts
    assert tok.encode_batch(["火星だ~2"])[1].tolist() != tok.encode_batch(["火星だ"])[1].tolist()   # the `~2` was tokenised with the clause
    _expect(lambda: tok.boolean_search(post, ctexts, 5, slop=2), "slop needs phrases=True")


def example_lines(docs, n_terms, doc_base, phrase, weight, slop, k):
    """the lines examples/token_stream.cpp --postings --phrase --slop prints for these hits"""
    ref = ref_of(docs, n_terms, doc_base, [phrase], [weight], [slop], k)
    return ["%d\t%08x\t%.9g\t%d" % (d, bits(s), float(s), f) for d, s, f in ref.hits[0]], ref


def main(argv):
    assert argv == ["--emu-hostile"], "usage: python -m tests.sloppysuite --emu-hostile"
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
