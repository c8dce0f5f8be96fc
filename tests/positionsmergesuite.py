"""The checks of the merge of positional segments (vpt_postings_merge_positional_device, vpt_postings_merge_positional;
kernels_postings_merge.hip) against the definitions of tests/positionsmergeref.py and tests/phraseref.py, run on the CPU emulator by
tests/test_postings_merge_positions_emu.py and on the MI355X by tests/test_postings_merge_positions_gpu.py; every comparison is exact equality
with the plain-Python definitions, never with the device's own one-pass call.

    python -m tests.positionsmergesuite --emu-hostile     the hostile segments on the emulator, in a child process (hipemu checks its red
                                                          zones when the workspace goes)

Every array handed to the call has exactly the size the call is told and guard words on both sides, checked after the sync with the inputs
unwritten; outputs are filled with SENTINEL first, so a write behind what the call had to write is seen.  T = vpt_postings_tile (4096); no
case has more than 3 T + 1 positions.  check_high_documents merges three contiguous positional segments at the two bases of
postingssuite.HIGH_BASES (documents on both sides of 2^31, the last document 0xFFFFFFFF) on both routes, a few hundred positions, swaps two of
them under the ordered route and runs a phrase search over the merged arrays."""
import random
import sys

import numpy as np

from tests import devmem, patterntagsuite, phraseref, phrasesuite, positionsmergeref, postingsmergesuite, postingssuite, vocabsuite
from vaporetto_amd import _lib, api

G = postingssuite.G
SENTINEL = postingssuite.SENTINEL
SMALL_ERROR = postingssuite.SMALL_ERROR
POS_SMALL_ERROR = "capacity_positions: smaller than the number of indexed tokens"
SEG_ERROR = postingsmergesuite.SEG_ERROR
OVERLAP_ERROR = postingsmergesuite.OVERLAP_ERROR
POSITIONS_ERROR = phrasesuite.POSITIONS_ERROR
predictor = postingssuite.predictor
tile = postingssuite.tile
csr = postingssuite.csr
_expect = postingssuite._expect
Ref = positionsmergeref.PositionsMergeRef
ROUTES = (True, False)   # ordered, general
ARRAYS = ("term", "docs", "tfs", "first", "ppos")
GARBAGE = 0x5A5A5A5A      # what the places behind a segment's positions hold


class PSeg:
    """a positional segment on the host: term [n_terms + 1], docs / tfs [cap], first [cap + 1], ppos [cap_pos]; SENTINEL behind the postings,
    GARBAGE behind the positions.  extra / extra_pos: places behind what it holds."""

    def __init__(self, term, docs, tfs, first, ppos, extra=0, extra_pos=0):
        self.term = np.asarray(term, np.uint64).copy()
        self.n_terms = len(self.term) - 1
        n, m = len(docs), len(ppos)
        self.cap, self.cap_pos = n + extra, m + extra_pos
        self.docs, self.tfs = np.full(max(self.cap, 1), SENTINEL, np.uint32), np.full(max(self.cap, 1), SENTINEL, np.uint32)
        self.first, self.ppos = np.full(self.cap + 1, SENTINEL, np.uint64), np.full(max(self.cap_pos, 1), GARBAGE, np.uint32)
        self.docs[:n], self.tfs[:n], self.first[:n + 1], self.ppos[:m] = docs, tfs, first, ppos

    def five(self):
        n = int(self.term[-1])
        return self.term, self.docs[:n], self.tfs[:n], self.first[:n + 1], self.ppos[:int(self.first[n])]

    def postings(self):
        term, docs, tfs, first, ppos = self.five()
        out = api.Postings(term, docs.copy(), tfs.copy(), first.copy(), None, 0)
        out.positions = ppos.copy()
        return out


def pseg_of(docs, n_terms, doc_base=0, positions=None, extra=0, extra_pos=0):
    """documents as lists of ids (and positions) -> the positional segment by the plain-Python definition"""
    return PSeg(*Ref.of_documents(docs, n_terms, doc_base, positions).arrays(), extra=extra, extra_pos=extra_pos)


def device_pseg(docs, n_terms, positions=None, batch=None, extra=0, extra_pos=0):
    """a positional segment as the device leaves it: the postings call with the optional pair and the positions call (doc_base 0: the caller
    puts empty documents in front), positions None = NULL token_positions"""
    toff, ids = csr(docs)
    r = phrasesuite.run_positions(toff, ids, n_terms, None if positions is None else phrasesuite.flat_positions(docs, positions), batch=batch)
    assert r.error is None, r.error
    n = int(r.counts[0])
    return PSeg(r.term, r.docs[:n], r.tfs[:n], r.first[:n + 1], r.ppos[:int(r.first[n])], extra, extra_pos)


class Result:
    def same_bytes(self, other):
        return self.error == other.error and all(getattr(self, k).tobytes() == getattr(other, k).tobytes() for k in ARRAYS + ("counts",))


def run(segs, n_terms_out, ordered, cap_out=None, cap_pos_out=None, batch=None, flags=None, n_terms_of=None):
    """vpt_postings_merge_positional_device on guarded arrays of exactly the sizes the call is told"""
    batch = batch or api.DeviceBatch(predictor())
    cap_out = sum(s.cap for s in segs) if cap_out is None else cap_out
    cap_pos_out = sum(s.cap_pos for s in segs) if cap_pos_out is None else cap_pos_out
    I = [tuple(G(a) for a in (s.term, s.docs, s.tfs, s.first, s.ppos)) for s in segs]
    O = {"term": G(np.full(n_terms_out + 1, SENTINEL, np.uint64)), "docs": G(np.full(max(cap_out, 1), SENTINEL, np.uint32)),
         "tfs": G(np.full(max(cap_out, 1), SENTINEL, np.uint32)), "first": G(np.full(cap_out + 1, SENTINEL, np.uint64)),
         "ppos": G(np.full(max(cap_pos_out, 1), SENTINEL, np.uint32)), "counts": G(np.full(3, SENTINEL, np.uint64))}
    r = Result()
    r.error = None
    try:
        batch.merge_positional_postings([tuple(a.ptr for a in t) + (s.n_terms if n_terms_of is None else n_terms_of[k], s.cap, s.cap_pos)
                                         for k, (s, t) in enumerate(zip(segs, I))], n_terms_out, O["term"].ptr, O["docs"].ptr, O["tfs"].ptr,
                                        O["first"].ptr, cap_out, O["ppos"].ptr, cap_pos_out, O["counts"].ptr, ordered, devmem.stream(), flags)
    except api.VaporettoError as e:
        r.error = str(e)
    try:
        batch.sync()
    except api.VaporettoError as e:
        r.error = r.error or str(e)
    bad = [k for k, a in O.items() if not a.guards_intact()] + [(k, j) for k, t in enumerate(I) for j, a in enumerate(t) if not a.guards_intact()]
    assert not bad, ("guard words overwritten", bad)
    assert all(a.get().tobytes() == a.sent.tobytes() for t in I for a in t), "an input was written"
    r.cap_out, r.cap_pos_out = cap_out, cap_pos_out
    for k in O:
        setattr(r, k, O[k].get())
    return r


def same_as(r, ref):
    """every output of a call that succeeded is the definition's, and nothing behind what it had to write was touched"""
    assert r.error is None, r.error
    term, docs, tfs, first, ppos = ref.arrays()
    n, m = len(docs), len(ppos)
    assert r.counts.tolist() == [n, ref.n_combined, m], (r.counts.tolist(), n, ref.n_combined, m)
    assert np.array_equal(r.term, term), [(k, int(a), int(b)) for k, (a, b) in enumerate(zip(r.term, term)) if a != b][:8]
    assert np.array_equal(r.docs[:n], docs) and np.array_equal(r.tfs[:n], tfs)
    assert np.array_equal(r.first[:n + 1], first), [(q, int(a), int(b)) for q, (a, b) in enumerate(zip(r.first, first)) if a != b][:8]
    assert np.array_equal(r.ppos[:m], ppos), [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(r.ppos, ppos)) if a != b][:8]
    assert int(r.first[0]) == 0 and int(r.first[n]) == m and np.array_equal(np.diff(r.first[:n + 1]), r.tfs[:n])
    assert (r.docs[n:r.cap_out] == SENTINEL).all() and (r.tfs[n:r.cap_out] == SENTINEL).all() and (r.first[n + 1:] == SENTINEL).all()
    assert (r.ppos[m:r.cap_pos_out] == SENTINEL).all()


def check_merge(segs, n_terms_out, routes=ROUTES, batch=None, whole=None):
    """the segments against the merge's definition (and, given, the one-pass definition of the whole batch) on the routes given"""
    ref = Ref.of_segments([s.five() for s in segs], n_terms_out)
    if whole is not None:
        assert all(np.array_equal(a, b) for a, b in zip(ref.arrays(), whole.arrays()))
    for ordered in routes:
        same_as(run(segs, n_terms_out, ordered, batch=batch), ref)
    return ref


def random_docs(rng, n_docs, n_terms, longest=30, dropped=True):
    docs = []
    for _ in range(n_docs):
        d = [rng.randrange(n_terms) for _ in range(0 if rng.random() < 0.15 else rng.randint(1, longest))]
        docs.append([rng.choice([-1, n_terms, n_terms + 5]) if dropped and rng.random() < 0.1 else x for x in d])
    return docs


def deal(docs, positions, owner, K):
    """tokens dealt to K segments: per segment the documents with its tokens only, every token keeping its position in its document"""
    positions = phraseref.default_positions(docs) if positions is None else positions
    return [([[x for x, o in zip(d, own) if o == s] for d, own in zip(docs, owner)],
             [[p for p, o in zip(ps, own) if o == s] for ps, own in zip(positions, owner)]) for s in range(K)]


# ---- 1
def check_ordered_equals_one_pass(seed=47):
    """ascending document ranges, each a device-made positional segment (NULL and gapped token_positions): both routes give the definition of
    the whole batch; empty segments and segments with fewer terms than n_terms_out among them"""
    rng = random.Random(seed)
    batch = api.DeviceBatch(predictor())
    n_terms = 6
    for gaps in (False, True):
        docs = random_docs(rng, 22, n_terms)
        docs[3], docs[4] = [], [n_terms + 5, -1]
        positions = phrasesuite.gapped(rng, docs) if gaps else None
        n = len(docs)
        whole = Ref.of_documents(docs, n_terms, 0, positions)
        for K, cut in ((1, [0, n]), (2, [0, 9, n]), (7, [0, 3, 3, 5, 5, 11, 17, n])):   # (7: two empty ranges, one of a dropped and an empty document)
            assert len(cut) == K + 1
            segs = []
            for lo, hi in zip(cut, cut[1:]):
                if lo == hi:   # no document: the empty segment of the definition
                    segs.append(pseg_of([], n_terms))
                    continue
                part = [[]] * lo + docs[lo:hi]
                segs.append(device_pseg(part, n_terms, None if positions is None else [[]] * lo + positions[lo:hi], batch,
                                        extra=rng.choice([0, 2]), extra_pos=rng.choice([0, 5])))
            assert sum(1 for s in segs if int(s.term[-1]) == 0) >= (2 if K == 7 else 0)
            check_merge(segs, n_terms, batch=batch, whole=whole)
    # segments with fewer terms than n_terms_out: the vocabulary grew between the batches
    a = pseg_of([[0, 0, 1]], 2)
    b = pseg_of([[], [3, 0, 3, 1]], 4)
    c = pseg_of([[], [], [5, 2, 5]], 6)
    ref = check_merge([a, b, c], 7, batch=batch)
    assert ref.terms[3] == {1: [0, 2]} and ref.terms[5] == {2: [0, 2]} and ref.n_combined == 0


# ---- 2
def check_general(seed=21):
    """tokens dealt to K segments at random (documents repeat across segments, token_positions keep the document positions): the general merge
    of the device-made segments is the definition of the whole batch; runs of 1, 2 and K; the ordered input through the general route"""
    rng = random.Random(seed)
    batch = api.DeviceBatch(predictor())
    for n_terms, K, gaps in ((4, 3, False), (9, 5, True)):
        docs = random_docs(rng, 18, n_terms)
        docs[0] = [1] * (2 * K)       # a posting that every segment shares: a run of K
        docs[1] = [2, 0]              # postings that stand in one segment only: runs of 1
        positions = phrasesuite.gapped(rng, docs) if gaps else phraseref.default_positions(docs)
        owner = [[rng.randrange(K) for _ in d] for d in docs]
        owner[0] = [j % K for j in range(2 * K)]
        owner[1] = [0, 1]
        whole = Ref.of_documents(docs, n_terms, 0, positions)
        segs = [device_pseg(d, n_terms, p, batch, extra_pos=rng.choice([0, 3])) for d, p in deal(docs, positions, owner, K)]
        ref = check_merge(segs, n_terms, routes=(False,), batch=batch, whole=whole)
        assert ref.n_combined > 0
        runs = {}
        for s in segs:
            term, sdocs = s.five()[:2]
            for k in range(s.n_terms):
                for q in range(int(term[k]), int(term[k + 1])):
                    runs[(k, int(sdocs[q]))] = runs.get((k, int(sdocs[q])), 0) + 1
        assert {1, 2, K} <= set(runs.values()), sorted(set(runs.values()))
    # ascending ranges through the general route
    docs = random_docs(rng, 12, 5)
    segs = [pseg_of([[]] * lo + docs[lo:hi], 5) for lo, hi in ((0, 4), (4, 4), (4, 12))]
    check_merge(segs, 5, routes=(False,), batch=batch, whole=Ref.of_documents(docs, 5))


# ---- 3
def places_segments(first_places, total_places, rng):
    """three segments over ascending documents whose capacity_positions are first_places, some, the rest of total_places"""
    n_terms = 5
    held = [min(first_places, 40), 30, 45]
    caps = [first_places, (total_places - first_places) // 2, total_places - first_places - (total_places - first_places) // 2]
    segs, docs, base = [], [], 0
    for h, c in zip(held, caps):
        h = min(h, c)
        part, left = [], h
        while left:
            m = min(left, rng.randint(1, 9))
            part.append([rng.randrange(n_terms) for _ in range(m)])
            left -= m
        segs.append(pseg_of([[]] * base + part, n_terms, extra=rng.choice([0, 1]), extra_pos=c - h))
        assert segs[-1].cap_pos == c
        docs += part
        base += len(part)
    assert sum(s.cap_pos for s in segs) == total_places
    return segs, Ref.of_documents(docs, n_terms)


def check_position_places():
    """the position places on the workgroup's edges, and a segment boundary inside a wave: GARBAGE fills the places behind the positions held"""
    rng = random.Random(3)
    batch = api.DeviceBatch(predictor())
    for first, total in ((100, 255), (100, 256), (100, 257), (100, 3 * 256 + 1), (63, 300), (64, 300), (65, 300)):
        segs, whole = places_segments(first, total, rng)
        check_merge(segs, 5, batch=batch, whole=whole)
    # full segments: every place holds a position
    docs = random_docs(rng, 40, 5, dropped=False)
    segs = [pseg_of([[]] * lo + docs[lo:hi], 5) for lo, hi in ((0, 13), (13, 14), (14, 40))]
    assert all(s.cap_pos == int(s.first[s.cap]) for s in segs)
    check_merge(segs, 5, batch=batch, whole=Ref.of_documents(docs, 5))


def check_positions_on_the_scan_tile(n):
    """n positions over three segments, tokens dealt at random: the general route's sort and scans on the tile's edges, and the ordered route
    over the same number"""
    rng = random.Random(n)
    n_terms = 40
    docs, left = [], n
    while left:
        m = min(left, rng.randint(1, 12))
        docs.append([postingssuite.zipf(rng, n_terms) for _ in range(m)])
        left -= m
    batch = api.DeviceBatch(predictor())
    whole = Ref.of_documents(docs, n_terms)
    assert len(whole.arrays()[4]) == n
    owner = [[rng.randrange(3) for _ in d] for d in docs]
    segs = [pseg_of(d, n_terms, 0, p) for d, p in deal(docs, None, owner, 3)]
    ref = check_merge(segs, n_terms, routes=(False,), batch=batch, whole=whole)
    assert ref.n_combined > 0
    cuts = [0, len(docs) // 3, len(docs) // 2, len(docs)]
    segs = [pseg_of([[]] * lo + docs[lo:hi], n_terms) for lo, hi in zip(cuts, cuts[1:])]
    check_merge(segs, n_terms, batch=batch, whole=whole)


def check_edges():
    batch = api.DeviceBatch(predictor())
    T = tile()
    # one posting holds all positions of a segment
    a = pseg_of([[2] * 300], 4)
    b = pseg_of([[], [2] * 7 + [0]], 4, extra_pos=9)
    assert int(a.term[-1]) == 1 and a.cap_pos == 300
    check_merge([a, b], 4, batch=batch)
    both = pseg_of([[2] * 150], 4, positions=[list(range(1, 300, 2))])   # and combined with another that holds the odd positions
    even = pseg_of([[2] * 150], 4, positions=[list(range(0, 300, 2))])
    ref = check_merge([even, both], 4, routes=(False,), batch=batch)
    assert ref.terms == {2: {0: list(range(300))}} and ref.n_combined == 1
    # a term present only in the last segment
    segs = [pseg_of([[0, 1, 0]], 5), pseg_of([[], [1, 1]], 5), pseg_of([[], [], [4, 0, 4, 3]], 5)]
    ref = check_merge(segs, 5, batch=batch)
    assert ref.terms[4] == {2: [0, 2]} and ref.terms[3] == {2: [3]}
    # capacity_positions far larger than the positions held; an empty segment; a segment of capacity 0; K = 1 copies
    big = pseg_of([[1, 0, 1]], 3, extra=T, extra_pos=T + 3)
    none = pseg_of([], 3)
    assert none.cap == 0 and none.cap_pos == 0 and (big.ppos[3:] == GARBAGE).all()
    check_merge([none, big, none], 3, batch=batch)
    check_merge([none], 3, batch=batch)
    check_merge([big], 3, batch=batch)
    # the same document in every segment, one position each: one posting of K positions
    segs = [pseg_of([[1]], 2, positions=[[9 - 2 * s]]) for s in range(5)]
    ref = check_merge(segs, 2, routes=(False,), batch=batch)
    assert ref.terms == {1: {0: [1, 3, 5, 7, 9]}} and ref.n_combined == 4


# ---- 4
def check_phrase_search_over_the_merge(seed=11):
    """vpt_postings_phrase_search_device on the merged arrays gives phraseref's hits of the whole batch, score bits exact: phrases whose terms
    stood in different segments' vocabularies, documents split across segments (general) and ranges (ordered)"""
    rng = random.Random(seed)
    batch = api.DeviceBatch(predictor())
    n_terms = 4
    docs = phrasesuite.random_docs(seed, 30, n_terms, 20)
    phrases = [[rng.randrange(n_terms) for _ in range(rng.randint(1, 4))] for _ in range(16)] + [[0, 1, 2, 3], [3, 3]]
    weights = phrasesuite.weights_of(docs, n_terms, phrases)
    dl = [len(d) for d in docs]
    ref = phraseref.PhraseRef(docs, n_terms, 7, phrases, weights, 5)
    assert sum(1 for ph, m in zip(phrases, ref.match_counts) if len(ph) > 1 and m > 0) >= 5
    owner = [[rng.randrange(3) for _ in d] for d in docs]
    split = [pseg_of(d, n_terms, 7, p, extra_pos=2) for d, p in deal(docs, None, owner, 3)]
    # ranges whose earlier segments know fewer terms: a phrase [.., 3] spans what were the segments' term spaces
    ranges = [pseg_of([[]] * lo + [[t for t in d if t < nt] for d in docs[lo:hi]], nt, 7,
                      [[]] * lo + [[p for p, t in enumerate(d) if t < nt] for d in docs[lo:hi]]) for lo, hi, nt in ((0, 10, n_terms), (10, 30, n_terms))]
    for segs, ordered in ((split, False), (ranges, True), (ranges, False)):
        r = run(segs, n_terms, ordered, batch=batch)
        assert r.error is None, r.error
        n = int(r.counts[0])
        merged = phrasesuite.PSeg(r.term, r.docs[:n], r.tfs[:n], r.first[:n + 1], r.ppos[:int(r.counts[2])], extra=1)
        phrasesuite.same_as(phrasesuite.run(merged, 7, dl, phrases, weights, 5, batch=batch), ref)
    assert Ref.of_segments([s.five() for s in split], n_terms).n_combined > 0
    # a vocabulary that grew: the first segment has terms 0, 1 only; the phrase [1, 2] occurs in the later documents alone, [0, 1] in both
    docs = [[0, 1, 0, 1], [1, 0, 1], [0, 1, 2, 1, 2], [2, 1, 2, 0, 1]]
    segs = [pseg_of(docs[:2], 2), pseg_of([[], []] + docs[2:], 3)]
    phrases, dl = [[0, 1], [1, 2], [1, 0, 1]], [len(d) for d in docs]
    weights = phrasesuite.weights_of(docs, 3, phrases)
    ref = phraseref.PhraseRef(docs, 3, 0, phrases, weights, 4)
    assert ref.pf[0] == {0: 2, 1: 1, 2: 1, 3: 1} and ref.pf[1] == {2: 2, 3: 1}
    for ordered in ROUTES:
        r = run(segs, 3, ordered, batch=batch)
        n = int(r.counts[0])
        merged = phrasesuite.PSeg(r.term, r.docs[:n], r.tfs[:n], r.first[:n + 1], r.ppos[:int(r.counts[2])])
        phrasesuite.same_as(phrasesuite.run(merged, 0, dl, phrases, weights, 4, batch=batch), ref)


# ---- 4b
def check_high_documents(name):
    """postingsmergesuite.check_high_documents with positions: segments over [base, base + 12), [base + 12, base + 13), [base + 13, base + 37),
    the ordered merge and the general merge of the segments in reverse against the definition (and the one pass), two segments swapped under
    the ordered route, and the phrase search over the merged arrays against phraseref on the 37 documents"""
    batch = api.DeviceBatch(predictor())
    cuts = postingsmergesuite.HIGH_CUTS
    n_terms = 4
    docs = phrasesuite.random_docs(29, cuts[-1], n_terms, 16)
    docs[2], docs[3] = [0, 1, 0, 1], [1, 0, 1]
    docs[11], docs[12], docs[13] = [0, 1, 2], [1, 0, 1, 0], [0, 1, 3, 3]
    docs[36] = [2, 0, 1]
    base = postingssuite.high_base(name, len(docs))
    segs = [pseg_of(docs[lo:hi], n_terms, base + lo, extra=e, extra_pos=ep) for (lo, hi), e, ep in zip(zip(cuts, cuts[1:]), (0, 2, 1), (3, 0, 5))]
    whole = Ref.of_documents(docs, n_terms, base)
    ref = Ref.of_segments([s.five() for s in segs], n_terms)
    assert all(np.array_equal(a, b) for a, b in zip(ref.arrays(), whole.arrays())) and ref.n_combined == 0 and len(ref.arrays()[4]) > 200
    zero = ref.terms[0]
    assert {base + d for d in (2, 3, 11, 12, 13, 36)} <= set(zero) and max(zero) >= 1 << 31
    assert (min(zero) < 1 << 31) == (name == "2^31-3") and (max(zero) == 0xFFFFFFFF) == (name == "2^32-n")
    phrases = [[0, 1], [1, 0, 1], [3, 3], [2, 0, 1], [1], [0, 1, 2, 3]]
    weights = phrasesuite.weights_of(docs, n_terms, phrases)
    dl = [len(d) for d in docs]
    pref = phraseref.PhraseRef(docs, n_terms, base, phrases, weights, 40)
    assert {base + 2, base + 3, base + 36} <= set(pref.pf[0]) and base + 36 in pref.pf[3] and max(pref.match_counts) < 40
    for these, ordered in ((segs, True), (segs[::-1], False), (segs, False)):
        r = run(these, n_terms, ordered, batch=batch)
        same_as(r, ref)
        n = int(r.counts[0])
        merged = phrasesuite.PSeg(r.term, r.docs[:n], r.tfs[:n], r.first[:n + 1], r.ppos[:int(r.counts[2])], extra=1)
        for k in (3, 40):
            phrasesuite.same_as(phrasesuite.run(merged, base, dl, phrases, weights, k, batch=batch),
                                pref if k == 40 else phraseref.PhraseRef(docs, n_terms, base, phrases, weights, k))
    for swapped in ([segs[1], segs[0], segs[2]], [segs[0], segs[2], segs[1]], segs[::-1]):
        r = run(swapped, n_terms, True, batch=batch)
        assert r.error is not None and OVERLAP_ERROR in r.error, r.error
    same_as(run(segs, n_terms, True, batch=batch), ref)   # on the workspace that reported


# ---- 5
def check_capacity(seed=2):
    rng = random.Random(seed)
    docs = random_docs(rng, 30, 6, dropped=False)
    batch = api.DeviceBatch(predictor())
    ranges = [pseg_of([[]] * lo + docs[lo:hi], 6) for lo, hi in ((0, 12), (12, 30))]
    owner = [[rng.randrange(2) for _ in d] for d in docs]
    split = [pseg_of(d, 6, 0, p) for d, p in deal(docs, None, owner, 2)]
    for segs, routes in ((ranges, ROUTES), (split, (False,))):
        ref = Ref.of_segments([s.five() for s in segs], 6)
        term, wdocs, tfs, first, ppos = ref.arrays()
        n, m = len(wdocs), len(ppos)
        for ordered in routes:
            for cap in (m - 1, 0):
                r = run(segs, 6, ordered, cap_pos_out=cap, batch=batch)
                assert r.error is not None and POS_SMALL_ERROR in r.error, r.error
                assert r.counts.tolist() == [n, ref.n_combined, m]
                assert np.array_equal(r.ppos[:cap], ppos[:cap]) and np.array_equal(r.first[:n + 1], first)   # (behind the capacity: the guards)
                assert np.array_equal(r.docs[:n], wdocs) and np.array_equal(r.tfs[:n], tfs)
            for cap in (n - 1, 0):
                r = run(segs, 6, ordered, cap_out=cap, batch=batch)
                assert r.error is not None and SMALL_ERROR in r.error, r.error
                assert int(r.counts[0]) == n and int(r.counts[2]) == m
                assert np.array_equal(r.docs[:cap], wdocs[:cap]) and np.array_equal(r.tfs[:cap], tfs[:cap]) and np.array_equal(r.first[:cap], first[:cap])
            same_as(run(segs, 6, ordered, cap_out=n, cap_pos_out=m, batch=batch), ref)
    # the host call returns the needs and writes nothing else
    pred = predictor()
    posts = [s.postings() for s in split]
    ref = Ref.of_segments([s.five() for s in split], 6)
    n, m = ref.n_out, len(ref.arrays()[4])
    e = _expect(lambda: api.Postings.merge(posts, predictor=pred, positions=True, capacity_positions=m - 1), POS_SMALL_ERROR)
    assert (e.n_postings, e.n_positions) == (n, m)
    e = _expect(lambda: api.Postings.merge(posts, predictor=pred, positions=True, capacity=n - 1), SMALL_ERROR)
    assert (e.n_postings, e.n_positions) == (n, m)
    got = api.Postings.merge(posts, predictor=pred, positions=True, capacity=n, capacity_positions=m)
    assert len(got) == n and len(got.positions) == m


# ---- 6
def check_errors():
    pred = predictor()
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    s = pseg_of([[0, 1, 0]], 2)
    for ordered in ROUTES:
        assert "n_segments: must be between 1 and 1024" in run([], 2, ordered).error
        assert "n_terms: must be between 1 and 2^24" in run([s], 0, ordered, n_terms_of=[0]).error
        assert "n_terms: must be between 1 and 2^24" in run([s], (1 << 24) + 1, ordered, cap_out=1).error
        assert "segment: n_terms above n_terms_out" in run([s], 1, ordered).error
    assert "flags: unknown bit" in run([s], 2, False, flags=2).error
    assert "flags: unknown bit" in run([s], 2, False, flags=1 << 31).error
    # a broken ordered promise is still the overlap message
    r = run([pseg_of([[], [0]], 2), pseg_of([[1, 0]], 2)], 2, True)
    assert r.error is not None and OVERLAP_ERROR in r.error, r.error
    batch = api.DeviceBatch(pred)
    names = ("toff", "docs", "tfs", "first", "ppos", "term", "odocs", "otfs", "ofirst", "oppos", "counts")
    A = {k: devmem.zeros(8, np.uint64) for k in names}

    def call(caps=((3, 3),), cap_pos_out=8, b=batch, **null):   # (every array has 64 bytes: capacity_out 7)
        p = {k: (0 if k in null else a.ptr) for k, a in A.items()}
        b.merge_positional_postings([(p["toff"], p["docs"], p["tfs"], p["first"], p["ppos"], 2, c, cp) for c, cp in caps], 2, p["term"], p["odocs"],
                                    p["otfs"], p["ofirst"], 7, p["oppos"], cap_pos_out, p["counts"], False, devmem.stream())

    for k in names:
        _expect(lambda: call(**{k: 1}), "NULL device pointer")
    _expect(lambda: call(caps=((1, 1),) * (api.DeviceBatch.postings_merge_limit() + 1)), "n_segments: must be between 1 and 1024")
    _expect(lambda: call(caps=((1 << 31, 1), (1 << 31, 1))), "fewer than 2\\^32 input places")
    _expect(lambda: call(caps=((1 << 32, 1),)), "fewer than 2\\^32 input places")
    _expect(lambda: call(caps=((1, 1 << 31), (1, 1 << 31))), "fewer than 2\\^32 positions")
    _expect(lambda: call(caps=((1, 1 << 32),)), "fewer than 2\\^32 positions")
    _expect(lambda: call(cap_pos_out=1 << 32), "fewer than 2\\^32 positions")
    _expect(lambda: call(b=phrasesuite._MismatchBatch(batch, other)), "batch: does not belong to this predictor")
    _expect(lambda: call(b=phrasesuite._MismatchBatch(api.DeviceBatch(other), pred)), "batch: does not belong to this predictor")
    import ctypes as C
    st = _lib.load().vpt_postings_merge_positional_device(pred.handle, batch._h, None, 1, 2, 0, A["term"].ptr, A["odocs"].ptr, A["otfs"].ptr, A["ofirst"].ptr,
                                                          7, A["oppos"].ptr, 8, A["counts"].ptr, devmem.stream())
    assert st == _lib.VPT_INVALID_ARGUMENT
    assert C.sizeof(_lib.PostingsPositionalSegment) == 64
    call()
    batch.sync()
    assert A["term"].get(3).tolist() == [0, 0, 0] and A["counts"].get(3).tolist() == [0, 0, 0] and int(A["ofirst"].get(1)[0]) == 0


# ---- 7
def check_bad_positions():
    batch = api.DeviceBatch(predictor())
    sound = pseg_of([[], [], [1, 0]], 2)
    for trio in ([0, 3, 3], [0, 4, 3]):   # term 0 of document 0 holds 0, 2, 3: an equal pair, a descending pair
        bad = pseg_of([[0, 1, 0, 0]], 2)
        assert bad.ppos[:4].tolist() == [0, 2, 3, 1]
        bad.ppos[:3] = trio
        for ordered in ROUTES:
            r = run([bad, sound], 2, ordered, batch=batch)
            assert r.error is not None and POSITIONS_ERROR in r.error, r.error
            check_merge([pseg_of([[0, 1, 0, 0]], 2), sound], 2, routes=(ordered,), batch=batch)   # the workspace takes the sound ones afterwards
    # positions that descend between two postings only are a segment's
    check_merge([pseg_of([[0, 1, 0]], 2, positions=[[5, 1, 9]]), sound], 2, batch=batch)
    # equal positions in two segments of one (term, document): the case the merge without positions combines
    a = pseg_of([[0, 1]], 2, positions=[[4, 6]])
    b = pseg_of([[1, 1]], 2, positions=[[6, 8]])
    r = run([a, b], 2, False, batch=batch)
    assert r.error is not None and POSITIONS_ERROR in r.error, r.error
    pred = predictor()
    post = pseg_of([[0, 1, 0], [1]], 2).postings()
    _expect(lambda: api.Postings.merge([post, post], predictor=pred, positions=True), POSITIONS_ERROR)
    plain = api.Postings.merge([post, post], predictor=pred)
    assert plain.positions is None and plain.first is None and plain.n_combined == 3 and plain.tfs.tolist() == [4, 2, 2]
    try:
        Ref.of_segments([post_five(post), post_five(post)], 2)
        assert False, "the definition takes a duplicate position"
    except positionsmergeref.DuplicatePosition:
        pass


def post_five(post):
    return post.term_offsets, post.docs, post.tfs, post.first, post.positions


# ---- 8
def hostile_cases():
    """name -> the first segment with one defect; the second segment is sound"""
    def base():
        # term 0 {1: [0, 2], 3: [1]}, term 1 {2: [0]}, term 3 {0: [0], 1: [1], 5: [0, 1, 2, 3]}: term 0 2 3 3 6; first 0 2 3 4 5 6 10
        return pseg_of([[3], [0, 3, 0], [1], [9, 0], [], [3, 3, 3, 3]], 4, extra=2, extra_pos=2)
    cases = {}

    def case(name, fn):
        s = base()
        fn(s)
        cases[name] = s
    case("post_first_above_zero", lambda s: s.first.__setitem__(0, 1))
    case("post_first_descends", lambda s: s.first.__setitem__(4, 3))
    case("post_first_descends_at_a_term_bound", lambda s: s.first.__setitem__(3, 1))
    case("post_first_ends_above_capacity_positions", lambda s: s.first.__setitem__(6, 13))
    case("post_first_far_above", lambda s: s.first.__setitem__(slice(4, 7), [1 << 40, 1 << 62, (1 << 64) - 1]))
    case("post_first_huge_everywhere", lambda s: s.first.__setitem__(slice(0, 7), [(1 << 64) - 1 - j for j in range(7)]))
    case("post_first_disagrees_with_the_tf", lambda s: s.tfs.__setitem__(0, 1))
    case("post_first_shifted_inside_a_term", lambda s: s.first.__setitem__(1, 1))
    case("term_offsets_end_above_capacity", lambda s: s.term.__setitem__(4, 9))
    case("term_offsets_huge", lambda s: s.term.__setitem__(slice(1, 5), [1 << 40, 1 << 41, 1 << 62, (1 << 64) - 1]))
    case("term_offsets_decrease", lambda s: s.term.__setitem__(2, 1))
    return base(), pseg_of([[], [], [], [], [], [], [0, 2, 2], [2]], 4), cases


N_HOSTILE = 11


def run_hostile():
    sound, second, cases = hostile_cases()
    assert len(cases) == N_HOSTILE
    assert sound.term.tolist() == [0, 2, 3, 3, 6] and sound.first[:7].tolist() == [0, 2, 3, 4, 5, 6, 10] and (sound.cap, sound.cap_pos) == (8, 12)
    batch = api.DeviceBatch(predictor())
    ran = 0
    for name, bad in cases.items():
        for ordered in ROUTES:
            for segs in ([bad, second], [second, bad] if not ordered else [bad]):
                r = run(segs, 4, ordered, batch=batch)
                assert r.error is not None and SEG_ERROR in r.error, (name, ordered, r.error)
            check_merge([sound, second], 4, routes=(ordered,), batch=batch)   # the sound ones on the same workspace
        ran += 1
    del batch
    return ran


# ---- 9
def check_determinism(seed=12):
    rng = random.Random(seed)
    T = tile()
    pred = predictor()
    one, two = api.DeviceBatch(pred), api.DeviceBatch(pred)
    docs = [[postingssuite.zipf(rng, 60) for _ in range(rng.randint(0, 25))] for _ in range(2 * T // 12)]
    cuts = [0, len(docs) // 4, len(docs) // 2, len(docs)]
    ranges = [pseg_of([[]] * lo + docs[lo:hi], 60) for lo, hi in zip(cuts, cuts[1:])]
    owner = [[rng.randrange(4) for _ in d] for d in docs]
    split = [pseg_of(d, 60, 0, p) for d, p in deal(docs, None, owner, 4)]
    whole = Ref.of_documents(docs, 60)
    assert T < len(whole.arrays()[4]) <= 3 * T + 1
    for ordered, these in ((True, ranges), (False, ranges), (False, split)):
        a = run(these, 60, ordered, batch=one)
        b = run(these, 60, ordered, batch=one)
        run([pseg_of([[1, 2, 1]], 4), pseg_of([[3], [1]], 4)], 4, False, batch=two)   # (the second workspace's scratch holds something else)
        c = run(these, 60, ordered, batch=two)
        assert a.error is None and a.same_bytes(b) and a.same_bytes(c)
        ref = Ref.of_segments([s.five() for s in these], 60)
        assert all(np.array_equal(x, y) for x, y in zip(ref.arrays(), whole.arrays()))
        same_as(a, ref)


# ---- 10
def check_host_call(seed=5):
    """vpt_postings_merge_positional through Postings.merge(positions=True): host arrays in and out, both routes, the counts"""
    rng = random.Random(seed)
    pred = predictor()
    docs = random_docs(rng, 40, 8)
    cuts = [0, 7, 7, 25, 40]
    ranges = [pseg_of([[]] * lo + docs[lo:hi], 8, 100) for lo, hi in zip(cuts, cuts[1:])]
    whole = Ref.of_documents(docs, 8, 100)
    want = whole.arrays()
    for ordered in ROUTES:
        posts = [s.postings() for s in ranges]
        for k, post in enumerate(posts):
            post.n_dropped = k
        got = api.Postings.merge(posts, ordered=ordered, predictor=pred, positions=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip((got.term_offsets, got.docs, got.tfs, got.first, got.positions), want))
        assert got.first.dtype == np.uint64 and got.positions.dtype == np.uint32 and got.order is None and got.n_dropped == 6 and got.n_combined == 0
        plain = api.Postings.merge(posts, ordered=ordered, predictor=pred)
        assert plain.first is None and plain.positions is None and postingssuite.same_postings(plain, got)
    owner = [[rng.randrange(3) for _ in d] for d in docs]
    split = [pseg_of(d, 8, 100, p).postings() for d, p in deal(docs, None, owner, 3)]
    got = api.Postings.merge(split, predictor=pred, positions=True, n_terms=10)
    assert all(np.array_equal(x, y) for x, y in zip((got.docs, got.tfs, got.first, got.positions), want[1:])) and got.n_combined > 0
    assert got.term_offsets.tolist() == want[0].tolist() + [int(want[0][-1])] * 2
    # phrase_search on the merged postings = on the one-pass postings
    dl = np.array([len(d) for d in docs], np.uint32)
    phrases = [[rng.randrange(8) for _ in range(rng.randint(1, 3))] for _ in range(10)]
    one = PSeg(*want).postings()
    hits, mc = got.phrase_search(phrases, 4, dl, 100, predictor=pred)
    hits1, mc1 = one.phrase_search(phrases, 4, dl, 100, predictor=pred)
    assert hits == hits1 and mc.tolist() == mc1.tolist() and int(mc.sum()) > 5
    _expect(lambda: api.Postings.merge(split, ordered=True, predictor=pred, positions=True), OVERLAP_ERROR)
    bare = api.Postings(split[0].term_offsets, split[0].docs, split[0].tfs, None, None, 0)
    _expect(lambda: api.Postings.merge([split[1], bare], predictor=pred, positions=True), "merge: a segment was made without positions")
    _expect(lambda: api.Postings.merge([], predictor=pred, n_terms=3, positions=True), "n_segments: must be between 1 and 1024")
    none = api.Postings.merge([pseg_of([], 4).postings()], predictor=pred, positions=True)
    assert len(none) == 0 and none.first.tolist() == [0] and len(none.positions) == 0


def check_index_batches():
    """VaporettoTokenizer.index_batches(positions=True) = index_batch(positions=True) of the concatenation in every array; phrase_search over
    it = over the one segment; the forms without the keyword are as they were"""
    from tests import searchsuite
    tok, texts = searchsuite.fixture_tokenizer()
    for doc_base in (0, 1000):
        whole = tok.index_batch(texts, doc_base, positions=True)
        assert len(whole) > 20 and whole.n_dropped > 0 and len(whole.positions) > len(whole)
        for cuts in ([0, len(texts)], [0, 1, 2, 40, 40, len(texts)]):
            batches = [texts[a:b] for a, b in zip(cuts, cuts[1:])]
            for ordered in ROUTES:
                got = tok.index_batches(batches, doc_base, ordered=ordered, positions=True)
                assert postingssuite.same_postings(got, whole) and got.n_combined == 0 and got.n_dropped == whole.n_dropped
                assert np.array_equal(got.first, whole.first) and np.array_equal(got.positions, whole.positions) and got.order is None
                assert np.array_equal(got.doc_lens, whole.doc_lens) and got.doc_base == whole.doc_base == doc_base
                hits, mc = tok.phrase_search(got, phrasesuite.PHRASE_TEXTS, 10)
                hits1, mc1 = tok.phrase_search(whole, phrasesuite.PHRASE_TEXTS, 10)
                assert hits == hits1 and mc.tolist() == mc1.tolist() and int(mc.sum()) > 3
        plain = tok.index_batches([texts[:30], texts[30:]], doc_base)
        assert plain.positions is None and plain.first is None and postingssuite.same_postings(plain, whole)
    none = tok.index_batches([], positions=True)
    assert len(none) == 0 and none.first.tolist() == [0]
    post = tok.index_batch(texts[:5], 0, positions=True)
    assert api.Postings.merge([post, post], predictor=tok.predictor).positions is None


def main(argv):
    assert argv == ["--emu-hostile"], "usage: python -m tests.positionsmergesuite --emu-hostile"
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
