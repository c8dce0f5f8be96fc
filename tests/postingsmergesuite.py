"""The checks of the postings merge (vpt_postings_merge_device, vpt_postings_merge; kernels_postings_merge.hip) against the definitions of
tests/postingsmergeref.py and tests/postingsref.py, run on the CPU emulator by tests/test_postings_merge_emu.py and on the MI355X by
tests/test_postings_merge_gpu.py; every comparison is exact integer equality, never against the device's own one-pass call.

    python -m tests.postingsmergesuite --emu-hostile     the hostile segments on the emulator, in a child process (hipemu checks its red
                                                         zones when the workspace goes)

Every array handed to the call has exactly the size the call is told and guard words on both sides, checked after the sync with the inputs
unwritten; outputs are filled with SENTINEL first.  T = vpt_postings_tile (4096); no case has more than 3 T + 1 input postings.
check_high_documents merges three contiguous device-made segments at the two bases of postingssuite.HIGH_BASES (documents on both sides of
2^31, the last document 0xFFFFFFFF) on both routes, a few hundred postings, and swaps two of them under the ordered route."""
import random
import sys

import numpy as np

from tests import devmem, patterntagsuite, postingsmergeref, postingsref, postingssuite, vocabsuite
from vaporetto_amd import _lib, api

G = postingssuite.G
SENTINEL = postingssuite.SENTINEL
SMALL_ERROR = postingssuite.SMALL_ERROR
SEG_ERROR = "segment: term_offsets or postings are not a segment's"
OVERLAP_ERROR = "segments: document ranges overlap or descend"
TF_ERROR = "tf: sum exceeds 32 bits"
predictor = postingssuite.predictor
tile = postingssuite.tile
csr = postingssuite.csr
zipf = postingssuite.zipf
_expect = postingssuite._expect
ROUTES = (True, False)   # ordered, general


class Seg:
    """a segment on the host: term [n_terms + 1], docs / tfs [max(cap, 1)] with SENTINEL behind the postings"""

    def __init__(self, term, docs, tfs, cap=None):
        self.term = np.asarray(term, np.uint64)
        self.cap = len(docs) if cap is None else cap
        self.docs, self.tfs = np.full(max(self.cap, 1), SENTINEL, np.uint32), np.full(max(self.cap, 1), SENTINEL, np.uint32)
        n = min(len(docs), self.cap)
        self.docs[:n], self.tfs[:n] = np.asarray(docs, np.uint32)[:n], np.asarray(tfs, np.uint32)[:n]
        self.n_terms = len(self.term) - 1

    def triple(self):
        n = int(self.term[-1])
        return self.term, self.docs[:n], self.tfs[:n]


def seg_of(terms, n_terms, extra=0):
    """{term: {document: tf}} -> Seg with `extra` SENTINEL places behind its postings"""
    df = np.zeros(n_terms + 1, np.uint64)
    docs, tfs = [], []
    for k in sorted(terms):
        df[k + 1] = len(terms[k])
        for d in sorted(terms[k]):
            docs.append(d)
            tfs.append(terms[k][d])
    return Seg(np.cumsum(df, dtype=np.uint64), docs, tfs, len(docs) + extra)


def device_segment(toff, ids, n_terms, doc_base, batch):
    """a segment as the device postings call leaves it: capacity = the tokens, SENTINEL behind the postings"""
    r = postingssuite.run(toff, ids, n_terms, doc_base, positions=False, batch=batch)
    assert r.error is None, r.error
    return Seg(r.term, r.docs[:r.cap_out], r.tfs[:r.cap_out], r.cap_out)


class Result:
    def same_bytes(self, other):
        return self.error == other.error and all(getattr(self, k).tobytes() == getattr(other, k).tobytes() for k in ("term", "docs", "tfs", "counts"))


def run(segs, n_terms_out, ordered, cap_out=None, batch=None, pred=None, flags=None, n_terms_of=None):
    """vpt_postings_merge_device on guarded arrays of exactly the sizes the call is told"""
    pred = pred or predictor()
    batch = batch or api.DeviceBatch(pred)
    cap_out = sum(s.cap for s in segs) if cap_out is None else cap_out
    I = [(G(s.term), G(s.docs), G(s.tfs)) for s in segs]
    O = {"term": G(np.full(n_terms_out + 1, SENTINEL, np.uint64)), "docs": G(np.full(max(cap_out, 1), SENTINEL, np.uint32)),
         "tfs": G(np.full(max(cap_out, 1), SENTINEL, np.uint32)), "counts": G(np.full(2, SENTINEL, np.uint64))}
    r = Result()
    r.error = None
    try:
        batch.merge_postings([(t.ptr, d.ptr, f.ptr, s.n_terms if n_terms_of is None else n_terms_of[k], s.cap)
                              for k, (s, (t, d, f)) in enumerate(zip(segs, I))], n_terms_out, O["term"].ptr, O["docs"].ptr, O["tfs"].ptr, cap_out,
                             O["counts"].ptr, ordered, devmem.stream(), flags)
    except api.VaporettoError as e:
        r.error = str(e)
    try:
        batch.sync()
    except api.VaporettoError as e:
        r.error = r.error or str(e)
    bad = [k for k, a in O.items() if not a.guards_intact()] + [(k, j) for k, t in enumerate(I) for j, a in enumerate(t) if not a.guards_intact()]
    assert not bad, ("guard words overwritten", bad)
    assert all(np.array_equal(a.get(), a.sent) for t in I for a in t), "an input was written"
    r.cap_out = cap_out
    for k in ("term", "docs", "tfs", "counts"):
        setattr(r, k, O[k].get())
    return r


def same_as(r, term, docs, tfs, n_combined):
    """every output of a call that succeeded is the definition's, and nothing behind what it had to write was touched"""
    assert r.error is None, r.error
    n = len(docs)
    assert r.counts.tolist() == [n, n_combined], (r.counts.tolist(), n, n_combined)
    assert np.array_equal(r.term, term), [(k, int(a), int(b)) for k, (a, b) in enumerate(zip(r.term, term)) if a != b][:8]
    assert int(r.term[0]) == 0 and int(r.term[-1]) == n
    assert np.array_equal(r.docs[:n], docs) and np.array_equal(r.tfs[:n], tfs)
    assert (r.docs[n:r.cap_out] == SENTINEL).all() and (r.tfs[n:r.cap_out] == SENTINEL).all()


def check_merge(segs, n_terms_out, routes=ROUTES, batch=None):
    """the segments against the merge's definition on the routes given"""
    ref = postingsmergeref.MergeRef([s.triple() for s in segs], n_terms_out)
    for ordered in routes:
        same_as(run(segs, n_terms_out, ordered, batch=batch), *ref.arrays(), ref.n_combined)
    return ref


# ---- 1
def random_docs(rng, n_terms, skew, n_docs):
    docs = []
    for _ in range(n_docs):
        n = rng.choice([0, 0, 1, 2]) if rng.random() < 0.2 else rng.randint(0, 120)
        d = [zipf(rng, n_terms) if skew else rng.randrange(n_terms) for _ in range(n)]
        docs.append([rng.choice([-1, n_terms, n_terms + 5, postingssuite.INT32_MIN, postingssuite.INT32_MAX]) if rng.random() < 0.1 else x for x in d])
    return docs


def check_ordered_equals_one_pass(seed):
    """contiguous groups of documents, each a segment of the device postings call with its doc_base: the ordered merge and the general merge
    are postingsref.Ref of the whole batch"""
    rng = random.Random(seed)
    batch = api.DeviceBatch(predictor())
    for n_terms, skew in ((1, False), (7, True), (300, False), (300, True), (70000, True)):
        a, b, c = (random_docs(rng, n_terms, skew, rng.randint(3, 12)) for _ in range(3))
        empties = [[]] * 3
        dropped = [[-1, n_terms, postingssuite.INT32_MAX], [n_terms + 5] * 4]
        docs = a + empties + b + dropped + c
        e0, b0, d0, c0, n = len(a), len(a) + 3, len(a) + 3 + len(b), len(a) + 3 + len(b) + 2, len(a) + 3 + len(b) + 2 + len(c)
        toff, ids = csr(docs)
        assert len(ids) <= 3 * tile() + 1
        whole = postingsref.Ref(toff, ids, n_terms, 11)
        term, wdocs, wtfs, _f, _o = whole.arrays()
        cuts = {1: [0, n], 2: [0, rng.randint(1, n - 1), n], 3: [0, e0, e0, n],                      # (3: an empty group)
                7: [0, e0, e0, b0, d0, c0, c0 + max(len(c) // 2, 1), n]}                            # (7: empty, only empty documents, all dropped)
        for K, cut in cuts.items():
            assert len(cut) == K + 1
            segs = [device_segment(*csr(docs[lo:hi]), n_terms, 11 + lo, batch) for lo, hi in zip(cut, cut[1:])]
            assert sum(int(s.term[-1]) for s in segs) == len(wdocs)
            for ordered in ROUTES:
                same_as(run(segs, n_terms, ordered, batch=batch), term, wdocs, wtfs, 0)


# ---- 2
def check_general(seed):
    """documents dealt to segments at random (the ranges interleave), then TOKENS dealt at random (documents repeat across segments): the
    general merge is the whole batch's postings, counts[1] the definition's"""
    rng = random.Random(seed)
    batch = api.DeviceBatch(predictor())
    for n_terms, skew, K in ((7, True, 3), (300, False, 5), (70000, True, 4)):
        docs = random_docs(rng, n_terms, skew, 25)
        toff, ids = csr(docs)
        whole = postingsref.Ref(toff, ids, n_terms, 5)
        term, wdocs, wtfs, _f, _o = whole.arrays()
        owner = [rng.randrange(K) for _ in docs]
        segs = [device_segment(*csr([d if owner[i] == s else [] for i, d in enumerate(docs)]), n_terms, 5, batch) for s in range(K)]
        same_as(run(segs, n_terms, False, batch=batch), term, wdocs, wtfs, 0)
        dealt = [[rng.randrange(K) for _ in d] for d in docs]
        segs = [device_segment(*csr([[x for x, o in zip(d, own) if o == s] for d, own in zip(docs, dealt)]), n_terms, 5, batch) for s in range(K)]
        ref = postingsmergeref.MergeRef([s.triple() for s in segs], n_terms)
        assert all(np.array_equal(x, y) for x, y in zip(ref.arrays(), (term, wdocs, wtfs))) and ref.n_combined > 0
        same_as(run(segs, n_terms, False, batch=batch), term, wdocs, wtfs, ref.n_combined)


# ---- 2b
HIGH_CUTS = (0, 12, 13, 37)


def high_docs(seed=33):
    """37 documents over 7 terms; the documents on both sides of every cut of HIGH_CUTS, the two on both sides of 2^31 at the lower base and the
    last one share terms, so neighbours in a term's merged list come from two segments and from both sides of the sign bit"""
    docs = random_docs(random.Random(seed), 7, True, 37)
    docs[2], docs[3] = [0, 1, 0], [1, 0]
    docs[11], docs[12], docs[13] = [0, 2], [1, 0, 1], [0, 3, 3]
    docs[36] = [2, 0]
    return docs


def check_high_documents(name):
    """segments over [base, base + 12), [base + 12, base + 13), [base + 13, base + 37): the ordered merge, and the general merge of the same
    segments handed over in reverse, are the definition's (and the one pass over the 37 documents); two segments swapped are the ordered
    route's error"""
    batch = api.DeviceBatch(predictor())
    docs = high_docs()
    base = postingssuite.high_base(name, len(docs))
    segs = [device_segment(*csr(docs[lo:hi]), 7, base + lo, batch) for lo, hi in zip(HIGH_CUTS, HIGH_CUTS[1:])]
    ref = postingsmergeref.MergeRef([s.triple() for s in segs], 7)
    term, wdocs, wtfs, _f, _o = postingsref.Ref(*csr(docs), 7, base).arrays()
    assert all(np.array_equal(x, y) for x, y in zip(ref.arrays(), (term, wdocs, wtfs))) and ref.n_combined == 0 and len(wdocs) > 100
    zero = ref.terms[0]
    assert {base + d for d in (2, 3, 11, 12, 13, 36)} <= set(zero) and max(zero) >= 1 << 31 and all(int(s.term[-1]) > 0 for s in segs)
    assert (min(zero) < 1 << 31) == (name == "2^31-3") and (max(zero) == 0xFFFFFFFF) == (name == "2^32-n")
    same_as(run(segs, 7, True, batch=batch), term, wdocs, wtfs, 0)
    same_as(run(segs[::-1], 7, False, batch=batch), term, wdocs, wtfs, 0)
    same_as(run(segs, 7, False, batch=batch), term, wdocs, wtfs, 0)
    for swapped in ([segs[1], segs[0], segs[2]], [segs[0], segs[2], segs[1]], segs[::-1]):   # (at both bases)
        r = run(swapped, 7, True, batch=batch)
        assert r.error is not None and OVERLAP_ERROR in r.error, r.error
    same_as(run(segs, 7, True, batch=batch), term, wdocs, wtfs, 0)   # on the workspace that reported


# ---- 3
def check_broken_promise():
    batch = api.DeviceBatch(predictor())
    a = seg_of({0: {0: 1, 4: 2}, 2: {2: 1}}, 3)
    b = seg_of({0: {3: 1}, 1: {7: 5}}, 3)                 # interleaved: 3 is inside a's range
    shared = seg_of({1: {4: 1, 9: 2}}, 3)                 # shares exactly the document 4 with a, in another term
    touch = seg_of({0: {5: 1}, 2: {5: 3, 6: 1}}, 3)       # a's largest + 1
    empty = seg_of({}, 3)
    for segs in ([a, b], [a, shared], [b, a], [a, empty, shared]):
        r = run(segs, 3, True, batch=batch)
        assert r.error is not None and OVERLAP_ERROR in r.error, r.error
        check_merge(segs, 3, routes=(False,), batch=batch)   # the general route takes them, on the workspace that reported the error
    check_merge([a, touch], 3, batch=batch)
    check_merge([a, empty, touch], 3, batch=batch)


# ---- 4
def check_vocabulary_growth():
    batch = api.DeviceBatch(predictor())
    s1 = seg_of({0: {0: 2, 1: 1}}, 1)
    s5 = seg_of({0: {2: 1}, 4: {2: 3, 3: 1}}, 5)
    s9 = seg_of({0: {4: 1}, 4: {5: 1}, 8: {4: 7}}, 9)
    ref = check_merge([s1, s5, s9], 9, batch=batch)
    assert ref.terms[4] == {2: 3, 3: 1, 5: 1} and ref.terms[8] == {4: 7} and ref.n_combined == 0
    check_merge([s9, s1, s5], 9, routes=(False,), batch=batch)
    check_merge([s1, s5], 12, batch=batch)   # n_terms_out above every segment's
    for ordered in ROUTES:
        r = run([s1, s9], 8, ordered, batch=batch)
        assert r.error is not None and "segment: n_terms above n_terms_out" in r.error and (r.term == SENTINEL).all() and (r.counts == SENTINEL).all()


# ---- 5
def spread_segments(n, K, n_terms, rng):
    """n postings over K segments with ascending document ranges: segment s's documents are s * 2^20 + ..."""
    sizes = [n // K + (1 if s < n % K else 0) for s in range(K)]
    segs = []
    for s, m in enumerate(sizes):
        ks = sorted(zipf(rng, n_terms) for _ in range(m))
        terms = {}
        for j, k in enumerate(ks):
            terms.setdefault(k, {})[(s << 20) + j] = rng.randint(1, 9)
        segs.append(seg_of(terms, n_terms, extra=rng.choice([0, 0, 3])))
    return segs


def check_input_postings(n):
    rng = random.Random(n)
    segs = spread_segments(n, 3, 50, rng)
    assert sum(int(s.term[-1]) for s in segs) == n
    check_merge(segs, 50)


def check_edges():
    T = tile()
    rng = random.Random(8)
    batch = api.DeviceBatch(predictor())
    # all postings in one term
    a = seg_of({3: {d: 1 + d % 5 for d in range(T // 2 + 1)}}, 5, extra=7)
    b = seg_of({3: {d: 2 for d in range(T // 2 + 1, T + 2)}}, 5)
    ref = check_merge([a, b], 5, batch=batch)
    assert len(ref.terms[3]) == T + 2
    # one posting in each of T + 1 terms
    a = seg_of({k: {k % 7: 1} for k in range(0, T + 1, 2)}, T + 1)
    b = seg_of({k: {7 + k % 3: 2} for k in range(1, T + 1, 2)}, T + 1, extra=2)
    check_merge([a, b], T + 1, batch=batch)
    # capacity larger than the postings, SENTINEL behind; a segment with capacity 0; K = 1 copies
    big = seg_of({0: {1: 1}, 2: {0: 4, 9: 1}}, 3, extra=T)
    none = seg_of({}, 3)
    assert none.cap == 0 and big.cap == T + 3 and (big.docs[3:] == SENTINEL).all()
    check_merge([none, big, none], 3, batch=batch)
    check_merge([none], 3, batch=batch)
    r = check_merge([big], 3, batch=batch)
    assert r.n_out == 3
    # the same document in every segment, general: one posting
    ref = check_merge([seg_of({1: {6: s + 1}}, 2) for s in range(5)], 2, routes=(False,), batch=batch)
    assert ref.terms == {1: {6: 15}} and ref.n_combined == 4
    del rng


def check_segment_limit():
    """K = the limit with one posting each; one more is refused"""
    K = api.DeviceBatch.postings_merge_limit()
    assert K >= 1024
    segs = [seg_of({s % 3: {s: 1 + s % 4}}, 3) for s in range(K)]
    check_merge(segs, 3)
    r = run(segs[:2] * 2, 3, False)   # (documents repeat: 0, 1, 0, 1)
    assert r.error is None and r.counts.tolist() == [2, 2]


# ---- 6
def check_capacity():
    rng = random.Random(2)
    segs = spread_segments(200, 3, 30, rng)
    twice = segs + [segs[1]]
    batch = api.DeviceBatch(predictor())
    for these, routes in ((segs, ROUTES), (twice, (False,))):
        ref = postingsmergeref.MergeRef([s.triple() for s in these], 30)
        term, docs, tfs = ref.arrays()
        needed = len(docs)
        for ordered in routes:
            for cap_out in (needed - 1, 0):
                r = run(these, 30, ordered, cap_out=cap_out, batch=batch)
                assert r.error is not None and SMALL_ERROR in r.error, r.error
                assert int(r.counts[0]) == needed
                assert np.array_equal(r.docs[:cap_out], docs[:cap_out]) and np.array_equal(r.tfs[:cap_out], tfs[:cap_out])   # (behind it: the guards)
            same_as(run(these, 30, ordered, cap_out=needed, batch=batch), term, docs, tfs, ref.n_combined)


# ---- 7
def hostile_cases():
    """name -> the first segment with one defect; the second segment is sound"""
    def base():
        return seg_of({0: {1: 1, 3: 2}, 1: {2: 1}, 3: {0: 1, 1: 1, 5: 4}}, 4, extra=2)   # term 0 2 3 3 6; cap 8
    cases = {}

    def case(name, fn):
        s = base()
        fn(s)
        cases[name] = s
    case("first_offset_above_zero", lambda s: s.term.__setitem__(0, 1))
    case("decrease", lambda s: s.term.__setitem__(2, 1))
    case("end_above_capacity", lambda s: s.term.__setitem__(4, 9))
    case("end_far_above_capacity", lambda s: s.term.__setitem__(4, (1 << 64) - 1))
    case("huge_offsets", lambda s: s.term.__setitem__(slice(1, 5), [1 << 40, 1 << 41, 1 << 62, (1 << 64) - 1]))
    case("equal_documents", lambda s: s.docs.__setitem__(4, 0))
    case("descending_documents", lambda s: s.docs.__setitem__(5, 0))
    case("zero_tf", lambda s: s.tfs.__setitem__(2, 0))
    return base(), seg_of({0: {9: 1}, 2: {8: 2}}, 4), cases


N_HOSTILE = 8


def run_hostile():
    sound, second, cases = hostile_cases()
    assert len(cases) == N_HOSTILE
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


# ---- 8
def check_tf_overflow():
    batch = api.DeviceBatch(predictor())
    one = seg_of({1: {7: 1}, 2: {3: 1}}, 3)
    r = run([seg_of({1: {7: 0xFFFFFFFF}}, 3), one], 3, False, batch=batch)
    assert r.error is not None and TF_ERROR in r.error, r.error
    ref = check_merge([seg_of({1: {7: 0xFFFFFFFE}}, 3), one], 3, routes=(False,), batch=batch)
    assert ref.terms[1] == {7: 0xFFFFFFFF} and ref.n_combined == 1


# ---- 9
def check_errors():
    pred = predictor()
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    s = seg_of({0: {1: 1}}, 2)
    for ordered in ROUTES:
        assert "n_segments: must be between 1 and 1024" in run([], 2, ordered).error
        assert "n_terms: must be between 1 and 2^24" in run([s], 0, ordered, n_terms_of=[0]).error
        assert "n_terms: must be between 1 and 2^24" in run([s], (1 << 24) + 1, ordered, cap_out=1).error
        assert "segment: n_terms above n_terms_out" in run([s], 1, ordered).error
    assert "n_segments: must be between 1 and 1024" in run([s] * (api.DeviceBatch.postings_merge_limit() + 1), 2, False).error
    assert "flags: unknown bit" in run([s], 2, False, flags=2).error
    assert "flags: unknown bit" in run([s], 2, False, flags=1 << 31).error
    batch = api.DeviceBatch(pred)
    A = {k: devmem.zeros(8, dt) for k, dt in (("toff", np.uint64), ("docs", np.uint32), ("tfs", np.uint32), ("term", np.uint64), ("odocs", np.uint32),
                                             ("otfs", np.uint32), ("counts", np.uint64))}

    def call(caps=(3,), **null):
        p = {k: (0 if k in null else a.ptr) for k, a in A.items()}
        batch.merge_postings([(p["toff"], p["docs"], p["tfs"], 2, c) for c in caps], 2, p["term"], p["odocs"], p["otfs"], 8, p["counts"], False, devmem.stream())

    for k in A:
        _expect(lambda: call(**{k: 1}), "NULL device pointer")
    _expect(lambda: call(caps=(1 << 31, 1 << 31)), "fewer than 2\\^32 input places")
    _expect(lambda: call(caps=(1 << 32,)), "fewer than 2\\^32 input places")
    segs = (_lib.PostingsSegment * 1)(_lib.PostingsSegment(A["toff"].ptr, A["docs"].ptr, A["tfs"].ptr, 2, 3))
    import ctypes as C
    for p_h, b_h, sg in ((other.handle, batch._h, segs), (pred.handle, api.DeviceBatch(other)._h, segs), (None, batch._h, segs), (pred.handle, None, segs),
                         (pred.handle, batch._h, None)):
        st = _lib.load().vpt_postings_merge_device(p_h, b_h, C.addressof(sg) if sg is not None else None, 1, 2, 0, A["term"].ptr, A["odocs"].ptr, A["otfs"].ptr,
                                                   8, A["counts"].ptr, devmem.stream())
        assert st == _lib.VPT_INVALID_ARGUMENT
        _expect(lambda: api._raise(st), "NULL device pointer" if sg is None else "batch: does not belong to this predictor")
    call()
    batch.sync()
    assert A["term"].get(3).tolist() == [0, 0, 0] and A["counts"].get(2).tolist() == [0, 0]


# ---- 10
def check_determinism(seed=12):
    rng = random.Random(seed)
    T = tile()
    pred = predictor()
    one, two = api.DeviceBatch(pred), api.DeviceBatch(pred)
    segs = spread_segments(2 * T + 5, 4, 500, rng)
    for ordered, these in ((True, segs), (False, segs), (False, segs + segs[1:3])):
        a = run(these, 500, ordered, batch=one)
        b = run(these, 500, ordered, batch=one)
        run([seg_of({1: {2: 3}}, 4)] * 2, 4, False, batch=two)   # (the second workspace's scratch holds something else)
        c = run(these, 500, ordered, batch=two)
        assert a.error is None and a.same_bytes(b) and a.same_bytes(c)
        ref = postingsmergeref.MergeRef([s.triple() for s in these], 500)
        same_as(a, *ref.arrays(), ref.n_combined)


# ---- 11
def as_postings(s, n_dropped=0):
    term, docs, tfs = s.triple()
    return api.Postings(term, docs.copy(), tfs.copy(), None, None, n_dropped)


def check_host_call(seed=5):
    """vpt_postings_merge through Postings.merge: host arrays in and out, both routes, the counts, too small a capacity"""
    rng = random.Random(seed)
    pred = predictor()
    segs = spread_segments(300, 4, 40, rng)
    ref = postingsmergeref.MergeRef([s.triple() for s in segs], 40)
    term, docs, tfs = ref.arrays()
    for ordered in ROUTES:
        got = api.Postings.merge([as_postings(s, k) for k, s in enumerate(segs)], ordered=ordered, predictor=pred)
        assert got.term_offsets.tobytes() == term.tobytes() and got.docs.tobytes() == docs.tobytes() and got.tfs.tobytes() == tfs.tobytes()
        assert got.docs.dtype == np.uint32 and got.term_offsets.dtype == np.uint64 and got.n_dropped == 6 and got.n_combined == 0
        assert got.first is None and got.order is None
    twice = [as_postings(s) for s in segs + segs[:2]]
    ref2 = postingsmergeref.MergeRef([s.triple() for s in segs + segs[:2]], 45)
    got = api.Postings.merge(twice, predictor=pred, n_terms=45)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((got.term_offsets, got.docs, got.tfs), ref2.arrays())) and got.n_combined == ref2.n_combined > 0
    _expect(lambda: api.Postings.merge(twice, ordered=True, predictor=pred), OVERLAP_ERROR)
    e = _expect(lambda: api.Postings.merge(twice, predictor=pred, capacity=ref2.n_out - 1), SMALL_ERROR)
    assert e.n_postings == ref2.n_out
    assert len(api.Postings.merge(twice, predictor=pred, capacity=ref2.n_out)) == ref2.n_out
    _expect(lambda: api.Postings.merge([], predictor=pred, n_terms=3), "n_segments: must be between 1 and 1024")
    _expect(lambda: api.Postings.merge(twice, predictor=pred, n_terms=39), "segment: n_terms above n_terms_out")
    _expect(lambda: api.Postings.merge(twice), "merge: no predictor")
    bad = as_postings(segs[0])
    bad.term_offsets = bad.term_offsets.copy()
    bad.term_offsets[-1] += 1   # an end above the arrays
    _expect(lambda: api.Postings.merge([bad], predictor=pred), SEG_ERROR)
    none = api.Postings.merge([as_postings(seg_of({}, 4))], predictor=pred)
    assert len(none) == 0 and none.term_offsets.tolist() == [0] * 5


def check_index_batches():
    """VaporettoTokenizer.index_batches over batches of tests/golden text = index_batch of the concatenation; the parts are merged on both routes"""
    from tests import kat
    raw, _ = kat.load_fixture("tantivy_model.bin")
    texts = postingssuite.fixture_corpus()
    norm = api.KyteaFullwidthFilter()
    plain = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR")
    distinct = sorted({norm.filter(t.text) for d in plain.token_stream_batch(texts) for t in d})
    tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DR", vocab=[s for k, s in enumerate(distinct) if k % 3 != 1])
    for doc_base in (0, 1000):
        whole = tok.index_batch(texts, doc_base)
        assert len(whole) > 20 and whole.n_dropped > 0
        for cuts in ([0, len(texts)], [0, 1, 2, 40, 40, len(texts)], list(range(0, len(texts), 9)) + [len(texts)]):
            batches = [texts[a:b] for a, b in zip(cuts, cuts[1:])]
            for ordered in ROUTES:
                got = tok.index_batches(batches, doc_base, ordered=ordered)
                assert postingssuite.same_postings(got, whole) and got.n_combined == 0, (cuts, ordered)
        got = tok.index_batches((b for b in [texts[:30], texts[30:]]), doc_base)   # any iterable
        assert postingssuite.same_postings(got, whole)
    none = tok.index_batches([])
    assert len(none) == 0 and not none.term_offsets.any()


def main(argv):
    assert argv == ["--emu-hostile"], "usage: python -m tests.postingsmergesuite --emu-hostile"
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
