"""The checks of the position lists of a segment and of the exact-phrase BM25 top-k search (vpt_postings_positions_device,
vpt_postings_phrase_search_device, vpt_postings_phrase_search, vpt_token_stream_positional_postings_batch; kernels_postings_phrase.hip) against
the definitions of tests/postingsref.py and tests/phraseref.py, run on the CPU emulator by tests/test_postings_phrase_emu.py and on the MI355X
by tests/test_postings_phrase_gpu.py; every comparison of documents, counts, frequencies and score BITS is exact equality with phraseref.

    python -m tests.phrasesuite --emu-hostile     the hostile inputs on the emulator, in a child process (hipemu checks its red zones when the
                                                  workspace goes)

Every array handed to a device call has exactly the size the call is told and guard words on both sides, checked after the sync with the
inputs unwritten; the outputs are filled with SENTINEL first (the scores are handed over as their uint32 bits), so an entry the call must not
write is seen to be left alone.  T = vpt_postings_tile (4096); no case has more than 3 T + 1 probes.

    python -m tests.phrasesuite --emu-hostile-high     the hostile postings at the top of the document range, in the same way

check_high_documents runs the random and the ties corpus at the two bases of postingssuite.HIGH_BASES (documents on both sides of 2^31, the
last document 0xFFFFFFFF) with two hostile postings at the upper one; check_tile_edge_ties cuts a group of n equal scores (n = T, T + 1,
2 T + 1 probes, the largest it uses and inside the cap above) with k on both sides of T and puts a phrase's last probe on records T - 2, T - 1
and T."""
import random
import sys

import numpy as np

from tests import devmem, patterntagsuite, phraseref, postingsmergesuite, postingsref, postingssuite, searchref, searchsuite, vocabsuite
from vaporetto_amd import _lib, api

G = postingssuite.G
SENTINEL = postingssuite.SENTINEL
CSR_ERROR = postingssuite.CSR_ERROR
SEG_ERROR = postingsmergesuite.SEG_ERROR
QCSR_ERROR = searchsuite.QCSR_ERROR
WEIGHT_ERROR = searchsuite.WEIGHT_ERROR
POSITIONS_ERROR = "positions: do not strictly ascend inside a document's list"
LONG_ERROR = "query: a phrase of more than 64 terms"
PROBES_ERROR = "capacity_probes: smaller than the number of probes"
predictor = postingssuite.predictor
tile = postingssuite.tile
csr = postingssuite.csr
_expect = postingssuite._expect
idf_of = searchsuite.idf_of
F = np.float32
OUTPUTS = ("hd", "hs", "hf", "hc", "mc")


def bits(x):
    return searchref.bits(x)


# ---- the positions call
class PositionsResult:
    pass


def run_positions(toff, ids, n_terms, positions=None, cap_in=None, batch=None, toff_for_positions=None):
    """vpt_postings_batch_device with the optional pair, then vpt_postings_positions_device, on guarded arrays of exactly the stated sizes.
    positions: a flat uint32 array per token, or None (NULL).  toff_for_positions: other token_offsets for the second call (hostile CSRs)."""
    batch = batch or api.DeviceBatch(predictor())
    toff, ids = np.asarray(toff, np.uint64), np.asarray(ids, np.int32)
    cap_in = len(ids) if cap_in is None else cap_in
    cap = max(cap_in, 1)
    I = {"toff": G(toff), "ids": G(ids[:cap_in] if cap_in else np.zeros(1, np.int32))}
    if positions is not None:
        I["pos"] = G(np.asarray(positions, np.uint32)[:cap_in] if cap_in else np.zeros(1, np.uint32))
    O = {"term": G(np.full(n_terms + 1, SENTINEL, np.uint64)), "docs": G(np.full(cap, SENTINEL, np.uint32)), "tfs": G(np.full(cap, SENTINEL, np.uint32)),
         "counts": G(np.full(2, SENTINEL, np.uint64)), "first": G(np.full(cap_in + 1, SENTINEL, np.uint64)), "order": G(np.full(cap, SENTINEL, np.uint32)),
         "ppos": G(np.full(cap, SENTINEL, np.uint32))}
    r = PositionsResult()
    r.error = None
    n_docs = len(toff) - 1
    try:
        batch.postings(I["toff"].ptr, n_docs, I["ids"].ptr, cap_in, n_terms, 0, O["term"].ptr, O["docs"].ptr, O["tfs"].ptr, cap_in, O["first"].ptr,
                       O["order"].ptr, O["counts"].ptr, devmem.stream())
        batch.sync()
        t2 = I["toff"]
        if toff_for_positions is not None:
            t2 = I["toff2"] = G(np.asarray(toff_for_positions, np.uint64))
        batch.postings_positions(t2.ptr, n_docs, cap_in, I["pos"].ptr if positions is not None else 0, O["term"].ptr, n_terms, O["first"].ptr, cap_in,
                                 O["order"].ptr, O["ppos"].ptr, devmem.stream())
    except api.VaporettoError as e:
        r.error = str(e)
    try:
        batch.sync()
    except api.VaporettoError as e:
        r.error = r.error or str(e)
    bad = [k for k, a in list(I.items()) + list(O.items()) if not a.guards_intact()]
    assert not bad, ("guard words overwritten", bad)
    assert all(np.array_equal(a.get(), a.sent) for a in I.values()), "an input was written"
    for k in O:
        setattr(r, k, O[k].get())
    return r


def flat_positions(docs, positions):
    return np.array([p for d in (positions if positions is not None else phraseref.default_positions(docs)) for p in d], np.uint32)


def check_positions_against_ref(docs, n_terms, positions=None, batch=None):
    """ppos[i] = the position of token order[i] for every i below the indexed tokens; SENTINEL behind them"""
    toff, ids = csr(docs)
    ref = postingsref.Ref(toff, ids, n_terms)
    _t, _d, _f, first, order = ref.arrays()
    flat = flat_positions(docs, positions)
    r = run_positions(toff, ids, n_terms, None if positions is None else flat, batch=batch)
    assert r.error is None, r.error
    n_idx = len(order)
    assert int(r.first[len(_d)]) == n_idx and np.array_equal(r.order[:n_idx], order)
    want = flat[order] if n_idx else np.zeros(0, np.uint32)
    assert np.array_equal(r.ppos[:n_idx], want), [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(r.ppos[:n_idx], want)) if a != b][:6]
    assert (r.ppos[n_idx:] == SENTINEL).all()
    for q in range(len(_d)):   # posting by posting: the token lists' positions, strictly ascending
        a, b = int(first[q]), int(first[q + 1])
        assert (np.diff(r.ppos[a:b].astype(np.int64)) > 0).all()
    return r, ref


def gapped(rng, docs):
    """positions as a stop-filtered stream leaves them: strictly ascending inside a document, with gaps"""
    out = []
    for d in docs:
        p, row = 0, []
        for _ in d:
            p += rng.choice([0, 0, 1, 3])
            row.append(p)
            p += 1
        out.append(row)
    return out


def check_positions(n):
    """n indexed tokens (T-1, T, T+1 of the key pass's tile) over documents with empty ones among them and dropped tokens, NULL positions and a
    filtered stream's"""
    rng = random.Random(n)
    n_terms = 5
    flat = [rng.randrange(n_terms) for _ in range(n)]
    docs, a = [[]], 0
    while a < n:
        b = min(n, a + rng.choice([0, 1, 2, 7, 30]))
        d = list(flat[a:b])
        if rng.random() < 0.3:
            d.insert(rng.randint(0, len(d)), -1)   # a dropped token: it has a position and no place in the segment
        docs.append(d)
        a = b
    docs += [[], []]
    batch = api.DeviceBatch(predictor())
    r, ref = check_positions_against_ref(docs, n_terms, batch=batch)
    assert len(ref.arrays()[4]) == n and ref.n_dropped > 0 and any(not d for d in docs[1:-2])
    check_positions_against_ref(docs, n_terms, gapped(rng, docs), batch=batch)


def check_positions_errors():
    batch = api.DeviceBatch(predictor())
    docs = [[1, 0, 1, 2], [], [0, 1, 1]]
    toff, ids = csr(docs)
    check_positions_against_ref(docs, 3, [[0, 1, 4, 9], [], [2, 3, 7]], batch=batch)
    for bad in ([[4, 1, 4, 9], [], [2, 3, 7]], [[5, 1, 4, 9], [], [2, 3, 7]], [[0, 1, 4, 9], [], [2, 8, 7]]):   # term 1 of document 0 / 2: equal, descending
        r = run_positions(toff, ids, 3, flat_positions(docs, bad), batch=batch)
        assert r.error is not None and POSITIONS_ERROR in r.error, r.error
    # positions that descend between two postings only are a segment's
    check_positions_against_ref(docs, 3, [[3, 4, 9, 0], [], [2, 3, 7]], batch=batch)
    # a workspace that reported is sound again; no token at all; no document
    check_positions_against_ref([[], []], 3, batch=batch)
    r = run_positions([0], [], 3, batch=batch)
    assert r.error is None and (r.ppos == SENTINEL).all()
    # errors at the call
    A = {k: devmem.zeros(8, np.uint64) for k in ("toff", "pos", "term", "first", "order", "ppos")}

    def call(n_terms=2, cap_in=3, **null):
        p = {k: (0 if k in null else a.ptr) for k, a in A.items()}
        batch.postings_positions(p["toff"], 2, cap_in, p["pos"], p["term"], n_terms, p["first"], 3, p["order"], p["ppos"], devmem.stream())

    for k in ("toff", "term", "first", "order", "ppos"):
        _expect(lambda: call(**{k: 1}), "NULL device pointer")
    for v in (0, (1 << 24) + 1):
        _expect(lambda: call(n_terms=v), "n_terms: must be between 1 and 2\\^24")
    _expect(lambda: call(cap_in=1 << 32), "fewer than 2\\^32 tokens")
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    wrong = _MismatchBatch(batch, other)
    _expect(lambda: wrong.postings_positions(A["toff"].ptr, 2, 3, 0, A["term"].ptr, 2, A["first"].ptr, 3, A["order"].ptr, A["ppos"].ptr),
            "batch: does not belong to this predictor")
    call(pos=1)
    call()
    batch.sync()


# ---- positional segments on the host
class PSeg:
    """a positional segment on the host, SENTINEL behind what it holds: term [n_terms + 1], docs / tfs [cap], first [cap + 1], ppos [cap_pos]"""

    def __init__(self, term, docs, tfs, first, ppos, extra=0):
        self.term = np.asarray(term, np.uint64)
        self.n_terms = len(self.term) - 1
        n, m = len(docs), len(ppos)
        self.cap, self.cap_pos = n + extra, m + extra
        self.docs, self.tfs = np.full(max(self.cap, 1), SENTINEL, np.uint32), np.full(max(self.cap, 1), SENTINEL, np.uint32)
        self.first, self.ppos = np.full(self.cap + 1, SENTINEL, np.uint64), np.full(max(self.cap_pos, 1), SENTINEL, np.uint32)
        self.docs[:n], self.tfs[:n], self.first[:n + 1], self.ppos[:m] = docs, tfs, first, ppos

    def postings(self):
        n = int(self.term[-1])
        out = api.Postings(self.term, self.docs[:n].copy(), self.tfs[:n].copy(), self.first[:n + 1].copy(), None, 0)
        out.positions = self.ppos[:int(self.first[n])].copy()
        return out


def pseg_of(docs, n_terms, doc_base=0, positions=None, extra=0):
    """documents as lists of ids (and positions) -> the positional segment, by the definition of the postings pass"""
    toff, ids = csr(docs)
    term, pdocs, tfs, first, order = postingsref.Ref(toff, ids, n_terms, doc_base).arrays()
    flat = flat_positions(docs, positions)
    return PSeg(term, pdocs, tfs, first, flat[order] if len(order) else np.zeros(0, np.uint32), extra)


class Result:
    def same_bytes(self, other):
        return self.error == other.error and all(getattr(self, k).tobytes() == getattr(other, k).tobytes() for k in OUTPUTS + ("counts",))

    def untouched(self):
        return all((getattr(self, k) == SENTINEL).all() for k in ("hd", "hs", "hf", "hc")) and (self.mc == np.uint64(SENTINEL)).all()


def probes_of(seg, phrases):
    """what the host call counts: per phrase that can match, the indexed tokens of its rarest term"""
    total = 0
    for ph in phrases:
        best = None
        for t in ph:
            if not 0 <= t < seg.n_terms:
                best = 0
                break
            a, b = int(seg.term[t]), int(seg.term[t + 1])
            if not (a < b <= seg.cap and int(seg.first[a]) <= int(seg.first[b]) <= seg.cap_pos):
                best = 0
                break
            n = int(seg.first[b]) - int(seg.first[a])
            best = n if best is None else min(best, n)
        total += best or 0
    return total


def run(seg, doc_base, dl, phrases, weights, k, k1=1.2, b=0.75, avgdl=None, cap_slots=None, cap_probes=None, batch=None, qoff=None, n_docs=None,
        freqs=True):
    """vpt_postings_phrase_search_device on guarded arrays of exactly the sizes the call is told"""
    batch = batch or api.DeviceBatch(predictor())
    flat = [t for ph in phrases for t in ph]
    cap_slots = len(flat) if cap_slots is None else cap_slots
    offsets = np.array([0] + list(np.cumsum([len(ph) for ph in phrases])), np.uint64) if qoff is None else np.asarray(qoff, np.uint64)
    spare = max(cap_slots - len(flat), 0)
    terms = np.array(flat + [0] * spare + [0], np.int64).astype(np.int32)[:max(cap_slots, 1)]
    dl = np.asarray(dl, np.uint32)
    avgdl = searchsuite.avgdl_of(dl) if avgdl is None else avgdl
    cap_probes = probes_of(seg, phrases) if cap_probes is None else cap_probes
    n_q = len(phrases)
    I = {"term": G(seg.term), "docs": G(seg.docs), "tfs": G(seg.tfs), "first": G(seg.first), "ppos": G(seg.ppos), "dl": G(dl), "qoff": G(offsets),
         "qterms": G(terms), "qweights": G(np.asarray(weights, np.float32))}
    O = {"hd": G(np.full(n_q * k, SENTINEL, np.uint32)), "hs": G(np.full(n_q * k, SENTINEL, np.uint32)), "hf": G(np.full(n_q * k, SENTINEL, np.uint32)),
         "hc": G(np.full(n_q, SENTINEL, np.uint32)), "mc": G(np.full(n_q, SENTINEL, np.uint64)), "counts": G(np.full(3, SENTINEL, np.uint64))}
    r = Result()
    r.error = None
    try:
        batch.phrase_search_postings(I["term"].ptr, I["docs"].ptr, I["tfs"].ptr, I["first"].ptr, I["ppos"].ptr, seg.n_terms, seg.cap, seg.cap_pos, doc_base,
                                     len(dl) if n_docs is None else n_docs, I["dl"].ptr, I["qoff"].ptr, I["qterms"].ptr, I["qweights"].ptr, n_q, cap_slots,
                                     k1, b, avgdl, k, cap_probes, O["hd"].ptr, O["hs"].ptr, O["hf"].ptr if freqs else 0, O["hc"].ptr, O["mc"].ptr,
                                     O["counts"].ptr, devmem.stream())
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


def same_as(r, ref, freqs=True):
    """every output of a call that succeeded is the definition's, bits included, and nothing behind a query's hit count was touched"""
    assert r.error is None, r.error
    assert r.counts.tolist() == ref.counts, (r.counts.tolist(), ref.counts)
    assert r.mc.tolist() == ref.match_counts, (r.mc.tolist(), ref.match_counts)
    assert r.hc.tolist() == [min(r.k, m) for m in ref.match_counts]
    for q, hits in enumerate(ref.hits):
        a, n = q * r.k, len(hits)
        got = list(zip(r.hd[a:a + n].tolist(), r.hs[a:a + n].tolist(), r.hf[a:a + n].tolist() if freqs else [f for _, _, f in hits]))
        want = [(d, bits(s), f) for d, s, f in hits]
        assert got == want, (q, [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w][:4])
        assert (r.hd[a + n:a + r.k] == SENTINEL).all() and (r.hs[a + n:a + r.k] == SENTINEL).all() and (r.hf[a + n:a + r.k] == SENTINEL).all(), q
    if not freqs:
        assert (r.hf == SENTINEL).all()


def weights_of(docs, n_terms, phrases):
    """tantivy's phrase weight where every slot is a term, else a weight the device must not use"""
    df = np.zeros(n_terms, np.int64)
    for d in docs:
        for t in set(x for x in d if 0 <= x < n_terms):
            df[t] += 1
    out = []
    for ph in phrases:
        if ph and all(0 <= t < n_terms for t in ph):
            for t in ph:
                idf_of(len(docs), int(df[t]))   # (vpt_okapi_idf against the definition, on the way)
            out.append(phraseref.phrase_weight(len(docs), df, ph))
        else:
            out.append(F(1.5))
    return out


def check(docs, n_terms, doc_base, phrases, k, positions=None, dl=None, batch=None, extra=0, weights=None, k1=1.2, b=0.75):
    weights = weights_of(docs, n_terms, phrases) if weights is None else weights
    seg = pseg_of(docs, n_terms, doc_base, positions, extra)
    dl = [len(d) for d in docs] if dl is None else dl
    ref = phraseref.PhraseRef(docs, n_terms, doc_base, phrases, weights, k, positions, dl, k1, b)
    same_as(run(seg, doc_base, dl, phrases, weights, k, k1, b, batch=batch), ref)
    return ref


# ---- 2
def random_docs(seed, n_docs=40, alphabet=3, longest=24):
    rng = random.Random(seed)
    return [[rng.randrange(alphabet) for _ in range(0 if rng.random() < 0.1 else rng.randint(1, longest))] for _ in range(n_docs)]


def check_random(seed=7):
    """an alphabet of 3 terms on random documents: the seed yields documents that hold all terms of a phrase but no occurrence, pf of 1 and above
    1, and phrases that match nothing -- asserted of the input"""
    docs = random_docs(seed)
    rng = random.Random(seed + 1)
    phrases = [[rng.randrange(3) for _ in range(rng.randint(1, 5))] for _ in range(20)] + [[0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2], [2, 2, 2, 2, 2, 2, 2, 2]]
    batch = api.DeviceBatch(predictor())
    for doc_base in (0, 1000):
        for k in (1, 3, 50):
            ref = check(docs, 3, doc_base, phrases, k, batch=batch, extra=3)
    pfs = [n for per in ref.pf for n in per.values()]
    assert 1 in pfs and max(pfs) > 1 and 0 in ref.match_counts and max(ref.match_counts) > 3
    holds_all_without_occurrence = sum(1 for ph, per in zip(phrases, ref.pf) for d, ids in enumerate(docs)
                                       if len(ph) > 1 and set(ph) <= set(ids) and 1000 + d not in per)
    assert holds_all_without_occurrence > 10
    # the device-made segment: the postings pass and the positions call, searched
    toff, ids = csr(docs)
    r = run_positions(toff, ids, 3, batch=batch)
    n_post, n_idx = int(r.counts[0]), int(r.first[int(r.counts[0])])
    seg = PSeg(r.term, r.docs[:n_post], r.tfs[:n_post], r.first[:n_post + 1], r.ppos[:n_idx], extra=2)
    weights = weights_of(docs, 3, phrases)
    same_as(run(seg, 0, [len(d) for d in docs], phrases, weights, 3, batch=batch), phraseref.PhraseRef(docs, 3, 0, phrases, weights, 3))
    same_as(run(seg, 0, [len(d) for d in docs], phrases, weights, 3, batch=batch, freqs=False), phraseref.PhraseRef(docs, 3, 0, phrases, weights, 3),
            freqs=False)


# ---- 3
def check_repeats():
    a, b = 0, 1
    docs = [[a, a, a, a], [a, b, a, b, a], [b, a], [a], [b, b, a, a]]
    phrases = [[a, a], [a, b, a], [a, a, a, a, a], [b, a], [a, b]]
    ref = check(docs, 2, 0, phrases, 5)
    assert ref.pf[0] == {0: 3, 4: 1} and ref.pf[1] == {1: 2} and ref.pf[2] == {} and ref.pf[3] == {1: 2, 2: 1, 4: 1} and ref.pf[4] == {1: 2}
    # an anchor position smaller than its slot index: a negative start.  Term 2 is the rarest and stands at position 0 and 1 only
    docs = [[2, 0, 1], [0, 2, 1], [0, 1, 2], [1, 0, 1, 0, 1]]
    ref = check(docs, 3, 0, [[0, 1, 2], [0, 2], [1, 0, 2]], 4)
    assert ref.pf == [{2: 1}, {1: 1}, {}]


# ---- 4
def check_gaps():
    docs = [[0, 1, 2], [0, 1, 2], [1, 2, 0, 1]]
    positions = [[0, 2, 3], [0, 1, 2], [5, 6, 9, 10]]
    ref = check(docs, 3, 0, [[0, 1], [1, 2], [0, 1, 2], [2, 0]], 3, positions=positions)
    assert ref.pf == [{1: 1, 2: 1}, {0: 1, 1: 1, 2: 1}, {1: 1}, {}]


# ---- 5
def check_anchor_independence(seed=21):
    """the same phrases over the same first documents, with filler documents that make each term in turn the most frequent (so another slot is
    the rarest: the anchor): what the first documents score is told by the definition each time, and the pf of the first documents is the same"""
    core = random_docs(seed, 25, 3, 18)
    phrases = [[0, 1, 2], [2, 1, 0], [1, 1], [0, 2, 2, 1], [1, 0]]
    batch = api.DeviceBatch(predictor())
    seen = []
    anchors = set()
    fillers = ([], [[0] * 30, [1] * 30 + [0] * 7], [[1] * 30, [2] * 30 + [1] * 7], [[2] * 30, [0] * 30 + [2] * 7], [[0] * 40 + [2] * 39 + [1] * 38])
    for filler in fillers:
        docs = core + filler
        ref = check(docs, 3, 0, phrases, 40, batch=batch)
        seen.append([{d: n for d, n in per.items() if d < len(core)} for per in ref.pf])
        count = [sum(d.count(t) for d in docs) for t in range(3)]
        anchors.add(min(range(3), key=lambda j: (count[phrases[0][j]], j)))
    assert all(s == seen[0] for s in seen) and anchors == {0, 1, 2} and any(seen[0])
    # the corpus statistics held fixed -- the caller's weights, avgdl and doc_lens -- while the fillers move the anchor: what the first
    # documents get is then identical across the variants, score bits included
    weights, avgdl = [F(1.25), F(0.5), F(2), F(3.75), F(1)], F(11.5)
    kept, moved = [], [set() for _ in phrases]
    for filler in fillers:
        docs = core + filler
        dl = [len(d) for d in docs]
        ref = phraseref.PhraseRef(docs, 3, 0, phrases, weights, len(docs), dl=dl, avgdl=avgdl)
        r = run(pseg_of(docs, 3), 0, dl, phrases, weights, len(docs), avgdl=avgdl, batch=batch)
        same_as(r, ref)
        kept.append([[(int(r.hd[q * r.k + j]), int(r.hs[q * r.k + j]), int(r.hf[q * r.k + j])) for j in range(int(r.hc[q]))
                      if int(r.hd[q * r.k + j]) < len(core)] for q in range(len(phrases))])
        count = [sum(d.count(t) for d in docs) for t in range(3)]
        for q, ph in enumerate(phrases):
            moved[q].add(min(range(len(ph)), key=lambda j: (count[ph[j]], j)))
    assert all(x == kept[0] for x in kept) and sum(len(h) for h in kept[0]) > 20
    assert moved[0] == {0, 1, 2} and all(len(m) >= 2 for q, m in enumerate(moved) if len(set(phrases[q])) > 1), moved


# ---- 6
def check_or_equivalence(seed=5):
    """L = 1: the bits of vpt_postings_search_device for one slot of the same weight (and the definition's)"""
    docs = random_docs(seed, 30, 4, 20)
    phrases = [[0], [1], [2], [3]]
    weights = weights_of(docs, 4, phrases)
    seg = pseg_of(docs, 4, 9)
    dl = [len(d) for d in docs]
    batch = api.DeviceBatch(predictor())
    r = run(seg, 9, dl, phrases, weights, 30, batch=batch)
    same_as(r, phraseref.PhraseRef(docs, 4, 9, phrases, weights, 30))
    oseg = postingsmergesuite.Seg(seg.term, seg.docs[:seg.cap], seg.tfs[:seg.cap], seg.cap)
    o = searchsuite.run(oseg, 9, dl, [[(t, w)] for (t,), w in zip(phrases, weights)], 30, batch=batch)
    assert o.error is None and o.hd.tobytes() == r.hd.tobytes() and o.hs.tobytes() == r.hs.tobytes() and o.hc.tobytes() == r.hc.tobytes()
    assert o.mc.tobytes() == r.mc.tobytes() and int(r.mc.sum()) > 40


# ---- 7
def check_query_edges():
    limit = api.DeviceBatch.postings_phrase_limit()
    assert limit == 64
    docs = [[0, 1, 0, 1, 3], [1] * (limit + 3), [3, 0], []]
    n_terms = 5   # term 2, term 4: df 0
    longest = [1] * limit
    phrases = [[0, -1], [1, n_terms], [], [0, 1], [], [], [2], [0, 2], [3, 0], longest, [-(1 << 31)], [(1 << 31) - 1, 0], []]
    batch = api.DeviceBatch(predictor())
    ref = check(docs, n_terms, 0, phrases, 3, batch=batch, extra=2)
    assert ref.counts[2] == 4 and ref.pf[3] == {0: 2} and ref.pf[6] == ref.pf[7] == {} and ref.pf[8] == {2: 1} and ref.pf[9] == {1: 4}
    weights = weights_of(docs, n_terms, phrases)
    seg = pseg_of(docs, n_terms, extra=2)
    dl = [len(d) for d in docs]
    r = run(seg, 0, dl, phrases[:9] + [longest + [1]] + phrases[10:], weights, 3, batch=batch, cap_probes=64)
    assert r.error is not None and LONG_ERROR in r.error and r.untouched(), r.error
    check(docs, n_terms, 0, phrases, 3, batch=batch)   # the workspace takes the sound batch afterwards
    # capacity_slots above the slots; no slot at all
    full = phraseref.PhraseRef(docs, n_terms, 0, phrases, weights, 3)
    same_as(run(seg, 0, dl, phrases, weights, 3, cap_slots=sum(len(p) for p in phrases) + 100, batch=batch), full)
    none = phraseref.PhraseRef(docs, n_terms, 0, [[], []], [F(1), F(1)], 2)
    same_as(run(seg, 0, dl, [[], []], [F(1), F(1)], 2, batch=batch), none)
    assert none.counts == [0, 0, 0]


# ---- 8
def check_topk():
    same = [1, 2, 2, 0]
    docs = [[3, 3], same, [0], same, same, [1, 2, 1, 2], same, same, [2]]
    batch = api.DeviceBatch(predictor())
    for doc_base in (0, 7):
        for k in (2, 3, 5, 9):   # 2, 3: inside the group of five equal scores; 9: above the matches
            ref = check(docs, 4, doc_base, [[1, 2], [2, 2, 0], [3, 3, 3]], k, batch=batch)
            group = [doc_base + d for d in (1, 3, 4, 6, 7)]
            assert [d for d, _, _ in ref.hits[1]] == group[:k] and len({bits(s) for _, s, _ in ref.hits[1]}) == 1
            assert ref.match_counts == [6, 5, 0] and ref.hits[0][0][0] == doc_base + 5 and ref.hits[0][0][2] == 2


# ---- 9
def check_probes(n):
    """n probes: the anchor term has n tokens, some documents hold it several times; and n probes over two phrases"""
    rng = random.Random(n)
    docs, left = [], n
    while left:
        m = min(left, rng.choice([1, 1, 2, 3]))
        d = []
        for _ in range(m):
            d += [0] * rng.randint(1, 2) + [1] + [2] * rng.randint(0, 1)
        docs.append(d)
        left -= m
    assert sum(d.count(1) for d in docs) == n
    batch = api.DeviceBatch(predictor())
    k = len(docs) + 2
    ref = check(docs, 3, 0, [[0, 1]], k, batch=batch)
    assert ref.counts[0] == n and ref.counts[1] == len(docs)
    ref = check(docs, 3, 0, [[1, 2], [], [0, 1, 2]], 5, batch=batch)
    assert ref.counts[0] == sum(d.count(2) for d in docs) * 2 and ref.match_counts[0] > 5


# ---- 10
def check_capacity(seed=7):
    docs = random_docs(seed)
    phrases = [[0, 1], [2], [1, 1, 2], []]
    weights = weights_of(docs, 3, phrases)
    seg, dl = pseg_of(docs, 3, 5), [len(d) for d in docs]
    ref = phraseref.PhraseRef(docs, 3, 5, phrases, weights, 3)
    need = ref.counts[0]
    assert need == probes_of(seg, phrases) > 50
    batch = api.DeviceBatch(predictor())
    for cap in (need - 1, 0):
        r = run(seg, 5, dl, phrases, weights, 3, cap_probes=cap, batch=batch)
        assert r.error is not None and PROBES_ERROR in r.error, r.error
        assert int(r.counts[0]) == need and r.untouched()
    same_as(run(seg, 5, dl, phrases, weights, 3, cap_probes=need, batch=batch), ref)
    same_as(run(seg, 5, dl, phrases, weights, 3, cap_probes=need + tile() + 1, batch=batch), ref)


# ---- 11
def check_errors():
    pred = predictor()
    other = patterntagsuite.predictor_of(patterntagsuite.tagged_model())
    batch = api.DeviceBatch(pred)
    names = ("term", "docs", "tfs", "first", "ppos", "dl", "qoff", "qterms", "qweights", "hd", "hs", "hf", "hc", "mc", "counts")
    A = {n: devmem.zeros(8, np.uint64) for n in names}

    def call(b=batch, n_terms=2, cap_post=2, cap_pos=2, doc_base=0, n_docs=2, n_q=1, cap_slots=1, k1=1.2, bb=0.75, avgdl=1.0, k=2, cap_probes=2, **null):
        p = {n: (0 if n in null else a.ptr) for n, a in A.items()}
        b.phrase_search_postings(p["term"], p["docs"], p["tfs"], p["first"], p["ppos"], n_terms, cap_post, cap_pos, doc_base, n_docs, p["dl"], p["qoff"],
                                 p["qterms"], p["qweights"], n_q, cap_slots, k1, bb, avgdl, k, cap_probes, p["hd"], p["hs"], p["hf"], p["hc"], p["mc"],
                                 p["counts"], devmem.stream())

    for n in names:
        if n != "hf":
            _expect(lambda: call(**{n: 1}), "NULL device pointer")
    for v in (0, (1 << 24) + 1):
        _expect(lambda: call(n_terms=v), "n_terms: must be between 1 and 2\\^24")
        _expect(lambda: call(n_q=v), "n_queries: must be between 1 and 2\\^24")
    _expect(lambda: call(k=0), "k: must be at least 1")
    _expect(lambda: call(n_q=1 << 16, k=1 << 16), "n_queries \\* k below 2\\^32")
    _expect(lambda: call(cap_slots=1 << 32), "fewer than 2\\^32 slots and probes")
    _expect(lambda: call(cap_probes=1 << 32), "fewer than 2\\^32 slots and probes")
    _expect(lambda: call(doc_base=(1 << 32) - 1, n_docs=2), "doc_base \\+ n_documents must not exceed 2\\^32")
    _expect(lambda: call(doc_base=(1 << 32) + 1, n_docs=0), "doc_base \\+ n_documents must not exceed 2\\^32")
    for v in (-1.0, 65537.0, float("nan"), float("inf")):
        _expect(lambda: call(k1=v), "k1: must be between 0 and 65536")
    for v in (-0.1, 1.5, float("nan")):
        _expect(lambda: call(bb=v), "b: must be between 0 and 1")
    for v in (0.0, 2.0 ** -33, 2.0 ** 33, float("nan"), -1.0):
        _expect(lambda: call(avgdl=v), "avgdl: must be between 2\\^-32 and 2\\^32")
    _expect(lambda: call(b=_MismatchBatch(batch, other)), "batch: does not belong to this predictor")
    _expect(lambda: call(b=_MismatchBatch(api.DeviceBatch(other), pred)), "batch: does not belong to this predictor")
    assert _lib.load().vpt_postings_phrase_limits(None) == _lib.VPT_INVALID_ARGUMENT
    batch.sync()
    call(k1=65536.0, bb=1.0, avgdl=2.0 ** 32, hf=1)   # the ends of the ranges are inside; all-zero arrays: one query without a slot
    batch.sync()
    assert A["counts"].get(3).tolist() == [0, 0, 0] and int(A["mc"].get(1)[0]) == 0


class _MismatchBatch(api.DeviceBatch):
    def __init__(self, batch, pred):
        self._h, self._p, self._keep = batch._h, pred, batch

    def __del__(self):
        pass


# ---- 12
HOSTILE_DOCS = [[0, 3, 0], [1], [3, 0, 3, 3], [], [3, 3]]   # documents 10 .. 14; terms 0, 1, 3 (term 2: df 0)
HOSTILE_PHRASES = [[0, 3], [], [1], [3, 3]]


def hostile_cases():
    """name -> (change to the segment or None, phrases, query_offsets or None, weights or None, the message)"""
    w = [F(1.25), F(1), F(0.5), F(2)]
    cases = {}

    def seg_case(name, fn):
        cases[name] = (fn, HOSTILE_PHRASES, None, w, SEG_ERROR)
    # postings: term 0 {10, 12} at 0, 1; term 1 {11} at 2; term 3 {10, 12, 14} at 3, 4, 5; first 0 2 3 4 5 8 10
    seg_case("post_first_decrease", lambda s: s.first.__setitem__(4, 3))                     # posting 3 (term 3, document 10): [5, 3)
    seg_case("post_first_above_capacity_positions", lambda s: s.first.__setitem__(6, 13))    # the end of term 3's run
    seg_case("post_first_far_above", lambda s: s.first.__setitem__(slice(4, 7), [1 << 40, 1 << 62, (1 << 64) - 1]))
    seg_case("post_first_disagree_with_tfs", lambda s: s.tfs.__setitem__(0, 1))             # posting 0 holds 2 positions
    seg_case("document_below_doc_base", lambda s: s.docs.__setitem__(0, 9))
    seg_case("document_at_the_end", lambda s: s.docs.__setitem__(1, 15))
    seg_case("document_far_outside", lambda s: s.docs.__setitem__(2, 0xFFFFFFFF))
    seg_case("descending_term_offsets", lambda s: s.term.__setitem__(3, 7))                  # term 3: [7, 6)
    seg_case("term_bound_above_capacity", lambda s: s.term.__setitem__(4, 9))
    seg_case("huge_term_offsets", lambda s: s.term.__setitem__(slice(1, 5), [1 << 40, 1 << 41, 1 << 62, (1 << 64) - 1]))
    cases["descending_query_offsets"] = (None, HOSTILE_PHRASES, [0, 2, 1, 3, 5], w, QCSR_ERROR)
    cases["query_offsets_end_above_capacity_slots"] = (None, HOSTILE_PHRASES, [0, 2, 2, 3, 6], w, QCSR_ERROR)
    cases["query_offsets_far_above"] = (None, HOSTILE_PHRASES, [0, 2, 2, 1 << 63, (1 << 64) - 1], w, QCSR_ERROR)
    for name, bad in (("nan_weight", F("nan")), ("negative_weight", F(-1.0)), ("negative_zero_weight", F(-0.0)), ("infinite_weight", F("inf"))):
        cases[name] = (None, HOSTILE_PHRASES, None, [w[0], w[1], bad, w[3]], WEIGHT_ERROR)
    return w, cases


N_HOSTILE = 17


def run_hostile():
    w, cases = hostile_cases()
    assert len(cases) == N_HOSTILE
    dl = [len(d) for d in HOSTILE_DOCS]
    sound = pseg_of(HOSTILE_DOCS, 4, 10, extra=2)
    assert sound.first[:7].tolist() == [0, 2, 3, 4, 5, 8, 10] and sound.cap_pos == 12 and sound.term.tolist() == [0, 2, 3, 3, 6]
    ref = phraseref.PhraseRef(HOSTILE_DOCS, 4, 10, HOSTILE_PHRASES, w, 3)
    assert ref.match_counts == [2, 0, 1, 2]
    batch = api.DeviceBatch(predictor())
    ran = 0
    for name, (change, phrases, qoff, weights, message) in cases.items():
        seg = pseg_of(HOSTILE_DOCS, 4, 10, extra=2)
        if change:
            change(seg)
        r = run(seg, 10, dl, phrases, weights, 3, cap_probes=16, qoff=qoff, batch=batch)
        assert r.error is not None and message in r.error, (name, r.error)
        assert r.untouched(), name
        same_as(run(sound, 10, dl, HOSTILE_PHRASES, w, 3, batch=batch), ref)   # the sound ones on the same workspace
        ran += 1
    # hostile token CSRs under the positions call: the id pass's message
    toff, ids = csr(HOSTILE_DOCS)
    n = len(ids)
    for bad in ([0, 3, 2, 8, 8, n], [0, 3, 4, 8, 8, n + 1000], [2, 3, 4, 8, 8, n], [0, 1 << 40, 1 << 41, 1 << 62, 1 << 63, (1 << 64) - 1]):
        r = run_positions(toff, ids, 4, batch=batch, toff_for_positions=bad)
        assert r.error is not None and CSR_ERROR in r.error, (bad, r.error)
    # unsorted positions with the search alone: it returns without touching a guard; the result is not compared
    seg = pseg_of(HOSTILE_DOCS, 4, 10, positions=[[5, 1, 0], [3], [9, 2, 7, 1], [], [4, 0]], extra=2)
    r = run(seg, 10, dl, HOSTILE_PHRASES, w, 3, batch=batch)
    assert r.error is None, r.error
    same_as(run(sound, 10, dl, HOSTILE_PHRASES, w, 3, batch=batch), ref)
    del batch
    return ran


# ---- 14
def check_determinism(seed=12):
    rng = random.Random(seed)
    T = tile()
    docs = [[postingssuite.zipf(rng, 6) for _ in range(rng.randint(0, 30))] for _ in range(3 * T // 32)]
    phrases = [[rng.randrange(6) for _ in range(rng.randint(0, 4))] for _ in range(23)]
    weights = weights_of(docs, 6, phrases)
    seg, dl = pseg_of(docs, 6), [len(d) for d in docs]
    pred = predictor()
    one, two = api.DeviceBatch(pred), api.DeviceBatch(pred)
    a = run(seg, 0, dl, phrases, weights, 10, batch=one)
    b = run(seg, 0, dl, phrases, weights, 10, batch=one)
    run(pseg_of([[1, 2, 1]], 4), 0, [3], [[1, 2]], [F(1)], 1, batch=two)   # (the second workspace's scratch holds something else)
    c = run(seg, 0, dl, phrases, weights, 10, batch=two)
    assert a.error is None and a.same_bytes(b) and a.same_bytes(c)
    ref = phraseref.PhraseRef(docs, 6, 0, phrases, weights, 10)
    assert T < ref.counts[0] <= 3 * T + 1, ref.counts
    same_as(a, ref)


# ---- 15
def check_host_call(seed=5):
    """vpt_postings_phrase_search through Postings.phrase_search: host arrays in and out, the default weights and the caller's"""
    docs = random_docs(seed, 50, 4, 30)
    pred = predictor()
    post = pseg_of(docs, 4, 100).postings()
    dl = np.array([len(d) for d in docs], np.uint32)
    rng = random.Random(seed)
    phrases = [[rng.randrange(4) for _ in range(rng.randint(1, 4))] for _ in range(9)] + [[], [-1, 2], [4]]
    weights = weights_of(docs, 4, phrases)
    weights = [w if ph and all(0 <= t < 4 for t in ph) else F(0) for w, ph in zip(weights, phrases)]   # (the wrapper's default for those)
    weights[10] = phraseref.phrase_weight(len(docs), post.df(), [2])   # (the wrapper sums the slots that are terms)
    for k in (1, 5, 60):
        ref = phraseref.PhraseRef(docs, 4, 100, phrases, weights, k)
        hits, mc = post.phrase_search(phrases, k, dl, 100, predictor=pred)
        assert [[(d, bits(s), f) for d, s, f in h] for h in hits] == [[(d, bits(s), f) for d, s, f in h] for h in ref.hits]
        assert all(type(s) is np.float32 for h in hits for _, s, _ in h) and mc.tolist() == ref.match_counts
        assert post.last_search_counts.tolist() == ref.counts
    mine = [F(0.25 + j) for j in range(len(phrases))]
    ref = phraseref.PhraseRef(docs, 4, 100, phrases, mine, 4, k1=0.9, b=0.4)
    hits, mc = post.phrase_search(phrases, 4, dl, 100, 0.9, 0.4, weights=mine, predictor=pred)
    assert [[(d, bits(s), f) for d, s, f in h] for h in hits] == [[(d, bits(s), f) for d, s, f in h] for h in ref.hits]
    _expect(lambda: post.phrase_search(phrases, 4, dl, 100), "phrase_search: no predictor")
    _expect(lambda: post.phrase_search(phrases, 4, predictor=pred), "phrase_search: the postings carry no doc_lens / doc_base")
    _expect(lambda: post.phrase_search(phrases, 0, dl, 100, predictor=pred), "k: must be at least 1")
    _expect(lambda: post.phrase_search(phrases, 4, dl, 100, weights=[F(-1)] * len(phrases), predictor=pred), WEIGHT_ERROR)
    _expect(lambda: post.phrase_search([[0] * 65], 4, dl, 100, predictor=pred), LONG_ERROR)
    bare = api.Postings(post.term_offsets, post.docs, post.tfs, None, None, 0)
    _expect(lambda: bare.phrase_search(phrases, 4, dl, 100, predictor=pred), "made without positions")
    assert bare.positions is None and post.phrase_search([], 4, dl, 100, predictor=pred)[0] == []
    if not devmem.EMULATED:   # Predictor.postings_packed uploads with torch
        toff, ids = csr(docs)
        packed = pred.postings_packed(toff, ids, 4, 100, positions=True)
        assert np.array_equal(packed.positions, post.positions) and packed.positions.dtype == np.uint32 and np.array_equal(packed.first, post.first)
        assert pred.postings_packed(toff, ids, 4, 100).positions is None
        gaps = gapped(random.Random(3), docs)
        packed = pred.postings_packed(toff, ids, 4, 100, positions=True, token_positions=flat_positions(docs, gaps))
        assert np.array_equal(packed.positions, pseg_of(docs, 4, 100, gaps).postings().positions)


# ---- 16
def hits_of(ref):
    return {d for h in ref.hits for d, _, _ in h}


def check_high_documents(name, hostile=True):
    """the corpora of check_random and check_topk at a doc_base of postingssuite.HIGH_BASES: documents on both sides of 2^31, or the last
    document 0xFFFFFFFF; at the upper base the two hostile postings too (hostile=False where they run in a process of their own)"""
    batch = api.DeviceBatch(predictor())
    docs = random_docs(7)
    rng = random.Random(8)
    phrases = [[rng.randrange(3) for _ in range(rng.randint(1, 5))] for _ in range(20)] + [[0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2], [2, 2, 2, 2, 2, 2, 2, 2]]
    doc_base = postingssuite.high_base(name, len(docs))
    last = doc_base + len(docs) - 1
    for k in (1, 3, 50):
        ref = check(docs, 3, doc_base, phrases, k, batch=batch, extra=3)
    assert max(ref.match_counts) < 50 and {doc_base, last} <= hits_of(ref) and last >= 1 << 31   # (k = 50: every match is a hit)
    assert (doc_base < 1 << 31) == (name == "2^31-3") and (last == 0xFFFFFFFF) == (name == "2^32-n")
    same = [1, 2, 2, 0]
    docs = [[3, 3], same, [0], same, same, [1, 2, 1, 2], same, same, [2]]
    doc_base = postingssuite.high_base(name, len(docs))
    for k in (2, 5):   # 2: inside the group of five equal scores, which stands on both sides of 2^31 at the lower base
        ref = check(docs, 4, doc_base, [[1, 2], [2, 2, 0], [3, 3, 3]], k, batch=batch)
        group = [doc_base + d for d in (1, 3, 4, 6, 7)]
        assert [d for d, _, _ in ref.hits[1]] == group[:k] and len({bits(s) for _, s, _ in ref.hits[1]}) == 1
        assert ref.match_counts == [6, 5, 0] and ref.hits[0][0][0] == doc_base + 5 and ref.hits[0][0][2] == 2
    assert group[-1] >= 1 << 31 and (group[0] < 1 << 31) == (name == "2^31-3")
    if hostile and name == "2^32-n":
        assert run_hostile_high(batch) == N_HOSTILE_HIGH


N_HOSTILE_HIGH = 2


def run_hostile_high(batch=None):
    """HOSTILE_DOCS as the documents 2^32 - 5 .. 2^32 - 1, and one posting outside them: the first of term 0's list, the anchor of the phrase
    [0, 3], so the list's own order is sound and only the range check can see it"""
    B = (1 << 32) - len(HOSTILE_DOCS)
    w = [F(1.25), F(1), F(0.5), F(2)]
    dl = [len(d) for d in HOSTILE_DOCS]
    sound = pseg_of(HOSTILE_DOCS, 4, B, extra=2)
    assert sound.docs[:6].tolist() == [B, B + 2, B + 1, B, B + 2, B + 4] and B + 4 == 0xFFFFFFFF
    ref = phraseref.PhraseRef(HOSTILE_DOCS, 4, B, HOSTILE_PHRASES, w, 3)
    assert ref.match_counts == [2, 0, 1, 2] and 0xFFFFFFFF in hits_of(ref)
    cases = {"document_below_doc_base": B - 1, "document_at_the_end_wrapped_to_zero": (B + len(HOSTILE_DOCS) - 1 + 1) & 0xFFFFFFFF}
    assert len(cases) == N_HOSTILE_HIGH and cases["document_at_the_end_wrapped_to_zero"] == 0
    batch = batch or api.DeviceBatch(predictor())
    ran = 0
    for name, d in cases.items():
        seg = pseg_of(HOSTILE_DOCS, 4, B, extra=2)
        seg.docs[0] = d
        r = run(seg, B, dl, HOSTILE_PHRASES, w, 3, cap_probes=16, batch=batch)
        assert r.error is not None and SEG_ERROR in r.error, (name, r.error)
        assert r.untouched(), name
        same_as(run(sound, B, dl, HOSTILE_PHRASES, w, 3, batch=batch), ref)   # the sound ones on the same workspace
        ran += 1
    return ran


# ---- 17
def check_tile_edge_ties(n):
    """n documents of six tokens that all hold the phrase [0, 1] once: n probes and n equal scores, a tie group over the records 0 .. n - 1 that
    k cuts at 1, T - 1, T and n; seven of the documents hold [2, 3] twice, another score.  Then two phrases over corpora in which term 1, the
    anchor of [0, 1], has T - 1, T and T + 1 tokens: the probes of [2, 3] start on record T - 1, T and T + 1.  (2 T + 1 probes: inside the
    suite's cap of 3 T + 1 for a case, so no size is dropped.)"""
    T = tile()
    assert T <= n <= 3 * T + 1
    batch = api.DeviceBatch(predictor())
    doc_base = 5
    seven = [(j * (n - 1)) // 6 for j in range(7)]   # the first and the last document among them
    plain, twice = [0, 1, 4, 4, 4, 4], [0, 1, 2, 3, 2, 3]
    docs = [twice if d in seven else plain for d in range(n)]
    weights = [F(1.25), F(0.75)]
    # what the input has to be, by the definition alone and before any device call
    whole = phraseref.PhraseRef(docs, 5, doc_base, [[0, 1]], weights[:1], n)
    other = phraseref.PhraseRef(docs, 5, doc_base, [[2, 3]], weights[1:], n)
    assert len(set(seven)) == 7 and whole.counts == [n, n, 0] and other.counts == [14, 7, 0]
    assert len({bits(s) for _, s, _ in whole.hits[0]}) == 1 and {f for _, _, f in whole.hits[0]} == {1} and {f for _, _, f in other.hits[0]} == {2}
    assert not {bits(s) for _, s, _ in whole.hits[0]} & {bits(s) for _, s, _ in other.hits[0]}
    pairs = []
    for c in (T - 1, T, T + 1):
        m = min(c, n)   # the documents that hold [0, 1]; a probe more than there are documents: the second one holds it twice
        cdocs = [([0, 1, 0, 1, 4, 4] if d == 1 and c > n else [0, 1, 4, 4, 4, 4]) if d < m else [0, 4, 4, 4, 4, 4] for d in range(n)]
        assert 1 not in seven
        for d in seven:
            cdocs[d] = cdocs[d][:2] + [2, 3, 2, 3]
        seg = pseg_of(cdocs, 5, doc_base)
        assert probes_of(seg, [[0, 1]]) == c and probes_of(seg, [[0, 1], [2, 3]]) == c + 14 and sum(d.count(1) for d in cdocs) == c   # the phrase changes on record c
        pairs.append((c, cdocs, seg))
    seg = pseg_of(docs, 5, doc_base, extra=1)
    dl = [6] * n
    for k in (1, T - 1, T, n):
        r = run(seg, doc_base, dl, [[0, 1]], weights[:1], k, batch=batch)
        same_as(r, searchsuite.cut(whole, k))   # (the reference is computed once)
        m = min(k, n)
        assert r.hd[:m].tolist() == list(range(doc_base, doc_base + m)) and len(set(r.hs[:m].tolist())) == 1 and set(r.hf[:m].tolist()) == {1}
        assert r.mc.tolist() == [n] and r.counts.tolist() == [n, n, 0]
    for c, cdocs, cseg in pairs:
        ref = phraseref.PhraseRef(cdocs, 5, doc_base, [[0, 1], [2, 3]], weights, 9)
        r = run(cseg, doc_base, dl, [[0, 1], [2, 3]], weights, 9, batch=batch)
        same_as(r, ref)
        assert int(r.counts[0]) == c + 14 and r.mc.tolist() == [min(c, n), 7] and r.hd[9:16].tolist() == [doc_base + d for d in seven]
        assert len(set(r.hs[9:16].tolist())) == 1 and sorted(r.hd[:9].tolist()) == list(range(doc_base, doc_base + 9))


PHRASE_TEXTS = ["火星猫", "東京特許許可局", "", "火星猫は東京だ", "まぁ良いだろう", "だだだ", "猫は東京", "１２３４５６円"]


def check_tokenizer():
    """index_batch(positions=True) and VaporettoTokenizer.phrase_search on the fixture model against the definition over the encoded ids"""
    tok, texts = searchsuite.fixture_tokenizer()
    toff, ids = tok.encode_batch(texts)
    docs = [ids[int(toff[i]):int(toff[i + 1])].tolist() for i in range(len(texts))]
    qoff, qids = tok.encode_batch(PHRASE_TEXTS)
    phrases = [qids[int(qoff[i]):int(qoff[i + 1])].tolist() for i in range(len(PHRASE_TEXTS))]
    for doc_base in (0, 1000):
        post = tok.index_batch(texts, doc_base, positions=True)
        plain = tok.index_batch(texts, doc_base)
        assert postingssuite.same_postings(post, plain) and plain.positions is None and plain.first is None and post.order is None
        n_terms = len(post.term_offsets) - 1
        want = pseg_of(docs, n_terms, doc_base).postings()
        assert np.array_equal(post.first, want.first) and np.array_equal(post.positions, want.positions) and post.positions.dtype == np.uint32
        assert np.array_equal(post.doc_lens, [len(d) for d in docs]) and post.doc_base == doc_base
        df = post.df()
        weights = [phraseref.phrase_weight(len(texts), df, [t for t in ph if 0 <= t < n_terms]) for ph in phrases]
        assert any(not 0 <= t < n_terms for ph in phrases for t in ph) and sum(1 for ph in phrases if len(ph) > 2) >= 3
        for k in (1, 10):
            ref = phraseref.PhraseRef(docs, n_terms, doc_base, phrases, weights, k)
            hits, mc = tok.phrase_search(post, PHRASE_TEXTS, k)
            assert mc.tolist() == ref.match_counts and mc.dtype == np.uint64
            assert [[(d, bits(s), f) for d, s, f in h] for h in hits] == [[(d, bits(s), f) for d, s, f in h] for h in ref.hits]
            assert post.last_search_counts.tolist() == ref.counts
        multi = [m for ph, m in zip(phrases, ref.match_counts) if len(ph) > 1 and all(0 <= t < n_terms for t in ph)]
        assert multi and max(multi) > 3 and ref.match_counts[2] == 0 and ref.counts[2] >= 1
        _expect(lambda: tok.phrase_search(plain, PHRASE_TEXTS, 3), "made without positions")
    merged = api.Postings.merge([post, post], predictor=tok.predictor)
    assert merged.positions is None


def example_lines(docs, n_terms, doc_base, phrase, weight, k):
    """the lines examples/token_stream.cpp --postings --phrase prints for these hits"""
    ref = phraseref.PhraseRef(docs, n_terms, doc_base, [phrase], [weight], k)
    return ["%d\t%08x\t%.9g\t%d" % (d, bits(s), float(s), f) for d, s, f in ref.hits[0]], ref


def main(argv):
    assert argv in (["--emu-hostile"], ["--emu-hostile-high"]), "usage: python -m tests.phrasesuite --emu-hostile | --emu-hostile-high"
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
