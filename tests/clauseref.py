"""The definition of the phrase lists and of the clause search (vpt_postings_phrase_lists_device, vpt_postings_clause_search_device,
vpt_postings_clause_search; include/vaporetto_hip.h) in plain Python, composed from the two definitions it joins: a phrase's list is
tests/phraseref.py's pf per document, straight from the documents' id sequences; the derived lists stand behind the segment's own lists as
terms n_terms, n_terms + 1, .. and tests/boolref.py's rule and sum run over the two together.  tests/clausesuite.py compares the device's
documents, counts and score BITS with this and with nothing else."""
import numpy as np

from tests import boolref, phraseref

F = np.float32
SHOULD, MUST, MUST_NOT = boolref.SHOULD, boolref.MUST, boolref.MUST_NOT


def term_lists(docs, n_terms, doc_base):
    """the segment's own lists by the definition of the postings pass: per term [(document, tf)], ascending"""
    lists = [{} for _ in range(n_terms)]
    for d, ids in enumerate(docs):
        for t in ids:
            if 0 <= t < n_terms:
                lists[t][doc_base + d] = lists[t].get(doc_base + d, 0) + 1
    return [sorted(x.items()) for x in lists]


class ListsRef:
    """phrases: lists of term ids.  -> lists[q] [(document, pf)] ascending, offsets, docs, tfs (the three arrays), counts [probes, entries,
    skipped phrases], bound: the sum over the phrases of the smallest df among their terms (what always suffices as capacity_lists)"""

    def __init__(self, docs, n_terms, doc_base, phrases, positions=None):
        ref = phraseref.PhraseRef(docs, n_terms, doc_base, phrases, [F(0)] * len(phrases), 1, positions)
        self.lists = [sorted(pf.items()) for pf in ref.pf]
        self.offsets = [0]
        for x in self.lists:
            self.offsets.append(self.offsets[-1] + len(x))
        self.docs = [d for x in self.lists for d, _ in x]
        self.tfs = [f for x in self.lists for _, f in x]
        assert all(f >= 1 for f in self.tfs)
        self.counts = [ref.counts[0], len(self.docs), ref.counts[2]]
        own = term_lists(docs, n_terms, doc_base)
        self.bound = sum(min(len(own[t]) for t in ph) if ph and all(0 <= t < n_terms for t in ph) else 0 for ph in phrases)
        assert all(len(x) <= (min(len(own[t]) for t in ph) if ph and all(0 <= t < n_terms for t in ph) else 0) for x, ph in zip(self.lists, phrases))


class ClauseRef(boolref.BoolRef):
    """queries: lists of slots (term, occur, weight); a term t in [n_terms, n_terms + len(lists)) names lists[t - n_terms], a list of
    (document, tf) pairs.  Everything boolref.BoolRef gives, over the segment's own lists and the derived ones."""

    def __init__(self, docs, n_terms, doc_base, lists, queries, k, dl=None, k1=1.2, b=0.75, avgdl=None):
        both = term_lists(docs, n_terms, doc_base) + [list(x) for x in lists]
        offsets = [0]
        for x in both:
            offsets.append(offsets[-1] + len(x))
        dl = [len(d) for d in docs] if dl is None else dl
        super().__init__(offsets, [d for x in both for d, _ in x], [f for x in both for _, f in x], doc_base, dl, queries, k, k1, b, avgdl)


def slots_of(n_terms, queries):
    """the host call's rule: queries of clauses (terms, occur, weight) -> (phrases, queries of slots, the phrases with a term out of range).
    A clause of one term is a slot of that term (out of range: -1); every other clause is a phrase and its slot names the phrase's list"""
    phrases, out, skipped = [], [], 0
    for q in queries:
        slots = []
        for terms, occur, weight in q:
            terms = [int(t) for t in terms]
            if len(terms) == 1:
                slots.append((terms[0] if 0 <= terms[0] < n_terms else -1, occur, weight))
                continue
            skipped += 1 if any(not 0 <= t < n_terms for t in terms) else 0
            slots.append((n_terms + len(phrases), occur, weight))
            phrases.append(terms)
        out.append(slots)
    return phrases, out, skipped


def of_clauses(docs, n_terms, doc_base, queries, k, positions=None, dl=None, k1=1.2, b=0.75):
    """vpt_postings_clause_search's result for queries of clauses: the ClauseRef over the lists of its phrases, counts[2] with the phrases
    that have a term out of range"""
    phrases, slots, skipped = slots_of(n_terms, queries)
    lists = ListsRef(docs, n_terms, doc_base, phrases, positions).lists if phrases else []
    ref = ClauseRef(docs, n_terms, doc_base, lists, slots, k, dl, k1, b)
    ref.counts[2] += skipped
    return ref
