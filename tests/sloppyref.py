"""The definition of the sloppy phrase search (vpt_postings_sloppy_phrase_search_device, include/vaporetto_hip.h) in plain Python, straight from
the documents' id and position sequences: no postings and no masks.  For slot j the ADJUSTED positions of a document are p - j over its tokens
(id, p) with id == phrase[j]; an integer s is an OCCURRENCE when every slot has an adjusted position in [s, s + slop] and some slot has s
itself; pf = the distinct occurrences.  `occurrences` checks that literally for every candidate s = p - j over the document's tokens;
`occurrences_by_tuples` is the other wording -- one position chosen per slot, the choice matches when max(p_j - j) - min(p_j - j) <= slop, the
occurrences are the distinct minima -- by enumerating the choices, for documents of at most 8 tokens.  The score is tests/searchref.py's term
function with f = float(pf) and the phrase's weight; hits are sorted(key=(-score, document)), as tests/phraseref.py does it.
tests/sloppysuite.py compares the device's documents, score BITS, frequencies and counts with this and with nothing else."""
import itertools

import numpy as np

from tests.phraseref import default_positions, phrase_weight   # noqa: F401  (for the suite)
from tests.searchref import bits, contribution   # noqa: F401

F = np.float32
PF_MAX = (1 << 32) - 1


def adjusted(ids, positions, phrase, n_terms):
    """per slot the set of adjusted positions p - j of the document's indexed tokens of that slot's term"""
    return [{int(p) - j for t, p in zip(ids, positions) if 0 <= t < n_terms and int(t) == term} for j, term in enumerate(phrase)]


def occurrences(ids, positions, phrase, n_terms, slop):
    """the distinct occurrences of `phrase` in one document, ascending: the definition, literally"""
    if not phrase:
        return []
    adj = adjusted(ids, positions, phrase, n_terms)
    candidates = {int(p) - j for p in positions for j in range(len(phrase))}
    out = []
    for s in sorted(candidates):
        every = all(any(s <= a <= s + slop for a in slot) for slot in adj)
        some = any(s in slot for slot in adj)
        if every and some:
            out.append(s)
    return out


def occurrences_by_tuples(ids, positions, phrase, n_terms, slop):
    """the same set as the distinct minima of the matching choices of one position per slot; small documents only"""
    assert len(ids) <= 8
    if not phrase:
        return []
    adj = adjusted(ids, positions, phrase, n_terms)
    found = set()
    for choice in itertools.product(*[sorted(slot) for slot in adj]):
        if max(choice) - min(choice) <= slop:
            found.add(min(choice))
    return sorted(found)


class SloppyRef:
    """docs: lists of ids; positions: lists of positions (default 0, 1, ..); dl: the documents' lengths (default their token counts); phrases:
    lists of term ids; weights: one per phrase; slops: one per phrase.  -> pf[q] {document: pf}, hits[q] [(document, score, pf)] the best k,
    match_counts, counts [probes, matches, skipped queries] -- probes: per phrase that can match, the indexed tokens of its rarest term."""

    def __init__(self, docs, n_terms, doc_base, phrases, weights, slops, k, positions=None, dl=None, k1=1.2, b=0.75, avgdl=None, max_terms=64,
                 max_slop=31):
        positions = default_positions(docs) if positions is None else positions
        dl = [len(d) for d in docs] if dl is None else [int(x) for x in dl]
        self.avgdl = F(float(sum(dl)) / float(len(dl))) if avgdl is None else F(avgdl)
        tokens = {}
        for d in docs:
            for t in d:
                if 0 <= t < n_terms:
                    tokens[t] = tokens.get(t, 0) + 1
        self.pf, self.hits, self.match_counts = [], [], []
        n_probes = n_skip = 0
        assert all(len(p) <= max_terms for p in phrases) and all(0 <= s <= max_slop for s in slops) and len(slops) == len(phrases)
        for phrase, w, slop in zip(phrases, weights, slops):
            phrase = [int(t) for t in phrase]
            per_doc = {}
            if any(not 0 <= t < n_terms for t in phrase):
                n_skip += 1
            elif phrase and all(tokens.get(t, 0) for t in phrase):
                n_probes += min(tokens[t] for t in phrase)
                for d, (ids, pos) in enumerate(zip(docs, positions)):
                    n = min(len(occurrences(ids, pos, phrase, n_terms, int(slop))), PF_MAX)
                    if n:
                        per_doc[doc_base + d] = n
            scored = [(d, contribution(w, n, dl[d - doc_base], k1, b, self.avgdl), n) for d, n in per_doc.items()]
            ranked = sorted(scored, key=lambda x: (-float(x[1]), x[0]))
            self.pf.append(per_doc)
            self.hits.append(ranked[:k])
            self.match_counts.append(len(ranked))
        self.counts = [n_probes, sum(self.match_counts), n_skip]

    def lists(self):
        """what the lists call writes: offsets, documents (ascending per phrase), pf"""
        off, docs, tfs = [0], [], []
        for per in self.pf:
            for d in sorted(per):
                docs.append(d)
                tfs.append(per[d])
            off.append(len(docs))
        return off, docs, tfs
