"""The definition of the exact-phrase BM25 top-k search (vpt_postings_phrase_search_device, include/vaporetto_hip.h) in plain Python, straight
from the documents' id sequences and positions: no postings -- for each document and each start the ids are compared.  The score is
tests/searchref.py's term function (numpy.float32, one operation per statement) with f = float(pf) and the phrase's weight; hits are
sorted(key=(-score, document)).  tests/phrasesuite.py compares the device's documents, score BITS, frequencies and counts with this and with
nothing else."""
import numpy as np

from tests.searchref import bits, contribution, idf   # noqa: F401  (bits, idf: for the suite)

F = np.float32


def default_positions(docs):
    return [list(range(len(d))) for d in docs]


def occurrences(ids, positions, phrase, n_terms):
    """the distinct starts of `phrase` in one document: tokens (id, position), only ids inside [0, n_terms) are indexed"""
    at = {}
    for t, p in zip(ids, positions):
        if 0 <= t < n_terms:
            at.setdefault(int(p), set()).add(int(t))
    return sorted(s for s in at if all(phrase[j] in at.get(s + j, ()) for j in range(len(phrase))))


def phrase_weight(n_documents, df, phrase):
    """tantivy's phrase weight: the binary32 sum, in slot order, of the idf of every slot's term"""
    total = None
    for t in phrase:
        w = idf(n_documents, int(df[t]))
        total = w if total is None else total + w
        assert type(total) is np.float32
    return F(0) if total is None else total


class PhraseRef:
    """docs: lists of ids; positions: lists of positions (default 0, 1, ..); dl: the documents' lengths (default their token counts);
    phrases: lists of term ids; weights: one per phrase.  -> pf[q] {document: pf}, hits[q] [(document, score, pf)] the best k, match_counts,
    counts [probes, matches, skipped queries] -- probes: per phrase that can match, the indexed tokens of its rarest term."""

    def __init__(self, docs, n_terms, doc_base, phrases, weights, k, positions=None, dl=None, k1=1.2, b=0.75, avgdl=None, max_terms=64):
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
        assert all(len(p) <= max_terms for p in phrases)
        for phrase, w in zip(phrases, weights):
            phrase = [int(t) for t in phrase]
            per_doc = {}
            if any(not 0 <= t < n_terms for t in phrase):
                n_skip += 1
            elif phrase and all(tokens.get(t, 0) for t in phrase):
                n_probes += min(tokens[t] for t in phrase)
                for d, (ids, pos) in enumerate(zip(docs, positions)):
                    n = len(occurrences(ids, pos, phrase, n_terms))
                    if n:
                        per_doc[doc_base + d] = n
            scored = [(d, contribution(w, n, dl[d - doc_base], k1, b, self.avgdl), n) for d, n in per_doc.items()]
            ranked = sorted(scored, key=lambda x: (-float(x[1]), x[0]))
            self.pf.append(per_doc)
            self.hits.append(ranked[:k])
            self.match_counts.append(len(ranked))
        self.counts = [n_probes, sum(self.match_counts), n_skip]
