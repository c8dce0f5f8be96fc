"""The definition of the BM25 top-k search over a postings segment (vpt_postings_search_device, include/vaporetto_hip.h) in plain Python: every
float is a numpy.float32 scalar, one operation per statement in the header's order, the contributions of a (query, document) added in slot
order starting from the first, and sorted(key=(-score, document)).  tests/searchsuite.py compares the device's documents, counts and score
BITS with this and with nothing else."""
import math

import numpy as np

F = np.float32


def contribution(w, tf, dl, k1, b, avgdl):
    """c of one slot (weight w) and one posting (tf) of a document of length dl"""
    w, k1, b, avgdl = F(w), F(k1), F(b), F(avgdl)
    r = F(dl) / avgdl
    br = b * r
    nb = F(1.0) - b
    norm = nb + br
    K = k1 * norm
    f = F(tf)
    k11 = k1 + F(1.0)
    num = f * k11
    den = f + K
    q = num / den
    c = w * q
    assert all(type(x) is np.float32 for x in (r, br, nb, norm, K, f, k11, num, den, q, c))
    return c


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def idf(n_documents, df):
    return F(math.log(1.0 + (float(n_documents - df) + 0.5) / (float(df) + 0.5)))


class SearchRef:
    """term_offsets / docs / tfs: the segment (host arrays); dl: the lengths of the documents doc_base ..; queries: lists of (term, weight).
    -> contributions[q] {document: [c in slot order]}, hits[q] [(document, score)] the best k, match_counts, counts [candidates, matches,
    skipped slots]"""

    def __init__(self, term_offsets, docs, tfs, doc_base, dl, queries, k, k1=1.2, b=0.75, avgdl=None):
        n_terms = len(term_offsets) - 1
        self.avgdl = F(float(sum(int(x) for x in dl)) / float(len(dl))) if avgdl is None else F(avgdl)
        self.k = k
        self.contributions, self.scores, self.hits, self.match_counts = [], [], [], []
        n_cand = n_skip = 0
        with np.errstate(over="ignore"):
            for query in queries:
                per_doc = {}
                for term, w in query:
                    if not 0 <= term < n_terms:
                        n_skip += 1
                        continue
                    for at in range(int(term_offsets[term]), int(term_offsets[term + 1])):
                        d, tf = int(docs[at]), int(tfs[at])
                        n_cand += 1
                        per_doc.setdefault(d, []).append(contribution(w, tf, int(dl[d - doc_base]), k1, b, self.avgdl))
                scored = {}
                for d, cs in per_doc.items():
                    s = cs[0]
                    for c in cs[1:]:
                        s = s + c
                    assert type(s) is np.float32
                    scored[d] = s
                ranked = sorted(scored.items(), key=lambda x: (-float(x[1]), x[0]))
                self.contributions.append(per_doc)
                self.scores.append(scored)
                self.hits.append(ranked[:k])
                self.match_counts.append(len(ranked))
        self.counts = [n_cand, sum(self.match_counts), n_skip]

    def order_matters(self):
        """the (query, document) pairs with three or more contributions whose float32 sum has other bits under another order of the slots"""
        import itertools
        found = []
        for q, per_doc in enumerate(self.contributions):
            for d, cs in per_doc.items():
                if len(cs) < 3:
                    continue
                want = bits(self.scores[q][d])
                for perm in itertools.permutations(cs[:6]):
                    s = perm[0]
                    for c in list(perm[1:]) + cs[6:]:
                        s = s + c
                    if bits(s) != want:
                        found.append((q, d))
                        break
        return found
