"""The definition of the BM25 top-k search with MUST / SHOULD / MUST_NOT slots (vpt_postings_boolean_search_device, include/vaporetto_hip.h) in
plain Python: every float is a numpy.float32 scalar, one operation per statement, a slot's c is tests/searchref.py's `contribution`, the c
values of a matching document are added in slot order starting from the first, and sorted(key=(-score, document)).  tests/boolsuite.py compares
the device's documents, counts and score BITS with this."""
import itertools

import numpy as np

from tests.searchref import bits, contribution

F = np.float32
SHOULD, MUST, MUST_NOT = 0, 1, 2


class BoolRef:
    """term_offsets / docs / tfs: the segment (host arrays); dl: the lengths of the documents doc_base ..; queries: lists of (term, occur, weight).
    -> contributions[q] {matching document: [c in slot order]}, scores, hits[q] [(document, score)] the best k, match_counts, counts [places,
    matches, skipped slots], anchors[q] (the anchor slot's index in the query or None), vetoes {"must": n, "must_not": n}: the documents that
    the query's place-dealing slots hold and a missing MUST / a present MUST_NOT drops"""

    def __init__(self, term_offsets, docs, tfs, doc_base, dl, queries, k, k1=1.2, b=0.75, avgdl=None):
        n_terms = len(term_offsets) - 1
        self.avgdl = F(float(sum(int(x) for x in dl)) / float(len(dl))) if avgdl is None else F(avgdl)
        self.k = k
        self.contributions, self.scores, self.hits, self.match_counts, self.anchors = [], [], [], [], []
        self.vetoes = {"must": 0, "must_not": 0}
        n_places = n_skip = 0

        def plist(term):
            """{document: tf} of a term, empty when it is out of range"""
            if not 0 <= term < n_terms:
                return {}
            return {int(docs[at]): int(tfs[at]) for at in range(int(term_offsets[term]), int(term_offsets[term + 1]))}

        with np.errstate(over="ignore"):
            for query in queries:
                lists = [plist(t) for t, _o, _w in query]
                n_skip += sum(1 for t, _o, _w in query if not 0 <= t < n_terms)
                must = [j for j, (_t, o, _w) in enumerate(query) if o == MUST]
                must_not = [j for j, (_t, o, _w) in enumerate(query) if o == MUST_NOT]
                should = [j for j, (_t, o, _w) in enumerate(query) if o == SHOULD]
                anchor = None
                if must:
                    anchor = min(must, key=lambda j: (len(lists[j]), j))   # the first of the smallest df
                    dead = any(len(lists[j]) == 0 for j in must)
                    pool = [] if dead else sorted(lists[anchor])
                    n_places += 0 if dead else len(lists[anchor])
                else:
                    pool = sorted(set().union(*[set(lists[j]) for j in should])) if should else []
                    n_places += sum(len(lists[j]) for j in should)
                per_doc = {}
                for d in pool:
                    if any(d not in lists[j] for j in must):
                        self.vetoes["must"] += 1
                        continue
                    if any(d in lists[j] for j in must_not):
                        self.vetoes["must_not"] += 1
                        continue
                    per_doc[d] = [contribution(query[j][2], lists[j][d], int(dl[d - doc_base]), k1, b, self.avgdl)
                                  for j in range(len(query)) if query[j][1] in (MUST, SHOULD) and d in lists[j]]
                scored = {}
                for d, cs in per_doc.items():
                    s = cs[0]
                    for c in cs[1:]:
                        s = s + c
                    assert type(s) is np.float32
                    scored[d] = s
                ranked = sorted(scored.items(), key=lambda x: (-float(x[1]), x[0]))
                self.anchors.append(anchor)
                self.contributions.append(per_doc)
                self.scores.append(scored)
                self.hits.append(ranked[:k])
                self.match_counts.append(len(ranked))
        self.counts = [n_places, sum(self.match_counts), n_skip]

    def order_matters(self, q=None):
        """the (query, document) pairs with three or more contributions whose float32 sum has other bits under another order of the slots"""
        found = []
        for i, per_doc in enumerate(self.contributions):
            if q is not None and i != q:
                continue
            for d, cs in per_doc.items():
                if len(cs) < 3:
                    continue
                want = bits(self.scores[i][d])
                for perm in itertools.permutations(cs[:6]):
                    s = perm[0]
                    for c in list(perm[1:]) + cs[6:]:
                        s = s + c
                    if bits(s) != want:
                        found.append((i, d))
                        break
        return found
