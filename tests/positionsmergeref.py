"""The definition of the merge of positional segments (vpt_postings_merge_positional_device, include/vaporetto_hip.h) in plain Python: per term a
dict document -> the sorted list of positions, the union of the lists of the segments that list the document; the tf is its length.  A position
that one (term, document) holds twice is an error.  No numpy in the definition itself; `arrays` lays the dict out as the call does."""
import numpy as np


class DuplicatePosition(ValueError):
    pass


class PositionsMergeRef:
    def __init__(self, n_terms_out):
        self.n_terms = int(n_terms_out)
        self.terms = {}       # term -> dict(document -> sorted positions)
        self.n_in = 0         # the input postings

    def add(self, term, doc, positions):
        """one input posting"""
        lst = self.terms.setdefault(int(term), {}).setdefault(int(doc), [])
        for p in positions:
            if int(p) in lst:
                raise DuplicatePosition((term, doc, int(p)))
            lst.append(int(p))
        lst.sort()
        self.n_in += 1

    @classmethod
    def of_segments(cls, segments, n_terms_out):
        """segments: (term_offsets, docs, tfs, first, positions) each, a segment's postings being term_offsets[-1]"""
        self = cls(n_terms_out)
        for term_offsets, docs, tfs, first, positions in segments:
            toff = [int(x) for x in term_offsets]
            for k in range(len(toff) - 1):
                for q in range(toff[k], toff[k + 1]):
                    a, b = int(first[q]), int(first[q + 1])
                    assert b - a == int(tfs[q])
                    self.add(k, docs[q], positions[a:b])
        return self

    @classmethod
    def of_documents(cls, docs, n_terms, doc_base=0, positions=None):
        """the whole batch in one pass: docs lists of ids, positions lists of positions (default 0, 1, ..); ids outside [0, n_terms) are dropped"""
        self = cls(n_terms)
        per = {}
        for d, ids in enumerate(docs):
            pos = range(len(ids)) if positions is None else positions[d]
            for t, p in zip(ids, pos):
                if 0 <= t < n_terms:
                    per.setdefault((int(t), doc_base + d), []).append(int(p))
        for (t, d), lst in per.items():
            self.add(t, d, lst)
        return self

    @property
    def n_out(self):
        return sum(len(lst) for lst in self.terms.values())

    @property
    def n_combined(self):
        return self.n_in - self.n_out

    def arrays(self):
        """(term_offsets uint64 [n_terms + 1], docs uint32, tfs uint32, first uint64 [postings + 1], positions uint32)"""
        df = np.zeros(self.n_terms + 1, np.uint64)
        docs, tfs, first, ppos = [], [], [0], []
        for k in sorted(self.terms):
            df[k + 1] = len(self.terms[k])
            for d in sorted(self.terms[k]):
                docs.append(d)
                tfs.append(len(self.terms[k][d]))
                ppos += self.terms[k][d]
                first.append(len(ppos))
        return (np.cumsum(df, dtype=np.uint64), np.array(docs, np.uint32), np.array(tfs, np.uint32), np.array(first, np.uint64),
                np.array(ppos, np.uint32))
