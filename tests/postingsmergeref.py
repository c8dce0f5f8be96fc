"""The definition of the postings merge (vpt_postings_merge_device, include/vaporetto_hip.h) in plain Python: per term a dict document -> the sum
of the tfs of the segments that list the document.  No numpy in the definition itself; `arrays` lays the dict out as the call does."""
import numpy as np


class MergeRef:
    def __init__(self, segments, n_terms_out):
        """segments: (term_offsets, docs, tfs) each, a segment's postings being term_offsets[-1]"""
        self.n_terms = int(n_terms_out)
        self.terms = {}       # term -> dict(document -> tf)
        self.n_in = 0         # the input postings
        for term_offsets, docs, tfs in segments:
            toff = [int(x) for x in term_offsets]
            for k in range(len(toff) - 1):
                for q in range(toff[k], toff[k + 1]):
                    lst = self.terms.setdefault(k, {})
                    lst[int(docs[q])] = lst.get(int(docs[q]), 0) + int(tfs[q])
                    self.n_in += 1
        self.n_out = sum(len(lst) for lst in self.terms.values())
        self.n_combined = self.n_in - self.n_out

    def arrays(self):
        """(term_offsets uint64 [n_terms + 1], docs uint32, tfs uint32)"""
        df = np.zeros(self.n_terms + 1, np.uint64)
        docs, tfs = [], []
        for k in sorted(self.terms):
            df[k + 1] = len(self.terms[k])
            for d in sorted(self.terms[k]):
                docs.append(d)
                tfs.append(self.terms[k][d])
        return np.cumsum(df, dtype=np.uint64), np.array(docs, np.uint32), np.array(tfs, np.uint32)
