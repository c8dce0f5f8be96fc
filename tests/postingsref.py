"""The definition of the postings pass (vpt_postings_batch_device, include/vaporetto_hip.h) in plain Python: a dict term -> ordered dict
document -> tf, plus every posting's token list.  No numpy in the definition itself; `arrays` lays the dict out as the call does."""
from collections import OrderedDict

import numpy as np


class Ref:
    def __init__(self, token_offsets, token_ids, n_terms, doc_base=0):
        toff = [int(x) for x in token_offsets]
        ids = [int(x) for x in token_ids]
        self.n_terms, self.doc_base = int(n_terms), int(doc_base)
        self.terms = {}            # term -> OrderedDict(document -> tf), documents ascending
        self.tokens = {}           # (term, document) -> the indexed tokens' indices, ascending
        self.n_dropped = 0
        for d in range(len(toff) - 1):
            for t in range(toff[d], toff[d + 1]):
                k = ids[t]
                if not 0 <= k < self.n_terms:
                    self.n_dropped += 1
                    continue
                docs = self.terms.setdefault(k, OrderedDict())
                docs[self.doc_base + d] = docs.get(self.doc_base + d, 0) + 1
                self.tokens.setdefault((k, self.doc_base + d), []).append(t)

    def arrays(self):
        """(term_offsets uint64 [n_terms + 1], docs uint32, tfs uint32, first uint64 [postings + 1], order uint32)"""
        df = np.zeros(self.n_terms + 1, np.uint64)
        docs, tfs, first, order = [], [], [0], []
        for k in sorted(self.terms):
            df[k + 1] = len(self.terms[k])
            for d, tf in self.terms[k].items():
                docs.append(d)
                tfs.append(tf)
                order += self.tokens[(k, d)]
                first.append(len(order))
        return (np.cumsum(df, dtype=np.uint64), np.array(docs, np.uint32), np.array(tfs, np.uint32), np.array(first, np.uint64),
                np.array(order, np.uint32))


def from_token_strings(docs, table, unk_id, doc_base=0):
    """documents as lists of token strings, a dict surface -> id: the Ref over their ids"""
    toff, ids = [0], []
    for toks in docs:
        ids += [table.get(t, unk_id) for t in toks]
        toff.append(len(ids))
    return Ref(toff, ids, len(table), doc_base)
