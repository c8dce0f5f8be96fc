"""TEST INFRASTRUCTURE: a plain-Python restatement of the vocabulary counter (vaporetto_amd/csrc/kernels_vocab_count.hip, vocab_count.hpp): a
collections.Counter over the surfaces of a span CSR with the skip rules, the KyteaFullwidthFilter image, the finish order and its cuts.  Nothing
here is on the product path."""
import collections

import numpy as np

from vaporetto_amd import api

_NORM = api.KyteaFullwidthFilter()


def token_bytes(docs, token_offsets, starts, ends):
    """docs: the documents' bytes.  starts None: a token starts where the one before it in its document ends, or at 0."""
    out = []
    for i, raw in enumerate(docs):
        a, b = int(token_offsets[i]), int(token_offsets[i + 1])
        for k in range(a, b):
            s = int(starts[k]) if starts is not None else (int(ends[k - 1]) if k > a else 0)
            out.append(raw[s:int(ends[k])])
    return out


class Ref:
    """What a counter holds after the calls it was fed: counts, n_counted, n_skipped."""

    def __init__(self, max_surface_chars=64):
        self.max_chars = max_surface_chars
        self.counts = collections.Counter()
        self.n_counted = self.n_skipped = 0

    def add_tokens(self, tokens, normalize):
        """tokens: bytes each.  Skipped: empty, not strict UTF-8 (Python's decoder refuses what a Rust String cannot hold), too many chars."""
        for t in tokens:
            try:
                s = t.decode("utf-8")
            except UnicodeDecodeError:
                s = None
            if not s or len(s) > self.max_chars:
                self.n_skipped += 1
                continue
            self.counts[_NORM.filter(s) if normalize else s] += 1
            self.n_counted += 1

    def add_csr(self, docs, token_offsets, starts, ends, normalize):
        self.add_tokens(token_bytes(docs, token_offsets, starts, ends), normalize)

    def finish(self, min_count=1, max_entries=None):
        """-> (surfaces, counts): count descending, then code points ascending (Python compares str by code point); the cuts."""
        items = sorted(((s, c) for s, c in self.counts.items() if c >= min_count), key=lambda x: (-x[1], x[0]))
        if max_entries:
            items = items[:max_entries]
        return [s for s, _ in items], np.array([c for _, c in items], np.uint64)

    def finish_raw(self, min_count=1, max_entries=None):
        surfaces, counts = self.finish(min_count, max_entries)
        raws = [s.encode("utf-8") for s in surfaces]
        off = np.zeros(len(raws) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in raws], dtype=np.uint64) if raws else []
        return np.frombuffer(b"".join(raws), np.uint8), off, counts
