"""TEST INFRASTRUCTURE: a plain restatement of vaporetto_tantivy's VaporettoTokenizer::token_stream (vaporetto_tantivy/src/lib.rs:62-229),
written from the reference's text on top of the CPU oracle's scores.  It shares nothing with kernels_tokens.hip or the C ABI's span calls:

  1. an empty text has no tokens (lib.rs:161-169);
  2. KyteaFullwidthFilter on a copy, always (lib.rs:172); a NUL in it is an error (Sentence::from_raw, sentence.rs:174-179);
  3. Predictor::new(model, false) + predict: the oracle's scores, label = score > 0;
  4. SplitLinebreaksFilter FIRST (lib.rs:72), then per char of wsconst, in order: D R H T K O -> KyteaWsConstFilter of that type,
     G -> ConcatGraphemeClustersFilter, anything else -> "Could not parse a wsconst value" (lib.rs:73-84);
  5. boundary_pos = the byte index IN THE ORIGINAL TEXT of every char that follows a WordBoundary, then len(text) (lib.rs:183-192);
     token k = [boundary_pos[k-1] or 0, boundary_pos[k]), position k, position_length len(boundary_pos) (lib.rs:204-219)."""
from typing import List, Sequence

import numpy as np

from oracle import cbind
from vaporetto_amd import api

WSCONST = {"D": 1, "R": 2, "H": 3, "T": 4, "K": 5, "O": 6}


class WsconstError(ValueError):
    pass


def check_wsconst(wsconst: str) -> None:
    for c in wsconst:
        if c not in WSCONST and c != "G":
            raise WsconstError("Could not parse a wsconst value")


def filter_labels(norm: str, labels: np.ndarray, wsconst: str) -> np.ndarray:
    """Step 4 on the labels of the normalised text `norm` (a copy)."""
    labels = np.array(labels, dtype=np.uint8)
    cps = np.frombuffer(norm.encode("utf-32-le"), dtype=np.uint32)
    if len(cps) < 2:
        return labels
    lb = (cps == 0x0A) | (cps == 0x0D)
    labels[lb[:-1] | lb[1:]] = 1                              # split_linebreaks.rs:9-36
    types = api._types_of(cps)
    for c in wsconst:
        if c == "G":                                          # concat_grapheme_clusters.rs:10-36
            start = 0
            for n in api.ConcatGraphemeClustersFilter.cluster_lengths(norm):
                labels[start:start + n - 1] = 0
                start += n
        else:                                                 # kytea_wsconst.rs:26-43
            t = WSCONST[c]
            labels[(types[:-1] == t) & (types[1:] == t)] = 0
    return labels


def ends_from_labels(text: str, labels: Sequence[int]) -> List[int]:
    """Step 5: boundary_pos of `text` for the labels of its boundaries."""
    out, at = [], 0
    chars = list(text)
    for i, ch in enumerate(chars):
        at += len(ch.encode("utf-8"))
        if i + 1 < len(chars) and labels[i] == 1:
            out.append(at)
    out.append(at)
    return out


def ends_batch(model_bytes: bytes, texts: Sequence[str], wsconst: str) -> List[List[int]]:
    """boundary_pos of every document (steps 1-5); [] for an empty one."""
    check_wsconst(wsconst)
    norm = api.KyteaFullwidthFilter()
    keep = [i for i, t in enumerate(texts) if t]
    out = [[] for _ in texts]
    if not keep:
        return out
    normed = [norm.filter(texts[i]) for i in keep]
    for t in normed:
        if "\0" in t:
            raise ValueError("text: must not contain NULL")
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in normed])
    scores, _, ooff, _ = cbind.OraclePredictor(model_bytes).predict_batch(utf8, boff)
    for k, i in enumerate(keep):
        labels = (scores[int(ooff[k]):int(ooff[k + 1])] > 0).astype(np.uint8)
        out[i] = ends_from_labels(texts[i], filter_labels(normed[k], labels, wsconst))
    return out


def tokens_from_ends(text: str, ends: Sequence[int]) -> List[list]:
    raw, toks, start = text.encode("utf-8"), [], 0
    for k, e in enumerate(ends):
        toks.append([raw[start:e].decode("utf-8"), start, e, k, len(ends)])
        start = e
    return toks


def token_stream(model_bytes: bytes, text: str, wsconst: str) -> List[list]:
    """[text, offset_from, offset_to, position, position_length] per token."""
    return tokens_from_ends(text, ends_batch(model_bytes, [text], wsconst)[0])


def csr(ends: Sequence[Sequence[int]]):
    """(token_offsets uint64 [S+1], token_ends uint32) of per-document boundary_pos lists."""
    toff = np.zeros(len(ends) + 1, dtype=np.uint64)
    toff[1:] = np.cumsum([len(e) for e in ends])
    flat = np.array([x for e in ends for x in e], dtype=np.uint32)
    return toff, flat
