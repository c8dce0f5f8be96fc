"""TEST INFRASTRUCTURE: a plain restatement of the `predict` CLI's output per line (predict/src/main.rs:66-93, 122-176) on top of the CPU
oracle's scores, labels, tags and tag scores (oracle/cbind.py).  It shares nothing with kernels_listing.hip or the C ABI's listing calls:

  N = KyteaFullwidthFilter(L) unless no_norm; scores = Predictor::predict(N); labels = score > 0, then the post-filters on N
  (KyteaWsConstFilter per type, ConcatGraphemeClustersFilter for "G", SplitLinebreaksFilter on request); fill_tags on N;
  T = write_tokenized_text of L with those labels (and tags);
  scores block = "{i}:{N[i]}{N[i+1]} {score}\\n" per boundary + "\\n"                                  (print_scores, main.rs:66-75)
  tag block    = per token of N: surface + per slot "\\t" + ",".join("tag:score") + "\\n"; then "\\n"  (print_tag_scores, main.rs:77-93;
                 Token::tag_candidates, sentence.rs:1228-1250: one candidate -> score 0)
  norm order:    T "\\n" [scores block] [tag block]       (main.rs:154-176)
  no-norm order: T [scores block] "\\n" [tag block]       (main.rs:129-144)"""
from typing import List, Sequence

import numpy as np

from oracle import cbind
from tests import tokenref
from vaporetto_amd import api, modelfmt


def _esc(s: str) -> str:
    return "".join("\\" + c if c in " \\/" else c for c in s)   # sentence.rs:871-880


def print_scores(norm: str, scores: Sequence[int]) -> str:
    return "".join("%d:%s%s %d\n" % (i, norm[i], norm[i + 1], int(s)) for i, s in enumerate(scores)) + "\n"


def token_ranges(n: int, labels: Sequence[int]):
    start = 0
    for i in range(n):
        if i == n - 1 or labels[i] == 1:
            yield start, i + 1
            start = i + 1


def oracle_scores(model_bytes: bytes, texts: Sequence[str], fullwidth: bool = True):
    """The CPU oracle's boundary scores of the batch and their offsets: what a caller who lists labels of its own passes along with them."""
    fw = api.KyteaFullwidthFilter()
    utf8, boff = api.pack_texts([(fw.filter(t) if fullwidth else t).encode("utf-8") for t in texts])
    sc, _, ooff, _ = cbind.OraclePredictor(model_bytes, False).predict_batch(utf8, boff)
    return sc, ooff


def listing_lines(model_bytes: bytes, texts: Sequence[str], scores: bool = False, tag_scores: bool = False, tagged: bool = False,
                  fullwidth: bool = True, wsconst: str = "", no_norm_order: bool = False, split_linebreaks: bool = False,
                  labels_override=None) -> List[bytes]:
    model, _ = modelfmt.decode_model(model_bytes)
    want_tags = tagged or tag_scores
    orc = cbind.OraclePredictor(model_bytes, want_tags)
    fw = api.KyteaFullwidthFilter()
    normed = [fw.filter(t) if fullwidth else t for t in texts]
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in normed])
    sc, _, ooff, _ = orc.predict_batch(utf8, boff)
    labels = (sc > 0).astype(np.uint8)
    for k, t in enumerate(normed):
        a, b = int(ooff[k]), int(ooff[k + 1])
        lab = labels[a:b]
        if not split_linebreaks:
            keep = lab.copy()
        lab2 = tokenref.filter_labels(t, lab, wsconst)
        if not split_linebreaks:
            # tokenref applies SplitLinebreaksFilter first; the CLI has no such filter: redo the others on the plain labels
            lab2 = _filters_without_linebreaks(t, keep, wsconst)
        labels[a:b] = lab2
    if labels_override is not None:
        labels = np.asarray(labels_override, dtype=np.uint8)
    tags = tsc = models = None
    if want_tags and orc.n_tags() > 0:
        tags, tsc, models = orc.fill_tags_batch(utf8, boff, ooff, labels)
    out = []
    for k, (orig, norm) in enumerate(zip(texts, normed)):
        a, b = int(ooff[k]), int(ooff[k + 1])
        g0 = a + k
        n = len(norm)
        lab = labels[a:b]
        toks, block = [], []
        for s, e in token_ranges(n, lab):
            g = g0 + e - 1
            m = int(models[g]) if models is not None else -1
            tok = _esc(orig[s:e])
            if tagged and m >= 0:
                chosen = [model.tag_models[m].tags[j][int(tags[g, j])] if int(tags[g, j]) >= 0 else None for j in range(tags.shape[1])]
                while chosen and chosen[-1] is None:
                    chosen.pop()
                tok += "".join("/" + (_esc(c) if c is not None else "") for c in chosen)
            toks.append(tok)
            line = norm[s:e]
            if m >= 0:
                z = 0
                for cands in model.tag_models[m].tags:
                    if len(cands) == 1:
                        line += "\t%s:0" % cands[0]
                    else:
                        line += "\t" + ",".join("%s:%d" % (c, int(tsc[g, z + q])) for q, c in enumerate(cands))
                        z += len(cands)
            block.append(line + "\n")
        T = " ".join(toks)
        sblock = print_scores(norm, sc[a:b]) if scores else ""
        tblock = "".join(block) + "\n" if tag_scores else ""
        text = T + sblock + "\n" + tblock if no_norm_order else T + "\n" + sblock + tblock
        out.append(text.encode("utf-8"))
    return out


def _filters_without_linebreaks(norm: str, labels: np.ndarray, wsconst: str) -> np.ndarray:
    labels = np.array(labels, dtype=np.uint8)
    cps = np.frombuffer(norm.encode("utf-32-le"), dtype=np.uint32)
    if len(cps) < 2:
        return labels
    types = api._types_of(cps)
    for c in wsconst:
        if c == "G":
            start = 0
            for n in api.ConcatGraphemeClustersFilter.cluster_lengths(norm):
                labels[start:start + n - 1] = 0
                start += n
        else:
            t = tokenref.WSCONST[c]
            labels[(types[:-1] == t) & (types[1:] == t)] = 0
    return labels
