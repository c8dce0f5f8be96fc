"""TEST INFRASTRUCTURE: a plain restatement of "the token spans with every token's tags" (include/vaporetto_hip.h, vpt_token_tags_batch_device)
for labels the caller holds: per document the tokens of tests/tokenref.py (ends_from_labels) and, per token, the tag STRING of every slot --
the host fill_tags of the predictor's model, then the host api.PatternMatchTagger.filter (tests/patterntagsuite.oracle), read at the token's
last char.  It shares nothing with kernels_tokens.hip or the tag vocabulary of the C ABI: strings come from the model, not from ids."""
from typing import List, Optional, Sequence

from tests import patterntagsuite, tokenref


def walk_vocabulary(model) -> List[str]:
    """The distinct tag strings of a modelfmt.Model in order of first appearance: tag models in order, then slots, then candidates."""
    out, seen = [], set()
    for tm in model.tag_models:
        for slot in tm.tags:
            for cand in slot:
                if cand not in seen:
                    seen.add(cand)
                    out.append(cand)
    return out


def tokens_of(text: str, labels: Sequence[int], char_tags: Sequence[Optional[str]], n_tags: int) -> List[list]:
    """[offset_from, offset_to, position, (tag or None per slot)] per token of one document; char_tags: Sentence.tags() (n_tags per char)."""
    out, start, at, k = [], 0, 0, 0
    chars = list(text)
    for i, ch in enumerate(chars):
        at += len(ch.encode("utf-8"))
        if i + 1 == len(chars) or labels[i] == 1:
            out.append([start, at, k, tuple(char_tags[i * n_tags + j] for j in range(n_tags))])
            start = at
            k += 1
    return out


def token_tags(pred, texts: Sequence[str], ooff, labels, tagger=None, fullwidth: bool = False) -> List[List[list]]:
    """tokens_of for every document of a batch without empty documents."""
    _, tags = patterntagsuite.oracle(pred, texts, ooff, labels, tagger, fullwidth)
    nt = pred.n_tags()
    docs = []
    for i, t in enumerate(texts):
        lab = labels[int(ooff[i]):int(ooff[i + 1])]
        toks = tokens_of(t, lab, tags[i], nt)
        assert [e for _, e, _, _ in toks] == tokenref.ends_from_labels(t, lab)
        docs.append(toks)
    return docs


def stream_labels(model_bytes: bytes, texts: Sequence[str], wsconst: str):
    """Steps 1-4 of tests/tokenref.py for a batch without empty documents: (out_offsets, labels) of the adapter's filters on the oracle's predict."""
    import numpy as np
    from oracle import cbind
    from vaporetto_amd import api
    tokenref.check_wsconst(wsconst)
    norm = api.KyteaFullwidthFilter()
    normed = [norm.filter(t) for t in texts]
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in normed])
    scores, _, ooff, _ = cbind.OraclePredictor(model_bytes).predict_batch(utf8, boff)
    labels = np.zeros(int(ooff[-1]), np.uint8)
    for k, t in enumerate(normed):
        a, b = int(ooff[k]), int(ooff[k + 1])
        labels[a:b] = tokenref.filter_labels(t, (scores[a:b] > 0).astype(np.uint8), wsconst)
    return ooff, labels


def stopped(tags, stop_pairs) -> bool:
    """The stop rule: for some listed (slot, string) the token's slot carries that string; None never matches."""
    return any(slot < len(tags) and tags[slot] is not None and tags[slot] == s for slot, s in stop_pairs)


def five_arrays(docs: List[List[list]], stop_pairs=None):
    """-> (token_offsets, starts, ends, positions, tag strings) over the kept tokens of per-document tokens_of lists, in plain Python."""
    offsets, starts, ends, positions, tags = [0], [], [], [], []
    for toks in docs:
        for a, b, k, tg in toks:
            if stop_pairs and stopped(tg, stop_pairs):
                continue
            starts.append(a); ends.append(b); positions.append(k); tags.append(tg)
        offsets.append(len(ends))
    return offsets, starts, ends, positions, tags


def token_stream_tagged(model_bytes: bytes, pred, texts: Sequence[str], wsconst: str, tagger=None, stop_pairs=None):
    """The whole restatement for documents that may be empty: five_arrays of the tagged tokens of every document."""
    keep = [i for i, t in enumerate(texts) if t]
    docs = [[] for _ in texts]
    if keep:
        kept = [texts[i] for i in keep]
        ooff, labels = stream_labels(model_bytes, kept, wsconst)
        for i, d in zip(keep, token_tags(pred, kept, ooff, labels, tagger, fullwidth=True)):
            docs[i] = d
    return five_arrays(docs, stop_pairs), [len(d) for d in docs]
