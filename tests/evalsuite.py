"""The checks of the evaluate compare kernel alone (evaluate_kernel, kernels_parse.hip, through vpt_evaluate_labels_batch_device) against the
restatement of tests/evalref.py, run on the CPU emulator by tests/test_evaluate_compare_emu.py and on the MI355X by
tests/test_evaluate_compare_gpu.py.  The label vectors, the texts and the gold lines are the tests' own, so sentences span several windows of 64
boundaries, the tag compare meets candidates that need unescaping and gold tags that differ in every way, and sentences lie in every front-end
run of fill_tags.  Every comparison is exact; the conditions a check relies on are asserted on its inputs from the reference alone."""
import random

import numpy as np

from oracle import cbind
from tests import devmem, evalref, kat, randmodel
from vaporetto_amd import _lib, api
from vaporetto_amd.modelfmt import TagModel, TagNgramData, TagWeight, encode_model

KEYS = ("tp", "tn", "fp", "fn", "n_sys", "n_ref", "n_cor", "n_sentences")
NONE, GOLD, PREDICTED = _lib.VPT_EVAL_TAGS_NONE, _lib.VPT_EVAL_TAGS_GOLD, _lib.VPT_EVAL_TAGS_PREDICTED
_PARSED = ("raw", "raw_offsets", "out_offsets", "labels", "n_tags", "tag_index", "span_offsets", "tag_bytes")
_PRED = {}   # name -> (Predictor, DeviceBatch) of the library loaded now; the modules clear it when they switch libraries


def reset():
    _PRED.clear()


def _workspace(name, make_raw, tags=True):
    if name not in _PRED:
        pred = api.Predictor(api.Model.read_slice(make_raw())[0], tags)
        _PRED[name] = (pred, api.DeviceBatch(pred))
    return _PRED[name]


# ---- the system side from the CPU oracle

def oracle_rows(orc, tag_models, texts, utf8, boff, ooff, labels, nt):
    """Sentence::fill_tags of the CPU oracle on `labels` as rows of tag strings, a row of nt slots per char"""
    tags, _, models = orc.fill_tags_batch(utf8, boff, ooff, labels, want_scores=False)
    rows = []
    for i, t in enumerate(texts):
        g0 = int(ooff[i]) + i
        rs = []
        for c in range(len(t)):
            m = int(models[g0 + c])
            cand = tag_models[m].tags if m >= 0 else []
            rs.append([cand[j][tags[g0 + c][j]] if m >= 0 and j < len(cand) and tags[g0 + c][j] >= 0 else None for j in range(nt)])
        rows.append(rs)
    return rows


def oracle_system(raw_model, tag_models, types, graphemes, predict_tags):
    """the system side of evalref.evaluate from the CPU oracle: the CLI's loop (evaluate/src/main.rs:103-121) -- KyteaFullwidthFilter
    on the text, predict, KyteaWsConstFilter (a boundary between two chars of one of `types` becomes NotWordBoundary,
    kytea_wsconst.rs:26-43), ConcatGraphemeClustersFilter, fill_tags"""
    orc = cbind.OraclePredictor(raw_model, predict_tags=True)

    def system(raws, normalised):
        texts = [api.KyteaFullwidthFilter().filter(t) for t in raws] if normalised else list(raws)
        utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
        _, labels, ooff, _ = orc.predict_batch(utf8, boff)
        labels = labels.copy()
        for i, t in enumerate(texts):
            ty = api._types_of(np.frombuffer(t.encode("utf-32-le"), dtype=np.uint32))
            for b in range(len(t) - 1):
                if ty[b] == ty[b + 1] and int(ty[b]) in types:
                    labels[int(ooff[i]) + b] = 0
        if graphemes:
            api.ConcatGraphemeClustersFilter().filter_packed(texts, ooff, labels)
        sys_b = [list(labels[int(ooff[i]):int(ooff[i + 1])]) for i in range(len(texts))]
        nt = orc.n_tags() if predict_tags else 0
        if not nt:
            return sys_b, None
        return sys_b, oracle_rows(orc, tag_models, texts, utf8, boff, ooff, labels, nt)
    return system


def merge_tokens(line, seed, share=0.1):
    """a tokenized line without tags with a seeded share of its spaces dropped: the gold side then has merged tokens"""
    rng = random.Random(seed)
    toks = line.split(" ")
    return toks[0] + "".join(("" if rng.random() < share else " ") + t for t in toks[1:])


# ---- the compare alone

def _pad(a):
    return np.concatenate([a, np.zeros(32, a.dtype)])


def run_compare(pred, batch, h, sys_labels, mode, start=None, calls=1, n_sent=None, fill=True):
    """vpt_evaluate_labels_batch_device `calls` times on the arrays of `h` (those of api.parse_tokenized_host; the ones a mode does not read
    may be missing), d_counts starting as `start`; PREDICTED: DeviceBatch.fill_tags on the same system labels first.  -> the counters"""
    S = len(h["out_offsets"]) - 1 if n_sent is None else n_sent
    d = {k: devmem.put(_pad(np.asarray(h[k]))) for k in _PARSED if k in h}
    d_sys = devmem.put(_pad(np.asarray(sys_labels, np.uint8)))
    d_counts = devmem.put(np.asarray([0] * 8 if start is None else start, np.uint64))
    ptr = lambda k: d[k].ptr if k in d else None
    if mode == PREDICTED and fill and S:
        batch.fill_tags(d["raw"].ptr, d["raw_offsets"].ptr, d["out_offsets"].ptr, S, int(h["out_offsets"][S]), d_sys.ptr, 0, devmem.stream())
    for _ in range(calls):
        st = _lib.load().vpt_evaluate_labels_batch_device(pred.handle, batch._h, ptr("out_offsets"), S, ptr("labels"), ptr("n_tags"), ptr("tag_index"),
                                                          ptr("span_offsets"), ptr("tag_bytes"), d_sys.ptr, mode, d_counts.ptr, devmem.stream())
        assert st == _lib.VPT_OK, _lib.last_error()
    batch.sync()
    return dict(zip(KEYS, (int(c) for c in d_counts.get())))


def _kat_workspace():
    return _workspace("kat", lambda: encode_model(kat.predictor_test_model()))


def _labels_batch(sents, gold_n_tags=None):
    """sents: (gold labels, system labels) per sentence -> (arrays for run_compare, system labels, the reference's input for modes GOLD / NONE)"""
    ooff = np.zeros(len(sents) + 1, np.uint64)
    ooff[1:] = np.cumsum([len(g) for g, _ in sents], dtype=np.uint64)
    cat = lambda k: np.concatenate([np.asarray(s[k], np.uint8) for s in sents] + [np.zeros(0, np.uint8)])
    nt = np.zeros(len(sents), np.uint32) if gold_n_tags is None else np.asarray(gold_n_tags, np.uint32)
    results = []
    for (g, s), t in zip(sents, nt):
        rt = [[None] * int(t)] * (len(g) + 1)
        results.append(([int(x) for x in g], rt, [int(x) for x in s], rt if gold_n_tags is None else [[]] * (len(g) + 1)))
    return {"out_offsets": ooff, "labels": cat(0), "n_tags": nt}, cat(1), results


def _placed(nb, agreed, disagreed):
    """a sentence of nb boundaries: agreed WordBoundaries and disagreements (FP and FN in turn) where the lists say, agreed NotWordBoundary elsewhere"""
    g, s = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
    g[agreed] = s[agreed] = 1
    for k, b in enumerate(disagreed):
        (s if k % 2 == 0 else g)[b] = 1
    return g, s


# (boundaries, agreed WordBoundaries, disagreements, n_cor): by hand -- a token ends at every agreed WordBoundary and at the sentence's end,
# and is correct when an agreed WordBoundary (or the sentence's start) and no disagreement lies between it and the one before
HAND = [
    # a disagreement in window 0, the next agreed WordBoundary in window 1 / 2 / 3, nothing between: 3 correct, the late one not, the end correct
    (100, [3, 69], [10], 2),
    (200, [3, 133], [10], 2),
    (260, [3, 197], [10], 2),
    # the agreed WordBoundary at 20 lies behind the disagreement at 10, the next one a window on: 3 correct, 20 not, 69 correct, the end correct
    (100, [3, 20, 69], [10], 3),
    (260, [20, 197], [10], 2),                # the same three windows on: 20 not, 197 correct, the end correct
    # a disagreement on lane 63, an agreed WordBoundary on lane 0 of the next window: 64 not, the end correct
    (100, [64], [63], 1),
    # the mirror image: 63 correct, the disagreement on lane 0 spoils the end
    (100, [63], [64], 1),
    (100, [63, 70], [64], 2),                 # ... and with one more token: 63 correct, 70 not, the end correct
    (100, [63, 65], [64], 2),                 # agreed 63, disagreement 64, agreed 65: 63 correct, 65 not, the end correct
    # the last token after a disagreement two windows back: 2 correct, the end not
    (150, [2], [5], 1),
    (150, [], [5], 0),
    (150, [2], [], 2),                        # ... and without the disagreement: both
    # whole windows, the deciding event in the last lane
    (64, [], [63], 0),                        # the end not
    (64, [63], [10], 1),                      # 63 not, the end correct
    (128, [], [127], 0),
    (128, [127], [], 2),
    (128, [127], [3], 1),                     # 127 not, the end correct
    (192, [191], [10], 1),                    # 191 not, the end correct
    (192, [5], [191], 1),                     # 5 correct, the end not
]
SIZES = [0, 1, 2, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 190, 191, 192, 193, 194, 255, 256, 257, 641]


def carry_verdicts(gold, sys):
    """-> (matched, not matched) over the agreed WordBoundaries whose verdict needs a carry: the later of the last agreed WordBoundary and the
    last disagreement in front of it lies in an earlier window of 64"""
    la, ld, m, u = -1, -2, 0, 0
    for b, (r, s) in enumerate(zip(gold, sys)):
        if r == s and s == 1:
            if max(la, ld) >= 0 and max(la, ld) // 64 < b // 64:
                m, u = m + (ld < la), u + (ld > la)
            la = b
        elif r != s:
            ld = b
    return m, u


def n_cor_forgetting_carries(results):
    """evalref.counts' n_cor, deliberately wrong: `matched` starts afresh at every 64th boundary"""
    n = 0
    for rb, rt, sb, st in results:
        matched = True
        for b, (r_b, r_t, s_b, s_t) in enumerate(zip(rb, rt, sb, st)):
            if b % 64 == 0:
                matched = True
            if r_b != s_b:
                matched = False
            elif s_b == 1:
                n += matched and r_t == s_t
                matched = True
        n += matched and rt[-1] == st[-1]
    return n


def _window_batch():
    rs = np.random.RandomState(17)
    sents = []
    # (the last ones: few events of either kind, so that many a window's first agreed WordBoundary follows a disagreement of a window before)
    for k, nb in enumerate(SIZES * 4 + [130, 193, 257, 641] * 4):
        rate, density = (rs.choice([0.0, 0.02, 0.1, 0.5]), rs.choice([0.02, 0.1, 0.5])) if k < 4 * len(SIZES) else (0.02, 0.02)
        s = (rs.random_sample(nb) < density).astype(np.uint8)
        sents.append((s ^ (rs.random_sample(nb) < rate).astype(np.uint8), s))
    for nb in (1, 64, 130, 257):   # all agree on WordBoundary, all agree on not, all disagree both ways
        sents += [(np.ones(nb, np.uint8),) * 2, (np.zeros(nb, np.uint8),) * 2, (np.ones(nb, np.uint8), np.zeros(nb, np.uint8)),
                  (np.zeros(nb, np.uint8), np.ones(nb, np.uint8))]
    sents += [_placed(nb, a, d) for nb, a, d, _ in HAND]
    order = list(range(len(sents)))
    random.Random(5).shuffle(order)
    return [sents[k] for k in order]


def check_window_carries():
    pred, batch = _kat_workspace()
    # the hand cases one by one: the kernel and the restatement both give the count written next to the case
    for nb, a, d, cor in HAND:
        h, sys_l, results = _labels_batch([_placed(nb, a, d)])
        want = evalref.counts(results)
        assert want["n_cor"] == cor and want["tp"] == len(a) and want["fp"] + want["fn"] == len(d), (nb, a, d)
        assert run_compare(pred, batch, h, sys_l, GOLD) == want, (nb, a, d)
    sents = _window_batch()
    m, u = (sum(x) for x in zip(*(carry_verdicts(g, s) for g, s in sents)))
    assert m + u >= 50 and m >= 20 and u >= 20, (m, u)
    assert {len(g) for g, _ in sents} >= set(SIZES)
    h, sys_l, results = _labels_batch(sents)
    want = evalref.counts(results)
    assert min(want[k] for k in ("tp", "tn", "fp", "fn")) > 0 and 0 < want["n_cor"] < want["n_ref"], want
    assert n_cor_forgetting_carries(results) != want["n_cor"]
    short = [r for r in results if len(r[0]) <= 64]   # (within one window the variant is the restatement)
    assert n_cor_forgetting_carries(short) == evalref.counts(short)["n_cor"]
    assert run_compare(pred, batch, h, sys_l, GOLD) == want
    # mode NONE: a third of the sentences have gold tags and are never correct
    nt = [(1 + k % 2) if k % 3 == 0 else 0 for k in range(len(sents))]
    h, sys_l, results = _labels_batch(sents, nt)
    want_none = evalref.counts(results)
    assert 0 < want_none["n_cor"] < want["n_cor"] and n_cor_forgetting_carries(results) != want_none["n_cor"]
    assert run_compare(pred, batch, h, sys_l, NONE) == want_none


def check_counts_add_up():
    pred, batch = _kat_workspace()
    h, sys_l, results = _labels_batch(_window_batch()[:40])
    want = evalref.counts(results)
    assert all(want[k] > 0 for k in KEYS), want
    start = [11, 23, 37, 41, 53, 67, 79, 83]
    got = run_compare(pred, batch, h, sys_l, GOLD, start=start, calls=2)
    assert got == {k: s + 2 * want[k] for k, s in zip(KEYS, start)}
    assert run_compare(pred, batch, h, sys_l, GOLD, start=start, n_sent=0) == dict(zip(KEYS, start))


def check_grid():
    """workgroups with idle waves, and 8192 x 4 x 2 + 5 sentences: every wave of the largest grid takes a second and a third sentence (about five
    seconds on the emulator)"""
    pred, batch = _kat_workspace()
    some = [_placed(70, [3, 69], [10]), _placed(3, [1], [2]), _placed(0, [], []), _placed(130, [64, 129], [63]), _placed(1, [], [0])]
    for n in (1, 3, 4, 5):
        for mode in (GOLD, NONE):
            h, sys_l, results = _labels_batch(some[:n], None if mode == GOLD else [0, 1, 0, 0, 2][:n])
            assert run_compare(pred, batch, h, sys_l, mode) == evalref.counts(results), (n, mode)
    rs = np.random.RandomState(23)
    S = 8192 * 4 * 2 + 5
    nbs = rs.randint(0, 4, S)
    lab = [rs.randint(0, 2, int(nbs.sum())).astype(np.uint8) for _ in range(2)]
    cut = np.cumsum(nbs)[:-1]
    sents = list(zip(np.split(lab[0], cut), np.split(lab[1], cut)))
    h, sys_l, results = _labels_batch(sents)
    want = evalref.counts(results)
    assert want["n_sentences"] == S and 0 < want["n_cor"] < want["n_ref"]
    assert run_compare(pred, batch, h, sys_l, GOLD) == want


# ---- mode PREDICTED: the tag compare and the run lookup

ALPHA = list("あいうカ漢字09AZaz、 /\\１Ａ")
TAGGED = ["あ", "カ", "い", "う", "漢字", "a /", "Az"]
PLAIN = ["0", "9", "A", "z", "、", "漢", "字", "１", "Ａ", " ", "/", "\\", "09", "aa", "z、0", "字漢"]
EDGES = (63, 64, 65, 127, 128)   # chars a tag model's surface ends on: the lanes on both sides of a window's edge


def tag_model_bytes(tag_models=True):
    """a random boundary model with hand-made tag models: candidates with ' ' '/' '\\' ':', a slot with one candidate, a slot with none, models of
    one slot and of two, a surface of two chars and one that needs escaping"""
    m = randmodel.rand_model(11, alphabet=ALPHA, wc=3, wt=2)

    def tm(tok, tags, bias, ngram=True):
        return TagModel(token=tok, tags=tags,
                        char_ngram_model=[TagNgramData(tok[-1], [TagWeight(0, list(range(1, len(bias) + 1)))])] if bias and ngram else [],
                        type_ngram_model=[], bias=bias)
    m.tag_models = [
        tm("あ", [["sp ace", "plain"], ["q", "r/s"]], [5, 0, 0, 5]),
        tm("カ", [["t\\u", "x:y"], ["only"]], [5, -7]),
        tm("い", [["first"]], []),
        tm("う", [[], ["p q", "r/s", "t\\u"]], [-3, 2, 9], ngram=False),
        tm("漢字", [["a\\ b/c", "k"]], [9, 0]),
        tm("a /", [["sp ace", "sl/ash"]], [1, 2]),
        tm("Az", [["x:y", ":"], ["\\", "/"]], [0, 3, 4, 0]),
    ] if tag_models else []
    return api.Model(m).to_vec()


def _tokens(rng, n):
    """tokens of n chars in all, tagged surfaces among them"""
    out = []
    while n > 0:
        t = rng.choice(TAGGED if rng.random() < 0.4 else PLAIN)
        if len(t) > n:
            t = rng.choice(PLAIN[:12])
        out.append(t)
        n -= len(t)
    return out


def _ending_on(rng, surface, end, total):
    """tokens of `total` chars: `surface` ends on char `end`"""
    return _tokens(rng, end + 1 - len(surface)) + [surface] + _tokens(rng, total - end - 1)


def esc(s):
    return "".join("\\" + c if c in " /\\" else c for c in s)


def gold_line(tokens, rows, merged=()):
    """write_tokenized_text's spelling (sentence.rs:850-886) of tokens with a row of tags each; "" prints as an empty field (None when parsed);
    a token in `merged` is joined to the next one and prints no tags"""
    out = ""
    for k, (t, r) in enumerate(zip(tokens, rows)):
        out += esc(t)
        if k not in merged:
            n = max([j + 1 for j, x in enumerate(r) if x is not None], default=0)
            out += "".join("/" + esc(x or "") for x in r[:n]) + (" " if k + 1 < len(tokens) else "")
    return out


KINDS = ("other", "dropped", "added", "prefix", "longer", "escaped", "empty", "extra")


def mutate(kind, row, cands, rng):
    """the gold row of a token whose system row is `row` (cands: its tag model's candidates, None without a model), or None where the kind does not apply"""
    row = list(row)
    some = [j for j, x in enumerate(row) if x is not None]
    if kind == "extra":
        return row + ["extra"]
    if kind == "added":
        return ["new"] + row[1:] if cands is None else None
    pick = {"other": [j for j in some if len(cands[j]) >= 2], "dropped": some, "prefix": [j for j in some if len(row[j]) >= 2], "longer": some,
            "escaped": [j for j in some if esc(row[j]) != row[j]], "empty": some[-1:]}[kind]
    if not pick:
        return None
    j = rng.choice(pick)
    row[j] = {"other": lambda: rng.choice([c for c in cands[j] if c != row[j]]), "dropped": lambda: None, "prefix": lambda: row[j][:-1],
              "longer": lambda: row[j] + "x", "escaped": lambda: esc(row[j]), "empty": lambda: ""}[kind]()
    return row


class _Tagged:
    """the texts of check_predicted_tags with the system side the CPU oracle's fill_tags gives for the tests' own labels"""

    def __init__(self):
        self.raw = tag_model_bytes()
        self.models = api.Model.read_slice(self.raw)[0].tag_models()
        self.orc = cbind.OraclePredictor(self.raw, predict_tags=True)
        self.nt = self.orc.n_tags()
        self.cands = {m.token: m.tags for m in self.models}

    def system(self, sents):
        """sents: token lists -> per sentence (system labels, rows per char, rows per token)"""
        texts = ["".join(t) for t in sents]
        utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
        labels = [np.zeros(len(t) - 1, np.uint8) for t in texts]
        for lab, toks in zip(labels, sents):
            lab[np.cumsum([len(t) for t in toks])[:-1] - 1] = 1
        ooff = np.zeros(len(texts) + 1, np.uint64)
        ooff[1:] = np.cumsum([len(x) for x in labels], dtype=np.uint64)
        rows = oracle_rows(self.orc, self.models, texts, utf8, boff, ooff, np.concatenate(labels + [np.zeros(1, np.uint8)]), self.nt)
        per_token = [[r[e - 1] for e in np.cumsum([len(t) for t in toks])] for r, toks in zip(rows, sents)]
        return labels, rows, per_token


def _reference(lines, labels, rows):
    """the restatement's input: the gold side parsed from the lines, the system side as given"""
    results = []
    for ln, lab, st in zip(lines, labels, rows):
        raw, rb, tags, nt = evalref.parse_tokenized(ln)
        assert len(raw) == len(st)
        results.append((rb, evalref.tag_rows(tags, nt, len(raw)), [int(x) for x in lab], st))
    return results


def _device(pred, batch, lines, labels, mode=PREDICTED, **kw):
    h = api.parse_tokenized_host([ln.encode("utf-8") for ln in lines])
    return run_compare(pred, batch, h, np.concatenate(list(labels) + [np.zeros(0, np.uint8)]), mode, **kw)


def check_predicted_tags():
    T = _Tagged()
    pred, batch = _workspace("tagged", lambda: T.raw)
    assert T.nt == 2 and pred.n_tags() == 2
    rng = random.Random(29)
    longs = [_ending_on(rng, s, e, 700 if (k + j) % 9 == 0 else e + 1 + rng.randrange(60)) for k, s in enumerate(TAGGED) for j, e in enumerate(EDGES)]
    shorts = [_tokens(rng, n) for n in list(range(1, 21)) * 2 + [1, 1, 2, 3]]
    assert max(len("".join(t)) for t in longs) == 700 and min(len("".join(t)) for t in shorts) == 1

    # every kind of difference in a one-sentence call of its own: one token's gold row changed lowers n_cor
    one = _ending_on(rng, "あ", 64, 200)
    lab, rows, per_token = T.system([one])
    base_line = gold_line(one, per_token[0])
    base = evalref.counts(_reference([base_line], lab, rows))
    assert base["n_cor"] == base["n_ref"] == len(one) and _device(pred, batch, [base_line], lab) == base
    for kind in KINDS:
        ks = [k for k, t in enumerate(one) if mutate(kind, per_token[0][k], T.cands.get(t), random.Random(k)) is not None]
        k = ks[len(ks) // 2]
        line = gold_line(one, [mutate(kind, r, T.cands.get(one[j]), random.Random(j)) if j == k else r for j, r in enumerate(per_token[0])])
        want = evalref.counts(_reference([line], lab, rows))
        assert want["n_cor"] < base["n_cor"] and (want["n_cor"] == 0) == (kind == "extra"), (kind, line)
        assert _device(pred, batch, [line], lab) == want, (kind, line)

    # the batch: long texts on the first and the last sentence of every front-end run, short ones between
    sents = longs + shorts
    S, chars = len(sents), sum(len("".join(t)) for t in sents)
    lab, rows, per_token = T.system(sents)
    _device(pred, batch, [gold_line(t, r) for t, r in zip(sents, per_token)], lab)
    R = batch.last_plan()["tag_run_sent"]
    edges = sorted({k for r0 in range(0, S, R) for k in (r0, min(r0 + R, S) - 1)})
    assert len(edges) <= len(longs) and len(edges) >= 5, (R, S, chars)
    rest = [k for k in range(S) if k >= len(edges)]
    rng.shuffle(rest)
    place, rest = {e: k for k, e in enumerate(edges)}, iter(rest)
    order = [place[i] if i in place else next(rest) for i in range(S)]
    sents = [sents[k] for k in order]
    lab, rows, per_token = ([x[k] for k in order] for x in (lab, rows, per_token))
    extra = set(rng.sample([i for i in range(S) if i not in place], 12))
    done, lines = dict.fromkeys(KINDS, 0), []
    for i, toks in enumerate(sents):
        gold, merged = [list(r) for r in per_token[i]], set()
        for k, t in enumerate(toks):
            if rng.random() < 0.15:
                kind = rng.choice(KINDS[:-1])
                new = mutate(kind, gold[k], T.cands.get(t), rng)
                if new is not None:
                    gold[k], done[kind] = new, done[kind] + 1
            elif rng.random() < 0.03 and k + 1 < len(toks):
                merged.add(k)
        if i in extra:
            k = rng.randrange(len(toks))
            gold[k], done["extra"] = mutate("extra", gold[k], None, rng), done["extra"] + 1
            merged.discard(k)
        lines.append(gold_line(toks, gold, merged))
    assert min(done.values()) >= 10, done
    results = _reference(lines, lab, rows)
    want = evalref.counts(results)
    assert 0 < want["n_cor"] < want["n_ref"] and want["fp"] > 0 and want["fn"] == 0, want
    # tokens that are correct because an escaped candidate matches: spelled as stored, the system side's tags would differ there
    stored = [(rb, rt, sb, [[x if x is None else esc(x) for x in r] for r in st]) for rb, rt, sb, st in results]
    assert want["n_cor"] - evalref.counts(stored)["n_cor"] >= 10
    got = _device(pred, batch, lines, lab)
    plan = batch.last_plan()
    assert plan["tag_runs"] >= 3 and plan["tag_run_sent"] == R, plan
    assert all(len("".join(sents[e])) > 63 for e in edges)
    assert got == want
    # the sentences on the runs' edges through a reference of their own, and alone on the device (no run to look up): a wrong run shows
    per = [evalref.counts([r]) for r in results]
    assert {k: sum(p[k] for p in per) for k in KEYS} == want
    assert all(per[e]["n_cor"] > 0 for e in edges if e not in extra)
    for e in edges:
        assert _device(pred, batch, [lines[e]], [lab[e]]) == per[e], e

    # a predictor without tag models: mode PREDICTED is mode NONE
    plain, pbatch = _workspace("untagged", lambda: tag_model_bytes(False))
    assert plain.n_tags() == 0
    want0 = evalref.counts([(rb, rt, sb, [[]] * len(st)) for rb, rt, sb, st in results])
    assert 0 < want0["n_cor"] < want["n_cor"]
    assert _device(plain, pbatch, lines, lab, NONE) == want0
    assert _device(plain, pbatch, lines, lab, PREDICTED) == want0
