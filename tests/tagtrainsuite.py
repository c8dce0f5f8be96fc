"""TEST INFRASTRUCTURE: seeded tagged corpora and the tag-trainer checks shared by the emulator tests (tests/test_train_tags_emu.py)
and the GPU tests (tests/test_train_tags_gpu.py), against the restatement of tests/tagtrainref.py.

A corpus holds: sentences with 0, 1 and 3 tag slots; None slots; Unknown boundaries inside and beside tagged tokens; one-char
sentences; tokens at both sentence edges; surfaces with 1, 2 and at least 4 candidates in a slot; a surface only in the tag dictionary;
non-BMP chars; a surface longer than five chars; and, in the LARGE case, a problem above the in-kernel size limit."""
import numpy as np
import pytest

from tests import tagtrainref, trainref, trainsuite
from vaporetto_amd import api, modelfmt

A = trainsuite.ALPHABET
LONG = "タナーン漢字東京"          # eight chars
FREQ = "あ"                        # the frequent surface: four candidates in slot 0, two in slot 1
NONBMP = "\U00020B9F"
FREQ_W = 60.0                      # its weight among the surfaces (the others 1)
END = "。"                         # one candidate
DICT_ONLY = "字東"                 # never a token of the corpus
TAG_DICTIONARY = [(DICT_ONLY, ["名詞", None, "ジトー"]), (FREQ, ["辞書"]), (DICT_ONLY, ["動詞"]), ("漢0", [None, None])]
LDS_DOUBLES = 7424                 # include/vaporetto_hip.h: in-kernel iff 7 * (features + 1) + 3 * rows <= 7424


def vocabulary(seed, n_fill):
    rng = np.random.default_rng(seed + 100)
    vocab = {FREQ: 4, LONG: 2, NONBMP: 2, END: 1, "か": 2, "0１": 3}
    while len(vocab) < 6 + n_fill:
        w = "".join(A[k] for k in rng.integers(0, len(A), int(rng.integers(1, 4))))
        if w not in vocab and w not in (DICT_ONLY, "漢0") and " " not in w:
            vocab[w] = int(rng.integers(1, 3))
    return vocab


def corpus(seed, n_sent, n_fill, unknown=0.04, none=0.1, decided=False):
    """[(text, boundaries, n_tags, tags)].  A token's tag in slot j is decided by the char behind it (and j), so that it can be learnt;
    `decided`: no Unknown, no None, every sentence ends with END and has one slot -- every tag is decided by an adjacent char."""
    rng = np.random.default_rng(seed)
    vocab = vocabulary(seed, n_fill)
    words = list(vocab)
    p = np.array([FREQ_W if w == FREQ else 1.0 for w in words])
    p /= p.sum()
    out = []
    for i in range(n_sent):
        n_tags = 1 if decided else (0, 1, 3)[i % 3]
        if not decided and i % 17 == 0:
            toks = [words[int(rng.integers(0, len(words)))][:1]]   # a one-char sentence
        else:
            toks = [words[k] for k in rng.choice(len(words), int(rng.integers(1, 9)), p=p)]
        if decided:
            toks.append(END)
        text = "".join(toks)
        bounds = np.zeros(len(text) - 1, np.uint8)
        tags = [None] * (len(text) * n_tags)
        pos = 0
        for k, tok in enumerate(toks):
            pos += len(tok)
            if pos < len(text):
                bounds[pos - 1] = 1
            nxt = ord(text[pos]) if pos < len(text) else 7
            for j in range(n_tags):
                if not decided and rng.random() < none:
                    continue
                n_c = max(1, vocab.get(tok, 1) - j) if j < 2 else 1
                tags[(pos - 1) * n_tags + j] = "t%d_%d" % (j, (nxt + j) % n_c)
        if not decided:
            bounds[rng.random(len(bounds)) < unknown] = 2
        out.append((text, bounds, n_tags, tags))
    return out


CASES = {  # name -> (seed, sentences, filler surfaces, charw, charn, typew, typen)
    "small": (11, 150, 20, 2, 2, 2, 1),
    "large": (12, 500, 120, 3, 3, 3, 2),   # typew = charw: a boundary model with typew < charw does not load (type weights use the char window)
}
DECIDED = (13, 300, 0, 2, 2, 2, 1)   # no fillers: the surfaces share no char, so the boundaries are decided too


def pack(sents):
    """The arrays of vpt_parse_tokenized_batch for the sentences."""
    utf8, boff = api.pack_texts([s[0].encode("utf-8") for s in sents])
    labels = np.concatenate([s[1] for s in sents]) if sents else np.zeros(0, np.uint8)
    n_tags, tindex, spans = [], [0], []
    for text, _, nt, tags in sents:
        n_tags.append(nt)
        for c in range(len(text)):
            row = list(tags[c * nt:(c + 1) * nt])
            while row and row[-1] is None:
                row.pop()
            spans += [(t or "").encode("utf-8") for t in row]
            tindex.append(len(spans))
    tb, so = api.pack_texts(spans)
    return utf8, boff, labels, np.array(n_tags, np.uint32), np.array(tindex, np.uint64), so, tb


def run_pair(params, sents, tag_dictionary=TAG_DICTIONARY, path=0):
    _, _, _, charw, charn, typew, typen = params
    t = api.Trainer(charw, charn, typew, typen, train_tags=True, tag_dictionary=tag_dictionary)
    t.set_tag_path(path)
    t.add_packed_tagged(*pack(sents))
    r = tagtrainref.RefTagTrainer(charn, typen, tag_dictionary)
    for s in sents:
        r.add_example(*s)
    return t, r


def check_problems(name):
    params = CASES[name]
    sents = corpus(params[0], params[1], params[2])
    t, r = run_pair(params, sents)
    models = r.models()
    ref = [(m["token"], p) for m in models for p in m["problems"]]
    got = t.tag_problems()
    assert t.n_tag_models() == len(models)
    assert [(g["surface"], g["slot"]) for g in got] == [(tok, p["slot"]) for tok, p in ref]
    for g, (tok, p) in zip(got, ref):
        assert g["candidates"] == p["candidates"]
        assert g["n_rows"] == len(p["y"])
        assert g["keys"] == p["keys"]
        assert np.array_equal(g["row_ptr"].astype(np.int64), p["row_ptr"])
        assert np.array_equal(g["cols"].astype(np.int64), p["cols"])
        assert np.array_equal(g["y"].astype(np.int64), p["y"])
    # the corpus holds what the suite promises
    assert any(len(m["tags"]) == 3 for m in models) and any(len(m["tags"]) == 1 for m in models)
    assert any(m["token"] == DICT_ONLY and m["tags"] == [["名詞"], [], ["ジトー"]] and not m["problems"] for m in models)
    assert not any(m["token"] == "漢0" for m in models)
    assert any(len(p["candidates"]) >= 4 for _, p in ref) and any(len(p["candidates"]) == 2 for _, p in ref)
    assert any(len(m["token"]) > 5 for m in models) and any(ord(m["token"][0]) > 0xFFFF for m in models)
    return t, r


def fits(p):
    return 7 * (len(p["keys"]) + 1) + 3 * len(p["y"]) <= LDS_DOUBLES


# (case, solver) -> problems (surface, slot, class) whose TRON path is NOT the restatement's step for step: only the order of the sums
# differs, CG amplifies it, and on these the iteration or CG counts part (see trainsuite.check_solver).  Recorded from the emulator and
# the MI355X; every other (problem, class) has equal counts and weights within 1e-7.
UNSTABLE = {}


def check_class_stats(st, p, y, wg, cost, solver):
    """The stats of one (problem, class) against the problem's 0/1 matrix alone (trainsuite's checks b and c): gnorm0 is the first
    gradient's norm bit for bit -- at w = 0 every partial sum is a multiple of 1/2 -- and gnorm and objective are |g| and f at the
    returned weights within the bound of fp64 summation in any order (trainref.stats_bounds).  The in-kernel solver sums in LDS and
    shares no code with the global-memory one; both are held to the same two checks."""
    ones = np.ones(len(p["cols"]))
    if cost == 1.0:
        trainref.check_gnorm0(st, p["row_ptr"], p["cols"], ones, y, len(p["keys"]), solver)
    return trainref.check_stats(st, p["row_ptr"], p["cols"], ones, y, wg[:-1], wg[-1], cost, solver)


LIMIT_PARAMS = (0, 0, 0, 1, 1, 1, 1)   # charn = typen = 1: a token's features are the char and the type on either side


def limit_corpus(total):
    """Sentences "<a|b>X<right>" of three one-char tokens whose only tag problem (surface X, two tags) has exactly
    7 * (features + 1) + 3 * rows == total: features = 2 left chars + the right chars + 1 left type + 2 right types, and 7424 needs
    features + 1 = 2 (mod 3), 7425 features + 1 = 0 (mod 3).  The tag follows the right char, one in ten flipped."""
    rights = {2: "c1", 0: "cd1"}[total % 3]
    nf = 2 + len(rights) + 1 + 2
    rows, rem = divmod(total - 7 * (nf + 1), 3)
    assert rem == 0
    rng = np.random.default_rng(total)
    flip = rng.random(rows) < 0.1
    out = []
    for i in range(rows):
        right = rights[i % len(rights)]
        tag = "t%d" % ((right == "1") ^ bool(flip[i]))
        out.append(("ab"[(i // 3) % 2] + "X" + right, np.array([1, 1], np.uint8), 1, [None, tag, None]))
    # the boundary model needs a boundary that is none
    return out + [("ab", np.array([0], np.uint8), 1, [None, None])] * 3


def check_limit(total, path, eps=0.01, cost=1.0):
    """A problem exactly at (7424, in-kernel) and one double past (7425, global-memory) the in-kernel solver's LDS limit: the path
    taken, and the stats of both solvers."""
    sents = limit_corpus(total)
    t, r = run_pair(LIMIT_PARAMS, sents, tag_dictionary=())
    (p,) = [q for m in r.models() for q in m["problems"]]
    assert 7 * (len(p["keys"]) + 1) + 3 * len(p["y"]) == total and fits(p) == (path == 1)
    X = tagtrainref.design(p)
    ((c, y),) = tagtrainref.class_targets(p)
    for solver in (2, 0):
        t.train_bytes(eps, cost, solver)
        stats = t.tag_stats()
        assert [q["path"] for q in stats["problems"]] == [path]
        wg = t.tag_weights(0)[c]
        pos = int((y > 0).sum())
        tol = eps * max(min(pos, len(y) - pos), 1) / len(y)
        g = trainref.gradient(X, y, wg, cost, solver)
        assert np.linalg.norm(g) <= tol * np.linalg.norm(trainref.gradient(X, y, np.zeros_like(wg), cost, solver)) * 1.01
        st = stats["problems"][0]["classes"][c]
        assert st["iterations"] >= 1
        check_class_stats(st, p, y, wg, cost, solver)


def check_solver(name, solver, path=0, eps=0.01, cost=1.0):
    params = CASES[name]
    sents = corpus(params[0], params[1], params[2])
    t, r = run_pair(params, sents, path=path)
    model = t.train_bytes(eps, cost, solver)
    models = r.models()
    ref = [(m["token"], p) for m in models for p in m["problems"]]
    stats = t.tag_stats()
    weights = []
    unstable = UNSTABLE.get((name, solver, path), set())
    seen_unstable = set()
    for i, (tok, p) in enumerate(ref):
        W = t.tag_weights(i)
        weights.append(W)
        assert stats["problems"][i]["path"] == (1 if path == 0 and fits(p) else 2)
        X = tagtrainref.design(p)
        k = len(p["candidates"])
        if k == 2:
            assert np.array_equal(W[1], -W[0])
        for c, y in tagtrainref.class_targets(p):
            wr, it, cg, g0, _ = trainref.tron(X, y, cost, eps, solver)
            wg = W[c]
            pos = int((y > 0).sum())
            tol = eps * max(min(pos, len(y) - pos), 1) / len(y)
            g = trainref.gradient(X, y, wg, cost, solver)
            assert np.linalg.norm(g) <= tol * np.linalg.norm(trainref.gradient(X, y, np.zeros_like(wg), cost, solver)) * 1.01, (tok, p["slot"], c)
            fg, fr = trainref.objective(X, y, wg, cost, solver), trainref.objective(X, y, wr, cost, solver)
            assert abs(fg - fr) <= 1e-3 * abs(fr), (tok, p["slot"], c)
            st = stats["problems"][i]["classes"][c]
            check_class_stats(st, p, y, wg, cost, solver)
            same = (st["iterations"], st["cg_steps"]) == (it, cg) and np.linalg.norm(wg - wr) <= 1e-7 * np.linalg.norm(wr)
            if not same:
                seen_unstable.add((tok, p["slot"], c))
    assert seen_unstable <= unstable, sorted(seen_unstable - unstable)
    sm = stats["summary"]
    assert sm["problems_in_kernel"] == sum(1 for q in stats["problems"] if q["path"] == 1)
    assert sm["problems_large"] == sum(1 for q in stats["problems"] if q["path"] == 2)
    # the model: the boundary part as the same trainer gives it without tags, then the restatement's quantisation and layout of the
    # library's weights, byte for byte
    _, _, _, charw, charn, typew, typen = params
    plain = api.Trainer(charw, charn, typew, typen)
    utf8, boff, labels = pack(sents)[:3]
    plain.add_packed(utf8, boff, labels)
    boundary = plain.train_bytes(eps, cost, solver)
    assert model == tagtrainref.with_tag_models(boundary, tagtrainref.tag_models(models, weights))
    md, used = modelfmt.decode_model(model)
    assert used == len(model) and len(md.tag_models) == len(models)
    assert t.train_bytes(eps, cost, solver) == model
    t2, _ = run_pair(params, sents, path=path)
    assert t2.train_bytes(eps, cost, solver) == model
    return model, stats


def decided_corpus():
    return corpus(DECIDED[0], DECIDED[1], DECIDED[2], decided=True)


def tokenized_lines(sents):
    out = []
    for text, bounds, nt, tags in sents:
        s = api.Sentence.from_raw(text)
        s._boundaries = np.asarray(bounds, np.uint8)
        s._tags, s._n_tags = list(tags), nt
        out.append(s.write_tokenized_text())
    return out


def check_round_trip(eps=0.01, cost=1.0, solver=2):
    """The model trained on the decided corpus, loaded with predict_tags: evaluate on the training lines counts every token correct
    (boundaries and tags), and the tagged writer gives the training lines back."""
    sents = decided_corpus()
    t, _ = run_pair(DECIDED, sents, tag_dictionary=())
    model = t.train(eps, cost, solver)
    pred = api.Predictor(model, predict_tags=True)
    lines = tokenized_lines(sents)
    r = pred.evaluate(lines, predict_tags=True, no_norm=True)
    n_tokens = sum(len(ln.split(" ")) for ln in lines)
    assert r["n_ref"] == n_tokens
    assert r["n_cor"] == r["n_ref"] == r["n_sys"], r
    assert pred.tokenize([s[0] for s in sents], tagged=True) == lines


def check_oracle_round_trip(name, eps=0.01, cost=1.0, solver=2):
    """The model trained on a suite corpus ("small", "large" or "decided"), loaded with predict_tags, against the CPU oracle run on
    the same model bytes: the tagged writer over the training sentences with their gold boundaries (Unknown ones included), and the
    `evaluate` counters with predicted tags over the training lines."""
    from oracle import cbind
    from tests import evalref
    from tests.test_evaluate_gpu import _oracle_system
    params = DECIDED if name == "decided" else CASES[name]
    sents = decided_corpus() if name == "decided" else corpus(params[0], params[1], params[2])
    # the decided corpus has one slot: the dictionary's three-slot surface would make every system tag vector three long
    t, _ = run_pair(params, sents, tag_dictionary=() if name == "decided" else TAG_DICTIONARY)
    raw = t.train_bytes(eps, cost, solver)
    model = api.Model.read_slice(raw)[0]
    assert any(m.char_ngram_model or m.type_ngram_model for m in model.tag_models())
    pred = api.Predictor(model, predict_tags=True)
    orc = cbind.OraclePredictor(raw, True)
    utf8, boff = api.pack_texts([s[0].encode("utf-8") for s in sents])
    # fill_tags for the gold boundaries, Unknown ones included: the candidate chosen per char and slot
    gold = np.concatenate([s[1] for s in sents])
    ooff = api.count_boundaries(utf8, boff)
    tags, _, models = orc.fill_tags_batch(utf8, boff, ooff, gold, want_scores=False)
    assert (models >= 0).any() and (tags > 0).any()   # trained candidates other than the first are chosen somewhere
    assert np.array_equal(pred.fill_tags_packed(utf8, boff, ooff, gold), tags)
    # the writer: the model's own boundaries (the writer takes no Unknown), fill_tags and the "/tag" suffixes
    scores, labels, ooff2 = pred.predict_packed(utf8, boff)
    o_scores, o_labels, _, _ = orc.predict_batch(utf8, boff)
    assert np.array_equal(ooff, ooff2) and np.array_equal(scores, o_scores) and np.array_equal(labels, o_labels)
    objs = []
    for i, (text, _, _, _) in enumerate(sents):
        s = api.Sentence.from_raw(text)
        s._boundaries = labels[int(ooff[i]):int(ooff[i + 1])].copy()
        objs.append(s)
    got = pred.write_tokenized_batch(objs, tagged=True)
    tags, _, models = orc.fill_tags_batch(utf8, boff, ooff, labels, want_scores=False)
    text, toff = orc.write_tokenized_batch(utf8, boff, ooff, labels, tags, models)
    want = [bytes(text[int(toff[i]):int(toff[i + 1])]).decode("utf-8") for i in range(len(sents))]
    assert got == want and any("/" in ln for ln in got)
    # evaluate: parse, predict, fill_tags and the counters
    lines = [ln for ln in tokenized_lines(sents) if ln]
    r = pred.evaluate(lines, predict_tags=True, no_norm=True)
    ref = evalref.evaluate(lines, _oracle_system(raw, model.tag_models(), [], False, True), predict_tags=True, no_norm=True)
    assert {k: r[k] for k in ref} == ref
    assert r["n_ref"] > 0 and r["n_cor"] > 0
    return r


def check_errors():
    plain = api.Trainer(2, 2, 2, 1)
    sents = corpus(11, 5, 3)
    arrays = pack(sents)
    with pytest.raises(api.VaporettoError, match="without VPT_TRAIN_TAGS"):
        plain.add_packed_tagged(*arrays)
    with pytest.raises(api.VaporettoError, match="without VPT_TRAIN_TAGS"):
        plain.tag_problems()
    with pytest.raises(api.VaporettoError, match="without VPT_TRAIN_TAGS"):
        plain.set_tag_dictionary([("あ", ["x"])])
    with pytest.raises(ValueError):
        api.Trainer(2, 2, 2, 1, ignore_tags=True, train_tags=True)
    # unknown flag bits
    import ctypes as C
    from vaporetto_amd import _lib
    for flags in (2, 3, 1 << 31):
        prm = _lib.TrainParams(2, 2, 2, 1, 0, flags)
        h = C.c_void_p()
        assert _lib.load().vpt_trainer_create(C.addressof(prm), None, None, 0, 0, C.byref(h)) == _lib.VPT_INVALID_ARGUMENT
        assert "flags: " in _lib.last_error()
    # a bad tag CSR is rejected, and nothing is added
    t = api.Trainer(2, 2, 2, 1, train_tags=True)
    utf8, boff, labels, n_tags, tindex, so, tb = arrays
    assert len(so) > 3
    bad = tindex.copy()
    k = int(np.flatnonzero(np.diff(bad.astype(np.int64)) > 0)[0])
    bad[k], bad[k + 1] = bad[k + 1], bad[k]
    with pytest.raises(api.VaporettoError, match="tag_index"):
        t.add_packed_tagged(utf8, boff, labels, n_tags, bad, so, tb)
    bad = tindex.copy()
    bad[-1] += 5
    with pytest.raises(api.VaporettoError, match="tag_index"):
        t.add_packed_tagged(utf8, boff, labels, n_tags, bad, so, tb)
    bad = so.copy()
    bad[-1] += 1000
    with pytest.raises(api.VaporettoError, match="span_offsets"):
        t.add_packed_tagged(utf8, boff, labels, n_tags, tindex, bad, tb)
    bad = so.copy()
    bad[1], bad[2] = bad[2] + 1, bad[1]
    with pytest.raises(api.VaporettoError, match="span_offsets"):
        t.add_packed_tagged(utf8, boff, labels, n_tags, tindex, bad, tb)
    nul = tb.copy()
    nul[0] = 0
    with pytest.raises(api.VaporettoError, match=r"must not contain NULL \(sentence \d+\)"):
        t.add_packed_tagged(utf8, boff, labels, n_tags, tindex, so, nul)
    overlong = tb.copy()
    overlong[:2] = (0xC0, 0x80)   # an overlong NUL: no NUL byte, and no UTF-8 that the model's loader takes
    with pytest.raises(api.VaporettoError, match=r"tags: invalid UTF-8 \(sentence \d+\)"):
        t.add_packed_tagged(utf8, boff, labels, n_tags, tindex, so, overlong)
    assert t.n_features() == 0 and t.tag_problems() == []
    t.add_packed_tagged(*arrays)
    for solver in (1, 3, 4, 5, 6, 7):
        with pytest.raises(api.VaporettoError, match="only 0 and 2 are implemented"):
            t.train_bytes(0.1, 1.0, solver)
    # a corpus without a tagged token: no tag models but the dictionary's
    u = api.Trainer(2, 2, 2, 1, train_tags=True, tag_dictionary=[("辞書", ["名詞"])])
    u.add_examples([api.Sentence.from_tokenized("これ は"), api.Sentence.from_tokenized("は これ")])
    md = modelfmt.decode_model(u.train_bytes(0.1, 1.0, 2))[0]
    assert [(m.token, m.tags) for m in md.tag_models] == [("辞書", [["名詞"]])]
