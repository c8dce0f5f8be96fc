"""TEST INFRASTRUCTURE: the checks of solver 5 for tag models (Trainer(l1r=True, train_tags=True, l1r_tags=True)) shared by the emulator
tests (tests/test_train_tags_l1_emu.py) and the GPU tests (tests/test_train_tags_l1_gpu.py), against the restatement of
tests/tagl1ref.py, on the corpora of tests/tagtrainsuite.py and on the smallest shapes that reach each path of the kernel."""
import functools

import numpy as np
import pytest

from tests import l1ref, tagl1ref, tagtrainref, tagtrainsuite, trainref
from vaporetto_amd import api, modelfmt

# eps: the objectives of two solves (the library's and the restatement's, or liblinear's) are compared to 1e-3 relative below.  Each
# stops at a violation sum of at most eps * min(pos, neg) / rows <= eps / 2 of the first, by another path once a sum in another order
# has turned one line search, so the bound asks for solves that are themselves closer than 1e-3: eps = 0.01 promises 5e-3 and no
# more (on seed 16 a pair ends 1.7e-3 apart), eps = 1e-3 promises 5e-4.
EPS, COST = 1e-3, 1.0
LDS_DOUBLES = 7256   # include/vaporetto_hip.h: solver 5 in-kernel iff (features + 1) + rows <= 7256
# The corpora: tagtrainsuite.CASES' shapes; the seed of "large" is chosen on the restatement alone, at this eps and at 0.01 (tests/test_train_tags_l1_ref.py holds
# it to that): on most seeds some problem of a handful of rows never meets the stopping rule -- a weight of some 1e-16, what a step to
# "zero" left behind in floating point, is not moved again (|d| < 1e-12 skips the column, as in liblinear) while its violation
# |G -+ 1| stays in every sweep's sum, and the sweeps run to kL1rMaxSweeps: with tagtrainsuite's seed 12 on 4 of 65 pairs, and on at
# least one pair with 21 of the seeds 13 .. 39.  Seed 16 has 72 pairs and none such, so every check below holds for every pair.
CASES = {"small": tagtrainsuite.CASES["small"], "large": (16,) + tagtrainsuite.CASES["large"][1:]}
# (case, surface, slot, class): pairs on which the restatement itself ends with violation(w) > tolerance * violation(0) (the sweep's sum
# is taken along the sweep); skipped for the violation check alone, at most 5 % of the pairs.  None with the seeds above.
REF_MISSES = set()
# (case, path) -> (surface, slot, class) whose sweeps or halvings are not the restatement's: the sums run in another order (tiles
# against numpy's), so a line search or the stopping decision can fall the other way.  Recorded from the emulator and the MI355X.
_WIDE = {("X", 0, c) for c in range(4)}   # some 2000 halvings over the four classes: one that turns moves the counts
UNSTABLE = {
    ("large", 0): {("あ", 0, 1)}, ("large", 1): {("あ", 0, 1)},
    ("halvings", 0): {("X", 0, 0)}, ("halvings", 1): {("X", 0, 0)},   # 4 halvings against the restatement's 2
    ("wide", 0): _WIDE, ("wide", 1): _WIDE,
}


def fits(p):
    return len(p["keys"]) + 1 + len(p["y"]) <= LDS_DOUBLES


def make_trainer(params, sents, tag_dictionary, path=0, **kw):
    _, _, _, charw, charn, typew, typen = params
    t = api.Trainer(charw, charn, typew, typen, train_tags=True, tag_dictionary=tag_dictionary, **kw)
    t.set_tag_path(path)
    t.add_packed_tagged(*tagtrainsuite.pack(sents))
    return t


# ---- the shapes the kernel can get wrong: charn = typen = 1, one problem (surface X), the right-hand char planted an exact number of times
def shape_corpus(counts, n_class=2, seed=0):
    """Sentences "<a|b>X<right>" of three one-char tokens; counts: right char -> how often.  X's tag follows the right char (its index
    mod n_class), one in ten drawn anew.  The features of X are the char and the type on either side, so the right char's column has
    exactly counts[right] nonzeros, the left type's as many as there are rows."""
    rng = np.random.default_rng(seed)
    rights = [ch for ch, n in counts.items() for _ in range(n)]
    order = rng.permutation(len(rights))
    idx = {ch: k for k, ch in enumerate(counts)}
    out = []
    for i, q in enumerate(order):
        right = rights[q]
        cls = int(rng.integers(0, n_class)) if rng.random() < 0.1 else idx[right] % n_class
        out.append(("ab"[i % 2] + "X" + right, np.array([1, 1], np.uint8), 1, [None, "t%d" % cls, None]))
    # the boundary model needs a boundary that is none
    return out + [("ab", np.array([0], np.uint8), 1, [None, None])] * 3


def _kanji(n):
    return {chr(0x4E00 + k): 2 for k in range(n)}


def limit_counts(total):
    """One problem with (features + 1) + rows == total: the features are 2 left chars, 2 right chars, 1 left type and 2 right types."""
    rows = total - 8
    return {"c": rows // 2, "1": rows - rows // 2}


SHAPES = {  # name -> (right char counts, classes, the path taken by size, the corpus's seed)
    "lane_wave": ({"c": 63, "d": 64, "e": 65, "1": 40}, 2, 1, 9),          # columns of exactly 63, 64 and 65 nonzeros
    "wave_block": ({"c": 1023, "d": 1024, "e": 1025, "1": 50}, 2, 1, 10),  # columns of exactly 1023, 1024 and 1025 nonzeros
    "wide": (_kanji(300), 4, 1, 4),                                         # a group of more than 256 columns; four candidates
    "limit": (limit_counts(LDS_DOUBLES), 2, 1, 5),                          # exactly at the fit rule's limit
    "past_limit": (limit_counts(LDS_DOUBLES + 1), 2, 2, 10),                # one double past it
    "halvings": ({"c": 30, "d": 20, "1": 10}, 2, 1, 5),                     # line searches that halve (the seed is chosen for it)
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(params, sentences, tag dictionary) of a suite corpus or a shape."""
    if name in SHAPES:
        counts, n_class, _, seed = SHAPES[name]
        return tagtrainsuite.LIMIT_PARAMS, shape_corpus(counts, n_class, seed), ()
    params = tagtrainsuite.DECIDED if name == "decided" else CASES[name]
    sents = tagtrainsuite.decided_corpus() if name == "decided" else tagtrainsuite.corpus(params[0], params[1], params[2])
    return params, sents, () if name == "decided" else tagtrainsuite.TAG_DICTIONARY


@functools.lru_cache(maxsize=None)
def reference(name):
    """(models, [(surface, problem, X, W, stats)] by the restatement): computed once, shared, read-only."""
    params, sents, td = case(name)
    r = tagtrainref.RefTagTrainer(params[4], params[6], td)
    for s in sents:
        r.add_example(*s)
    models = r.models()
    out = []
    for m in models:
        for p in m["problems"]:
            W, st = tagl1ref.solve(p, EPS, COST)
            W.flags.writeable = False
            out.append((m["token"], p, tagtrainref.design(p), W, st))
    return models, out


@functools.lru_cache(maxsize=None)
def trained(name, path):
    """The library's solver-5 training of a case on a path: (trainer, model bytes, tag_stats, weights per problem)."""
    params, sents, td = case(name)
    t = make_trainer(params, sents, td, path, l1r=True, l1r_tags=True)
    model = t.train_bytes(EPS, COST, 5)
    stats = t.tag_stats()
    weights = [t.tag_weights(i) for i in range(len(stats["problems"]))]
    return t, model, stats, weights


def check_solution(name, path):
    """Checks 1, 2, 4 (counts) and 5 of every (problem, class), and the path taken."""
    _, ref = reference(name)
    _, _, stats, weights = trained(name, path)
    assert len(ref) == len(weights)
    unstable, seen_unstable = UNSTABLE.get((name, path), set()), set()
    for i, (tok, p, X, Wr, st_r) in enumerate(ref):
        W = weights[i]
        assert stats["problems"][i]["path"] == (1 if path == 0 and fits(p) else 2)
        if len(p["candidates"]) == 2:
            assert np.array_equal(W[1], -W[0])                                                     # 5
        for c, y in tagtrainref.class_targets(p):
            st = stats["problems"][i]["classes"][c]
            fg, fr = l1ref.objective_l1(X, y, W[c], COST), l1ref.objective_l1(X, y, Wr[c], COST)
            tol = l1ref.tolerance(y, EPS)
            vg, v_zero = l1ref.violation(X, y, W[c], COST), l1ref.violation(X, y, 0 * W[c], COST)
            print("%s path %d %r slot %d class %d: %d sweeps (restatement %d), %d halvings (%d), objective %.9g (%.9g), violation / "
                  "violation(0) %.3g (tol %.3g)" % (name, path, tok, p["slot"], c, st["iterations"], st_r[c][0], st["cg_steps"], st_r[c][1],
                                                    fg, fr, vg / v_zero, tol))
            assert abs(fg - fr) <= 1e-3 * abs(fr), (tok, p["slot"], c)                             # 1
            if (name, tok, p["slot"], c) not in REF_MISSES:
                assert vg <= tol * v_zero * 1.01, (tok, p["slot"], c)                              # 2
            if (st["iterations"], st["cg_steps"]) != st_r[c][:2]:
                seen_unstable.add((tok, p["slot"], c))
    assert seen_unstable <= unstable, sorted(seen_unstable - unstable)                             # 4
    sm = stats["summary"]
    assert sm["problems_in_kernel"] == sum(1 for q in stats["problems"] if q["path"] == 1)
    assert sm["problems_large"] == sum(1 for q in stats["problems"] if q["path"] == 2)
    return stats


def check_library_stats(name, path):
    """Check 3: the library's own stats of every (problem, class)."""
    _, ref = reference(name)
    _, _, stats, weights = trained(name, path)
    bad = []
    for i, (tok, p, X, _, _) in enumerate(ref):
        for c, y in tagtrainref.class_targets(p):
            st = stats["problems"][i]["classes"][c]
            tol = l1ref.tolerance(y, EPS)
            fg = l1ref.objective_l1(X, y, weights[i][c], COST)
            print("%s path %d %r slot %d class %d: %d sweeps, gnorm / gnorm0 %.3g (tol %.3g), objective %.12g (numpy %.12g)"
                  % (name, path, tok, p["slot"], c, st["iterations"], st["gnorm"] / st["gnorm0"], tol, st["objective"], fg))
            if not (st["gnorm"] <= tol * st["gnorm0"] and 1 <= st["iterations"] < 1000 and abs(st["objective"] - fg) <= 1e-9 * fg):
                bad.append((tok, p["slot"], c))
    assert not bad, bad


def check_paths_agree(name):
    """Check 4: both paths use one summation tree: the same sweeps and halvings, the weights to 1e-7 relative."""
    _, _, s0, w0 = trained(name, 0)
    _, _, s1, w1 = trained(name, 1)
    assert {q["path"] for q in s1["problems"]} == {2} and 1 in {q["path"] for q in s0["problems"]}
    for i, (a, b) in enumerate(zip(w0, w1)):
        for c in range(a.shape[0]):
            x, y = s0["problems"][i]["classes"][c], s1["problems"][i]["classes"][c]
            assert (x["iterations"], x["cg_steps"]) == (y["iterations"], y["cg_steps"]), (i, c)
            assert np.linalg.norm(a[c] - b[c]) <= 1e-7 * np.linalg.norm(b[c]), (i, c)


def n_tag_weights(model_bytes):
    md = modelfmt.decode_model(model_bytes)[0]
    return sum(int(np.count_nonzero(w.weights)) for m in md.tag_models for part in (m.char_ngram_model, m.type_ngram_model)
               for d in part for w in d.weights)


def check_model(name, path):
    """Checks 6 and 7: the model bytes, determinism, and fewer tag n-gram weights than solver 2 writes."""
    params, sents, td = case(name)
    models, _ = reference(name)
    t, model, _, weights = trained(name, path)
    _, _, _, charw, charn, typew, typen = params
    plain = api.Trainer(charw, charn, typew, typen, l1r=True)
    plain.add_packed(*tagtrainsuite.pack(sents)[:3])
    boundary = plain.train_bytes(EPS, COST, 5)
    assert model == tagtrainref.with_tag_models(boundary, tagtrainref.tag_models(models, weights))   # 6
    md, used = modelfmt.decode_model(model)
    assert used == len(model) and len(md.tag_models) == len(models)
    t2 = make_trainer(params, sents, td, path, l1r=True, l1r_tags=True)
    assert t2.train_bytes(EPS, COST, 5) == model
    dense = t.train_bytes(EPS, COST, 2)
    print("%s path %d: %d tag n-gram weights, solver 2 %d" % (name, path, n_tag_weights(model), n_tag_weights(dense)))
    assert n_tag_weights(model) < n_tag_weights(dense)                                               # 7
    assert t.train_bytes(EPS, COST, 5) == model


def check_tron_unchanged(name):
    """Check 8: with the three flags solvers 0 and 2 give the bytes of a train_tags trainer without them."""
    params, sents, td = case(name)
    full = make_trainer(params, sents, td, l1r=True, l1r_tags=True)
    tags = make_trainer(params, sents, td)
    for solver in (0, 2):
        assert full.train_bytes(EPS, COST, solver) == tags.train_bytes(EPS, COST, solver)


def check_shape(name):
    """Check 9: a shape on the path its size gives it and on the global-memory path, each with checks 1 to 5."""
    _, n_class, path, _ = SHAPES[name]
    _, ref = reference(name)
    ((_, p, X, _, _),) = ref
    assert len(p["candidates"]) == n_class and fits(p) == (path == 1)
    col_len = np.diff(X.tocsc().indptr)
    for paths in (0, 1):
        stats = check_solution(name, paths)
        assert [q["path"] for q in stats["problems"]] == [path if paths == 0 else 2]
        check_library_stats(name, paths)
    if path == 1:
        check_paths_agree(name)
    return p, col_len


def check_round_trip():
    """Check 10: the solver-5 model of the decided corpus, loaded with predict_tags: fill_tags through the library equals the CPU
    oracle's on the training lines.  An L1 model need not give its training tags back: that count is printed."""
    from oracle import cbind
    params, sents, td = case("decided")
    t = make_trainer(params, sents, td, l1r=True, l1r_tags=True)
    raw = t.train_bytes(EPS, COST, 5)
    model = api.Model.read_slice(raw)[0]
    assert any(m.char_ngram_model or m.type_ngram_model for m in model.tag_models())
    pred = api.Predictor(model, predict_tags=True)
    orc = cbind.OraclePredictor(raw, True)
    utf8, boff = api.pack_texts([s[0].encode("utf-8") for s in sents])
    gold = np.concatenate([s[1] for s in sents])
    ooff = api.count_boundaries(utf8, boff)
    tags, _, models = orc.fill_tags_batch(utf8, boff, ooff, gold, want_scores=False)
    assert (models >= 0).any()
    assert np.array_equal(pred.fill_tags_packed(utf8, boff, ooff, gold), tags)
    lines = tagtrainsuite.tokenized_lines(sents)
    r = pred.evaluate(lines, predict_tags=True, no_norm=True)
    print("decided corpus, solver 5: %d of %d tokens with boundaries and tags as trained" % (r["n_cor"], r["n_ref"]))


def check_errors():
    import ctypes as C
    from vaporetto_amd import _lib
    for flags in (8, 8 | 1, 8 | 4):
        prm = _lib.TrainParams(2, 2, 2, 1, 0, flags)
        h = C.c_void_p()
        assert _lib.load().vpt_trainer_create(C.addressof(prm), None, None, 0, 0, C.byref(h)) == _lib.VPT_INVALID_ARGUMENT
        assert _lib.last_error().split(": ", 1)[1].startswith("flags: ")
    for kw in ({}, {"l1r": True}, {"train_tags": True}):
        with pytest.raises(ValueError):
            api.Trainer(2, 2, 2, 1, l1r_tags=True, **kw)
    params, sents, td = case("small")
    t = make_trainer(params, sents[:20], td, l1r=True, l1r_tags=True)
    for solver in (1, 3, 4, 6, 7):
        with pytest.raises(api.VaporettoError, match="solver: only 0, 2 and 5 are implemented"):
            t.train_bytes(EPS, COST, solver)
    assert t.train_bytes(EPS, COST, 5)
    # without the third flag the pair is refused as before
    both = make_trainer(params, sents[:20], td, l1r=True)
    with pytest.raises(api.VaporettoError, match="solver 5: tag models are trained with solvers 0 and 2 only"):
        both.train_bytes(EPS, COST, 5)
