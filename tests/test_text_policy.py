"""The specialised scoring kernel loads a launch's text plain or non-temporal (ScoreParams::text_nt): the host decides per launch from the bytes
the launch streams (capi_internal.hpp, text_policy_for), `VPT_TEXT_POLICY=plain|nt` forces a side, `last_plan()["text_policy"]` reports it.
A policy decides where a line is kept, never what is read: both forms of the staging loop must give the CPU oracle's scores and labels bit
for bit -- on the emulator (where both are the plain load, but the branch and the rule are the product's) and on the device (the real loads)
-- at the shapes where the loop can go wrong: one chunk, a partial last chunk, a text that does not start on a 16-byte boundary, a text that
ends on one, several tiles, cut tiles with their halos, the wider row window, and a text rewritten in place between two calls."""
import gc

import ctypes as C
import numpy as np
import pytest

from oracle import cbind
from tests import devmem, randmodel
from vaporetto_amd import _lib, api
from vaporetto_amd.modelfmt import encode_model


@pytest.fixture(scope="module", params=["emulator", pytest.param("device", marks=pytest.mark.gpu)])
def backend(request):
    if request.param == "device":
        yield request.param
        return
    from tests import emu
    lib = emu.load()
    saved, saved_emulated = _lib._lib, devmem.EMULATED
    _lib._lib = lib
    devmem.EMULATED = True
    yield request.param
    gc.collect()   # handles made by the emulated library are destroyed by it
    devmem.EMULATED = saved_emulated
    _lib._lib = saved


MODELS = {
    "mixed": lambda: randmodel.rand_model(21, alphabet="mixed", wc=3, wt=3, n_char=120, n_dict=120, max_word=6),       # 1-, 2-, 3- and 4-byte chars
    "kana": lambda: randmodel.rand_model(77, alphabet="kana", wc=3, wt=3, n_char=150, n_dict=250, max_word=9),
    "charw4": lambda: randmodel.rand_model(5, alphabet="mixed", wc=4, wt=4, max_n=4, n_char=120, n_dict=60, max_word=6),  # row window 4: launch_wide
}


@pytest.fixture(scope="module")
def predictors(backend):
    """name -> (model, predictor, oracle), each compiled once per backend and destroyed by the library that made it."""
    made = {}

    def get(name):
        if name not in made:
            m = MODELS[name]()
            raw = encode_model(m)
            pred = api.Predictor(api.Model.read_slice(raw)[0], False)
            assert pred.info()["packed"] == 1   # the specialised kernel scores it
            made[name] = (m, pred, cbind.OraclePredictor(raw))
        return made[name]
    yield get
    made.clear()
    gc.collect()


def _force(monkeypatch, policy):
    """The knob is read when a workspace is made: set it before DeviceBatch()."""
    if policy is None:
        monkeypatch.delenv("VPT_TEXT_POLICY", raising=False)
    else:
        monkeypatch.setenv("VPT_TEXT_POLICY", policy)


GUARD_S, GUARD_L = 0x5A5A5A5A, 0xA5


class _Resident:
    """A batch in device buffers, scored in place by vpt_predict_batch_device.  The text starts `mis` bytes past a 16-byte boundary; scores and
    labels lie between two guard words that no launch may touch."""

    def __init__(self, pred, orc, texts, mis=0):
        self.orc = orc
        self.utf8, self.boff = api.pack_texts([t.encode("utf-8") for t in texts])
        _, _, ooff, _ = orc.predict_batch(self.utf8, self.boff, nthreads=4)
        self.S, self.nb = len(texts), int(ooff[-1])
        self.mb = int(np.max(np.diff(self.boff.astype(np.int64))))
        self.d_text = devmem.zeros(48 + len(self.utf8) + 32, np.uint8)
        self.t_off = 16 + (mis - self.d_text.ptr) % 16          # 16 .. 31 bytes in: the aligned chunk in front of the text is the buffer's own
        assert (self.d_text.ptr + self.t_off) % 16 == mis
        self.d_boff, self.d_ooff = devmem.put(self.boff.astype(np.uint64)), devmem.put(ooff.astype(np.uint64))
        self.d_scores = devmem.put(np.full(self.nb + 2, GUARD_S, np.int32))
        self.d_labels = devmem.put(np.full(self.nb + 2, GUARD_L, np.uint8))
        self.batch = api.DeviceBatch(pred)

    def predict_and_check(self, texts=None):
        utf8 = self.utf8
        if texts is not None:
            utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
            assert np.array_equal(boff, self.boff)   # the same shape, byte for byte
        host = np.zeros(48 + len(utf8) + 32, np.uint8)
        host[self.t_off:self.t_off + len(utf8)] = utf8
        self.d_text.set(host)
        self.batch.predict(self.d_text.ptr + self.t_off, self.d_boff.ptr, self.d_ooff.ptr, self.S, self.nb, self.mb, self.d_scores.ptr + 4,
                           self.d_labels.ptr + 1, devmem.stream())
        self.batch.sync()
        o_scores, o_labels, _, _ = self.orc.predict_batch(utf8, self.boff, nthreads=4)
        scores, labels = self.d_scores.get(self.nb + 2), self.d_labels.get(self.nb + 2)
        assert np.array_equal(scores[1:-1], o_scores) and np.array_equal(labels[1:-1], o_labels)
        assert scores[0] == GUARD_S and scores[-1] == GUARD_S and labels[0] == GUARD_L and labels[-1] == GUARD_L
        return self.batch.last_plan()


def _mixed_texts(m, n, seed, max_len=70):
    return randmodel.rand_sentences(seed, m, n, alphabet="mixed", min_len=1, max_len=max_len)


def _staging_cases(m):
    """name -> (texts, misalignment of the text's first byte)"""
    twenty = _mixed_texts(m, 20, 400)
    assert {len(c.encode("utf-8")) for t in twenty for c in t} == {1, 2, 3, 4} and min(map(len, twenty)) >= 1 and max(map(len, twenty)) <= 70
    on_chunk = _mixed_texts(m, 5, 401, max_len=30)
    on_chunk[-1] += "A" * (-sum(len(t.encode("utf-8")) for t in on_chunk) % 16)   # the last sentence ends exactly on a 16-byte chunk
    assert sum(len(t.encode("utf-8")) for t in on_chunk) % 16 == 0
    cases = {"one char": (["あ"], 0), "two chars": (["あ漢"], 0), "twenty sentences": (twenty, 0), "ends on a chunk": (on_chunk, 0)}
    for mis in (1, 7, 15):
        cases["text at +%d" % mis] = (twenty, mis)
    return cases


CASE_NAMES = ["one char", "two chars", "twenty sentences", "ends on a chunk", "text at +1", "text at +7", "text at +15"]


@pytest.mark.parametrize("policy", ["nt", "plain", None], ids=["nt", "plain", "rule"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_both_loads_give_the_oracles_outputs(backend, predictors, monkeypatch, case, policy):
    """Whole-sentence tiles of 256 flat positions: twenty sentences of 1 .. 70 chars put several into a tile and need a second one."""
    m, pred, orc = predictors("mixed")
    texts, mis = _staging_cases(m)[case]
    _force(monkeypatch, policy)
    monkeypatch.setenv("VPT_TILE_FLAT", "256")
    r = _Resident(pred, orc, texts, mis)
    assert r.nb == sum(len(t) - 1 for t in texts)
    plan = r.predict_and_check()
    assert plan["kind"] == "whole-sentence tiles" and plan["text_policy"] == (policy or "plain")
    if case == "twenty sentences":
        assert plan["tiles"] >= 2


@pytest.mark.parametrize("policy", ["nt", "plain"])
def test_cut_tiles_stage_their_halos_under_both_policies(backend, predictors, monkeypatch, policy):
    """Three sentences of a few hundred chars in tiles of 256 positions cut anywhere: every tile stages a halo that its neighbour stages too."""
    m, pred, orc = predictors("kana")
    rng = np.random.default_rng(11)
    alpha = randmodel.ALPHABETS["kana"]
    texts = ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), n)) for n in (310, 457, 289)]
    _force(monkeypatch, policy)
    monkeypatch.setenv("VPT_FORCE_CUT_TILES", "1")
    monkeypatch.setenv("VPT_TILE_FLAT", "256")
    plan = _Resident(pred, orc, texts).predict_and_check()
    assert plan["kind"] == "cut tiles" and plan["tiles"] >= 4 and plan["text_policy"] == policy


@pytest.mark.parametrize("policy", ["nt", "plain"])
def test_row_window_four_under_both_policies(backend, predictors, monkeypatch, policy):
    m, pred, orc = predictors("charw4")
    assert m.char_window_size == 4
    _force(monkeypatch, policy)
    plan = _Resident(pred, orc, _mixed_texts(m, 10, 402)).predict_and_check()
    assert plan["kind"] == "whole-sentence tiles" and plan["text_policy"] == policy


def _rule(text_bytes, boundaries, scores=True, labels=True):
    pol, thr = C.c_uint32(7), C.c_uint64(0)
    assert _lib.load().vpt_text_policy_for(text_bytes, boundaries, int(scores), int(labels), C.byref(pol), C.byref(thr)) == _lib.VPT_OK
    assert pol.value in (0, 1)
    return ("plain", "nt")[pol.value], thr.value


def test_the_rule(backend, predictors, monkeypatch):
    """nt exactly when text bytes + output bytes (4 a score, 1 a label) exceed the threshold; monotone; a small batch is plain; the knob wins."""
    thr = _rule(0, 0)[1]
    assert thr >= 1 << 20
    assert _rule(0, 0)[0] == "plain" and _rule(thr, 0)[0] == "plain" and _rule(thr + 1, 0)[0] == "nt"
    b = thr // 10
    assert _rule(thr - 5 * b, b)[0] == "plain" and _rule(thr - 5 * b + 1, b)[0] == "nt"                      # scores and labels: 5 bytes a boundary
    assert _rule(thr - 4 * b, b, labels=False)[0] == "plain" and _rule(thr - 4 * b + 1, b, labels=False)[0] == "nt"   # scores only: 4
    assert _rule(thr - b, b, scores=False)[0] == "plain" and _rule(thr - b + 1, b, scores=False)[0] == "nt"           # labels only: 1
    assert _rule(thr - 4 * b, b)[0] == "nt" and _rule(thr - 4 * b, b, scores=False)[0] == "plain"
    seen = [_rule(n, n // 3)[0] for n in range(0, 2 * thr, thr // 16)]
    assert seen == sorted(seen, reverse=True) and seen[0] == "plain" and seen[-1] == "nt"                     # "plain" ... "plain", "nt" ... "nt"
    m, pred, orc = predictors("mixed")
    texts = _mixed_texts(m, 6, 403)
    for policy in (None, "nt", "plain"):
        _force(monkeypatch, policy)
        assert _Resident(pred, orc, texts).predict_and_check()["text_policy"] == (policy or "plain")


def test_text_rewritten_in_place_under_nt(backend, predictors, monkeypatch):
    """The same buffers scored again after the text in them has changed, and once more after it has changed back: a non-temporal load must
    not be served a byte of the call before from anywhere."""
    m, pred, orc = predictors("kana")
    lens = [61, 61, 61, 61, 1, 40, 1, 70, 13, 33, 64, 64, 7]
    alpha = randmodel.ALPHABETS["kana"]

    def texts(seed):
        rng = np.random.default_rng(seed)
        return ["".join(alpha[int(i)] for i in rng.integers(0, len(alpha), n)) for n in lens]
    a, b = texts(3), texts(4)
    assert a != b
    _force(monkeypatch, "nt")
    monkeypatch.setenv("VPT_TILE_FLAT", "256")
    r = _Resident(pred, orc, a)
    assert r.predict_and_check(a)["text_policy"] == "nt"
    r.predict_and_check(b)
    r.predict_and_check(a)
