"""The scoring kernel reads and writes global memory through a cache policy per class of access (device_common.h, MemPolicy;
kernels_fast.hip, kPol*).  A policy may only change where a line is kept, never what is read or written: these tests run the
paths behind every class -- deep entries, deep rows and `xrows`, several tiles and their edges, text and outputs rewritten in
place between two calls, the `xcid` side table -- through the C ABI and compare scores and labels bit for bit with the CPU
oracle, on the emulator (the plain stand-ins) and on the device (the real loads and stores)."""
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
    import gc
    gc.collect()   # handles made by the emulated library are destroyed by it
    devmem.EMULATED = saved_emulated
    _lib._lib = saved


def _predictor(m):
    raw = encode_model(m)
    pred = api.Predictor(api.Model.read_slice(raw)[0], False)
    assert pred.info()["packed"] == 1   # the specialised kernel scores it
    return pred, cbind.OraclePredictor(raw)


def _check_packed(pred, orc, texts):
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    scores, labels, ooff = pred.predict_packed(utf8, boff)
    o_scores, o_labels, o_ooff, _ = orc.predict_batch(utf8, boff, nthreads=4)
    assert np.array_equal(ooff, o_ooff) and np.array_equal(scores, o_scores) and np.array_equal(labels, o_labels)


class _Resident:
    """A batch resident in device buffers, scored in place by vpt_predict_batch_device."""

    def __init__(self, pred, orc, texts):
        self.orc = orc
        utf8, self.boff = api.pack_texts([t.encode("utf-8") for t in texts])
        _, _, ooff, _ = orc.predict_batch(utf8, self.boff, nthreads=4)
        self.S, self.nb = len(texts), int(ooff[-1])
        self.mb = int(np.max(np.diff(self.boff.astype(np.int64))))
        self.d_text = devmem.put(np.concatenate([utf8, np.zeros(16, np.uint8)]))
        self.d_boff, self.d_ooff = devmem.put(self.boff.astype(np.uint64)), devmem.put(ooff.astype(np.uint64))
        self.d_scores, self.d_labels = devmem.zeros(self.nb + 1, np.int32), devmem.zeros(self.nb + 1, np.uint8)
        self.batch = api.DeviceBatch(pred)

    def predict_and_check(self, texts):
        utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
        assert np.array_equal(boff, self.boff)   # the same shape, byte for byte
        self.d_text.set(np.concatenate([utf8, np.zeros(16, np.uint8)]))
        self.batch.predict(self.d_text.ptr, self.d_boff.ptr, self.d_ooff.ptr, self.S, self.nb, self.mb, self.d_scores.ptr, self.d_labels.ptr, devmem.stream())
        self.batch.sync()
        o_scores, o_labels, _, _ = self.orc.predict_batch(utf8, boff, nthreads=4)
        assert np.array_equal(self.d_scores.get(self.nb), o_scores) and np.array_equal(self.d_labels.get(self.nb), o_labels)
        assert self.d_scores.get(self.nb + 1)[-1] == 0 and self.d_labels.get(self.nb + 1)[-1] == 0   # nothing past the batch's last boundary


def _deep_model(big):
    return randmodel.rand_model(77, alphabet="kana", wc=3, wt=3, n_char=150, n_dict=250, max_word=9, big=big)


@pytest.mark.parametrize("big", [False, True], ids=["rows in their fields", "big rows"])
def test_deep_entries_deep_rows_and_xrows(backend, big):
    """Dictionary words of 4 .. 9 chars: trie steps below depth 3 read deep entries and their rows; with big=True nearly every row has a
    value outside its fields, so deep rows come from `xrows` and the short patterns' rows from the general tables."""
    m = _deep_model(big)
    assert sum(len(r.word) > 3 for r in m.dict_model) > 100
    pred, orc = _predictor(m)
    _check_packed(pred, orc, randmodel.rand_sentences(12, m, 500, alphabet="kana", max_len=70))


def _kana_text(rng, n):
    alpha = randmodel.ALPHABETS["kana"]
    return "".join(alpha[int(i)] for i in rng.integers(0, len(alpha), n))


def _tile_edge_texts(seed):
    """Tiles of 256 flat positions at row window 3 (a sentence of n chars takes n + 3 of them): four sentences of 61 chars fill tile 0 to its
    last slot, a sentence of one char opens tile 1, and the rest makes more than three tiles."""
    lens = [61, 61, 61, 61, 1, 40, 1, 70, 13] + [int(n) for n in np.random.default_rng(1).integers(1, 71, 40)]   # the same for every seed
    rng = np.random.default_rng(seed)
    return [_kana_text(rng, n) for n in lens]


@pytest.mark.parametrize("force_cut", [False, True], ids=["whole-sentence tiles", "cut tiles"])
def test_tile_edges_and_outputs_rewritten_in_place(backend, force_cut, monkeypatch):
    """(ii) three tiles and more, a sentence that ends on a tile's last slot and a sentence of one char; (iii) the same buffers predicted
    again after the text in them has changed, and once more after it has changed back: a bypassed L1 or a line dropped from the L2 must
    never serve a text byte, a score or a label of the call before."""
    monkeypatch.setenv("VPT_TILE_FLAT", "256")
    if force_cut:
        monkeypatch.setenv("VPT_FORCE_CUT_TILES", "1")
    pred, orc = _predictor(_deep_model(False))
    a, b = _tile_edge_texts(3), _tile_edge_texts(4)
    assert a != b and [len(t) for t in a] == [len(t) for t in b]
    r = _Resident(pred, orc, a)
    r.predict_and_check(a)
    plan = r.batch.last_plan()
    assert plan["kind"] == ("cut tiles" if force_cut else "whole-sentence tiles") and plan["tile_flat"] == 256 and plan["tiles"] >= 3
    flat_start = np.cumsum([0] + [len(t) + 3 for t in a])
    assert flat_start[4] == 256 and len(a[4]) == 1   # sentence 3's last char sits in slot 255; the one-char sentence starts the next tile
    r.predict_and_check(b)
    r.predict_and_check(a)


def test_non_bmp_alphabet_through_xcid(backend):
    """Pattern chars outside the BMP get their ids from the side table `xcid`, probed by the lanes that hold such a char."""
    m = randmodel.rand_model(21, alphabet="mixed", wc=3, wt=3, n_char=120, n_dict=120, max_word=6)
    assert any(ord(c) >= 0x10000 for d in m.char_ngram_model for c in d.ngram) and any(ord(c) >= 0x10000 for r in m.dict_model for c in r.word)
    pred, orc = _predictor(m)
    _check_packed(pred, orc, randmodel.rand_sentences(3, m, 400, alphabet="mixed", max_len=70))
