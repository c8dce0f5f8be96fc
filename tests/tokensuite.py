"""The checks of the token-stream feature (vpt_token_stream_batch, vpt_token_spans_batch[_device], api.VaporettoTokenizer) against the restatement
of tests/tokenref.py, run on the CPU emulator by tests/test_token_stream_emu.py and on the MI355X by tests/test_token_stream_gpu.py.  Every
comparison is exact."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

from tests import devmem, randmodel, tokenref
from vaporetto_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "token_stream_kat.json"), encoding="utf-8"))
KAT_MODEL = open(os.path.join(HERE, "golden", KAT["model"]), "rb").read()

# 1- to 4-byte chars of every CharacterType; digits and Latin (KyteaFullwidthFilter changes their byte length); linebreaks and spaces
ALPHABET = list("あいうカキ漢字09AZaz、。-") + ["𠮷", "🤌", "é", "ß", "１", "Ａ", "ｱ", "\n", "\r", "\r\n", " ", "\n\n", " \n", "\r "]
WSCONSTS = ["", "O", "D", "DR", "HTKO", "DRHTKO", "KO", "RD"]
# (char window, type window): the specialised kernels (windows up to 3) and the general ones
WINDOWS = [(1, 1), (2, 3), (3, 2), (5, 4), (8, 4)]


def predictor_for(seed, wc, wt):
    m = randmodel.rand_model(seed, alphabet=[a for a in ALPHABET if len(a) == 1], wc=wc, wt=wt)
    raw = api.Model(m).to_vec()
    return raw, api.Predictor(api.Model.read_slice(raw)[0], False, device=0)


def rand_doc(rng, lo, hi):
    n = rng.randint(lo, hi)
    return "".join(rng.choice(ALPHABET) for _ in range(n))


def batches(seed, big=200_000, tiny=3000):
    rng = random.Random(seed)
    small = ["", ""] + [rand_doc(rng, 1, 60) for _ in range(120)] + ["", "", ""] + ["あ", "a", "\n", "🤌"] + [rand_doc(rng, 1, 60) for _ in range(60)] + [""]
    many = [rand_doc(rng, 1, 3) for _ in range(tiny)]
    long_doc = rand_doc(rng, big, big + 50)      # every entry is a char at least: >= `big` chars, many runs of one document, many tiles
    mix = [rand_doc(rng, 1, 3) for _ in range(700)] + ["", long_doc[:big // 4]] + [rand_doc(rng, 1, 40) for _ in range(300)] + [long_doc[:7000], ""]
    return {"small": small, "tiny": many, "long": [long_doc], "mix": mix}


def check_csr(raw, pred, texts, wsconst):
    want_off, want_ends = tokenref.csr(tokenref.ends_batch(raw, texts, wsconst))
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    toff, ends = pred.token_stream_packed(utf8, boff, wsconst)
    assert np.array_equal(toff, want_off), (wsconst, int(np.argmax(toff != want_off)))
    assert np.array_equal(ends, want_ends), (wsconst, int(np.argmax(ends != want_ends[:len(ends)])) if len(ends) == len(want_ends) else (len(ends), len(want_ends)))
    toff2, ends2 = pred.token_stream_packed(utf8, boff, wsconst)          # two runs give identical arrays
    assert np.array_equal(toff, toff2) and np.array_equal(ends, ends2)
    return utf8, boff, toff, ends


def check_kat_cabi(case):
    pred = api.Predictor(api.Model.read_slice(KAT_MODEL)[0], False, device=0)
    if "G" in case["wsconst"]:
        pytest.skip("G is a host filter: covered through VaporettoTokenizer")   # (never reached: the callers pass the cases without G)
    utf8, boff = api.pack_texts([case["text"].encode("utf-8")])
    toff, ends = pred.token_stream_packed(utf8, boff, case["wsconst"])
    assert tokenref.tokens_from_ends(case["text"], [int(e) for e in ends]) == case["tokens"]
    assert int(toff[1]) == len(case["tokens"])


def check_kat_tokenizer(case):
    tok = api.VaporettoTokenizer(api.Model.read_slice(KAT_MODEL)[0], case["wsconst"], device=0)
    got = tok.token_stream(case["text"])
    assert [list(t._key()) for t in got] == case["tokens"]
    again = api.VaporettoTokenizer.deserialize(tok.predictor.save_compiled(), case["wsconst"], device=0)
    assert again.token_stream(case["text"]) == got


def check_random(seed, wc, wt, big=200_000, tiny=3000, names=("small", "tiny", "long", "mix")):
    raw, pred = predictor_for(seed, wc, wt)
    rng = random.Random(seed * 7 + 1)
    B = batches(seed, big, tiny)
    for name in names:
        texts = B[name]
        sample = ["O", rng.choice(WSCONSTS)] if name in ("long", "mix") else ["", "O"] + rng.sample(WSCONSTS, 2)
        for ws in dict.fromkeys(sample):
            check_csr(raw, pred, texts, ws)
    # the tokenizer class, with and without the grapheme filter
    texts = B["small"]
    for ws in ("", "OG", "GDR", "DRHTKOG"):
        tok = api.VaporettoTokenizer(api.Model.read_slice(raw)[0], ws, device=0)
        got = tok.token_stream_batch(texts)
        want = tokenref.ends_batch(raw, texts, ws)
        assert [[list(t._key()) for t in d] for d in got] == [tokenref.tokens_from_ends(t, e) for t, e in zip(texts, want)], ws


def check_caller_labels(seed, big=200_000, tiny=3000):
    raw, pred = predictor_for(seed, 3, 3)
    B = batches(seed, big, tiny)
    rng = np.random.default_rng(seed)
    for name in ("small", "tiny", "long", "mix"):
        texts = [t for t in B[name] if t]
        utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
        ooff = api.count_boundaries(utf8, boff)
        nb = int(ooff[-1])
        for labels in (np.zeros(nb, np.uint8), np.ones(nb, np.uint8), rng.integers(0, 2, nb).astype(np.uint8)):
            want_off, want_ends = tokenref.csr([tokenref.ends_from_labels(t, labels[int(ooff[i]):int(ooff[i + 1])]) for i, t in enumerate(texts)])
            toff, ends = pred.token_spans_packed(utf8, boff, ooff, labels)
            assert np.array_equal(toff, want_off) and np.array_equal(ends, want_ends), name


def _unescape_lengths(line: bytes):
    """Byte lengths of the surfaces of a tokenized line (tokens split at unescaped spaces, a '\\\\' escapes the next byte)."""
    out, n, i = [], 0, 0
    while i < len(line):
        if line[i] == 0x5C:
            n += 1
            i += 2
        elif line[i] == 0x20:
            out.append(n)
            n = 0
            i += 1
        else:
            n += 1
            i += 1
    out.append(n)
    return out


def check_consistency_with_tokenize(seed):
    """On texts without linebreaks the spans are what the existing vpt_tokenize_batch output implies for the same flags."""
    raw, pred = predictor_for(seed, 3, 2)
    rng = random.Random(seed)
    alpha = [a for a in ALPHABET if "\n" not in a and "\r" not in a] + ["/", "\\"]
    texts = ["".join(rng.choice(alpha) for _ in range(rng.randint(1, 80))) for _ in range(400)]
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    for ws in ("", "O", "DRK"):
        flags = _lib.VPT_FLAG_KYTEA_FULLWIDTH | api.wsconst_flags(ws)
        text, toff = pred.tokenize_packed(utf8, boff, flags=flags)
        line_bytes = bytes(text)
        want = [list(np.cumsum(_unescape_lengths(line_bytes[int(toff[i]):int(toff[i + 1])]))) for i in range(len(texts))]
        want_off, want_ends = tokenref.csr(want)
        got_off, got_ends = pred.token_stream_packed(utf8, boff, ws)
        assert np.array_equal(got_off, want_off) and np.array_equal(got_ends, want_ends), ws


def _expect(status, text):
    assert status == _lib.VPT_INVALID_ARGUMENT, status
    assert text in _lib.last_error(), _lib.last_error()


def check_errors(seed=5):
    L = _lib.load()
    raw, pred = predictor_for(seed, 3, 3)
    texts = ["あいa\nb", "漢字カ", "x\0y", "09"]
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in texts])
    with pytest.raises(api.VaporettoError, match="must not contain NULL"):
        pred.token_stream_packed(utf8, boff, "")
    with pytest.raises(api.VaporettoError, match="Could not parse a wsconst value"):
        pred.token_stream_packed(utf8, boff, "X")
    with pytest.raises(api.VaporettoError, match="Could not parse a wsconst value"):
        api.VaporettoTokenizer(api.Model.read_slice(raw)[0], "DZ")
    toff = np.zeros(len(texts) + 1, np.uint64)
    ends = np.zeros(64, np.uint32)
    _expect(L.vpt_token_stream_batch(pred.handle, utf8.ctypes.data, boff.ctypes.data, len(texts), 1 << 7, toff.ctypes.data, ends.ctypes.data, 64),
            "Could not parse a wsconst value")
    # capacity one short, host buffers: the status, and nothing behind the capacity is touched
    good = ["あいa\nb", "漢字カ", "xy", "09"]
    utf8, boff = api.pack_texts([t.encode("utf-8") for t in good])
    ooff = api.count_boundaries(utf8, boff)
    labels = np.ones(int(ooff[-1]), np.uint8)
    n_tok = int(ooff[-1]) + len(good)
    for call in ("spans", "stream"):
        ends = np.full(n_tok + 8, 0xDEADBEEF, np.uint32)
        if call == "spans":
            st = L.vpt_token_spans_batch(pred.handle, utf8.ctypes.data, boff.ctypes.data, len(good), ooff.ctypes.data, labels.ctypes.data,
                                         toff.ctypes.data, ends.ctypes.data, n_tok - 1)
        else:
            full_off, full_ends = pred.token_stream_packed(utf8, boff, "")
            st = L.vpt_token_stream_batch(pred.handle, utf8.ctypes.data, boff.ctypes.data, len(good), 0, toff.ctypes.data, ends.ctypes.data,
                                          len(full_ends) - 1)
            n_tok_stream = len(full_ends)
        _expect(st, "capacity: smaller than the number of tokens")
        assert np.all(ends[(n_tok if call == "spans" else n_tok_stream) - 1:] == 0xDEADBEEF)
    # ... and the device call: a guard region behind the buffer stays untouched, the verdict comes at the sync
    d_text, d_boff, d_ooff, d_lab = devmem.put(np.concatenate([utf8, np.zeros(32, np.uint8)])), devmem.put(boff), devmem.put(ooff), devmem.put(labels)
    guard = 64
    d_ends = devmem.put(np.full(n_tok + guard, 0xDEADBEEF, np.uint32))
    d_toff = devmem.zeros(len(good) + 1, np.uint64)
    batch = api.DeviceBatch(pred)
    batch.token_spans(d_text.ptr, d_boff.ptr, d_ooff.ptr, len(good), int(ooff[-1]), d_lab.ptr, d_toff.ptr, d_ends.ptr, n_tok - 1, devmem.stream())
    with pytest.raises(api.VaporettoError, match="text_capacity"):
        batch.sync()
    assert np.all(d_ends.get()[n_tok - 1:] == 0xDEADBEEF)
    batch.token_spans(d_text.ptr, d_boff.ptr, d_ooff.ptr, len(good), int(ooff[-1]), d_lab.ptr, d_toff.ptr, d_ends.ptr, n_tok, devmem.stream())
    batch.sync()
    want_off, want_ends = tokenref.csr([tokenref.ends_from_labels(t, labels[int(ooff[i]):int(ooff[i + 1])]) for i, t in enumerate(good)])
    assert np.array_equal(d_toff.get(), want_off) and np.array_equal(d_ends.get()[:n_tok], want_ends)
    assert np.all(d_ends.get()[n_tok:] == 0xDEADBEEF)
    # an Unknown label
    unknown = labels.copy()
    unknown[2] = 2
    with pytest.raises(api.VaporettoError, match="labels"):
        pred.token_spans_packed(utf8, boff, ooff, unknown)
    # out_offsets that do not match the text
    wrong = ooff.copy()
    wrong[1] += 1
    with pytest.raises(api.VaporettoError, match="out_offsets"):
        pred.token_spans_packed(utf8, boff, wrong, np.ones(int(wrong[-1]) + 4, np.uint8))
    wrong = ooff.copy()
    wrong[1:] -= 1
    with pytest.raises(api.VaporettoError, match="out_offsets"):
        pred.token_spans_packed(utf8, boff, wrong, labels)
