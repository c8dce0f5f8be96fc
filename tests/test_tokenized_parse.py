"""Sentence::from_tokenized (vaporetto/src/sentence.rs:285-514) without a GPU: the reference's own vectors through api.Sentence (the
library's host parser, vpt_parse_tokenized_batch) and through the test-only restatement (tests/evalref.py); then the device kernels
(kernels_parse.hip) on the CPU emulator (tests/emu.py) against the restatement on seeded random corpora."""
import random

import numpy as np
import pytest

from tests import devmem, emu, evalref, kat
from vaporetto_amd import _lib, api, build
from vaporetto_amd.modelfmt import encode_model

NWB, WB = 0, 1
D, R, H, T, K, O = 1, 2, 3, 4, 5, 6

# (tokenized text, raw text, boundaries, char types, {char: tags} (the other chars: None in every slot), n_tags) -- sentence.rs:1620-2626
VECTORS = [
    ("あ", "あ", [], [H], {}, 0),                                                                   # :1620-1630
    ("Rust で 良い プログラミング 体験 を ！", "Rustで良いプログラミング体験を！",                              # :1645-1707
     [NWB, NWB, NWB, WB, WB, NWB, WB, NWB, NWB, NWB, NWB, NWB, NWB, WB, NWB, WB, WB],
     [R, R, R, R, H, K, H, T, T, T, T, T, T, T, K, K, H, O], {}, 0),
    ("Rust/名詞 で 良い/形容詞 プログラミング 体験 を ！/補助記号", "Rustで良いプログラミング体験を！",          # :1775-1862
     [NWB, NWB, NWB, WB, WB, NWB, WB, NWB, NWB, NWB, NWB, NWB, NWB, WB, NWB, WB, WB],
     [R, R, R, R, H, K, H, T, T, T, T, T, T, T, K, K, H, O], {3: ["名詞"], 6: ["形容詞"], 17: ["補助記号"]}, 1),
    ("Rust/名詞 で 良い/形容詞/イイ プログラミング 体験 を ！/補助記号", "Rustで良いプログラミング体験を！",    # :1953-2059
     [NWB, NWB, NWB, WB, WB, NWB, WB, NWB, NWB, NWB, NWB, NWB, NWB, WB, NWB, WB, WB],
     [R, R, R, R, H, K, H, T, T, T, T, T, T, T, K, K, H, O], {3: ["名詞", None], 6: ["形容詞", "イイ"], 17: ["補助記号", None]}, 2),
    ("Rust//ラスト で 良い/形容詞/イイ プログラミング 体験 を ！//ビックリ", "Rustで良いプログラミング体験を！",  # :2168-2274
     [NWB, NWB, NWB, WB, WB, NWB, WB, NWB, NWB, NWB, NWB, NWB, NWB, WB, NWB, WB, WB],
     [R, R, R, R, H, K, H, T, T, T, T, T, T, T, K, K, H, O], {3: [None, "ラスト"], 6: ["形容詞", "イイ"], 17: [None, "ビックリ"]}, 2),
    ("火星 猫 の 生態 ( M \\  et\\ al. )", "火星猫の生態(M et al.)",                                     # :2383-2441
     [NWB, WB, WB, WB, NWB, WB, WB, WB, WB, NWB, NWB, NWB, NWB, NWB, WB],
     [K, K, K, H, K, K, O, R, O, R, R, O, R, R, O, O], {}, 0),
    ("改行 に \\\\n を 用い る", "改行に\\nを用いる",                                                      # :2505-2543
     [NWB, WB, WB, NWB, WB, WB, NWB, WB], [K, K, H, O, R, H, K, H, H], {}, 0),
    ("品詞 に \\/ を 用い る", "品詞に/を用いる",                                                          # :2586-2624
     [NWB, WB, WB, WB, WB, NWB, WB], [K, K, H, O, H, K, H, H], {}, 0),
]

# (tokenized text, message) -- sentence.rs:1480-1618
ERRORS = [
    ("", "must contain at least one character"),
    ("A1あ\0ア亜", "must not contain NULL"),
    (" Rust で 良い プログラミング 体験 を ！", "must not start with a whitespace"),
    ("Rust で 良い プログラミング 体験 を ！ ", "must not end with a whitespace"),
    ("Rust で 良い  プログラミング 体験 を ！", "must not contain consecutive whitespaces"),
    # sentence.rs:334-339 (no test there): a slash at the start or right after a space
    ("/名詞 で", "a slash must follow a character"),
    ("Rust /名詞", "a slash must follow a character"),
    ("a/x\0", "must not contain NULL"),
    # no char at all: the reference divides by zero (sentence.rs:450); here the empty-text error
    ("\\", "must contain at least one character"),
]


def _expected_tags(raw, tags, n_tags):
    out = []
    for c in range(len(raw)):
        out += list(tags.get(c, [None] * n_tags))
    return out


@pytest.fixture(scope="module")
def _built():
    build.build_hip()


@pytest.mark.parametrize("vec", VECTORS, ids=lambda v: v[0][:12])
def test_from_tokenized_reference_vectors(_built, vec):
    text, raw, bounds, types, tags, n_tags = vec
    for s in (api.Sentence.from_tokenized(text), _updated(text)):
        assert s.as_raw_text() == raw
        assert list(s.boundaries()) == bounds
        assert list(s.char_types()) == types
        assert s.n_tags() == n_tags
        assert s.tags() == _expected_tags(raw, tags, n_tags)
        assert len(s.boundary_scores()) == 0


def _updated(text):
    s = api.Sentence.from_raw("12345")
    s.update_tokenized(text)
    return s


@pytest.mark.parametrize("vec", VECTORS, ids=lambda v: v[0][:12])
def test_restatement_reference_vectors(vec):
    text, raw, bounds, types, tags, n_tags = vec
    r, b, t, nt = evalref.parse_tokenized(text)
    assert (r, b, nt) == (raw, bounds, n_tags)
    assert t == _expected_tags(raw, tags, n_tags)


@pytest.mark.parametrize("text,msg", ERRORS)
def test_from_tokenized_errors(_built, text, msg):
    with pytest.raises(api.VaporettoError) as e:
        api.Sentence.from_tokenized(text)
    assert e.value.kind == "InvalidArgument" and str(e.value) == "InvalidArgumentError: tokenized_text: " + msg
    s = api.Sentence.from_tokenized("a b")
    with pytest.raises(api.VaporettoError):
        s.update_tokenized(text)
    assert s.as_raw_text() == " " and s.n_tags() == 0 and s.tags() == []        # set_default (sentence.rs:140-158)
    with pytest.raises(evalref.ParseError) as e2:
        evalref.parse_tokenized(text)
    assert str(e2.value) == "InvalidArgumentError: tokenized_text: " + msg


def test_host_batch_names_the_first_failing_line(_built):
    with pytest.raises(api.VaporettoError) as e:
        api.parse_tokenized_host([b"a b", b"c  d", b" x"])
    assert str(e.value) == "InvalidArgumentError: tokenized_text: must not contain consecutive whitespaces (line 1)"


# ---- random corpora

_ALPHA = ["a", "b", "Z", "0", "あ", "漢", "ア", "\U0001F600", "\U00020000", "é", "・"]


def _token(rng):
    out = []
    for _ in range(rng.randint(1, 4)):
        r = rng.random()
        if r < 0.2:
            out.append("\\" + rng.choice([" ", "/", "\\", "x", "あ"]))
        else:
            out.append(rng.choice(_ALPHA))
    return "".join(out)


def _tag(rng):
    r = rng.random()
    if r < 0.15:
        return ""
    return "".join(rng.choice(["名詞", "x", "\\/", "\\ ", "\\\\", "ヒト", "\U0001F600"]) for _ in range(rng.randint(1, 3)))


def random_line(rng, n_tokens):
    toks = []
    for _ in range(n_tokens):
        t = _token(rng)
        for _ in range(rng.choice([0, 0, 0, 1, 2, 3])):
            t += "/" + _tag(rng)
        toks.append(t)
    return " ".join(toks)


def random_bad_line(rng, reason):
    good = random_line(rng, rng.randint(1, 6))
    if reason == 1:
        return rng.choice(["", "\\"])
    if reason == 2:
        return " " + good
    if reason == 3:
        return good + "  x"
    if reason == 4:
        return good + " "
    if reason == 5:
        return rng.choice(["/" + good, good + " /x"])
    return good[:len(good) // 2] + "\0" + good[len(good) // 2:]


def backslash_runs(rng):
    """runs of 1-5 '\\' before ' ' / '/' / '\\' at every offset mod 16 (and so across the 64-byte windows)"""
    lines = []
    for off in range(80):
        for run in range(1, 6):
            for nxt in (" ", "/", "\\"):
                prefix = "a" * (off + 1)
                s = prefix + "\\" * run + nxt + "b"
                if s.endswith("\\"):
                    s += "c"
                lines.append(s)
    return lines


def _expect(lines):
    """what vpt_parse_tokenized_batch must write, from the restatement (None: the line is rejected)"""
    out = []
    for ln in lines:
        try:
            out.append(evalref.parse_tokenized(ln))
        except evalref.ParseError as e:
            out.append(e)
    return out


def check_parsed(p, lines, expect):
    raw = bytes(p["raw"])
    ro, oo, ti, so, tb = p["raw_offsets"], p["out_offsets"], p["tag_index"], p["span_offsets"], bytes(p["tag_bytes"])
    for i, (ln, ex) in enumerate(zip(lines, expect)):
        r, b, t, nt = ex
        assert raw[int(ro[i]):int(ro[i + 1])].decode("utf-8") == r, (i, ln)
        assert list(p["labels"][int(oo[i]):int(oo[i + 1])]) == b, (i, ln)
        assert int(p["n_tags"][i]) == nt, (i, ln)
        g0 = int(oo[i]) + i
        got = []
        for c in range(len(r)):
            own = [tb[int(so[k]):int(so[k + 1])].decode("utf-8") for k in range(int(ti[g0 + c]), int(ti[g0 + c + 1]))]
            own += [""] * (nt - len(own))
            got += [x if x else None for x in own]
        assert got == t, (i, ln)


def test_host_parser_random_corpus(_built):
    rng = random.Random(7)
    lines = [random_line(rng, rng.randint(1, 40)) for _ in range(400)] + backslash_runs(rng)
    lines = [ln for ln, ex in zip(lines, _expect(lines)) if not isinstance(ex, Exception)]
    p = api.parse_tokenized_host([ln.encode("utf-8") for ln in lines])
    check_parsed(p, lines, _expect(lines))


# ---- the kernels on the CPU emulator

@pytest.fixture(scope="module")
def emulated():
    lib = emu.load()
    saved = _lib._lib
    _lib._lib = lib
    devmem.EMULATED = True
    yield lib
    import gc
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


def device_parse(lib, pred, batch, lines, expect_error=None):
    import ctypes as C
    utf8, boff = api.pack_texts([ln.encode("utf-8") for ln in lines])
    S, B = len(lines), len(utf8)
    bufs = {"raw": devmem.zeros(B + 1, np.uint8), "raw_offsets": devmem.zeros(S + 1, np.uint64), "out_offsets": devmem.zeros(S + 1, np.uint64),
            "labels": devmem.zeros(B + 1, np.uint8), "n_tags": devmem.zeros(S + 1, np.uint32), "tag_index": devmem.zeros(B + 1, np.uint64),
            "span_offsets": devmem.zeros(B + 1, np.uint64), "tag_bytes": devmem.zeros(B + 1, np.uint8)}
    d_text, d_boff = devmem.put(np.concatenate([utf8, np.zeros(16, np.uint8)])), devmem.put(boff)
    st = lib.vpt_parse_tokenized_batch_device(pred, batch, d_text.ptr, d_boff.ptr, S, B, *[bufs[k].ptr for k in
                                              ("raw", "raw_offsets", "out_offsets", "labels", "n_tags", "tag_index", "span_offsets", "tag_bytes")],
                                              devmem.stream())
    assert st == 0
    st = lib.vpt_batch_sync(batch)
    if expect_error is not None:
        assert st == _lib.VPT_INVALID_ARGUMENT
        assert lib.vpt_last_error().decode() == expect_error
        return None
    assert st == 0, lib.vpt_last_error()
    h = {k: v.get() for k, v in bufs.items()}
    return api._trim_parsed(h, S)


@pytest.fixture(scope="module")
def emu_handles(emulated):
    import ctypes as C
    raw = encode_model(kat.predictor_test_model())
    pred, batch = C.c_void_p(), C.c_void_p()
    assert emulated.vpt_predictor_create(raw, len(raw), 1, 0, C.byref(pred)) == 0
    assert emulated.vpt_batch_create(pred, C.byref(batch)) == 0
    yield emulated, pred, batch
    emulated.vpt_batch_destroy(batch)
    emulated.vpt_predictor_destroy(pred)


def test_parse_kernel_random_corpus_on_emulator(emu_handles):
    lib, pred, batch = emu_handles
    rng = random.Random(11)
    lines = [random_line(rng, rng.randint(1, 30)) for _ in range(150)] + backslash_runs(rng)
    lines += [random_line(rng, 120)]                                       # a line of several 64-byte windows
    lines += ["\U0001F600" * 40 + " " + "\\ " * 50 + "/" + "x\\/" * 30]    # 4-byte chars, escapes across windows, a long tag
    lines = [ln for ln, ex in zip(lines, _expect(lines)) if not isinstance(ex, Exception)]
    p = device_parse(lib, pred, batch, lines)
    check_parsed(p, lines, _expect(lines))
    h = api.parse_tokenized_host([ln.encode("utf-8") for ln in lines])   # bit for bit what the host parser writes
    for k in h:
        assert np.array_equal(np.asarray(p[k]), np.asarray(h[k])), k


@pytest.mark.parametrize("reason", [1, 2, 3, 4, 5, 6])
def test_parse_kernel_errors_name_the_first_line_on_emulator(emu_handles, reason):
    lib, pred, batch = emu_handles
    rng = random.Random(100 + reason)
    lines = [random_line(rng, rng.randint(1, 8)) for _ in range(40)]
    bad_at = 17
    bad = random_bad_line(rng, reason)
    lines[bad_at] = bad
    lines[33] = random_bad_line(rng, 1 + reason % 6)                      # a later failing line does not win
    msg = "InvalidArgumentError: tokenized_text: %s (line %d)" % (evalref.MSG[reason], bad_at)
    device_parse(lib, pred, batch, lines, expect_error=msg)
    # the workspace is clean afterwards
    p = device_parse(lib, pred, batch, ["a b"])
    assert bytes(p["raw"]) == b"ab"


def test_parse_kernel_reports_a_capacity_too_small_on_emulator(emu_handles):
    import ctypes as C
    lib, pred, batch = emu_handles
    lines = [b"a/xyz b/uvw", b"c d"]
    utf8, boff = api.pack_texts(lines)
    S, cap = len(lines), 4                                   # the raw text alone takes 4 bytes + 2: too small
    bufs = [devmem.zeros(n, dt) for n, dt in ((cap, np.uint8), (S + 1, np.uint64), (S + 1, np.uint64), (cap, np.uint8), (S, np.uint32),
                                                (cap + 1, np.uint64), (cap + 1, np.uint64), (cap, np.uint8))]
    d_text, d_boff = devmem.put(np.concatenate([utf8, np.zeros(16, np.uint8)])), devmem.put(boff)
    assert lib.vpt_parse_tokenized_batch_device(pred, batch, d_text.ptr, d_boff.ptr, S, cap, *[b.ptr for b in bufs], devmem.stream()) == 0
    assert lib.vpt_batch_sync(batch) == _lib.VPT_INVALID_ARGUMENT
    assert "smaller than" in lib.vpt_last_error().decode()
    assert bytes(bufs[0].get()) == b"abcd"                   # nothing past the buffer
    p = device_parse(lib, pred, batch, ["a b"])              # the workspace is clean afterwards
    assert bytes(p["raw"]) == b"ab"
