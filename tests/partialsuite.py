"""Partial annotation on the device, both ways: the checks tests/test_partial_emu.py runs on the CPU emulator and tests/test_partial_gpu.py on the
MI355X.  The oracle is the host restatement (api.Sentence.from_partial_annotation / write_partial_annotation_text, pinned to the reference's own
vectors by tests/test_partial_ref.py); lines are built from structure, so what the parsers must write is known element for element.

`ctx` is (lib, predictor handle, workspace handle): the C ABI called directly, device buffers through tests/devmem.py."""
import random

import numpy as np

from tests import devmem
from vaporetto_amd import _lib, api

KEYS = ("raw", "raw_offsets", "out_offsets", "labels", "n_tags", "tag_index", "span_offsets", "tag_bytes")
DTYPES = dict(zip(KEYS, (np.uint8, np.uint64, np.uint64, np.uint8, np.uint32, np.uint64, np.uint64, np.uint8)))
MARKS = "-| "          # label 0, 1, 2
SPECIALS = " -|/\\"
ALPHA = ["a", "b", "Z", "0", " ", "-", "|", "/", "\\", "é", "あ", "漢", "\U0001F600", "\U00020000"]
TAG_ALPHA = ["x", "名", "詞", "é", "\U0001F600", "\0", " ", "-", "|", "/", "\\"]
PREFIX = "InvalidArgumentError: partial_annotation_text: "
GUARD = 64


# ---- lines from structure: [(char, [tag, ...]), ...] + labels; a tag is a list of items, an item a code point or ("esc", code point)

def render(chars, labels):
    out = []
    for k, (ch, tags) in enumerate(chars):
        if k:
            out.append(MARKS[labels[k - 1]])
        out.append(ch)
        for tag in tags:
            out.append("/")
            for it in tag:
                cp = it[1] if isinstance(it, tuple) else it
                out.append("\\" + cp if isinstance(it, tuple) or cp in SPECIALS else cp)
    return "".join(out)


def tag_text(tag):
    return "".join(it[1] if isinstance(it, tuple) else it for it in tag)


def plain(s):
    return list(s)


def random_tag(rng, clean):
    if rng.random() < 0.2:
        return []
    alpha = [c for c in TAG_ALPHA if c not in SPECIALS] if clean else TAG_ALPHA
    return [("esc", c) if (not clean and rng.random() < 0.1) else c for c in (rng.choice(alpha) for _ in range(rng.randint(1, 4)))]


def random_struct(rng, n_chars, clean=False, p_tags=0.4):
    chars = []
    for _ in range(n_chars):
        tags = [random_tag(rng, clean) for _ in range(rng.randint(0, 3))] if rng.random() < p_tags else []
        if clean and tags and not tags[-1]:
            tags[-1] = ["x"]
        chars.append((rng.choice(ALPHA), tags))
    return chars, [rng.randrange(3) for _ in range(n_chars - 1)]


def roundtrips(struct):
    """write_partial_annotation_text does not escape tags and drops a char's trailing empty tags: parse(write(x)) is x where no tag holds a
    special and no char's last tag is empty."""
    return all(not any(c in SPECIALS for c in tag_text(t)) for _, tags in struct[0] for t in tags) and \
        all(not tags or tags[-1] for _, tags in struct[0])


def chain(n, first="a"):
    """first + n - 1 times a, labels alternating: marks at every other byte"""
    return [(first, [])] + [("a", [])] * (n - 1), [k % 3 for k in range(n - 1)]


def fixed_structs():
    out = []
    for nbytes in (1, 63, 64, 65, 127, 128, 129):                      # lines of exactly these sizes
        out.append(chain((nbytes + 1) // 2) if nbytes % 2 else chain(nbytes // 2, "é"))
    emoji = "\U0001F600"
    for p in (61, 62, 63, 64):                                         # a 4-byte char that starts at byte p, as a char and inside a tag
        ch, lab = chain(p // 2, "a") if p % 2 == 0 else chain((p - 1) // 2, "é")
        out.append((ch + [(emoji, [])], lab + [1]))
        out.append(([("a", [plain("x" * (p - 2) + emoji + "y")])], []))
    for run in (4, 5):                                                 # 8 and 9 backslashes from byte 60: across the window's edge, even and odd
        tag = plain("x" * 58) + ["\\"] * 4 + ([("esc", "y")] if run == 5 else ["y"])
        out.append(([("a", [tag]), ("b", [])], [2]))
    out.append(chain(40, "a"))                                         # "a-a-..": a mark as byte 63, the last of a window
    out.append(chain(40, "é"))                                         # "é-a-..": a mark as byte 64, the first of a window
    out.append(([("a", [plain("x" * 150)]), ("b", [plain("y")])], [0]))   # a tag over three windows
    out.append(([(c, [plain("t%d" % k)]) for k, c in enumerate("あいうえおabc|/")], [k % 3 for k in range(9)]))   # a tag on every char
    out.append(([("漢", [])], []))                                      # one char
    return out


QUIRKS = ["a||-b", "a\\", "a/x\\", "a/\0|b", "/|/", "\\-\\", "a/|b", "a//x b"]

_cache = {}


def parity_batch(n_lines):
    """(structs, lines): the fixed lines, one of about 70 000 bytes, random ones up to n_lines; at least a quarter round-trip"""
    if n_lines not in _cache:
        rng = random.Random(1000 + n_lines)
        structs = fixed_structs()
        structs.append(random_struct(rng, 13700, p_tags=0.3))
        while len(structs) < n_lines:
            structs.append(random_struct(rng, rng.randint(1, 60), clean=len(structs) % 3 == 0))
        lines = [render(*s) for s in structs]
        assert 65000 < max(len(ln.encode("utf-8")) for ln in lines) < 75000
        assert sum(roundtrips(s) for s in structs) * 4 >= len(structs)
        _cache[n_lines] = (structs, lines)
    return _cache[n_lines]


def expected_arrays(structs):
    """what the parsers must write for lines rendered from these structures"""
    raw, ro, oo, labels, n_tags, ti, so, tb = bytearray(), [0], [0], [], [], [0], [0], bytearray()
    for chars, labs in structs:
        for ch, tags in chars:
            raw += ch.encode("utf-8")
            for t in tags:
                tb += tag_text(t).encode("utf-8")
                so.append(len(tb))
            ti.append(len(so) - 1)
        labels += labs
        ro.append(len(raw))
        oo.append(len(labels))
        n_tags.append(max(len(tags) for _, tags in chars))
    vals = (np.frombuffer(bytes(raw), np.uint8), ro, oo, labels, n_tags, ti, so, np.frombuffer(bytes(tb), np.uint8))
    return {k: np.asarray(v, DTYPES[k]) for k, v in zip(KEYS, vals)}


def restated(line):
    """(raw, labels, tags, n_tags) of the restatement, or its message"""
    try:
        s = api.Sentence.from_partial_annotation(line)
    except api.VaporettoError as e:
        return str(e)
    return s.as_raw_text(), [int(b) for b in s.boundaries()], list(s.tags()), s.n_tags()


def c_message(msg, line):
    """the library's message for the restatement's: the batch's line behind it; a C string ends at a NUL"""
    return (msg + " (line %d)" % line).split("\0")[0]


def check_against_restatement(p, lines):
    raw, tb = bytes(p["raw"]), bytes(p["tag_bytes"])
    ro, oo, ti, so = p["raw_offsets"], p["out_offsets"], p["tag_index"], p["span_offsets"]
    for i, ln in enumerate(lines):
        r, b, t, nt = restated(ln)
        assert raw[int(ro[i]):int(ro[i + 1])].decode("utf-8") == r, (i, ln)
        assert list(p["labels"][int(oo[i]):int(oo[i + 1])]) == b, (i, ln)
        assert int(p["n_tags"][i]) == nt, (i, ln)
        g0, got = int(oo[i]) + i, []
        for c in range(len(r)):
            own = [tb[int(so[k]):int(so[k + 1])].decode("utf-8") for k in range(int(ti[g0 + c]), int(ti[g0 + c + 1]))]
            got += [x if x else None for x in own + [""] * (nt - len(own))]
        assert got == t, (i, ln)


def assert_same(got, want, what=""):
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


# ---- the library

def pack(lines):
    return api.pack_texts([ln.encode("utf-8") if isinstance(ln, str) else ln for ln in lines])


def parse_buffers(S, cap, fill=0):
    sizes = dict(zip(KEYS, (cap, S + 1, S + 1, cap, max(S, 1), cap + 1, cap + 1, cap)))
    return sizes, {k: devmem.put(np.full(sizes[k] + GUARD, fill, DTYPES[k])) for k in KEYS}


def device_parse(ctx, lines, capacity=None, bufs=None, expect_error=None, kind="partial"):
    """-> the trimmed arrays, or None when the expected error came; the guard elements behind every buffer must be untouched.  kind: "partial" or
    "tokenized", the device parser that reads the lines"""
    lib, pred, batch = ctx
    utf8, boff = pack(lines)
    S, cap = len(lines), len(utf8) if capacity is None else capacity
    fill = 0xAB
    sizes, own = parse_buffers(S, cap, fill)
    bufs = bufs or own
    d_text, d_boff = devmem.put(np.concatenate([utf8, np.zeros(16, np.uint8)])), devmem.put(boff)
    st = getattr(lib, "vpt_parse_%s_batch_device" % kind)(pred, batch, d_text.ptr, d_boff.ptr, S, cap, *[bufs[k].ptr for k in KEYS], devmem.stream())
    assert st == 0, lib.vpt_last_error()
    st = lib.vpt_batch_sync(batch)
    h = {k: bufs[k].get() for k in KEYS}
    for k in KEYS:
        assert (h[k][sizes[k]:] == np.full(1, fill, DTYPES[k])[0]).all(), k
    if expect_error is not None:
        assert st == _lib.VPT_INVALID_ARGUMENT
        assert lib.vpt_last_error().decode("utf-8") == expect_error
        return None
    assert st == 0, lib.vpt_last_error()
    return api._trim_parsed(h, S)


def host_parse_error(lines):
    try:
        api.parse_partial_host([ln.encode("utf-8") for ln in lines])
    except api.VaporettoError as e:
        return str(e)
    return None


def device_write(ctx, p, utf8=None, tags=True, capacity=None, expect_error=None):
    lib, pred, batch = ctx
    S = len(p["raw_offsets"]) - 1
    n_t = len(p["span_offsets"]) + len(p["tag_bytes"]) if tags else 0
    cap = len(p["raw"]) + len(p["labels"]) + n_t if capacity is None else capacity

    def put(k):
        a = np.asarray(p[k], DTYPES[k])
        return devmem.put(a if len(a) else np.zeros(1, DTYPES[k]))
    d = {k: put(k) for k in KEYS}
    out, toff = devmem.put(np.full(cap + GUARD, 0xAB, np.uint8)), devmem.zeros(S + 1, np.uint64)
    tp = [d[k].ptr if tags else None for k in ("n_tags", "tag_index", "span_offsets", "tag_bytes")]
    st = lib.vpt_write_partial_batch_device(pred, batch, d["raw"].ptr, d["raw_offsets"].ptr, S, d["out_offsets"].ptr, d["labels"].ptr, *tp,
                                            out.ptr, cap, toff.ptr, devmem.stream())
    assert st == 0, lib.vpt_last_error()
    st = lib.vpt_batch_sync(batch)
    o = out.get()
    assert (o[cap:] == 0xAB).all()
    if expect_error is not None:
        assert st == _lib.VPT_INVALID_ARGUMENT and expect_error in lib.vpt_last_error().decode("utf-8")
        return None
    assert st == 0, lib.vpt_last_error()
    t = toff.get()
    return bytes(o[:int(t[S])]), t


def split(text, toff):
    return [text[int(toff[i]):int(toff[i + 1])].decode("utf-8") for i in range(len(toff) - 1)]


def host_write(p, tags=True, capacity=None):
    a = [p["raw"], p["raw_offsets"], p["out_offsets"], p["labels"]] + ([p[k] for k in ("n_tags", "tag_index", "span_offsets", "tag_bytes")] if tags else [])
    text, toff = api.write_partial_host(*a, capacity=capacity)
    return bytes(text), toff


# ---- the checks

def check_parity(ctx, n_lines):
    """host C ABI and device against the structure (every array, element for element) and against the restatement; the writer on the same batch;
    parse(write(x)) == x on the lines that can round-trip"""
    structs, lines = parity_batch(n_lines)
    want = expected_arrays(structs)
    host = api.parse_partial_host([ln.encode("utf-8") for ln in lines])
    assert_same(host, want, "host")
    check_against_restatement(host, lines)
    dev = device_parse(ctx, lines)
    assert_same(dev, want, "device")
    # the writer: every line what the restatement's Sentence writes
    texts = [api.Sentence.from_partial_annotation(ln).write_partial_annotation_text() for ln in lines]
    ht, hoff = host_write(host)
    assert split(ht, hoff) == texts
    dt, doff = device_write(ctx, dev)
    assert dt == ht and np.array_equal(doff, hoff)
    # round trip on the lines that can
    sub = [s for s in structs if roundtrips(s)]
    x = expected_arrays(sub)
    wt, woff = device_write(ctx, x)
    back = device_parse(ctx, split(wt, woff))
    assert_same(back, x, "round trip")
    assert_same(api.parse_partial_host([t.encode("utf-8") for t in split(*host_write(x))]), x, "host round trip")


def check_quirks(ctx):
    for q in QUIRKS:
        r = restated(q)
        assert not isinstance(r, str), q
        for p in (api.parse_partial_host([q.encode("utf-8")]), device_parse(ctx, [q])):
            check_against_restatement(p, [q])
    host, dev = api.parse_partial_host([q.encode("utf-8") for q in QUIRKS]), device_parse(ctx, QUIRKS)
    assert_same(dev, host, "quirks")
    assert bytes(host["raw"][:3]) == b"a|b" and list(host["labels"][:2]) == [1, 0]
    texts = [api.Sentence.from_partial_annotation(q).write_partial_annotation_text() for q in QUIRKS]
    assert split(*device_write(ctx, dev)) == texts == split(*host_write(host))


def check_small_batches(ctx):
    lib, pred, batch = ctx
    p = device_parse(ctx, [])
    assert len(p["raw"]) == 0 and list(p["raw_offsets"]) == [0] and list(p["tag_index"]) == [0] and list(p["span_offsets"]) == [0]
    h = api.parse_partial_host([])
    assert_same(p, h, "S = 0")
    assert device_write(ctx, p)[0] == b"" and host_write(h)[0] == b""
    for line in ("a", "あ/名/詞|b"):
        one = device_parse(ctx, [line])
        assert_same(one, api.parse_partial_host([line.encode("utf-8")]), "S = 1")
        check_against_restatement(one, [line])
        assert split(*device_write(ctx, one)) == [line]


def check_capacity(ctx):
    """capacity == B passes; B - 1 is the text_capacity error with nothing written behind the buffers (device_parse checks the guards)"""
    lines = ["a", "あ", "b", "\U0001F600"]           # one char a line: the raw text is the input, B bytes
    B = len(pack(lines)[0])
    p = device_parse(ctx, lines, capacity=B)
    assert bytes(p["raw"]).decode("utf-8") == "".join(lines)
    device_parse(ctx, lines, capacity=B - 1, expect_error="InvalidArgumentError: text_capacity: smaller than the tokenized text")
    assert_same(device_parse(ctx, lines), p, "after the error")
    # the writer: exactly what it takes, and one byte less
    x = device_parse(ctx, ["a/x|b", "c d/yy"])
    text, toff = device_write(ctx, x, capacity=11)
    assert text == b"a/x|bc d/yy"
    device_write(ctx, x, capacity=10, expect_error="text_capacity")
    try:
        host_write(x, capacity=10)
        assert False
    except api.VaporettoError as e:
        assert "text_capacity" in str(e)


def _bad(reason, k=0):
    """a failing tail for state `annotation` (behind a char): 2 NUL where a char stands, 3 an ordinary code point, 5 an escaped one, 4 a mark at the end"""
    off = ["?", "é", "漢", "\U0001F600"][k % 4]
    return {2: "-\0", 3: off, 5: "\\" + off, 4: "|"}[reason]


REASONS = (1, 2, 3, 5, 4)   # empty line, NUL, invalid boundary character (ordinary / escaped), invalid annotation


def bad_line(rng, reason, k=0, second=None):
    if reason == 1:
        return ""
    good = render(*random_struct(rng, rng.randint(1, 12)))
    line = good + "-a" + _bad(reason, k)   # (behind a char without tags: the tail means what _bad says)
    if second is not None and reason != 4:
        line += "a" + _bad(second, k + 1)
    return line


def check_errors(ctx, n_lines):
    lib, pred, batch = ctx
    rng = random.Random(77)
    valid = [render(*random_struct(rng, rng.randint(1, 20))) for _ in range(n_lines)]

    def expect(lines):
        for i, ln in enumerate(lines):
            r = restated(ln)
            if isinstance(r, str):
                return c_message(r, i)
        return None

    def both(lines):
        msg = expect(lines)
        assert msg is not None
        assert host_parse_error(lines) == msg
        device_parse(ctx, lines, expect_error=msg)
    # each reason alone; in line 0, the last line, and two lines at once
    for reason in REASONS:
        for at in ([17], [0], [len(valid) - 1], [9, 30]):
            lines = list(valid)
            for a in at:
                lines[a] = bad_line(rng, reason, k=a)
            both(lines)
        # ... and in front of a smaller line's other reason
        for other in REASONS:
            lines = list(valid)
            lines[5], lines[25] = bad_line(rng, reason), bad_line(rng, other, k=1)
            both(lines)
    # a second error behind the first in one line: the first wins
    for first in (2, 3, 5):
        for second in (2, 3, 5, 4):
            lines = list(valid)
            lines[11] = bad_line(rng, first, k=2, second=second)
            r = restated(lines[11])
            assert r.startswith(PREFIX + {2: "must not contain NULL", 3: "contains an invalid", 5: "contains an invalid"}[first])
            both(lines)
    # the offender: 1 to 4 bytes, anywhere and as the last lane of a window (byte 63), ordinary and escaped; NUL as an offender
    head = render(*chain(32))   # 63 bytes, a char last
    for k in range(4):
        off = ["?", "é", "漢", "\U0001F600"][k]
        for line in ("a-b" + off + "-z", head + off + "|b", render(*chain(31, "é")) + "\\" + off, "a\\\0b", "a\0"):
            lines = list(valid[:20])
            lines[7] = line
            assert ("'%s'" % off) in restated(line) or "\0" in line
            both(lines)
    both([""])
    both(["a-"])
    # the workspace is clean afterwards
    check_against_restatement(device_parse(ctx, ["a|b"]), ["a|b"])


def check_mutated(ctx, n_lines):
    """a batch in which every reason occurs at least 10 times and at most half the lines are invalid (checked on the restatement first): the library
    names the smallest failing line; with that line mended, the next one; and so on for a few"""
    rng = random.Random(5)
    lines = [render(*random_struct(rng, rng.randint(1, 20))) for _ in range(n_lines)]
    slots = rng.sample(range(n_lines), 50)
    for j, at in enumerate(slots):
        lines[at] = bad_line(rng, REASONS[j % 5], k=j)
    verdict = [restated(ln) for ln in lines]
    msgs = [v for v in verdict if isinstance(v, str)]
    for needle in ("at least one character", "must not contain NULL", "invalid boundary character", "invalid annotation"):
        assert sum(needle in m for m in msgs) >= 10, needle
    assert sum("\\" + m[-2] in ln for m, ln in zip(verdict, lines) if isinstance(m, str) and "invalid boundary" in m) >= 10   # the escaped flavour
    assert len(msgs) * 2 <= n_lines
    for _ in range(6):
        i = next(k for k, v in enumerate(verdict) if isinstance(v, str))
        assert host_parse_error(lines) == c_message(verdict[i], i)
        device_parse(ctx, lines, expect_error=c_message(verdict[i], i))
        lines[i], verdict[i] = "a", None


def check_writer(ctx):
    """hand-built CSRs against Sentence.write_partial_annotation_text"""
    def sent(raw, labels, tags, n_tags):
        s = api.Sentence.from_raw(raw)
        s._boundaries = np.array(labels, np.uint8)
        s._tags, s._n_tags = tags, n_tags
        return s
    # trailing Nones are trimmed, an inner None is an empty field, a char whose tags are all None prints no '/'
    s1 = sent("abc", [1, 2], ["x", None, "y", None, None, None, None, "z", None], 3)
    s2 = sent("漢d", [0], [None, None, "t", "u"], 2)
    assert s1.write_partial_annotation_text() == "a/x//y|b c//z" and s2.write_partial_annotation_text() == "漢-d/t/u"
    p = {"raw": np.frombuffer("abc漢d".encode("utf-8"), np.uint8), "raw_offsets": [0, 3, 7], "out_offsets": [0, 2, 3], "labels": [1, 2, 0],
         "n_tags": [3, 2], "tag_index": [0, 3, 6, 9, 11, 13], "span_offsets": [0, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 4, 5],
         "tag_bytes": np.frombuffer(b"xyztu", np.uint8)}
    p = {k: np.asarray(v, DTYPES[k]) for k, v in p.items()}
    want = [s1.write_partial_annotation_text(), s2.write_partial_annotation_text()]
    assert split(*device_write(ctx, p)) == want == split(*host_write(p))
    # n_tags NULL: no tags
    bare = ["a|b c", "漢-d"]
    assert split(*device_write(ctx, p, tags=False)) == bare == split(*host_write(p, tags=False))
    assert [sent("abc", [1, 2], [], 0).write_partial_annotation_text(), sent("漢d", [0], [], 0).write_partial_annotation_text()] == bare
    # a label of 3
    q = dict(p)
    q["labels"] = np.array([1, 3, 0], np.uint8)
    device_write(ctx, q, expect_error="InvalidArgumentError: labels: not a CharacterBoundary")
    try:
        host_write(q)
        assert False
    except api.VaporettoError as e:
        assert e.kind == "InvalidArgument" and "labels" in str(e)
    assert split(*device_write(ctx, p)) == want   # the workspace is clean afterwards


def check_determinism_and_reuse(ctx):
    structs, lines = parity_batch(120)
    long_lines, short_lines = lines[:60], ["a|b/t", "漢"]
    a, b = device_parse(ctx, long_lines), device_parse(ctx, long_lines)
    assert_same(a, b, "twice")
    assert device_write(ctx, a)[0] == device_write(ctx, b)[0]
    # a long batch, then a short one into the same buffers (refilled with the guard pattern): nothing behind the short one's ends
    S, cap = len(long_lines), len(pack(long_lines)[0])
    sizes, bufs = parse_buffers(S, cap, 0xAB)
    device_parse(ctx, long_lines, bufs=bufs)
    for k in KEYS:
        bufs[k].set(np.full(sizes[k] + GUARD, 0xAB, DTYPES[k]))
    lib, pred, batch = ctx
    utf8, boff = pack(short_lines)
    d_text, d_boff = devmem.put(np.concatenate([utf8, np.zeros(16, np.uint8)])), devmem.put(boff)
    assert lib.vpt_parse_partial_batch_device(pred, batch, d_text.ptr, d_boff.ptr, 2, cap, *[bufs[k].ptr for k in KEYS], devmem.stream()) == 0
    assert lib.vpt_batch_sync(batch) == 0
    want = api.parse_partial_host([ln.encode("utf-8") for ln in short_lines])
    fill = {k: np.full(1, 0xAB, DTYPES[k])[0] for k in KEYS}
    for k in KEYS:
        got = bufs[k].get()
        n = len(want[k])
        assert np.array_equal(got[:n], want[k]), k
        assert (got[n:] == fill[k]).all(), k
