"""The frame the two device parsers share (parse_lines_kernel, kernels_parse.hip), checked through both syntaxes: the checks tests/test_parse_frame_emu.py
runs on the CPU emulator and tests/test_parse_frame_gpu.py on the MI355X.  The oracle is the host parser of the same syntax (pinned to the
restatements by tests/test_tokenized_parse.py and tests/test_partial_ref.py), compared array by array.

`ctx` is (lib, predictor handle, workspace handle), as in tests/partialsuite.py.  Byte positions count from 0: byte 63 is a window's last lane, byte 64
the first lane of the next window."""
import random

from tests import evalref, partialsuite
from tests.test_tokenized_parse import _expect, check_parsed, random_line
from vaporetto_amd import api

KINDS = ("tokenized", "partial")
EMOJI = "\U0001F600"
GRID_LINES = 4 * 8192   # what the capped grid takes in one stride: 8192 workgroups of four waves, a line a wave


def host_parse(kind, lines):
    return (api.parse_tokenized_host if kind == "tokenized" else api.parse_partial_host)([ln.encode("utf-8") for ln in lines])


def _byte(line, at):
    return line.encode("utf-8")[at:at + 1]


def tokenized_edge_lines():
    out = []
    for n in (1, 63, 64, 65, 127, 128, 129):                               # lines of exactly these sizes
        out.append("a" + " a" * ((n - 1) // 2) if n % 2 else "é" + " a" * ((n - 2) // 2))
        assert len(out[-1].encode("utf-8")) == n
    for p in (61, 62, 63, 64):                                             # a 4-byte char whose lead is byte p, as a surface char and inside a tag
        out.append(("a " * 40)[:p] + EMOJI + " b")
        out.append("a/" + "x" * (p - 2) + EMOJI + "y b")
        assert all(_byte(ln, p) == b"\xf0" for ln in out[-2:])
    for run in (8, 9):                                                     # runs of '\\' from byte 60 across the window's edge, even and odd
        for nxt in (" ", "/"):
            out.append("a " * 30 + "\\" * run + nxt + "b")
            assert out[-1].encode("utf-8")[59:60 + run + 1] == b" " + b"\\" * run + nxt.encode()
    out += ["a" * 63 + " b", "a" * 64 + " b"]                               # a space as byte 63 and as byte 64
    out.append("a" * 63 + "/x/yy/z b/q")                                   # a '/' as byte 63, its char in byte 62, the char's 2nd and 3rd tag in the next window
    assert _byte(out[-1], 63) == b"/"
    out.append("a/" + "x" * 150 + " b/y")                                  # a tag over three windows
    out.append("a/" + "x" * 70 + "/" + "y" * 70 + "/z b")                  # a window of tag bytes alone with a '/' in it: the carried count grows there
    return out


def edge_lines(kind):
    if kind == "tokenized":
        return tokenized_edge_lines()
    long_tags = ([("a", [list("x" * 70), list("y" * 70), ["z"]]), ("b", [])], [1])   # (as the tokenized list's last line)
    return [partialsuite.render(*s) for s in partialsuite.fixed_structs() + [long_tags]]


def check_window_edges(ctx, kind):
    """every line, in one batch and as a batch of its own (where it closes the CSR arrays), against the host parser; the host parser against the
    restatement"""
    lines = edge_lines(kind)
    host = host_parse(kind, lines)
    if kind == "tokenized":
        check_parsed(host, lines, _expect(lines))
        assert list(host["n_tags"][-3:]) == [3, 1, 3]                      # (the slot count carried over the window's edge)
    else:
        partialsuite.check_against_restatement(host, lines)
    partialsuite.assert_same(partialsuite.device_parse(ctx, lines, kind=kind), host, kind)
    for ln in lines:
        partialsuite.assert_same(partialsuite.device_parse(ctx, [ln], kind=kind), host_parse(kind, [ln]), (kind, ln))


def grid_stride_lines(kind):
    """one line more than a stride of the capped grid and four behind it, one char each; the last five are not the rest's, one has a tag"""
    return ["a"] * GRID_LINES + ["漢", "b/t", "\\ " if kind == "tokenized" else "|", "é", EMOJI]


def check_grid_stride(ctx, kind):
    lines = grid_stride_lines(kind)
    host = host_parse(kind, lines)
    assert len(host["labels"]) == 0 and list(host["n_tags"][-5:]) == [0, 1, 0, 0, 0] and bytes(host["tag_bytes"]) == b"t"
    assert bytes(host["raw"][GRID_LINES:]).decode("utf-8") == "漢b" + (" " if kind == "tokenized" else "|") + "é" + EMOJI
    partialsuite.assert_same(partialsuite.device_parse(ctx, lines, kind=kind), host, kind)


# the failing construct of every reason as byte 63 and as byte 64 of its line.  Reasons 1 and 2 cannot sit there: a line without any char is "" or a lone
# '\\', and only a line's first byte can be a space in front of every char -- they stand as they can, one of them in front of a second window.
TOKENIZED_BAD = {1: ["", "\\"], 2: [" " + "a" * 70, " a"],
                 3: ["a" * 62 + "  b", "a" * 63 + "  b"], 4: ["a" * 63 + " ", "a" * 64 + " "],
                 5: ["a" * 62 + " /x", "a" * 63 + " /x"], 6: ["a" * 63 + "\0b", "a" * 64 + "\0b"]}


def check_tokenized_first_errors(ctx):
    """every reason with its construct at the window's edge: alone in front of a later line's other reason, then behind an earlier line that fails
    for another reason -- the message names the smallest failing line and that line's reason, on the host and on the device"""
    rng = random.Random(31)
    valid = [random_line(rng, rng.randint(1, 8)) for _ in range(40)]
    assert not any(isinstance(e, Exception) for e in _expect(valid))

    def both(lines, reason, at):
        verdicts = _expect(lines)
        first = next(i for i, e in enumerate(verdicts) if isinstance(e, Exception))
        assert (first, verdicts[first].reason) == (at, reason)
        msg = "InvalidArgumentError: tokenized_text: %s (line %d)" % (evalref.MSG[reason], at)
        try:
            host_parse("tokenized", lines)
            assert False, "the host parser accepted the batch"
        except api.VaporettoError as e:
            assert str(e) == msg
        partialsuite.device_parse(ctx, lines, expect_error=msg, kind="tokenized")
    for reason in range(1, 7):
        other = 1 + reason % 6
        for k, bad in enumerate(TOKENIZED_BAD[reason]):
            if reason >= 3:
                assert bad.encode("utf-8")[63 + k] in b" /\0"
            lines = list(valid)
            lines[20], lines[33] = bad, TOKENIZED_BAD[other][k]
            both(lines, reason, 20)
            lines[9] = TOKENIZED_BAD[other][1 - k]
            both(lines, other, 9)
    # the workspace is clean afterwards
    p = partialsuite.device_parse(ctx, ["a b"], kind="tokenized")
    assert bytes(p["raw"]) == b"ab" and list(p["labels"]) == [1]
