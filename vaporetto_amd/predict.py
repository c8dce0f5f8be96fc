"""`python -m vaporetto_amd.predict`: the reference's `predict` CLI (predict/src/main.rs) over this library.

Lines on stdin, tokenized lines on stdout, byte for byte what the reference prints, with the same three stderr lines.  With --scores every
line is followed by "{i}:{c}{c'} {score}" per boundary and an empty line, with --tag-scores by every token's surface and "\\ttag:score,..."
per tag slot and an empty line.  Scoring, the post-filters, fill_tags, the tokenized text and BOTH listings are made on the device
(Predictor.predict_listing_arena -> vpt_predict_listing_batch); the host cuts stdin into chunks of lines and writes the arena of each chunk as
it came from the device, with one write and no per-line work on the output path.  "G" (ConcatGraphemeClustersFilter) is a flag of the same call.

Order of the pieces of a line, as in the reference: normalising (default) `T "\\n" [scores] [tag scores]` (main.rs:154-176); with --no-norm
`T [scores] "\\n" [tag scores]` (main.rs:129-144) -- the first score line follows T without a newline between them.  That is the reference's
order and it is reproduced here.

Divergences: a line that Sentence::update_raw rejects (empty, or with a NUL) prints "\\n" as in the reference, but with --tag-scores the
reference then lists the PREVIOUS sentence's stale state (and panics when the line is the first): here nothing more is printed for such a
line.  --tag-scores without --predict-tags panics in the reference: here the arguments are rejected.  The model file must be un-compressed
(the reference reads it through zstd: decompress it first, e.g. `zstd -d`)."""
import argparse
import sys
import time

import numpy as np

from .evaluate import _WSCONST, _ZSTD_MAGIC, rust_f64, split_lines

_CHUNK_LINES = 1 << 16   # lines per device batch (train.py's chunk): bounds the memory of a long stream


def _lines_of(data: bytes):
    """split_lines; when the bytes are not UTF-8, first the lines in front of the failing one (the reference prints every line until its
    reader fails), then the error."""
    try:
        return split_lines(data), None
    except UnicodeDecodeError as e:
        return split_lines(data[:data.rfind(b"\n", 0, e.start) + 1]), e


def _read_lines(stream, chunk_lines):
    """Chunks of at most chunk_lines lines of a binary stream, split as BufRead::lines() splits them (evaluate.split_lines)."""
    pending = b""
    while True:
        block = stream.read(1 << 22)
        if not block:
            break
        pending += block
        cut = pending.rfind(b"\n")
        if cut < 0:
            continue
        lines, bad = _lines_of(pending[:cut + 1])
        pending = pending[cut + 1:]
        for c0 in range(0, len(lines), chunk_lines):
            yield lines[c0:c0 + chunk_lines]
        if bad is not None:
            raise bad
    if pending:
        lines, bad = _lines_of(pending)
        if lines:
            yield lines
        if bad is not None:
            raise bad


def _chunk_bytes(predictor, lines, args, types, graphemes):
    """The stdout bytes of a chunk of lines, as one buffer: the arena the device made (Predictor.predict_listing_arena), with a "\n" spliced
    in for every line that Sentence::update_raw rejects (sentence.rs:264-283) -- by offset arithmetic, nothing is done per line."""
    ok = np.fromiter((len(ln) > 0 and "\0" not in ln for ln in lines), dtype=bool, count=len(lines))
    n_good = int(np.count_nonzero(ok))
    if n_good == 0:
        return b"\n" * len(lines)
    good = lines if n_good == len(lines) else [ln for ln, k in zip(lines, ok) if k]
    arena, offs = predictor.predict_listing_arena(good, scores=args.scores, tag_scores=args.tag_scores, tagged=args.predict_tags,
                                                  fullwidth=not args.no_norm, wsconst=types + (["G"] if graphemes else []),
                                                  no_norm_order=args.no_norm)
    if n_good == len(lines):
        return arena
    before = np.cumsum(ok)[~ok]   # per rejected line: the good lines in front of it; its "\n" goes where the next good line starts
    return np.insert(arena, offs[before].astype(np.int64), 0x0A)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="predict", description="A program to perform tokenization with Vaporetto.")
    ap.add_argument("--model", required=True, help="The model file to use when tokenizing text")
    ap.add_argument("--predict-tags", action="store_true", help="Predicts tags.")
    ap.add_argument("--wsconst", action="append", default=[], choices=sorted(_WSCONST),
                    help="Do not segment some character types: {D, R, H, T, K, O, G}.")
    ap.add_argument("--scores", action="store_true", help="Prints scores.")
    ap.add_argument("--tag-scores", action="store_true", help="Prints tag scores.")
    ap.add_argument("--no-norm", action="store_true", help="Do not normalize input strings before prediction.")
    args = ap.parse_args(argv)
    if args.tag_scores and not args.predict_tags:
        ap.error("--tag-scores requires --predict-tags")

    from . import api
    print("Loading model file...", file=sys.stderr)
    raw = open(args.model, "rb").read()
    if raw[:4] == _ZSTD_MAGIC:
        print("Error: %s is zstd-compressed: decompress it first (zstd -d)" % args.model, file=sys.stderr)
        return 1
    types = [_WSCONST[w] for w in args.wsconst if w != "G"]
    graphemes = "G" in args.wsconst
    out = sys.stdout.buffer if hasattr(sys.stdout, "buffer") else sys.stdout
    try:
        model, _ = api.Model.read_slice(raw)
        predictor = api.Predictor(model, args.predict_tags)
        print("Start tokenization", file=sys.stderr)
        start = time.perf_counter()
        for lines in _read_lines(sys.stdin.buffer, _CHUNK_LINES):
            out.write(memoryview(_chunk_bytes(predictor, lines, args, types, graphemes)))
            out.flush()
    except api.VaporettoError as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    except UnicodeDecodeError:
        print("Error: stream did not contain valid UTF-8", file=sys.stderr)
        return 1
    print("Elapsed: %s [sec]" % rust_f64(time.perf_counter() - start), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
