"""`python -m vaporetto_amd.evaluate`: the reference's `evaluate` CLI (evaluate/src/main.rs) over this library.

Reads tokenized lines ("token/tag token/tag ...") from stdin, predicts them with the model and prints the char-level P / R / F1 and
TP / TN / FP / FN, or Nagata's word-level P / R / F1 -- the same stdout, byte for byte, and the same two stderr lines.  Parsing,
prediction, the post-filters, fill_tags and the counting run on the device (Predictor.evaluate); only the counters come back.
The model file must be un-compressed (the reference reads it through zstd: decompress it first, e.g. `zstd -d`)."""
import argparse
import decimal
import math
import sys

_WSCONST = {"D": 1, "R": 2, "H": 3, "T": 4, "K": 5, "O": 6, "G": "G"}
_ZSTD_MAGIC = b"\x28\xb5\x2f\xfd"


def rust_f64(x: float) -> str:
    """Rust's `{}` for an f64: the shortest digits that round-trip, never an exponent, no ".0" on an integer, NaN / inf."""
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    r = repr(float(x))
    if "e" in r or "E" in r:
        r = format(decimal.Decimal(r), "f")
    if r.endswith(".0"):
        r = r[:-2]
    return r


def split_lines(data: bytes):
    """BufRead::lines(): split at '\\n', a '\\r' right in front of a '\\n' belongs to the terminator (one at the end of a last line without
    '\\n' stays), no empty last line after a final '\\n'.  Invalid UTF-8 is UnicodeDecodeError (the reference's io error)."""
    text = data.decode("utf-8")
    lines = text.split("\n")
    last = lines.pop()
    out = [ln[:-1] if ln.endswith("\r") else ln for ln in lines]
    if last:
        out.append(last)
    return out


def report(r: dict, metric: str) -> str:
    out = "Precision: %s\nRecall: %s\nF1: %s\n"
    if metric == "char":
        out = out % (rust_f64(r["char_precision"]), rust_f64(r["char_recall"]), rust_f64(r["char_f1"]))
        return out + "TP: %d, TN: %d, FP: %d, FN: %d\n" % (r["tp"], r["tn"], r["fp"], r["fn"])
    return out % (rust_f64(r["word_precision"]), rust_f64(r["word_recall"]), rust_f64(r["word_f1"]))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="evaluate", description="A program to evaluate the accuracy of Vaporetto.")
    ap.add_argument("--model", required=True, help="The model file to use when analyzing text")
    ap.add_argument("--predict-tags", action="store_true", help="Predicts POS tags.")
    ap.add_argument("--wsconst", action="append", default=[], choices=sorted(_WSCONST),
                    help="Do not segment some character types: {D, R, H, T, K, O, G}.")
    ap.add_argument("--no-norm", action="store_true", help="Do not normalize input strings before prediction.")
    ap.add_argument("--metric", choices=["char", "word"], default="char", help="Evaluation metric: {char, word}.")
    args = ap.parse_args(argv)

    from . import api
    print("Loading model file...", file=sys.stderr)
    raw = open(args.model, "rb").read()
    if raw[:4] == _ZSTD_MAGIC:
        print("Error: %s is zstd-compressed: decompress it first (zstd -d)" % args.model, file=sys.stderr)
        return 1
    try:
        model, _ = api.Model.read_slice(raw)
        predictor = api.Predictor(model, args.predict_tags)
        print("Start tokenization", file=sys.stderr)
        lines = split_lines(sys.stdin.buffer.read())
        r = predictor.evaluate(lines, predict_tags=args.predict_tags, wsconst=[_WSCONST[w] for w in args.wsconst], no_norm=args.no_norm)
    except api.VaporettoError as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    except UnicodeDecodeError:
        print("Error: stream did not contain valid UTF-8", file=sys.stderr)
        return 1
    sys.stdout.write(report(r, args.metric))
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
