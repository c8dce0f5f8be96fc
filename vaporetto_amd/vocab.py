"""`python -m vaporetto_amd.vocab --model FILE [--wsconst K ...] [--no-norm] [--min-count N] [--max-size N] < corpus.txt`

Lines on stdin (a document each), the corpus' vocabulary on stdout: `count<TAB>surface` per line, most frequent first, ties by code points --
the order of vpt_vocab_counter_finish, whose second column is what api.Vocabulary takes.  The documents are tokenized as the token stream
tokenizes them (api.VaporettoTokenizer) and counted on the device (VaporettoTokenizer.count_batch -> vpt_token_stream_count_batch): no token
string leaves the device before the vocabulary itself is read out.  The surface counted is the KyteaFullwidthFilter image of a token (the
text as it was scored) unless --no-norm.  Empty lines and lines holding a NUL are no documents and are left out."""
import argparse
import sys

from .evaluate import _WSCONST, _ZSTD_MAGIC
from .predict import _CHUNK_LINES, _read_lines


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="vocab", description="Counts the token surfaces of a corpus on the device.")
    ap.add_argument("--model", required=True, help="The model file to use when tokenizing text")
    ap.add_argument("--wsconst", action="append", default=[], choices=sorted(_WSCONST),
                    help="Do not segment some character types: {D, R, H, T, K, O, G}.")
    ap.add_argument("--no-norm", action="store_true", help="Count the surfaces as they stand in the input, not their fullwidth image.")
    ap.add_argument("--min-count", type=int, default=1, help="Leave out surfaces counted fewer times.")
    ap.add_argument("--max-size", type=int, default=0, help="Print at most this many surfaces (0: all).")
    ap.add_argument("--max-keys", type=int, default=1 << 20, help="The distinct surfaces the counter can hold.")
    args = ap.parse_args(argv)

    from . import api
    raw = open(args.model, "rb").read()
    if raw[:4] == _ZSTD_MAGIC:
        print("Error: %s is zstd-compressed: decompress it first (zstd -d)" % args.model, file=sys.stderr)
        return 1
    out = sys.stdout.buffer if hasattr(sys.stdout, "buffer") else sys.stdout
    try:
        model, _ = api.Model.read_slice(raw)
        tokenizer = api.VaporettoTokenizer(model, "".join(args.wsconst), vocab_normalize=not args.no_norm)
        counter = api.VocabularyCounter(tokenizer.predictor, args.max_keys)
        for lines in _read_lines(sys.stdin.buffer, _CHUNK_LINES):
            docs = [ln for ln in lines if ln and "\0" not in ln]
            if docs:
                tokenizer.count_batch(docs, counter)
        surfaces, counts = counter.finish(args.min_count, args.max_size)
    except api.VaporettoError as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    except UnicodeDecodeError:
        print("Error: stream did not contain valid UTF-8", file=sys.stderr)
        return 1
    out.write("".join("%d\t%s\n" % (int(c), s) for s, c in zip(surfaces, counts)).encode("utf-8"))
    out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
