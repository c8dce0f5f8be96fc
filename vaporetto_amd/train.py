"""`python -m vaporetto_amd.train`: the reference's `train` CLI (train/src/main.rs) over this library.

Reads tokenized (--tok) and partially annotated (--part) corpora and word dictionaries (--dict), normalises them with
KyteaFullwidthFilter unless --no-norm, trains the boundary model on the device (api.Trainer: features, ids and the TRON solver all
run there) and writes the model un-compressed (the `evaluate` CLI reads it as it is; the reference writes zstd).  Progress goes to
stderr as the reference prints it.  Tokenized and partially annotated lines are parsed by the library's batch parsers
(vpt_parse_tokenized_batch, vpt_parse_partial_batch) in chunks.

With --train-tags (ours) the tags of the corpora are kept and the tag models are trained on the device too (api.Trainer(train_tags=True):
the parser's arrays go straight into add_packed_tagged), the dictionary lines become the tag dictionary (main.rs:131-157), and the
reference's `Tags: n/n` line is printed once, at the end.

With --l1r (ours) the trainer is made with l1r=True and --solver 5 (L1-regularised L2-loss SVC, the reference README's solver) trains by
coordinate descent over column groups on the device; most weights end at exactly 0, so the model is small.  With --l1r-tags (ours)
beside --l1r and --train-tags, --solver 5 trains the tag models too, by the same coordinate descent.  With --l1r-lr (ours) the trainer
is made with l1r_lr=True and --solver 6 (L1-regularised logistic regression) trains the boundary model by liblinear's newGLMNET on the
device: a sparse model again, with the logistic loss.  With --l1r-lr-tags (ours) beside --l1r-lr and --train-tags, --solver 6 trains the
tag models too, by the same newGLMNET: sparse tag models whose --tag-scores are log-odds.

Divergences: without --train-tags tag models are not trained, so a corpus or dictionary line that carries a tag is an error naming the
file and line unless --ignore-tags (ours) drops the tags; only solvers 0 and 2 are implemented, and solver 5 only with --l1r (ours: without
it --solver 5 is refused like the others; with it and --train-tags it is refused too unless --l1r-tags is given), and solver 6 only with
--l1r-lr (ours; refused together with --train-tags unless --l1r-lr-tags is given); --zstd-workers does not exist."""
import argparse
import sys

import numpy as np

from .evaluate import split_lines

_CHUNK_LINES = 1 << 16


class CorpusError(Exception):
    pass


def _lines(path):
    with open(path, "rb") as fh:
        try:
            return split_lines(fh.read())
        except UnicodeDecodeError:
            raise CorpusError("%s: stream did not contain valid UTF-8" % path) from None


def _parse_chunks(path, lines, ignore_tags, parse):
    """Chunks of the library's batch parser `parse`: yields (raw utf8, raw byte offsets, labels, the parser's arrays) per chunk; errors name the
    file and line."""
    from . import api
    for c0 in range(0, len(lines), _CHUNK_LINES):
        chunk = [ln.encode("utf-8") for ln in lines[c0:c0 + _CHUNK_LINES]]
        try:
            p = parse(chunk)
        except api.VaporettoError as e:
            msg = str(e)
            k = msg.rfind(" (line ")
            if k >= 0:
                line = c0 + int(msg[k + 7:msg.index(")", k)]) + 1
                msg = msg[:k]
                raise CorpusError("%s:%d: %s" % (path, line, msg)) from None
            raise CorpusError("%s: %s" % (path, msg)) from None
        if not ignore_tags and len(p["tag_bytes"]):
            # the first line with a non-empty tag: per char its tags tag_index[g] .. tag_index[g + 1]
            span = np.diff(p["span_offsets"].astype(np.int64)) > 0
            has = np.concatenate([[0], np.cumsum(span)])
            oo, S = p["out_offsets"].astype(np.int64), len(chunk)
            first = oo[:S] + np.arange(S)
            last = oo[1:] + np.arange(1, S + 1)
            ti = p["tag_index"].astype(np.int64)
            tagged = has[ti[last]] - has[ti[first]] > 0
            i = int(np.argmax(tagged))
            if tagged[i]:
                raise CorpusError("%s:%d: carries tags; tag models are not trained (--ignore-tags drops them, --train-tags trains them)" % (path, c0 + i + 1))
        yield p["raw"], p["raw_offsets"], p["labels"], p


def _parse_tokenized(path, lines, ignore_tags):
    """vpt_parse_tokenized_batch in chunks"""
    from . import api
    return _parse_chunks(path, lines, ignore_tags, api.parse_tokenized_host)


def _parse_partial(path, lines, ignore_tags):
    """vpt_parse_partial_batch in chunks: the same arrays, labels 0 / 1 / 2 and tags on any char"""
    from . import api
    return _parse_chunks(path, lines, ignore_tags, api.parse_partial_host)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="train", description="A program to train models of Vaporetto.")
    ap.add_argument("--tok", action="append", default=[], help="A tokenized training corpus")
    ap.add_argument("--part", action="append", default=[], help="A partially annotated training corpus")
    ap.add_argument("--dict", action="append", default=[], help="A word dictionary file")
    ap.add_argument("--model", required=True, help="The file to write the trained model to")
    ap.add_argument("--charw", type=int, default=3, help="The character window to use for word segmentation")
    ap.add_argument("--charn", type=int, default=3, help="The character n-gram length to use for word segmentation")
    ap.add_argument("--typew", type=int, default=3, help="The character type window to use for word segmentation")
    ap.add_argument("--typen", type=int, default=3, help="The character type n-gram length to use for word segmentation")
    ap.add_argument("--dictn", type=int, default=4, help="Dictionary words longer than this value will be grouped together")
    ap.add_argument("--eps", type=float, default=0.01, help="The epsilon stopping criterion for classifier training")
    ap.add_argument("--cost", type=float, default=1.0, help="The cost hyperparameter for classifier training")
    ap.add_argument("--solver", type=int, required=True, choices=range(8), metavar="{0..7}",
                    help="The solver. {0, 1, 2, 3, 4, 5, 6, 7} (only 0 and 2 are implemented here, 5 with --l1r and 6 with --l1r-lr)")
    ap.add_argument("--no-norm", action="store_true", help="Do not normalize training data.")
    ap.add_argument("--ignore-tags", action="store_true", help="Drop tags of the corpora and dictionaries (no tag models are trained).")
    ap.add_argument("--train-tags", action="store_true", help="Keep the tags of the corpora and dictionaries and train the tag models.")
    ap.add_argument("--l1r", action="store_true", help="Make the trainer accept --solver 5 (L1-regularised L2-loss SVC).")
    ap.add_argument("--l1r-tags", action="store_true", help="With --l1r and --train-tags: --solver 5 trains the tag models too.")
    ap.add_argument("--l1r-lr", action="store_true", help="Make the trainer accept --solver 6 (L1-regularised logistic regression).")
    ap.add_argument("--l1r-lr-tags", action="store_true", help="With --l1r-lr and --train-tags: --solver 6 trains the tag models too.")
    args = ap.parse_args(argv)
    if not args.tok and not args.part:
        ap.error("one of --tok or --part is required")
    if args.train_tags and args.ignore_tags:
        ap.error("--train-tags and --ignore-tags exclude each other")
    if args.l1r_tags and not (args.l1r and args.train_tags):
        print("Error: --l1r-tags needs both --l1r and --train-tags", file=sys.stderr)
        return 1
    if args.l1r_lr_tags and not (args.l1r_lr and args.train_tags):
        print("Error: --l1r-lr-tags needs both --l1r-lr and --train-tags", file=sys.stderr)
        return 1
    skip_tags = args.ignore_tags or args.train_tags   # either way a tag is no error

    from . import api
    fw = api.KyteaFullwidthFilter()
    try:
        print("Loading dataset...", file=sys.stderr)
        batches, n_sent = [], 0
        for path in args.tok:
            print("Loading %r ..." % path, file=sys.stderr)
            lines = _lines(path)
            for raw, roff, labels, p in _parse_tokenized(path, lines, skip_tags):
                batches.append((raw, roff, labels, p if args.train_tags else None))
            n_sent += len(lines)
            print("# of sentences: %d" % n_sent, file=sys.stderr)
        for path in args.part:
            print("Loading %r ..." % path, file=sys.stderr)
            lines = _lines(path)
            for raw, roff, labels, p in _parse_partial(path, lines, skip_tags):
                batches.append((raw, roff, labels, p if args.train_tags else None))
            n_sent += len(lines)
            print("# of sentences: %d" % n_sent, file=sys.stderr)
        words, tag_dictionary = set(), []
        for path in args.dict:
            print("Loading %r ..." % path, file=sys.stderr)
            lines = _lines(path)
            for raw, roff, labels, p in _parse_tokenized(path, lines, skip_tags):
                oo = p["out_offsets"]
                ti, so, tb = p["tag_index"], p["span_offsets"], bytes(p["tag_bytes"])
                for i in range(len(roff) - 1):
                    text = bytes(raw[int(roff[i]):int(roff[i + 1])]).decode("utf-8")
                    if not args.no_norm:
                        text = fw.filter(text)   # a 1:1 char map: the boundaries keep their places
                    s = api.Sentence.from_raw(text)
                    s._boundaries = labels[int(oo[i]):int(oo[i + 1])].copy()
                    words.update(s.iter_tokens())
                    if args.train_tags:   # the tokens with the tags of their last chars, the text normalised and the tags as they are
                        nt, g0 = int(p["n_tags"][i]), int(oo[i]) + i
                        for a, e in s._token_ranges():
                            own = [tb[int(so[k]):int(so[k + 1])].decode("utf-8") for k in range(int(ti[g0 + e]), int(ti[g0 + e + 1]))]
                            tag_dictionary.append((text[a:e + 1], [(t or None) for t in own] + [None] * (nt - len(own))))
            print("# of words: %d" % len(words), file=sys.stderr)
        dictionary = sorted(words)   # BTreeSet<String>: code point order (main.rs:132-161)

        print("Extracting into features...", file=sys.stderr)
        trainer = api.Trainer(args.charw, args.charn, args.typew, args.typen, dictionary, args.dictn, ignore_tags=args.ignore_tags,
                              train_tags=args.train_tags, tag_dictionary=tag_dictionary, l1r=args.l1r, l1r_tags=args.l1r_tags, l1r_lr=args.l1r_lr,
                              l1r_lr_tags=args.l1r_lr_tags)
        for utf8, boff, labels, p in batches:
            if p is not None:
                trainer.add_packed_tagged(utf8, boff, labels, p["n_tags"], p["tag_index"], p["span_offsets"], p["tag_bytes"],
                                          fullwidth=not args.no_norm)
            else:
                trainer.add_packed(utf8, boff, labels, fullwidth=not args.no_norm)
        print("# of features: %d" % trainer.n_features(), file=sys.stderr)
        print("Start training...", file=sys.stderr)
        model = trainer.train_bytes(args.eps, args.cost, args.solver)
        if args.train_tags:
            print("Tags: %d/%d" % ((trainer.n_tag_models(),) * 2), file=sys.stderr)
        print("Finish training.", file=sys.stderr)
    except CorpusError as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    except api.VaporettoError as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    with open(args.model, "wb") as fh:
        fh.write(model)
    return 0


if __name__ == "__main__":
    sys.exit(main())
