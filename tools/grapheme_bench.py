"""`--wsconst G` end to end on the GPU box: python tools/grapheme_bench.py [--lines N] [--iters K] [--rounds R] -- one JSON line per corpus.

Two corpora of synthetic Japanese lines (the benchmark's model and text generator, 64 chars a line): "plain", and "mixed" -- the same lines
with an emoji, flag, ZWJ or combining sequence spliced into about 1 % of them.  Each is timed as Predictor.tokenize(.., wsconst=("G",)) and
as Predictor.tokenize(..) without the filter, the two alternating round by round in one process (what is compared shares the host's weather);
a timing is a host clock around the call, which ends in a device synchronise.  Per variant: the median and the minimum over all timed calls
and the spread of the rounds' medians.  The script uses only what Predictor.tokenize offered before the filter moved to the device, so the
same file run from a checkout of an earlier commit times the three-call host path: run it there for the "before" figure.  The filter launches'
own time comes from `rocprofv3 --kernel-trace --stats -- python tools/grapheme_bench.py --iters 5 --rounds 1` (the grapheme_* kernels)."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaporetto_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lines", type=int, default=100000)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--label", default="")
args = ap.parse_args()

SEQS = ["\U0001f44f\U0001f3fd", "\U0001f468‍\U0001f469‍\U0001f466", "\U0001f1ef\U0001f1f5", "が", "é", "\U0001f3bb️", "\U0001f1fa\U0001f1f8\U0001f1ef\U0001f1f5"]

raw = synth.synth_model(1)
utf8, boff = synth.synth_sentences(raw, args.lines, 64, 64, seed=synth.SEED_BASE + 2)
text = bytes(utf8)
plain = [text[int(boff[i]):int(boff[i + 1])].decode("utf-8") for i in range(args.lines)]
rng = random.Random(7)
mixed = list(plain)
for i in rng.sample(range(args.lines), max(1, args.lines // 100)):
    at = rng.randrange(1, len(mixed[i]))
    mixed[i] = mixed[i][:at] + rng.choice(SEQS) + mixed[i][at:]
pred = api.Predictor(api.Model.read_slice(raw)[0], False)


def timed(lines, ws):
    t0 = time.perf_counter()
    out = pred.tokenize(lines, fullwidth=True, wsconst=ws)
    return time.perf_counter() - t0, out


for name, lines in (("plain", plain), ("mixed", mixed)):
    variants = {"with_G": ("G",), "without_G": ()}
    times = {k: [] for k in variants}
    medians = {k: [] for k in variants}
    outs = {}
    for k, ws in variants.items():
        for _ in range(args.warmup):
            outs[k] = timed(lines, ws)[1]
    for _ in range(args.rounds):
        for k, ws in variants.items():
            ts = [timed(lines, ws)[0] for _ in range(args.iters)]
            times[k] += ts
            medians[k].append(float(np.median(ts)))
    chars = sum(len(ln) for ln in lines)
    res = {"label": args.label, "corpus": name, "lines": len(lines), "chars": chars, "calls_per_variant": args.iters * args.rounds,
           "lines_changed_by_G": sum(a != b for a, b in zip(outs["with_G"], outs["without_G"]))}
    for k in variants:
        res[k] = {"ms_median": round(1e3 * float(np.median(times[k])), 3), "ms_min": round(1e3 * min(times[k]), 3),
                  "ms_round_medians": [round(1e3 * m, 3) for m in medians[k]]}
    res["G_minus_plain_ms_median"] = round(res["with_G"]["ms_median"] - res["without_G"]["ms_median"], 3)
    print(json.dumps(res, ensure_ascii=False), flush=True)
