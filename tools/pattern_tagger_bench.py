"""PatternMatchTagger on the GPU box: python tools/pattern_tagger_bench.py [--sentences N] [--rules 10000,1000000] [--iters K] -- one JSON line per
rule count.

configs[4]'s text (synthetic M3: M1 + tag models, sentences of 8 .. 512 chars), scored once; then, on one workspace with device buffers and HIP
events on the stream, the median over --iters of: fill_tags without a tagger, fill_tags with the tagger bound (the difference is the tagger's
launches: pattern_match_kernel, the scan, pattern_merge_kernel), and the tagged writer over either set of records.  The rules: half of them
tokens of the text that have no tag model (numbers and symbols of the alphabet included), half random strings of 1 .. 6 chars that are no token.
"without" uses nothing this feature added, so the same figures come from a checkout of the parent commit with --rules 0.  The launches one by
one: `rocprofv3 --kernel-trace --stats -- python tools/pattern_tagger_bench.py --iters 5`."""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaporetto_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sentences", type=int, default=1_000_000)
ap.add_argument("--rules", default="10000,1000000")
ap.add_argument("--iters", type=int, default=11)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="")
args = ap.parse_args()

raw = synth.synth_model(3)
utf8, boff = synth.synth_sentences(raw, args.sentences, 8, 512, seed=synth.SEED_BASE + 2)
pred = api.Predictor(api.Model.read_slice(raw)[0], True)
_, labels, ooff = pred.predict_packed(utf8, boff)
S, nb = args.sentences, len(labels)
total_c = nb + S


def dev(a):
    signed = {np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


d_text, d_boff, d_ooff = dev(np.concatenate([utf8, np.zeros(32, np.uint8)])), dev(boff), dev(ooff)
d_lab = dev(np.concatenate([labels, np.zeros(16, np.uint8)]))
stream = torch.cuda.current_stream().cuda_stream
# tokens of a sample of the text, for the rules that hit
text = bytes(utf8)
rng = random.Random(3)
tokens = set()
for i in rng.sample(range(S), min(S, 20000)):
    t = text[int(boff[i]):int(boff[i + 1])].decode("utf-8")
    cut = [0] + [k + 1 for k in range(len(t) - 1) if labels[int(ooff[i]) + k] == 1] + [len(t)]
    tokens.update(t[a:b] for a, b in zip(cut, cut[1:]) if b - a <= 6)
tokens = sorted(tokens)
alpha = sorted(set("".join(tokens)))


def timed(fn):
    ts = []
    for k in range(args.warmup + args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= args.warmup:
            ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4)


for n_rules in [int(x) for x in args.rules.split(",")]:
    pairs, seen = [], set()
    for t in tokens[:n_rules // 2]:
        seen.add(t)
        pairs.append((t, ["R%d" % (len(pairs) % 50), None if len(pairs) % 3 == 0 else "y%d" % (len(pairs) % 1000)]))
    while len(pairs) < n_rules:
        t = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 6)))
        if t not in seen:
            seen.add(t)
            pairs.append((t, ["R%d" % (len(pairs) % 50), "z"]))
    tagger = api.PatternMatchTagger(pairs) if n_rules else None
    cap = 3 * len(utf8) + total_c * (pred.max_tag_suffix() + (tagger.max_tag_suffix(pred) if tagger else 0)) + 16
    d_out, d_off = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda"), torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    batch = api.DeviceBatch(pred)
    res = {"label": args.label, "sentences": S, "chars": total_c, "rules": n_rules}
    if tagger:
        res.update(tagger.info(pred))
    for name, tg in (("without", None), ("with", tagger)) if tagger else (("without", None),):
        batch.set_pattern_tagger(tg)
        res["fill_tags_ms_" + name] = timed(lambda: batch.fill_tags(d_text.data_ptr(), d_boff.data_ptr(), d_ooff.data_ptr(), S, nb, d_lab.data_ptr(), 0, stream))
        res["write_tagged_ms_" + name] = timed(lambda: batch.write_tagged(d_text.data_ptr(), d_boff.data_ptr(), d_ooff.data_ptr(), S, nb, d_lab.data_ptr(), 0,
                                                                          d_out.data_ptr(), cap, d_off.data_ptr(), stream))
        batch.sync()
        res["tokenized_bytes_" + name] = int(d_off[S].item())
    if tagger:
        res["tagger_ms"] = round(res["fill_tags_ms_with"] - res["fill_tags_ms_without"], 4)
    print(json.dumps(res, ensure_ascii=False), flush=True)
