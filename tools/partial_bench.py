"""Times the partial-annotation path on one GPU beside the tokenized parser: vpt_parse_partial_batch_device and vpt_parse_tokenized_batch_device
on synthetic corpora with the same number of bytes (the same words and tags, once as "ま-ぁ/名詞|社-長", once as "まぁ/名詞 社長": the tokenized
lines are padded with further tokens up to the partial corpus's size), and vpt_write_partial_batch_device on what the partial parser wrote.
The outputs are checked against the host forms outside the timed region.
    python tools/partial_bench.py [--lines N] [--reps R]"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vaporetto_amd import _lib, api  # noqa: E402

WORDS = ["まぁ", "社長", "は", "火星", "猫", "だ", "良い", "だろう", "東京", "特許", "許可", "局", "の", "人", "地球", "プログラミング", "体験", "を", "Rust", "で"]
TAGS = ["名詞", "助詞", "動詞", "形容詞", "マー", "シャチョー"]
KEYS = ("raw", "raw_offsets", "out_offsets", "labels", "n_tags", "tag_index", "span_offsets", "tag_bytes")


def corpora(n, seed):
    rng = random.Random(seed)
    part, tok = [], []
    for _ in range(n):
        words = [rng.choice(WORDS) for _ in range(rng.randint(8, 20))]
        tags = [["/" + rng.choice(TAGS) for _ in range(rng.choice([0, 0, 1, 2]))] for _ in words]
        p = "|".join("-".join(w) + "".join(t) for w, t in zip(words, tags))
        t = " ".join(w + "".join(tg) for w, tg in zip(words, tags))
        while len(t.encode("utf-8")) < len(p.encode("utf-8")) - 8:
            t += " " + rng.choice(WORDS)
        part.append(p)
        tok.append(t)
    return part, tok


def timed(fn, reps, torch):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    L = _lib.load()
    raw_model = open(os.path.join(ROOT, "tests", "golden", "model.bin"), "rb").read()
    pred = api.Predictor(api.Model.read_slice(raw_model)[0], False)
    batch = api.DeviceBatch(pred)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    part, tok = corpora(a.lines, 1)
    res, ok, parsed = {"lines": a.lines}, True, None

    def d(n, dt):
        return torch.zeros(max(n, 1), dtype=dt, device=dev)
    for name, lines, fn, host in (("partial", part, L.vpt_parse_partial_batch_device, api.parse_partial_host),
                                  ("tokenized", tok, L.vpt_parse_tokenized_batch_device, api.parse_tokenized_host)):
        enc = [ln.encode("utf-8") for ln in lines]
        utf8, boff = api.pack_texts(enc)
        S, B = len(enc), len(utf8)
        d_text = torch.from_numpy(np.concatenate([utf8, np.zeros(16, np.uint8)])).to(dev)
        d_boff = torch.from_numpy(boff.view(np.int64)).to(dev)
        o = [d(B, torch.uint8), d(S + 1, torch.int64), d(S + 1, torch.int64), d(B, torch.uint8), d(S, torch.int32), d(B + 1, torch.int64),
             d(B + 1, torch.int64), d(B, torch.uint8)]

        def parse():
            assert fn(pred.handle, batch._h, d_text.data_ptr(), d_boff.data_ptr(), S, B, *[t.data_ptr() for t in o], stream) == 0
        res[name + "_bytes"] = B
        res[name + "_parse_ms"] = round(timed(parse, a.reps, torch), 4)
        batch.sync()
        h = host(enc)                                      # (outside the timed region)
        for k, t in zip(KEYS, o):
            ok = ok and np.array_equal(t.cpu().numpy().view(h[k].dtype)[:len(h[k])], h[k])
        if name == "partial":
            parsed, keep = h, o
            cap = len(h["raw"]) + len(h["labels"]) + len(h["span_offsets"]) + len(h["tag_bytes"])
            d_out, d_toff = d(cap, torch.uint8), d(S + 1, torch.int64)

            def write():
                assert L.vpt_write_partial_batch_device(pred.handle, batch._h, keep[0].data_ptr(), keep[1].data_ptr(), S, keep[2].data_ptr(),
                                                        keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), keep[6].data_ptr(),
                                                        keep[7].data_ptr(), d_out.data_ptr(), cap, d_toff.data_ptr(), stream) == 0
            res["partial_write_ms"] = round(timed(write, a.reps, torch), 4)
            batch.sync()
            ok = ok and bytes(d_out.cpu().numpy()[:B]) == bytes(utf8)    # these tags hold no special: the corpus comes back byte for byte
    res["parse_ratio_partial_over_tokenized"] = round(res["partial_parse_ms"] / res["tokenized_parse_ms"], 3)
    res["partial_parse_GBs_in"] = round(res["partial_bytes"] / res["partial_parse_ms"] / 1e6, 1)
    res["tokenized_parse_GBs_in"] = round(res["tokenized_bytes"] / res["tokenized_parse_ms"] / 1e6, 1)
    res["outputs_ok"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
