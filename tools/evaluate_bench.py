"""Times the tokenized-text path on one GPU: the parse kernel (vpt_parse_tokenized_batch_device), the compare kernel
(vpt_evaluate_labels_batch_device, tags from fill_tags' records) and vpt_evaluate_batch end to end beside vpt_tokenize_batch on the same
lines.  Gold corpus: synthetic lines tokenized (tagged) by the model itself, with a seeded share of boundaries and tags flipped on the host.
The counters are checked against a host computation outside the timed region.
    python tools/evaluate_bench.py [--lines N] [--reps R]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vaporetto_amd import _lib, api  # noqa: E402

HBM_GBS = 8000.0
WORDS = ["まぁ", "社長", "は", "火星", "猫", "だ", "良い", "だろう", "東京", "特許", "許可", "局", "の", "人", "地球", "プログラミング", "体験", "を", "Rust", "で"]


def corpus(pred, n, seed):
    rng = random.Random(seed)
    texts = ["".join(rng.choice(WORDS) for _ in range(rng.randint(8, 20))) for _ in range(n)]
    gold = []
    for t in pred.tokenize(texts, tagged=True):
        toks = t.split(" ")
        for k in range(len(toks) - 1):
            if rng.random() < 0.08 and "/" not in toks[k]:       # merge with the next token: a boundary flipped
                toks[k + 1] = toks[k] + toks[k + 1]
                toks[k] = None
        toks = [x for x in toks if x is not None]
        toks = [x.replace("/名詞", "/動詞", 1) if rng.random() < 0.05 else x for x in toks]   # a wrong tag
        gold.append(" ".join(toks))
    return gold


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
    ap.add_argument("--lines", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    L = _lib.load()
    raw_model = open(os.path.join(ROOT, "tests", "golden", "model.bin"), "rb").read()
    pred = api.Predictor(api.Model.read_slice(raw_model)[0], True)
    lines = corpus(pred, a.lines, 1)
    enc = [ln.encode("utf-8") for ln in lines]
    utf8, boff = api.pack_texts(enc)
    S, B = len(lines), len(utf8)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def d(n, dt):
        return torch.zeros(max(n, 1), dtype=dt, device=dev)
    d_text = torch.from_numpy(np.concatenate([utf8, np.zeros(16, np.uint8)])).to(dev)
    d_boff = torch.from_numpy(boff.view(np.int64)).to(dev)
    o = [d(B, torch.uint8), d(S + 1, torch.int64), d(S + 1, torch.int64), d(B, torch.uint8), d(S, torch.int32), d(B + 1, torch.int64),
         d(B + 1, torch.int64), d(B, torch.uint8)]
    batch = api.DeviceBatch(pred)

    def parse():
        st = L.vpt_parse_tokenized_batch_device(pred.handle, batch._h, d_text.data_ptr(), d_boff.data_ptr(), S, B, *[t.data_ptr() for t in o], stream)
        assert st == 0
    parse_ms = timed(parse, a.reps, torch)
    batch.sync()
    h = api.parse_tokenized_host(enc)                     # (outside the timed region)
    roff, ooff = h["raw_offsets"], h["out_offsets"]
    nb, n_tags_total = int(ooff[S]), int(h["tag_index"][-1])
    out_bytes = int(roff[S]) + nb + 16 * S + 4 * S + 8 * (nb + S + 1) + 8 * (n_tags_total + 1) + len(h["tag_bytes"])
    parse_gbs = (B + 8 * (S + 1) + out_bytes) / parse_ms / 1e6

    # the system side: predict (normalised) on the raw text, fill_tags on the workspace, then the compare alone
    _, sys_l, sys_ooff = pred.predict_packed(h["raw"], roff, fullwidth=True)
    d_sys = torch.from_numpy(np.concatenate([sys_l, np.zeros(1, np.uint8)])).to(dev)
    batch.set_flags(_lib.VPT_FLAG_KYTEA_FULLWIDTH)
    batch.fill_tags(o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), S, nb, d_sys.data_ptr(), 0, stream)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)

    def compare():
        st = L.vpt_evaluate_labels_batch_device(pred.handle, batch._h, o[2].data_ptr(), S, o[3].data_ptr(), o[4].data_ptr(), o[5].data_ptr(),
                                                o[6].data_ptr(), o[7].data_ptr(), d_sys.data_ptr(), _lib.VPT_EVAL_TAGS_PREDICTED, counts.data_ptr(), stream)
        assert st == 0
    compare_ms = timed(compare, a.reps, torch)
    batch.sync()
    compare_gbs = (2 * nb + 8 * (S + 1) + 4 * S) / compare_ms / 1e6

    # end to end: host lines in, counters out; beside vpt_tokenize_batch on the raw lines
    cnt = np.zeros(8, np.uint64)
    flags = _lib.VPT_FLAG_KYTEA_FULLWIDTH

    def e2e():
        st = L.vpt_evaluate_batch(pred.handle, utf8.ctypes.data, boff.ctypes.data, S, flags, 1, cnt.ctypes.data)
        assert st == 0, _lib.last_error()

    def tok():
        pred.tokenize_packed(h["raw"], roff, tagged=True, flags=flags)
    walls = {}
    for name, fn in (("evaluate_batch", e2e), ("tokenize_batch", tok)):
        fn()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        walls[name] = (time.perf_counter() - t0) / a.reps * 1e3

    # check (outside the timed regions): char counters and token counts from the host parse and the predicted labels
    g = h["labels"].astype(np.int64)
    s = sys_l[:nb].astype(np.int64)
    want = {"tp": int(((g == s) & (s == 1)).sum()), "tn": int(((g == s) & (s == 0)).sum()), "fp": int(((g != s) & (s == 1)).sum()),
            "fn": int(((g != s) & (s == 0)).sum()), "n_sys": int(s.sum()) + S, "n_ref": int(g.sum()) + S, "n_sentences": S}
    got = dict(zip(("tp", "tn", "fp", "fn", "n_sys", "n_ref", "n_cor", "n_sentences"), (int(x) for x in cnt)))
    ok = all(got[k] == v for k, v in want.items()) and got["n_cor"] <= min(got["n_sys"], got["n_ref"])
    kc = counts.cpu().numpy().view(np.uint64)
    ok = ok and int(kc[6]) % (a.reps + 1) == 0 and int(kc[6]) // (a.reps + 1) == got["n_cor"]
    print(json.dumps({"lines": S, "tokenized_bytes": B, "boundaries": nb,
                      "parse_ms": round(parse_ms, 4), "parse_GBs": round(parse_gbs, 1), "parse_frac_hbm": round(parse_gbs / HBM_GBS, 3),
                      "compare_ms": round(compare_ms, 4), "compare_GBs": round(compare_gbs, 1), "compare_frac_hbm": round(compare_gbs / HBM_GBS, 3),
                      "evaluate_batch_ms": round(walls["evaluate_batch"], 3), "tokenize_batch_ms": round(walls["tokenize_batch"], 3),
                      "counters": got, "counters_ok": bool(ok)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
