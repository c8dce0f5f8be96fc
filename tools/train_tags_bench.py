#!/usr/bin/env python
"""Times tag-model training on a synthetic tagged corpus: extraction (add), problem construction, and the solver -- the batched
in-kernel TRON against the same problems pushed one by one through the global-memory TRON (Trainer.set_tag_path(1)), in one process,
after an untimed warm-up run (--solver 5 and --solver 6: the L1 solvers' legs instead, below).  The ratio is taken over the problems the kernel solved, the one-by-one side counting its TRON runs only.

Corpus: `--surfaces` random surfaces of 1-3 kana with Zipf-like weights 1 / rank, one tag slot, 2-8 candidates per surface, the tag
decided by the char behind the token; `--sentences` sentences of 4-16 tokens.  Prints one JSON line with the sizes and the seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vaporetto_amd import api  # noqa: E402


def corpus(n_sent, n_surf, seed):
    rng = np.random.default_rng(seed)
    kana = [chr(c) for c in range(0x3042, 0x3082)]
    surfaces = []
    while len(surfaces) < n_surf:
        w = "".join(kana[k] for k in rng.integers(0, len(kana), int(rng.integers(1, 4))))
        if w not in surfaces:
            surfaces.append(w)
    n_cand = rng.integers(2, 9, n_surf)
    p = 1.0 / np.arange(1, n_surf + 1)
    p /= p.sum()
    lines = []
    for _ in range(n_sent):
        ids = rng.choice(n_surf, int(rng.integers(4, 17)), p=p)
        toks = [surfaces[i] for i in ids]
        out = []
        for k, i in enumerate(ids):
            nxt = ord(toks[k + 1][0]) if k + 1 < len(toks) else 0
            out.append("%s/t%d" % (toks[k], nxt % int(n_cand[i])))
        lines.append(" ".join(out).encode("utf-8"))
    return lines


def l1_leg(arrays, res, out):
    """--solver 5: a Trainer(l1r=True, train_tags=True, l1r_tags=True) trains the corpus with solver 5 and then with solver 2, each once
    untimed and once timed, by size; the tag solvers' seconds, problems per path, sweeps, halvings and the share of exactly-zero weights
    go to `out` with solver 2's numbers of the same run beside them."""
    import numpy as np
    t = api.Trainer(2, 2, 2, 2, train_tags=True, l1r=True, l1r_tags=True)
    t.add_packed_tagged(*arrays)
    for solver in (5, 2):
        t.train_bytes(0.01, 1.0, solver)   # warm-up
        t0 = time.perf_counter()
        model = t.train_bytes(0.01, 1.0, solver)
        t1 = time.perf_counter()
        st = t.tag_stats()
        sm = st["summary"]
        w = np.concatenate([t.tag_weights(i).ravel() for i in range(len(st["problems"]))])
        res["solver_%d" % solver] = {
            "train_total_s": t1 - t0, "seconds_in_kernel": sm["seconds_in_kernel"], "seconds_large": sm["seconds_large"],
            "seconds_large_solve": sm["seconds_large_solve"], "problems_in_kernel": sm["problems_in_kernel"], "problems_large": sm["problems_large"],
            "iterations": int(sum(c["iterations"] for q in st["problems"] for c in q["classes"])),
            "cg_steps_or_halvings": int(sum(c["cg_steps"] for q in st["problems"] for c in q["classes"])),
            "classes_at_max_iterations": int(sum(c["iterations"] >= 1000 for q in st["problems"] for c in q["classes"])),
            "zero_weight_share": float((w == 0.0).mean()), "model_bytes": len(model)}
    print(json.dumps(res))
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


def l1lr_leg(arrays, res, out):
    """--solver 6: one Trainer with every flag (train_tags, l1r, l1r_tags, l1r_lr, l1r_lr_tags) trains the corpus with solvers 6, 5 and
    2, each once untimed and once timed, by size; per solver the tag solvers' seconds, problems per path, iterations (Newton iterations,
    sweeps or TRON iterations), inner steps (sweeps, halvings or CG steps), the share of exactly-zero weights, the model's size and its
    SHA-256 go to `out`."""
    import hashlib
    t = api.Trainer(2, 2, 2, 2, train_tags=True, l1r=True, l1r_tags=True, l1r_lr=True, l1r_lr_tags=True)
    t.add_packed_tagged(*arrays)
    for solver in (6, 5, 2):
        t.train_bytes(0.01, 1.0, solver)   # warm-up
        t0 = time.perf_counter()
        model = t.train_bytes(0.01, 1.0, solver)
        t1 = time.perf_counter()
        st = t.tag_stats()
        sm = st["summary"]
        w = np.concatenate([t.tag_weights(i).ravel() for i in range(len(st["problems"]))])
        res["solver_%d" % solver] = {
            "train_total_s": t1 - t0, "seconds_in_kernel": sm["seconds_in_kernel"], "seconds_large": sm["seconds_large"],
            "seconds_large_solve": sm["seconds_large_solve"], "problems_in_kernel": sm["problems_in_kernel"], "problems_large": sm["problems_large"],
            "iterations": int(sum(c["iterations"] for q in st["problems"] for c in q["classes"])),
            "inner_steps": int(sum(c["cg_steps"] for q in st["problems"] for c in q["classes"])),
            "zero_weight_share": float((w == 0.0).mean()), "model_bytes": len(model), "model_sha256": hashlib.sha256(model).hexdigest()}
    print(json.dumps(res))
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=4000)
    ap.add_argument("--surfaces", type=int, default=300)
    ap.add_argument("--solver", type=int, default=2)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default="profiles/train_tags_l1_bench.json", help="where --solver 5 writes its result; --solver 6 writes to it too (profiles/train_tags_l1lr_bench.json is its run's)")
    args = ap.parse_args()
    p = api.parse_tokenized_host(corpus(args.sentences, args.surfaces, args.seed))
    arrays = (p["raw"], p["raw_offsets"], p["labels"], p["n_tags"], p["tag_index"], p["span_offsets"], p["tag_bytes"])
    res = {"sentences": args.sentences, "surfaces": args.surfaces, "solver": args.solver, "chars": int(len(p["tag_index"]) - 1),
           "charn": 2, "typen": 2}
    if args.solver == 5:
        return l1_leg(arrays, res, args.out)
    if args.solver == 6:
        return l1lr_leg(arrays, res, args.out)
    # warm-up: one whole run by size (the device, the allocator and the code objects), not timed
    w = api.Trainer(2, 2, 2, 2, train_tags=True)
    w.add_packed_tagged(*arrays)
    w.train_bytes(0.01, 1.0, args.solver)
    del w
    runs = {}
    for mode, name in ((0, "by_size"), (1, "one_by_one")):
        t = api.Trainer(2, 2, 2, 2, train_tags=True)
        t.set_tag_path(mode)
        t0 = time.perf_counter()
        t.add_packed_tagged(*arrays)
        t1 = time.perf_counter()
        probs = t.tag_problems()
        t2 = time.perf_counter()
        t.train_bytes(0.01, 1.0, args.solver)
        t3 = time.perf_counter()
        st = t.tag_stats()
        runs[name] = st
        if mode == 0:
            res.update(problems=len(probs), rows=int(sum(q["n_rows"] for q in probs)), nonzeros=int(sum(len(q["cols"]) for q in probs)),
                       classes=int(sum(len(q["candidates"]) for q in probs)),
                       extraction_s=t1 - t0, extraction_host_interning_s=st["summary"]["seconds_add_host"],
                       construction_s=st["summary"]["seconds_construction"],
                       construction_host_grouping_s=st["summary"]["seconds_construction_host"])
        res[name] = dict(st["summary"], train_total_s=t3 - t2)
    # the comparison: the problems the kernel solved, against the same problems one by one through the global-memory TRON
    # (its TRON runs alone: the per-problem upload and CSC construction are counted apart)
    small = [i for i, q in enumerate(runs["by_size"]["problems"]) if q["path"] == 1]
    one = runs["one_by_one"]["problems"]
    res["in_kernel_problems"] = len(small)
    res["in_kernel_s"] = runs["by_size"]["summary"]["seconds_in_kernel"]
    res["same_problems_one_by_one_solve_s"] = sum(one[i]["seconds_solve"] for i in small)
    res["same_problems_one_by_one_setup_s"] = sum(one[i]["seconds_setup"] for i in small)
    if res["in_kernel_s"] > 0:
        res["one_by_one_over_in_kernel"] = res["same_problems_one_by_one_solve_s"] / res["in_kernel_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
