#!/usr/bin/env python
"""Prints a SHA-256 per training case over the raw bytes of every weight and every field of the TRON stats, through the public Python
API alone: the same file run on two builds (`--root` names the checkout whose package and suites are imported) says whether a change
of the solver's code moved a bit.  The digests depend on the platform's exp and log; they compare two builds on one machine.

Cases: the boundary trainer on the three suite corpora and the "medium" shaped corpus, the tag suite's corpora with set_tag_path(0)
and (1), and the two problems at the in-kernel solver's LDS limit, each with solvers 0 and 2.  `--emulated` runs the kernel sources on
the CPU emulator (tests/emu.py) and leaves out "medium"."""
import argparse
import hashlib
import os
import struct
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--emulated", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from tests import tagtrainsuite, trainsuite  # noqa: E402
from vaporetto_amd import _lib  # noqa: E402

if args.emulated:
    from tests import emu
    _lib._lib = emu.load()

STATS = struct.Struct("<IIddd")


def stats_bytes(st):
    return STATS.pack(st["iterations"], st["cg_steps"], st["gnorm0"], st["gnorm"], st["objective"])


def boundary(t, eps, solver):
    t.train_bytes(eps, 1.0, solver)
    w, b, _ = t.weights()
    st = t.last_stats()
    return np.append(w, b).tobytes() + stats_bytes(st), "%d it %d cg" % (st["iterations"], st["cg_steps"])


def tags(t, solver):
    t.train_bytes(0.01, 1.0, solver)
    st = t.tag_stats()["problems"]
    h = b"".join(t.tag_weights(i).tobytes() + b"".join(stats_bytes(c) for c in p["classes"]) for i, p in enumerate(st))
    return h, "%d problems, %d in the kernel, %d cg" % (len(st), sum(p["path"] == 1 for p in st), sum(c["cg_steps"] for p in st for c in p["classes"]))


def cases():
    for solver in (0, 2):
        for case in trainsuite.CASES:
            yield "boundary seed %d solver %d" % (case[0], solver), lambda: boundary(trainsuite.run_pair(case, solver)[0], 0.01, solver)
        if not args.emulated:
            labels = trainsuite.shaped_labels("medium", "learnable")
            yield "boundary medium solver %d" % solver, lambda: boundary(trainsuite.shaped_trainer("medium", labels), 0.01, solver)
        for name, params in sorted(tagtrainsuite.CASES.items()):
            sents = tagtrainsuite.corpus(params[0], params[1], params[2])
            for path in (0, 1):
                yield "tags %s path %d solver %d" % (name, path, solver), lambda: tags(tagtrainsuite.run_pair(params, sents, path=path)[0], solver)
        for total in (7424, 7425):
            sents = tagtrainsuite.limit_corpus(total)
            yield "tags limit %d solver %d" % (total, solver), lambda: tags(tagtrainsuite.run_pair(tagtrainsuite.LIMIT_PARAMS, sents, tag_dictionary=())[0], solver)


for name, run in cases():
    data, note = run()
    print("%s  %-34s %s" % (hashlib.sha256(data).hexdigest(), name, note), flush=True)
