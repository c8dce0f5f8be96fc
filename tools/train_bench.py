"""The trainer on a synthetic corpus: random text labelled by the golden model's predictions, then api.Trainer with --solver 2 (the
default), 5 (a Trainer(l1r=True)) or 6 (a Trainer(l1r_lr=True)); the option may be given more than once: the solvers then train one
after the other on the same trainer and matrix, a line each.

Reports one JSON line per solver: feature extraction (vpt_trainer_add_batch) and id assignment / design matrix (the first vpt_trainer_n_features)
with keys per second, the TRON iterations and CG steps, the training time and the mean time per CG step (one Xw, one Xᵀv and the
reductions).  Xw and Xᵀv are not timed on their own.  For solver 5 the line holds the sweeps, the seconds per sweep, the line-search
halvings and the first and last violation sums instead, for solver 6 the Newton iterations, the inner sweeps, the seconds per inner
sweep (the whole training over the sweeps: the launches over all columns and the line searches are in it) and the two violation sums;
every line ends with the nonzero weights and the model's bytes.  A CPU
comparison with sklearn's liblinear is not part of it yet."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHABET = "0123456789abcdefABCあいうえおかきくけこカキクケコー漢字東京都市。、"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=1_000_000)
    ap.add_argument("--chars", type=int, default=64)
    ap.add_argument("--batch", type=int, default=250_000)
    ap.add_argument("--solver", type=int, action="append", choices=(2, 5, 6))
    a = ap.parse_args()
    solvers = a.solver or [2]
    from vaporetto_amd import api
    raw = open(os.path.join(ROOT, "tests", "golden", "model.bin"), "rb").read()
    labeler = api.Predictor(api.Model.read_slice(raw)[0], False, device=0)
    rng = np.random.default_rng(0)
    alpha = np.array([c.encode() for c in ALPHABET], dtype=object)
    t = api.Trainer(3, 3, 3, 3, l1r=5 in solvers, l1r_lr=6 in solvers)
    t_add, n_b = 0.0, 0
    for s0 in range(0, a.sentences, a.batch):
        n = min(a.batch, a.sentences - s0)
        idx = rng.integers(0, len(ALPHABET), (n, a.chars))
        texts = [b"".join(alpha[row]) for row in idx]
        utf8, boff = api.pack_texts(texts)
        _, labels, _ = labeler.predict_packed(utf8, boff)
        t0 = time.perf_counter()
        t.add_packed(utf8, boff, labels)
        t_add += time.perf_counter() - t0
        n_b += len(labels)
    t0 = time.perf_counter()
    nf = t.n_features()
    t_build = time.perf_counter() - t0
    ptr, _, _ = t.csr()
    nnz = int(ptr[-1])
    base = {"sentences": a.sentences, "chars": a.chars, "boundaries": n_b, "features": nf, "nonzeros": nnz,
            "extract_s": round(t_add, 3), "ids_and_matrix_s": round(t_build, 3),
            "keys_per_s": round(nnz / (t_add + t_build), 1) if t_add + t_build else None}
    for solver in solvers:
        t0 = time.perf_counter()
        model = t.train_bytes(0.01, 1.0, solver)
        t_train = time.perf_counter() - t0
        st = t.last_stats()
        w, b, _ = t.weights()
        out = dict(base, solver=solver, train_s=round(t_train, 3))
        if solver == 5:
            out.update(sweeps=st["iterations"], s_per_sweep=round(t_train / max(st["iterations"], 1), 4), halvings=st["cg_steps"],
                       violation0=st["gnorm0"], violation=st["gnorm"])
        elif solver == 6:
            out.update(newton_iterations=st["iterations"], inner_sweeps=st["cg_steps"], s_per_inner_sweep=round(t_train / max(st["cg_steps"], 1), 4),
                       violation0=st["gnorm0"], violation=st["gnorm"])
        else:
            out.update(tron_iterations=st["iterations"], cg_steps=st["cg_steps"], ms_per_cg_step=round(1e3 * t_train / max(st["cg_steps"], 1), 3),
                       xw_ms="not measured", xtv_ms="not measured")
        out.update(objective=st["objective"], nonzero_weights=int(np.count_nonzero(w)) + int(b != 0), model_bytes=len(model))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
