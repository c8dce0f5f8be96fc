"""Times the predict CLI's listings on the device (vpt_predict_listing_batch_device) with HIP events: bench.py's configs[1] workload (100 K
sentences x 64 chars, synthetic M1) for the scores block, the tagged synthetic M3 of configs[4] for the tag block -- scores and labels already
on the device -- beside the untagged writer on the same batch (vpt_write_tokenized_batch_device) and the host's time to format the same bytes
in Python from copied-back scores.  What is timed is the whole listing CALL: the offset check, decode_chars or (with tags) fill_tags, the
writer's T, then the listing's own count / scan / write launches -- the C ABI has no entry that runs those three alone, so HIP events
cannot bracket them.  The launches one by one come from a kernel trace of this tool (`rocprofv3 --kernel-trace --stats -- python
tools/listing_bench.py`, profiles/listing_kernel_stats.csv): compare the listing's kernels there with emit_flat_kernel's row, like with
like; `listing_over_writer_rate` here sets a whole call against one kernel and is a lower bound of that.  Prints one JSON line; --out
writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaporetto_amd import _lib, api, synth   # noqa: E402


def dev(arr):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(arr.dtype)
    return torch.from_numpy(arr.view(signed) if signed else arr).cuda()


def timed(fn, sync, warmup, runs):
    ms = []
    for k in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        sync()
        b.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def run(kind, listing, sentences, length, warmup, runs, host_sample):
    raw = synth.synth_model(kind, synth.SEED_BASE + 2, 1.0)
    tags = bool(listing & (_lib.VPT_LISTING_TAG_SCORES | _lib.VPT_LISTING_TAGGED))
    pred = api.Predictor(api.Model.read_slice(raw)[0], tags, device=0)
    utf8, boff = synth.synth_sentences(raw, sentences, length, length, seed=synth.SEED_BASE + 2)
    ooff = api.count_boundaries(utf8, boff)
    S, nb = sentences, int(ooff[-1])
    d_text, d_boff, d_ooff = dev(np.concatenate([utf8, np.zeros(64, np.uint8)])), dev(boff), dev(ooff)
    d_scores, d_labels = torch.zeros(nb + 16, dtype=torch.int32, device="cuda"), torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")
    cap = pred.listing_capacity(len(utf8), nb + S, S, listing)
    d_out, d_off = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda"), torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    batch = api.DeviceBatch(pred)
    batch.set_flags(_lib.VPT_FLAG_KYTEA_FULLWIDTH)
    batch.predict(d_text.data_ptr(), d_boff.data_ptr(), d_ooff.data_ptr(), S, nb, int(np.max(np.diff(boff.astype(np.int64)))), d_scores.data_ptr(),
                  d_labels.data_ptr(), stream)
    batch.sync()
    lst_ms, _ = timed(lambda: batch.predict_listing(d_text.data_ptr(), d_boff.data_ptr(), d_ooff.data_ptr(), S, nb, len(utf8), d_scores.data_ptr(),
                                                    d_labels.data_ptr(), listing, d_out.data_ptr(), cap, d_off.data_ptr(), stream), batch.sync, warmup, runs)
    lst_bytes = int(d_off[S].item())
    wr_ms, _ = timed(lambda: batch.write_tokenized(d_text.data_ptr(), d_boff.data_ptr(), d_ooff.data_ptr(), S, nb, d_labels.data_ptr(), d_out.data_ptr(),
                                                   3 * len(utf8), d_off.data_ptr(), stream), batch.sync, warmup, runs)
    t_bytes = int(d_off[S].item())
    # the only way before this entry point: copy the scores back and format on the host, one f-string per boundary (a sample, scaled)
    n = min(host_sample, S)
    t0 = time.perf_counter()
    sc = d_scores[:int(ooff[n])].cpu().numpy()
    fw = api.KyteaFullwidthFilter()
    total = 0
    for i in range(n):
        s = fw.filter(bytes(utf8[int(boff[i]):int(boff[i + 1])]).decode("utf-8"))
        a = int(ooff[i])
        total += len("".join("%d:%s%s %d\n" % (j, s[j], s[j + 1], sc[a + j]) for j in range(len(s) - 1)).encode("utf-8"))
    host_s = (time.perf_counter() - t0) * S / n
    return dict(model="synthetic-" + {1: "M1", 3: "M3"}[kind], sentences=S, chars_per_sentence=length, listing_flags=listing,
                listing_ms=round(lst_ms, 4), listing_bytes=lst_bytes, listing_gb_per_s=round(lst_bytes / lst_ms / 1e6, 2),
                writer_ms=round(wr_ms, 4), writer_bytes=t_bytes, writer_gb_per_s=round(t_bytes / wr_ms / 1e6, 2),
                listing_over_writer_rate=round((lst_bytes / lst_ms) / (t_bytes / wr_ms), 3),
                host_python_scores_block_s_extrapolated=round(host_s, 2), host_sample_sentences=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--host-sample", type=int, default=2000)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = dict(tool="listing_bench", device=torch.cuda.get_device_name(0),
               scores_block=run(1, _lib.VPT_LISTING_SCORES, a.sentences, 64, a.warmup, a.runs, a.host_sample),
               tag_block=run(3, _lib.VPT_LISTING_TAG_SCORES | _lib.VPT_LISTING_TAGGED, a.sentences, 64, a.warmup, a.runs, a.host_sample))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
