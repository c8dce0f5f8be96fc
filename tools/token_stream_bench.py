"""Token streams on the GPU box: the span kernel beside the untagged writer, and vpt_token_stream_batch end to end beside the two routes a caller
had to the same arrays before it.
    python tools/token_stream_bench.py [--configs 2,5] [--sentences N] [--steps 15] [--rounds 3] [--ids] [--out profiles/token_stream_bench.json]
Per workload (bench.py's configs[2] batch -- --sentences of it, 0: all -- and its documents workload):
  (a) kernels, by device events on the labels a predict call left on the device, in ONE process, alternating, `--rounds` rounds of `--steps` calls:
      token_spans_kernel and the untagged emit_flat_kernel (same text and labels in; the writer stores the tokens' text, the span kernel 4 bytes a
      token).  `spread` = (max - min) / min of a kernel's per-round medians: what a difference between the two has to exceed to mean anything.
  (b) end to end, pinned buffers, median of `--steps` calls that end in a synchronise:
      stream   vpt_token_stream_batch
      labels   vpt_predict_batch_flags (labels only, the adapter's filters as flags) + the numpy conversion of labels and text to the CSR
      text     vpt_tokenize_batch + numpy parsing of the tokenized text to the CSR (same flags without the linebreak ones: the synthetic text has none)
      and the host share of the two older routes on its own.
  (c) bytes over PCIe each way for the three.
  --ids: the vocabulary id pass (kernels_vocab.hip) on the span kernel's CSR by device events -- the vocabulary every other distinct surface of the
      first --vocab-docs documents -- as ms and ms per 100 K documents, and vpt_token_stream_ids_batch end to end (untagged route; its outputs are
      fresh pageable numpy arrays, the stream route's pinned) beside vpt_token_stream_batch; its ids must equal the device call's.
  --postings: the postings pass (kernels_postings.hip: four launches, the sort and the scan) over the ids of --ids by device events, in the same run.
  --merge K[,K..]: with --postings, the batch's documents as K equal ranges: the K segment calls, the ordered and the general merge
      (kernels_postings_merge.hip) and a device-to-device copy of the bytes the ordered merge must move, each the median of --rounds rounds of
      --steps calls by device events, beside the one-pass call of the same run (profiles/postings_merge_bench.json).
      Its `positional` row: the same ranges as positional segments (each with its positions call), the ordered and the general positional merge
      beside the merges without positions over the same segments and a copy of the bytes the ordered positional merge must move
      (profiles/postings_merge_positions_bench.json).
  --search Q,L,K: with --postings, Q queries of L terms drawn from the vocabulary by count (a term's tokens in the batch), top K, over the one-pass
      segment (kernels_postings_search.hip) by device events, beside two yardsticks of the same run: the general merge over one segment of as
      many input places as the search has candidates, and a device-to-device copy of half of 8 bytes a candidate plus 8 bytes a hit (a copy of
      B bytes moves B in and B out).  Q is halved until the candidates are at most --search-max-candidates (profiles/postings_search_bench.json).
  --boolean Q,L,K: with --postings, three settings over the one-pass segment (kernels_postings_boolean.hip) by device events, each beside the OR
      search of the same run over the same slots and a device-to-device copy of half of 8 bytes a place plus 8 bytes a hit: (a) Q queries of L
      terms drawn by count as --search draws them, all MUST; (b) Q all-MUST queries of L consecutive tokens of a random document as --phrase
      draws them, so each matches at least once (every_query_matches); (c) the queries of (a) as all-SHOULD (equals_or_search: the OR search's
      bytes).  Places against candidates, matches, times and ratios (profiles/postings_boolean_bench.json).
  --sloppy Q,L,S,K: with --postings, the phrases --phrase Q,L,K draws (the same generator and seed), top K, timed three ways in one process by
      device events: the exact phrase search, the sloppy search (vpt_postings_sloppy_phrase_search_device) with every slop 0 -- whose bytes
      the run checks against the exact search's -- and the sloppy search at slop S; the probes, the matches and both ratios
      (profiles/postings_sloppy_bench.json).
  --phrase Q,L,K: with --postings, Q phrases of L consecutive tokens of random documents (windows whose tokens all have a vocabulary entry, so
      every phrase occurs at least once), top K, over the one-pass segment with its position lists (kernels_postings_phrase.hip) by device
      events, beside yardsticks of the same process: the OR search of --search (the parent's kernels) over the same queries, every token a slot
      with its idf; the phrase search over every phrase's anchor slot alone (the same probes, scans and sort, none of the other slots'
      bisections: the difference is what those bisections cost); and a device-to-device copy of half of 4 bytes a probe plus 12 bytes a hit.
      Q is halved until the probes and the OR search's candidates are at most --search-max-candidates (profiles/postings_phrase_bench.json).
  --clause Q,L,K: with --postings, Q all-MUST queries over the one-pass segment with its position lists, each one window of L consecutive tokens
      of a random document as ONE phrase clause plus one SHOULD term drawn by count, top K, by device events: the lists call
      (vpt_postings_phrase_lists_device), the clause search over its lists, the two chained with no sync between them; the yardsticks of the
      same process are the parent commit's boolean search over the same tokens as L independent MUST slots plus the SHOULD slot, and its
      phrase search over the same phrases.  The run checks that the lists' probes and entries are the phrase search's probes and matches and
      that the clause search's match counts are the phrase search's (profiles/postings_clause_bench.json).
  --count: the vocabulary counter's count call (kernels_vocab_count.hip, three launches) on the same CSR by device events, in the same run as
      --ids: the first call on an empty counter (insert and commit) once, then rounds of calls on the filled counter; finish's wall time once.
Parity in the same run: the three routes' arrays equal each other on the whole batch, and equal tests/tokenref.py (the restatement on the CPU oracle)
on the first --parity-docs documents."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def csr_from_labels(utf8, boff, ooff, labels):
    """The host scan a caller of vpt_predict_batch_flags needed: (token_offsets, token_ends) from labels and text, vectorised."""
    S = len(boff) - 1
    lead = np.flatnonzero((utf8 & 0xC0) != 0x80).astype(np.int64)        # byte position of every char
    nchars = len(lead)
    first = (ooff[:-1] + np.arange(S, dtype=np.uint64)).astype(np.int64)  # the documents' first chars
    is_first = np.zeros(nchars, dtype=bool)
    is_first[first] = True
    doc_start = np.repeat(boff[:-1].astype(np.int64), np.diff(first, append=nchars))
    mark = np.ones(nchars, dtype=bool)                                    # a document's first char closes the one before it
    mark[~is_first] = labels[:nchars - S] == 1
    mark[0] = False
    value = lead - doc_start
    value[first[1:]] = np.diff(boff[:-1].astype(np.int64))                # ... with that document's length
    ends = np.concatenate([value[mark], [int(boff[-1] - boff[-2])]]).astype(np.uint32)
    per_doc = np.add.reduceat((mark & ~is_first).astype(np.int64), first) + 1
    toff = np.zeros(S + 1, dtype=np.uint64)
    toff[1:] = np.cumsum(per_doc)
    return toff, ends


def csr_from_tokenized(text, toff_text, S):
    """The host parse a caller of vpt_tokenize_batch needed (texts without '\\\\': the synthetic batches; else the slow exact loop)."""
    if (text == 0x5C).any():
        raise SystemExit("the batch needs un-escaping: not a synthetic one")
    sep = text == 0x20
    n_sep_before = np.cumsum(sep) - sep
    starts = toff_text[:-1].astype(np.int64)
    stops = toff_text[1:].astype(np.int64)
    sep_pos = np.flatnonzero(sep)
    line_idx = np.searchsorted(starts, sep_pos, side="right") - 1
    raw_start = starts - n_sep_before[np.minimum(starts, len(text) - 1)]   # raw bytes in front of the line = its text position minus the separators before
    ends_sep = sep_pos - n_sep_before[sep_pos] - raw_start[line_idx]
    doc_len = (stops - starts) - (np.add.reduceat(sep.astype(np.int64), starts) if len(text) else 0)
    per_doc = np.bincount(line_idx, minlength=S) + 1
    toff = np.zeros(S + 1, dtype=np.uint64)
    toff[1:] = np.cumsum(per_doc)
    ends = np.zeros(int(toff[-1]), dtype=np.uint32)
    last = toff[1:].astype(np.int64) - 1
    ends[last] = doc_len
    keep = np.ones(len(ends), dtype=bool)
    keep[last] = False
    ends[keep] = ends_sep
    return toff, ends


def med(xs):
    return float(np.median(xs))


def merge_rows(torch, batch, stream, dev, args, K, S, n_terms, dev_off, d_soff, d_ids, d_term, d_pdocs, d_ptfs, n_post, one_pass_ms):
    """--merge K: the batch's documents in K equal ranges, each a segment of the postings call (its token_offsets rebased to 0, its ids and its
    posting arrays slices of the batch's, doc_base its first document); by device events: the K segment calls together, the ordered merge, the
    general merge, and device-to-device copies of as many bytes as the ordered merge must move (8 bytes a posting in and out, the K
    term_offsets arrays in -- a copy of B bytes moves B in and B out, so 8 * postings and 4 * K * (n_terms + 1) bytes are copied).  The ordered
    merge's three arrays must be the one-pass call's bytes."""
    cuts = [S * s // K for s in range(K + 1)]
    tok = [int(dev_off[c]) for c in cuts]
    seg_off = [(d_soff[a:b + 1] - d_soff[a]).contiguous() for a, b in zip(cuts, cuts[1:])]
    seg_term = torch.empty(K * (n_terms + 1), dtype=torch.int64, device=dev)
    seg_docs, seg_tfs = torch.empty(tok[-1] + 1, dtype=torch.int32, device=dev), torch.empty(tok[-1] + 1, dtype=torch.int32, device=dev)
    seg_cnt = torch.zeros(2 * K, dtype=torch.int64, device=dev)
    out_term = torch.empty(n_terms + 1, dtype=torch.int64, device=dev)
    out_docs, out_tfs = torch.empty(tok[-1] + 1, dtype=torch.int32, device=dev), torch.empty(tok[-1] + 1, dtype=torch.int32, device=dev)
    out_cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    descr = [(seg_term.data_ptr() + 8 * s * (n_terms + 1), seg_docs.data_ptr() + 4 * tok[s], seg_tfs.data_ptr() + 4 * tok[s], n_terms, tok[s + 1] - tok[s])
             for s in range(K)]

    def segments():
        for s in range(K):
            batch.postings(seg_off[s].data_ptr(), cuts[s + 1] - cuts[s], d_ids.data_ptr() + 4 * tok[s], tok[s + 1] - tok[s], n_terms, cuts[s], descr[s][0],
                           descr[s][1], descr[s][2], tok[s + 1] - tok[s], 0, 0, seg_cnt.data_ptr() + 16 * s, stream)

    def merge(ordered):
        batch.merge_postings(descr, n_terms, out_term.data_ptr(), out_docs.data_ptr(), out_tfs.data_ptr(), tok[-1], out_cnt.data_ptr(), ordered, stream)
    a_post, b_post = torch.empty(2 * n_post + 2, dtype=torch.int32, device=dev), torch.empty(2 * n_post + 2, dtype=torch.int32, device=dev)
    a_term, b_term = torch.empty(K * (n_terms + 1) // 2 + 1, dtype=torch.int64, device=dev), torch.empty(K * (n_terms + 1) // 2 + 1, dtype=torch.int64, device=dev)

    def floor():
        b_post.copy_(a_post)
        b_term.copy_(a_term)
    segments()
    batch.sync()
    out = {"K": K, "n_terms": n_terms, "input_places": tok[-1], "postings": n_post, "table_bytes": 8 * K * (n_terms + 1),
           "floor_bytes_copied": 8 * n_post + 4 * K * (n_terms + 1), "one_pass_ms": one_pass_ms}
    for name, fn in (("segments", segments), ("ordered", lambda: merge(True)), ("general", lambda: merge(False)), ("floor", floor)):
        fn()
        batch.sync()
        if name == "ordered":
            n = int(out_cnt[0].item())
            out["ordered_equals_one_pass"] = bool(n == n_post and int(out_cnt[1].item()) == 0 and torch.equal(out_term, d_term)
                                                  and torch.equal(out_docs[:n], d_pdocs[:n]) and torch.equal(out_tfs[:n], d_ptfs[:n]))
        if name == "general":
            n = int(out_cnt[0].item())
            out["general_equals_one_pass"] = bool(n == n_post and int(out_cnt[1].item()) == 0 and torch.equal(out_term, d_term)
                                                  and torch.equal(out_docs[:n], d_pdocs[:n]) and torch.equal(out_tfs[:n], d_ptfs[:n]))
        r = []
        for _ in range(args.rounds):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for a, b in ev:
                a.record(); fn(); b.record()
            torch.cuda.synchronize()
            r.append(med([a.elapsed_time(b) for a, b in ev]))
        batch.sync()
        out[name + "_ms"] = round(med(r), 4)
        out[name + "_rounds_ms"] = [round(x, 4) for x in r]
    for name in ("ordered", "general"):
        out[name + "_over_floor"] = round(out[name + "_ms"] / out["floor_ms"], 2)
        out[name + "_over_one_pass"] = round(out[name + "_ms"] / one_pass_ms, 3)
    out["segments_plus_ordered_over_one_pass"] = round((out["segments_ms"] + out["ordered_ms"]) / one_pass_ms, 3)
    out["segments_over_one_pass"] = round(out["segments_ms"] / one_pass_ms, 3)
    out["positional"] = positional_merge_row(torch, batch, stream, dev, args, K, S, n_terms, cuts, tok, seg_off, descr, seg_cnt, d_soff, d_ids, n_post,
                                             out["ordered_ms"], out["general_ms"])
    return out


def positional_merge_row(torch, batch, stream, dev, args, K, S, n_terms, cuts, tok, seg_off, descr, seg_cnt, d_soff, d_ids, n_post, ordered_ms, general_ms):
    """The positional row of --merge K: the same K document ranges, each a POSITIONAL segment (its postings call with the
    optional pair and its positions call, NULL token_positions); by device events: the K pairs of calls together, the ordered and the general
    positional merge, and device-to-device copies of as many bytes as the ordered positional merge must move (8 bytes a posting, 8 bytes a
    post_first entry and 4 bytes a position in and out, the K term_offsets arrays in).  The yardsticks of the same process: the merges without
    positions over the same segments (ordered_ms, general_ms of the row above) and that copy.  Both routes' five arrays must be the bytes of
    the one-pass positional segment of the whole batch."""
    T = tok[-1]
    i64, i32 = torch.int64, torch.int32
    w_term, w_first, w_cnt = torch.empty(n_terms + 1, dtype=i64, device=dev), torch.empty(T + 2, dtype=i64, device=dev), torch.zeros(2, dtype=i64, device=dev)
    w_docs, w_tfs, w_order, w_ppos = (torch.empty(T + 1, dtype=i32, device=dev) for _ in range(4))
    batch.postings(d_soff.data_ptr(), S, d_ids.data_ptr(), T, n_terms, 0, w_term.data_ptr(), w_docs.data_ptr(), w_tfs.data_ptr(), T, w_first.data_ptr(),
                   w_order.data_ptr(), w_cnt.data_ptr(), stream)
    batch.postings_positions(d_soff.data_ptr(), S, T, 0, w_term.data_ptr(), n_terms, w_first.data_ptr(), T, w_order.data_ptr(), w_ppos.data_ptr(), stream)
    batch.sync()
    assert int(w_cnt[0].item()) == n_post
    n_idx = int(w_first[n_post].item())
    seg_first = torch.empty(T + K + 1, dtype=i64, device=dev)                     # segment s: tok[s] + s .. tok[s + 1] + s + 1
    seg_order, seg_ppos = torch.empty(T + 1, dtype=i32, device=dev), torch.empty(T + 1, dtype=i32, device=dev)
    first_at = [seg_first.data_ptr() + 8 * (tok[s] + s) for s in range(K)]
    order_at = [seg_order.data_ptr() + 4 * tok[s] for s in range(K)]
    ppos_at = [seg_ppos.data_ptr() + 4 * tok[s] for s in range(K)]
    pdescr = [(descr[s][0], descr[s][1], descr[s][2], first_at[s], ppos_at[s], n_terms, tok[s + 1] - tok[s], tok[s + 1] - tok[s]) for s in range(K)]
    o_term, o_first, o_cnt = torch.empty(n_terms + 1, dtype=i64, device=dev), torch.empty(T + 2, dtype=i64, device=dev), torch.zeros(3, dtype=i64, device=dev)
    o_docs, o_tfs, o_ppos = (torch.empty(T + 1, dtype=i32, device=dev) for _ in range(3))

    def segments():
        for s in range(K):
            n_s, docs_s = tok[s + 1] - tok[s], cuts[s + 1] - cuts[s]
            batch.postings(seg_off[s].data_ptr(), docs_s, d_ids.data_ptr() + 4 * tok[s], n_s, n_terms, cuts[s], descr[s][0], descr[s][1], descr[s][2], n_s,
                           first_at[s], order_at[s], seg_cnt.data_ptr() + 16 * s, stream)
            batch.postings_positions(seg_off[s].data_ptr(), docs_s, n_s, 0, descr[s][0], n_terms, first_at[s], n_s, order_at[s], ppos_at[s], stream)

    def merge(ordered):
        batch.merge_positional_postings(pdescr, n_terms, o_term.data_ptr(), o_docs.data_ptr(), o_tfs.data_ptr(), o_first.data_ptr(), T, o_ppos.data_ptr(), T,
                                        o_cnt.data_ptr(), ordered, stream)
    half = lambda n_bytes, dt, size: (torch.empty(n_bytes // (2 * size) + 1, dtype=dt, device=dev), torch.empty(n_bytes // (2 * size) + 1, dtype=dt, device=dev))
    copies = [half(2 * 8 * n_post, i32, 4), half(2 * 8 * (n_post + 1), i64, 8), half(2 * 4 * n_idx, i32, 4), half(8 * K * (n_terms + 1), i64, 8)]

    def floor():
        for a, b in copies:
            b.copy_(a)
    segments()
    batch.sync()
    out = {"K": K, "input_places": T, "position_places": T, "postings": n_post, "positions": n_idx, "table_bytes": 2 * 8 * K * (n_terms + 1),
           "floor_bytes_copied": 8 * n_post + 8 * (n_post + 1) + 4 * n_idx + 4 * K * (n_terms + 1),
           "ordered_without_positions_ms": ordered_ms, "general_without_positions_ms": general_ms}
    for name, fn in (("segments", segments), ("ordered", lambda: merge(True)), ("general", lambda: merge(False)), ("floor", floor)):
        fn()
        batch.sync()
        if name in ("ordered", "general"):
            n, m = int(o_cnt[0].item()), int(o_cnt[2].item())
            out[name + "_equals_one_pass"] = bool(n == n_post and m == n_idx and int(o_cnt[1].item()) == 0 and torch.equal(o_term, w_term)
                                                  and torch.equal(o_docs[:n], w_docs[:n]) and torch.equal(o_tfs[:n], w_tfs[:n])
                                                  and torch.equal(o_first[:n + 1], w_first[:n + 1]) and torch.equal(o_ppos[:m], w_ppos[:m]))
        r = []
        for _ in range(args.rounds):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for a, b in ev:
                a.record(); fn(); b.record()
            torch.cuda.synchronize()
            r.append(med([a.elapsed_time(b) for a, b in ev]))
        batch.sync()
        out[name + "_ms"] = round(med(r), 4)
        out[name + "_rounds_ms"] = [round(x, 4) for x in r]
    for name, plain in (("ordered", ordered_ms), ("general", general_ms)):
        out[name + "_over_floor"] = round(out[name + "_ms"] / out["floor_ms"], 2)
        out[name + "_over_without_positions"] = round(out[name + "_ms"] / plain, 3)
    return out


def search_rows(torch, batch, stream, dev, args, spec, S, n_terms, dev_off, d_term, d_pdocs, d_ptfs, n_post):
    """--search Q,L,K over the one-pass segment; see the module's docstring"""
    from vaporetto_amd import api
    Q, L, K = (int(x) for x in spec.split(","))
    term = d_term.cpu().numpy().astype(np.int64)
    df = np.diff(term)
    tfs = d_ptfs[:n_post].cpu().numpy().astype(np.int64)
    count = np.add.reduceat(np.concatenate([tfs, [0]]), np.minimum(term[:-1], n_post)) * (df > 0)
    rng = np.random.default_rng(7)
    while True:
        terms = rng.choice(n_terms, size=Q * L, p=count / count.sum()).astype(np.int32)
        n_cand = int(df[terms].sum())
        if n_cand <= args.search_max_candidates or Q == 1:
            break
        Q //= 2
    if n_cand >= 1 << 32:
        raise SystemExit("--search: %d candidates" % n_cand)
    idf = {int(t): float(api.bm25_idf(S, int(df[t]))) for t in set(terms.tolist())}
    dl = np.diff(dev_off.astype(np.int64))
    avgdl = float(np.float32(float(dl.sum()) / S))
    d_dl = torch.from_numpy(dl.astype(np.int32)).to(dev)
    d_qoff = torch.from_numpy(np.arange(0, Q * L + 1, L, dtype=np.int64)).to(dev)
    d_qt = torch.from_numpy(terms).to(dev)
    d_qw = torch.from_numpy(np.array([idf[int(t)] for t in terms], np.float32)).to(dev)
    d_hd, d_hs = torch.zeros(Q * K, dtype=torch.int32, device=dev), torch.zeros(Q * K, dtype=torch.float32, device=dev)
    d_hc, d_mc, d_cnt = torch.zeros(Q, dtype=torch.int32, device=dev), torch.zeros(Q, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)

    def search():
        batch.search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), n_terms, n_post, 0, S, d_dl.data_ptr(), d_qoff.data_ptr(), d_qt.data_ptr(),
                              d_qw.data_ptr(), Q, Q * L, 1.2, 0.75, avgdl, K, n_cand, d_hd.data_ptr(), d_hs.data_ptr(), d_hc.data_ptr(), d_mc.data_ptr(),
                              d_cnt.data_ptr(), stream)
    search()
    batch.sync()
    cnt = d_cnt.cpu().numpy()
    matches = int(cnt[1])
    # the yardsticks: one segment of n_cand input places (the batch's postings in front, its term bounds cut there) through the general merge
    y_term = torch.clamp(d_term, max=n_cand).contiguous()
    y_docs, y_tfs = torch.zeros(n_cand + 1, dtype=torch.int32, device=dev), torch.zeros(n_cand + 1, dtype=torch.int32, device=dev)
    m = min(n_cand, n_post)
    y_docs[:m].copy_(d_pdocs[:m]); y_tfs[:m].copy_(d_ptfs[:m])
    o_term = torch.empty(n_terms + 1, dtype=torch.int64, device=dev)
    o_docs, o_tfs = torch.empty(n_cand + 1, dtype=torch.int32, device=dev), torch.empty(n_cand + 1, dtype=torch.int32, device=dev)
    o_cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def merge():
        batch.merge_postings([(y_term.data_ptr(), y_docs.data_ptr(), y_tfs.data_ptr(), n_terms, n_cand)], n_terms, o_term.data_ptr(), o_docs.data_ptr(),
                             o_tfs.data_ptr(), n_cand, o_cnt.data_ptr(), False, stream)
    copy_bytes = (8 * n_cand + 8 * matches) // 2
    a_buf, b_buf = torch.empty(copy_bytes + 8, dtype=torch.uint8, device=dev), torch.empty(copy_bytes + 8, dtype=torch.uint8, device=dev)

    def floor():
        b_buf.copy_(a_buf)
    out = {"spec": spec, "queries": Q, "slots_per_query": L, "k": K, "n_terms": n_terms, "documents": S, "postings": n_post, "candidates": int(cnt[0]),
           "matches": matches, "skipped": int(cnt[2]), "candidates_equal_host_count": bool(int(cnt[0]) == n_cand), "copy_bytes": copy_bytes,
           "sort_passes": {"group": min((S.bit_length() + 7) // 8, 4) + (Q.bit_length() + 7) // 8, "rank": 4 + (Q.bit_length() + 7) // 8,
                           "merge": 4 + (n_terms.bit_length() + 7) // 8}}
    for name, fn in (("search", search), ("merge", merge), ("floor", floor)):
        fn()
        batch.sync()
        r = []
        for _ in range(args.rounds):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for a, b in ev:
                a.record(); fn(); b.record()
            torch.cuda.synchronize()
            r.append(med([a.elapsed_time(b) for a, b in ev]))
        batch.sync()
        out[name + "_ms"] = round(med(r), 4)
        out[name + "_rounds_ms"] = [round(x, 4) for x in r]
    out["hit_counts_sum"] = int(d_hc.to(torch.int64).sum().item())
    out["candidates_per_s"] = round(int(cnt[0]) / out["search_ms"] * 1e3, 1)
    out["search_over_merge"] = round(out["search_ms"] / out["merge_ms"], 3)
    out["search_over_floor"] = round(out["search_ms"] / out["floor_ms"], 2)
    return out


def phrase_rows(torch, batch, stream, dev, args, spec, S, n_terms, dev_off, host_ids, d_soff, d_ids, cap_ends, d_term, d_pdocs, d_ptfs, n_post, seg,
                sloppy=False):
    """--phrase Q,L,K over the one-pass segment and its position lists (seg: post_first, post_positions, the indexed tokens); see the module's
    docstring.  sloppy: --sloppy Q,L,S,K -- the phrases --phrase Q,L,K draws, timed as the exact search, the sloppy call with every slop 0 and
    the sloppy call at S"""
    from vaporetto_amd import api
    if sloppy:
        Q, L, slop, K = (int(x) for x in spec.split(","))
    else:
        Q, L, K = (int(x) for x in spec.split(","))
    d_first, d_ppos, n_idx = seg
    term = d_term.cpu().numpy().astype(np.int64)
    df = np.diff(term)
    tfs = d_ptfs[:n_post].cpu().numpy().astype(np.int64)
    count = np.add.reduceat(np.concatenate([tfs, [0]]), np.minimum(term[:-1], n_post)) * (df > 0)
    toff = dev_off.astype(np.int64)
    dl = np.diff(toff)
    known = (host_ids >= 0) & (host_ids < n_terms)
    run = np.concatenate([[0], np.cumsum(~known)])   # a window [a, a + L) is all known when run[a + L] == run[a]
    long_docs = np.flatnonzero(dl >= L)
    rng = np.random.default_rng(7)
    phrases = []
    for _ in range(64 * Q):
        if len(phrases) == Q or len(long_docs) == 0:
            break
        d = int(long_docs[rng.integers(len(long_docs))])
        a = int(toff[d]) + int(rng.integers(int(dl[d]) - L + 1))
        if run[a + L] == run[a]:
            phrases.append(host_ids[a:a + L].astype(np.int32))
    if not phrases:
        raise SystemExit("--phrase: no window of %d tokens with vocabulary entries" % L)
    while True:
        terms = np.concatenate(phrases)
        n_probes = int(sum(int(count[ph].min()) for ph in phrases))
        n_cand = int(df[terms].sum())
        if max(n_probes, n_cand) <= args.search_max_candidates or len(phrases) == 1:
            break
        phrases = phrases[:len(phrases) // 2]
    Q = len(phrases)
    if max(n_probes, n_cand) >= 1 << 32:
        raise SystemExit("--phrase: %d probes, %d candidates" % (n_probes, n_cand))
    idf = {int(t): api.bm25_idf(S, int(df[t])) for t in set(terms.tolist())}
    weights = []
    for ph in phrases:   # tantivy's phrase weight: the float32 sum in slot order
        w = idf[int(ph[0])]
        for t in ph[1:]:
            w = np.float32(w + idf[int(t)])
        weights.append(w)
    anchors = np.array([ph[int(np.argmin(count[ph]))] for ph in phrases], np.int32)
    avgdl = float(np.float32(float(dl.sum()) / S))
    d_dl = torch.from_numpy(dl.astype(np.int32)).to(dev)
    d_qoff = torch.from_numpy(np.arange(0, Q * L + 1, L, dtype=np.int64)).to(dev)
    d_qt = torch.from_numpy(terms).to(dev)
    d_qw = torch.from_numpy(np.array(weights, np.float32)).to(dev)
    d_sw = torch.from_numpy(np.array([idf[int(t)] for t in terms], np.float32)).to(dev)
    d_aoff = torch.from_numpy(np.arange(0, Q + 1, dtype=np.int64)).to(dev)
    d_at = torch.from_numpy(anchors).to(dev)
    d_hd, d_hs, d_hf = (torch.zeros(Q * K, dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.int32))
    d_hc, d_mc, d_cnt = torch.zeros(Q, dtype=torch.int32, device=dev), torch.zeros(Q, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)

    def phrase():
        batch.phrase_search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), d_first.data_ptr(), d_ppos.data_ptr(), n_terms, n_post, n_idx,
                                     0, S, d_dl.data_ptr(), d_qoff.data_ptr(), d_qt.data_ptr(), d_qw.data_ptr(), Q, Q * L, 1.2, 0.75, avgdl, K, n_probes,
                                     d_hd.data_ptr(), d_hs.data_ptr(), d_hf.data_ptr(), d_hc.data_ptr(), d_mc.data_ptr(), d_cnt.data_ptr(), stream)

    def anchor_only():
        batch.phrase_search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), d_first.data_ptr(), d_ppos.data_ptr(), n_terms, n_post, n_idx,
                                     0, S, d_dl.data_ptr(), d_aoff.data_ptr(), d_at.data_ptr(), d_qw.data_ptr(), Q, Q, 1.2, 0.75, avgdl, K, n_probes,
                                     d_hd.data_ptr(), d_hs.data_ptr(), d_hf.data_ptr(), d_hc.data_ptr(), d_mc.data_ptr(), d_cnt.data_ptr(), stream)

    def or_search():
        batch.search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), n_terms, n_post, 0, S, d_dl.data_ptr(), d_qoff.data_ptr(), d_qt.data_ptr(),
                              d_sw.data_ptr(), Q, Q * L, 1.2, 0.75, avgdl, K, n_cand, d_hd.data_ptr(), d_hs.data_ptr(), d_hc.data_ptr(), d_mc.data_ptr(),
                              d_cnt.data_ptr(), stream)
    out = {"spec": spec, "queries": Q, "slots_per_query": L, "k": K, "n_terms": n_terms, "documents": S, "postings": n_post, "positions": n_idx}
    if sloppy:
        d_zero = torch.zeros(Q, dtype=torch.int32, device=dev)
        d_slops = torch.full((Q,), slop, dtype=torch.int32, device=dev)

        def sloppy_call(d_s):
            batch.phrase_search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), d_first.data_ptr(), d_ppos.data_ptr(), n_terms, n_post,
                                         n_idx, 0, S, d_dl.data_ptr(), d_qoff.data_ptr(), d_qt.data_ptr(), d_qw.data_ptr(), Q, Q * L, 1.2, 0.75, avgdl, K,
                                         n_probes, d_hd.data_ptr(), d_hs.data_ptr(), d_hf.data_ptr(), d_hc.data_ptr(), d_mc.data_ptr(), d_cnt.data_ptr(),
                                         stream, slops=d_s.data_ptr())
        out["slop"] = slop
        seen = {}
        for name, fn in (("phrase", phrase), ("sloppy0", lambda: sloppy_call(d_zero)), ("sloppy", lambda: sloppy_call(d_slops))):
            fn()
            batch.sync()
            cnt = d_cnt.cpu().numpy()
            seen[name] = (d_hd.clone(), d_hs.clone(), d_hf.clone(), d_hc.clone(), d_mc.clone())
            out.update({name + "_probes": int(cnt[0]), name + "_matches": int(cnt[1]), name + "_occurrences_in_hits": int(d_hf.to(torch.int64).sum().item())})
        out["sloppy0_equals_phrase_bytes"] = bool(all(torch.equal(a, b) for a, b in zip(seen["phrase"], seen["sloppy0"])))
        out["probes_equal_host_count"] = bool(out["phrase_probes"] == out["sloppy_probes"] == n_probes)
        for name, fn in (("phrase", phrase), ("sloppy0", lambda: sloppy_call(d_zero)), ("sloppy", lambda: sloppy_call(d_slops))):
            fn()
            batch.sync()
            r = []
            for _ in range(args.rounds):
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                for a, b in ev:
                    a.record(); fn(); b.record()
                torch.cuda.synchronize()
                r.append(med([a.elapsed_time(b) for a, b in ev]))
            batch.sync()
            out[name + "_ms"] = round(med(r), 4)
            out[name + "_rounds_ms"] = [round(x, 4) for x in r]
        out["sloppy0_over_phrase"] = round(out["sloppy0_ms"] / out["phrase_ms"], 3)
        out["sloppy_over_phrase"] = round(out["sloppy_ms"] / out["phrase_ms"], 3)
        out["probes_per_s"] = round(n_probes / out["sloppy_ms"] * 1e3, 1)
        return out
    or_search()
    batch.sync()
    cnt = d_cnt.cpu().numpy()
    out.update({"or_candidates": int(cnt[0]), "or_matches": int(cnt[1])})
    anchor_only()
    batch.sync()
    out["anchor_only_matches"] = int(d_cnt.cpu().numpy()[1])
    phrase()
    batch.sync()
    cnt = d_cnt.cpu().numpy()
    matches = int(cnt[1])
    out.update({"probes": int(cnt[0]), "matches": matches, "skipped": int(cnt[2]), "probes_equal_host_count": bool(int(cnt[0]) == n_probes),
                "every_phrase_matches": bool(int(d_mc.min().item()) >= 1), "hit_counts_sum": int(d_hc.to(torch.int64).sum().item()),
                "occurrences_in_hits": int(d_hf.to(torch.int64).sum().item())})
    copy_bytes = (4 * n_probes + 12 * matches) // 2
    a_buf, b_buf = torch.empty(copy_bytes + 8, dtype=torch.uint8, device=dev), torch.empty(copy_bytes + 8, dtype=torch.uint8, device=dev)
    out["copy_bytes"] = copy_bytes

    def floor():
        b_buf.copy_(a_buf)
    for name, fn in (("phrase", phrase), ("anchor_only", anchor_only), ("or_search", or_search), ("floor", floor)):
        fn()
        batch.sync()
        r = []
        for _ in range(args.rounds):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for a, b in ev:
                a.record(); fn(); b.record()
            torch.cuda.synchronize()
            r.append(med([a.elapsed_time(b) for a, b in ev]))
        batch.sync()
        out[name + "_ms"] = round(med(r), 4)
        out[name + "_rounds_ms"] = [round(x, 4) for x in r]
    out["probes_per_s"] = round(n_probes / out["phrase_ms"] * 1e3, 1)
    out["phrase_over_or_search"] = round(out["phrase_ms"] / out["or_search_ms"], 3)
    out["phrase_over_floor"] = round(out["phrase_ms"] / out["floor_ms"], 2)
    out["other_slots_share"] = round((out["phrase_ms"] - out["anchor_only_ms"]) / out["phrase_ms"], 4)
    return out


def clause_rows(torch, batch, stream, dev, args, spec, S, n_terms, dev_off, host_ids, d_term, d_pdocs, d_ptfs, n_post, seg):
    """--clause Q,L,K over the one-pass segment and its position lists: Q all-MUST queries, each one window of L consecutive tokens of a random
    document as ONE phrase clause plus one SHOULD term drawn by count.  Timed: the lists call, the clause search over its lists, the two
    chained with no sync between them; the yardsticks, in the same process: the boolean search over the same tokens as L independent MUST
    slots (plus the SHOULD slot), and the phrase search over the same phrases"""
    from vaporetto_amd import api
    Q, L, K = (int(x) for x in spec.split(","))
    d_first, d_ppos, n_idx = seg
    term = d_term.cpu().numpy().astype(np.int64)
    df = np.diff(term)
    tfs = d_ptfs[:n_post].cpu().numpy().astype(np.int64)
    count = np.add.reduceat(np.concatenate([tfs, [0]]), np.minimum(term[:-1], n_post)) * (df > 0)
    toff = dev_off.astype(np.int64)
    dl = np.diff(toff)
    known = (host_ids >= 0) & (host_ids < n_terms)
    run = np.concatenate([[0], np.cumsum(~known)])
    long_docs = np.flatnonzero(dl >= L)
    rng = np.random.default_rng(7)
    phrases = []
    for _ in range(64 * Q):
        if len(phrases) == Q or len(long_docs) == 0:
            break
        d = int(long_docs[rng.integers(len(long_docs))])
        a = int(toff[d]) + int(rng.integers(int(dl[d]) - L + 1))
        if run[a + L] == run[a]:
            phrases.append(host_ids[a:a + L].astype(np.int32))
    if not phrases:
        raise SystemExit("--clause: no window of %d tokens with vocabulary entries" % L)
    while True:
        terms = np.concatenate(phrases)
        should = rng.choice(n_terms, size=len(phrases), p=count / count.sum()).astype(np.int32)
        n_probes = int(sum(int(count[ph].min()) for ph in phrases))
        n_bound = int(sum(int(df[ph].min()) for ph in phrases))   # the list entries at most, and so the places of both searches
        if max(n_probes, n_bound) <= args.search_max_candidates or len(phrases) == 1:
            break
        phrases = phrases[:len(phrases) // 2]
    Q = len(phrases)
    idf = {int(t): api.bm25_idf(S, int(df[t])) for t in set(terms.tolist()) | set(should.tolist())}
    weights = []
    for ph in phrases:   # tantivy's phrase weight: the float32 sum in slot order
        w = idf[int(ph[0])]
        for t in ph[1:]:
            w = np.float32(w + idf[int(t)])
        weights.append(w)
    avgdl = float(np.float32(float(dl.sum()) / S))
    d_dl = torch.from_numpy(dl.astype(np.int32)).to(dev)
    d_poff = torch.from_numpy(np.arange(0, Q * L + 1, L, dtype=np.int64)).to(dev)
    d_pt = torch.from_numpy(terms).to(dev)
    d_pw = torch.from_numpy(np.array(weights, np.float32)).to(dev)
    d_loff = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    d_ldocs, d_ltfs = torch.zeros(n_bound + 1, dtype=torch.int32, device=dev), torch.zeros(n_bound + 1, dtype=torch.int32, device=dev)
    d_lcnt = torch.zeros(3, dtype=torch.int64, device=dev)
    # the clause search's slots: list q MUST under the phrase weight, the SHOULD term
    c_terms = np.stack([n_terms + np.arange(Q, dtype=np.int32), should], axis=1).reshape(-1)
    c_w = np.stack([np.array(weights, np.float32), np.array([idf[int(t)] for t in should], np.float32)], axis=1).reshape(-1)
    d_cqoff = torch.from_numpy(np.arange(0, 2 * Q + 1, 2, dtype=np.int64)).to(dev)
    d_cqt, d_cqw = torch.from_numpy(c_terms).to(dev), torch.from_numpy(c_w).to(dev)
    d_cqo = torch.from_numpy(np.tile(np.array([1, 0], np.uint8), Q)).to(dev)
    # the boolean yardstick's: the window's tokens as L MUST slots, the SHOULD term
    b_terms = np.concatenate([np.stack(phrases), should[:, None]], axis=1).reshape(-1).astype(np.int32)
    d_bqoff = torch.from_numpy(np.arange(0, Q * (L + 1) + 1, L + 1, dtype=np.int64)).to(dev)
    d_bqt = torch.from_numpy(b_terms).to(dev)
    d_bqw = torch.from_numpy(np.array([idf[int(t)] for t in b_terms], np.float32)).to(dev)
    d_bqo = torch.from_numpy(np.tile(np.array([1] * L + [0], np.uint8), Q)).to(dev)
    d_hd, d_hs, d_hf = (torch.zeros(Q * K, dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.int32))
    d_hc, d_mc, d_cnt = torch.zeros(Q, dtype=torch.int32, device=dev), torch.zeros(Q, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)

    def lists():
        batch.phrase_lists_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), d_first.data_ptr(), d_ppos.data_ptr(), n_terms, n_post, n_idx, 0, S,
                                    d_poff.data_ptr(), d_pt.data_ptr(), Q, Q * L, n_probes, d_loff.data_ptr(), d_ldocs.data_ptr(), d_ltfs.data_ptr(), n_bound,
                                    d_lcnt.data_ptr(), stream)

    def clause():
        batch.clause_search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), n_terms, n_post, d_loff.data_ptr(), d_ldocs.data_ptr(),
                                     d_ltfs.data_ptr(), Q, n_bound, 0, S, d_dl.data_ptr(), d_cqoff.data_ptr(), d_cqt.data_ptr(), d_cqw.data_ptr(),
                                     d_cqo.data_ptr(), Q, 2 * Q, 1.2, 0.75, avgdl, K, n_bound, d_hd.data_ptr(), d_hs.data_ptr(), d_hc.data_ptr(),
                                     d_mc.data_ptr(), d_cnt.data_ptr(), stream)

    def chained():
        lists()
        clause()

    def boolean():
        batch.boolean_search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), n_terms, n_post, 0, S, d_dl.data_ptr(), d_bqoff.data_ptr(),
                                      d_bqt.data_ptr(), d_bqw.data_ptr(), d_bqo.data_ptr(), Q, Q * (L + 1), 1.2, 0.75, avgdl, K, n_bound, d_hd.data_ptr(),
                                      d_hs.data_ptr(), d_hc.data_ptr(), d_mc.data_ptr(), d_cnt.data_ptr(), stream)

    def phrase():
        batch.phrase_search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), d_first.data_ptr(), d_ppos.data_ptr(), n_terms, n_post, n_idx,
                                     0, S, d_dl.data_ptr(), d_poff.data_ptr(), d_pt.data_ptr(), d_pw.data_ptr(), Q, Q * L, 1.2, 0.75, avgdl, K, n_probes,
                                     d_hd.data_ptr(), d_hs.data_ptr(), d_hf.data_ptr(), d_hc.data_ptr(), d_mc.data_ptr(), d_cnt.data_ptr(), stream)
    out = {"spec": spec, "queries": Q, "phrase_terms": L, "k": K, "n_terms": n_terms, "documents": S, "postings": n_post, "positions": n_idx,
           "list_bound": n_bound}
    boolean()
    batch.sync()
    cnt = d_cnt.cpu().numpy()
    out.update({"boolean_places": int(cnt[0]), "boolean_matches": int(cnt[1])})
    phrase()
    batch.sync()
    cnt = d_cnt.cpu().numpy()
    phrase_mc = d_mc.clone()
    out.update({"probes": int(cnt[0]), "phrase_matches": int(cnt[1])})
    chained()
    batch.sync()
    lcnt, cnt = d_lcnt.cpu().numpy(), d_cnt.cpu().numpy()
    out.update({"list_entries": int(lcnt[1]), "lists_probes_equal_phrase_search": bool(int(lcnt[0]) == out["probes"]),
                "list_entries_equal_phrase_matches": bool(int(lcnt[1]) == out["phrase_matches"]), "places": int(cnt[0]), "matches": int(cnt[1]),
                "places_equal_list_entries": bool(int(cnt[0]) == int(lcnt[1])),   # (every query is anchored on its list: its only MUST slot)
                "match_counts_equal_phrase_search": bool(torch.equal(d_mc, phrase_mc)), "every_query_matches": bool(int(d_mc.min().item()) >= 1),
                "hit_counts_sum": int(d_hc.to(torch.int64).sum().item())})
    for name, fn in (("lists", lists), ("clause", clause), ("chained", chained), ("boolean", boolean), ("phrase", phrase)):
        fn()
        batch.sync()
        r = []
        for _ in range(args.rounds):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for a, b in ev:
                a.record(); fn(); b.record()
            torch.cuda.synchronize()
            r.append(med([a.elapsed_time(b) for a, b in ev]))
        batch.sync()
        out[name + "_ms"] = round(med(r), 4)
        out[name + "_rounds_ms"] = [round(x, 4) for x in r]
    out["lists_over_phrase"] = round(out["lists_ms"] / out["phrase_ms"], 3)
    out["clause_over_boolean"] = round(out["clause_ms"] / out["boolean_ms"], 3)
    out["chained_over_boolean"] = round(out["chained_ms"] / out["boolean_ms"], 3)
    out["chained_over_lists_plus_clause"] = round(out["chained_ms"] / (out["lists_ms"] + out["clause_ms"]), 3)
    out["places_per_s"] = round(out["places"] / out["clause_ms"] * 1e3, 1)
    return out


def boolean_rows(torch, batch, stream, dev, args, spec, S, n_terms, dev_off, host_ids, d_term, d_pdocs, d_ptfs, n_post):
    """--boolean Q,L,K over the one-pass segment; see the module's docstring"""
    from vaporetto_amd import api
    Q, L, K = (int(x) for x in spec.split(","))
    term = d_term.cpu().numpy().astype(np.int64)
    df = np.diff(term)
    tfs = d_ptfs[:n_post].cpu().numpy().astype(np.int64)
    count = np.add.reduceat(np.concatenate([tfs, [0]]), np.minimum(term[:-1], n_post)) * (df > 0)
    toff = dev_off.astype(np.int64)
    dl = np.diff(toff)
    rng = np.random.default_rng(7)
    while True:   # (a), (c): the terms --search draws
        drawn = rng.choice(n_terms, size=Q * L, p=count / count.sum()).astype(np.int32)
        if int(df[drawn].sum()) <= args.search_max_candidates or Q == 1:
            break
        Q //= 2
    known = (host_ids >= 0) & (host_ids < n_terms)
    run = np.concatenate([[0], np.cumsum(~known)])   # a window [a, a + L) is all known when run[a + L] == run[a]
    long_docs = np.flatnonzero(dl >= L)
    windows = []
    for _ in range(64 * Q):   # (b): the windows --phrase draws
        if len(windows) == Q or len(long_docs) == 0:
            break
        d = int(long_docs[rng.integers(len(long_docs))])
        a = int(toff[d]) + int(rng.integers(int(dl[d]) - L + 1))
        if run[a + L] == run[a]:
            windows.append(host_ids[a:a + L].astype(np.int32))
    while windows and int(df[np.concatenate(windows)].sum()) > args.search_max_candidates and len(windows) > 1:
        windows = windows[:len(windows) // 2]
    avgdl = float(np.float32(float(dl.sum()) / S))
    d_dl = torch.from_numpy(dl.astype(np.int32)).to(dev)
    rows = []
    settings = [("a_must_by_count", drawn, Q, 1), ("c_should_by_count", drawn, Q, 0)]
    if windows:
        settings.insert(1, ("b_must_windows", np.concatenate(windows), len(windows), 1))
    for name, terms, n_q, occur in settings:
        n_cand = int(df[terms].sum())
        per_q = df[terms].reshape(n_q, L)
        n_places = int(per_q.min(axis=1).sum()) if occur else n_cand
        if max(n_cand, n_places) >= 1 << 32:
            raise SystemExit("--boolean: %d candidates" % n_cand)
        idf = {int(t): float(api.bm25_idf(S, int(df[t]))) for t in set(terms.tolist())}
        d_qoff = torch.from_numpy(np.arange(0, n_q * L + 1, L, dtype=np.int64)).to(dev)
        d_qt = torch.from_numpy(terms).to(dev)
        d_qw = torch.from_numpy(np.array([idf[int(t)] for t in terms], np.float32)).to(dev)
        d_qo = torch.full((n_q * L,), occur, dtype=torch.uint8, device=dev)
        d_hd, d_hs = torch.zeros(n_q * K, dtype=torch.int32, device=dev), torch.zeros(n_q * K, dtype=torch.float32, device=dev)
        d_hc, d_mc, d_cnt = torch.zeros(n_q, dtype=torch.int32, device=dev), torch.zeros(n_q, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)

        def boolean():
            batch.boolean_search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), n_terms, n_post, 0, S, d_dl.data_ptr(), d_qoff.data_ptr(),
                                          d_qt.data_ptr(), d_qw.data_ptr(), d_qo.data_ptr(), n_q, n_q * L, 1.2, 0.75, avgdl, K, n_places, d_hd.data_ptr(),
                                          d_hs.data_ptr(), d_hc.data_ptr(), d_mc.data_ptr(), d_cnt.data_ptr(), stream)

        def or_search():
            batch.search_postings(d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), n_terms, n_post, 0, S, d_dl.data_ptr(), d_qoff.data_ptr(), d_qt.data_ptr(),
                                  d_qw.data_ptr(), n_q, n_q * L, 1.2, 0.75, avgdl, K, n_cand, d_hd.data_ptr(), d_hs.data_ptr(), d_hc.data_ptr(), d_mc.data_ptr(),
                                  d_cnt.data_ptr(), stream)
        out = {"setting": name, "spec": spec, "queries": n_q, "slots_per_query": L, "k": K, "n_terms": n_terms, "documents": S, "postings": n_post}
        or_search()
        batch.sync()
        cnt = d_cnt.cpu().numpy()
        or_hits = (d_hd.clone(), d_hs.clone(), d_hc.clone(), d_mc.clone())
        out.update({"or_candidates": int(cnt[0]), "or_matches": int(cnt[1])})
        boolean()
        batch.sync()
        cnt = d_cnt.cpu().numpy()
        matches = int(cnt[1])
        out.update({"places": int(cnt[0]), "matches": matches, "skipped": int(cnt[2]), "places_equal_host_count": bool(int(cnt[0]) == n_places),
                    "places_over_candidates": round(int(cnt[0]) / max(n_cand, 1), 5), "hit_counts_sum": int(d_hc.to(torch.int64).sum().item())})
        if name == "b_must_windows":
            out["every_query_matches"] = bool(int(d_mc.min().item()) >= 1)
        if occur == 0:   # all SHOULD: the OR search's bytes
            out["equals_or_search"] = bool(all(torch.equal(x, y) for x, y in zip(or_hits, (d_hd, d_hs, d_hc, d_mc))))
        copy_bytes = (8 * int(cnt[0]) + 8 * matches) // 2
        a_buf, b_buf = torch.empty(copy_bytes + 8, dtype=torch.uint8, device=dev), torch.empty(copy_bytes + 8, dtype=torch.uint8, device=dev)
        out["copy_bytes"] = copy_bytes

        def floor():
            b_buf.copy_(a_buf)
        for fname, fn in (("boolean", boolean), ("or_search", or_search), ("floor", floor)):
            fn()
            batch.sync()
            r = []
            for _ in range(args.rounds):
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                for a, b in ev:
                    a.record(); fn(); b.record()
                torch.cuda.synchronize()
                r.append(med([a.elapsed_time(b) for a, b in ev]))
            batch.sync()
            out[fname + "_ms"] = round(med(r), 4)
            out[fname + "_rounds_ms"] = [round(x, 4) for x in r]
        out["places_per_s"] = round(int(cnt[0]) / out["boolean_ms"] * 1e3, 1)
        out["boolean_over_or_search"] = round(out["boolean_ms"] / out["or_search_ms"], 3)
        out["boolean_over_floor"] = round(out["boolean_ms"] / out["floor_ms"], 2)
        rows.append(out)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,5")
    ap.add_argument("--sentences", type=int, default=0, help="sentences of configs[2]'s batch (0: all of it)")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parity-docs", type=int, default=2000)
    ap.add_argument("--wsconst", default="")
    ap.add_argument("--ids", action="store_true", help="also time the vocabulary id pass and vpt_token_stream_ids_batch")
    ap.add_argument("--vocab-docs", type=int, default=20000)
    ap.add_argument("--count", action="store_true", help="also time the vocabulary counter's count call (three launches) and finish once")
    ap.add_argument("--postings", action="store_true", help="also time the postings pass over the id pass's ids (needs --ids)")
    ap.add_argument("--merge", default="", help="with --postings: K[,K..] equal document ranges as segments, then the ordered and the general merge")
    ap.add_argument("--search", action="append", default=[], help="with --postings: Q,L,K -- Q queries of L terms by count, top K (may be repeated)")
    ap.add_argument("--phrase", action="append", default=[], help="with --postings: Q,L,K -- Q phrases of L consecutive tokens of random documents, top K (may be repeated)")
    ap.add_argument("--boolean", action="append", default=[], help="with --postings: Q,L,K -- Q all-MUST queries of L terms by count, Q all-MUST windows of L tokens, the first as all-SHOULD (may be repeated)")
    ap.add_argument("--search-max-candidates", type=int, default=1 << 26)
    ap.add_argument("--count-keys", type=int, default=1 << 24, help="max_keys of the counter of --count")
    ap.add_argument("--sloppy", action="append", default=[], help="with --postings: Q,L,S,K -- the phrases of --phrase Q,L,K as the exact search, the sloppy search with every slop 0 and the sloppy search at slop S, top K (may be repeated)")
    ap.add_argument("--clause", action="append", default=[], help="with --postings: Q,L,K -- Q all-MUST queries, each a window of L tokens as ONE phrase clause plus one SHOULD term by count, top K (may be repeated)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tests import tokenref
    from vaporetto_amd import _lib, api
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    ncores = min(os.cpu_count() or 1, 16)
    stream = torch.cuda.current_stream().cuda_stream
    L = _lib.load()
    rows = []
    for cid in [int(c) for c in args.configs.split(",")]:
        cfg = bench.CONFIGS[cid]
        raw, name = bench.load_model_bytes(cfg["kind"], 1.0)
        utf8, boff, ooff, _, S = bench.make_shard(cfg, raw, 0, 1, ncores, args.sentences if cid == 2 else 0)
        S = len(boff) - 1
        nb, nbytes = int(ooff[-1]), int(boff[-1])
        pred = api.Predictor(api.Model.read_slice(raw)[0], False, device=0)
        ws_flags = api.wsconst_flags(args.wsconst)
        flags = _lib.VPT_FLAG_KYTEA_FULLWIDTH | _lib.VPT_FLAG_SPLIT_LINEBREAKS | _lib.VPT_FLAG_LINEBREAKS_FIRST | ws_flags
        row = {"workload": cfg["name"], "model": name, "documents": S, "text_bytes": nbytes, "chars": nb + S, "wsconst": args.wsconst, "steps": args.steps}
        # ---- (a) the kernels, alternating
        d_text = torch.from_numpy(np.concatenate([utf8, np.zeros(64, np.uint8)])).to(dev)
        d_boff = torch.from_numpy(boff.astype(np.int64)).to(dev)
        d_ooff = torch.from_numpy(ooff.astype(np.int64)).to(dev)
        max_bytes = int(np.max(np.diff(boff.astype(np.int64))))
        batch = api.DeviceBatch(pred)
        batch.set_flags(flags)
        d_labels = torch.empty(nb + 16, dtype=torch.uint8, device=dev)
        batch.predict(d_text.data_ptr(), d_boff.data_ptr(), d_ooff.data_ptr(), S, nb, max_bytes, 0, d_labels.data_ptr(), stream)
        batch.sync()
        cap_text, cap_ends = 3 * nbytes + 64, nb + S
        d_out = torch.empty(cap_text + 1, dtype=torch.uint8, device=dev)
        d_toff = torch.empty(S + 1, dtype=torch.int64, device=dev)
        d_ends = torch.empty(cap_ends + 1, dtype=torch.int32, device=dev)
        d_soff = torch.empty(S + 1, dtype=torch.int64, device=dev)

        def emit():
            batch.write_tokenized(d_text.data_ptr(), d_boff.data_ptr(), d_ooff.data_ptr(), S, nb, d_labels.data_ptr(), d_out.data_ptr(), cap_text, d_toff.data_ptr(), stream)

        def spans():
            batch.token_spans(d_text.data_ptr(), d_boff.data_ptr(), d_ooff.data_ptr(), S, nb, d_labels.data_ptr(), d_soff.data_ptr(), d_ends.data_ptr(), cap_ends, stream)
        for _ in range(3):
            emit(); spans()
        batch.sync()
        per_round = {"emit": [], "spans": []}
        for _ in range(args.rounds):
            for which, fn in (("emit", emit), ("spans", spans)):
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                for a, b in ev:
                    a.record(); fn(); b.record()
                torch.cuda.synchronize()
                per_round[which].append(med([a.elapsed_time(b) for a, b in ev]))
        batch.sync()
        n_tokens = int(d_soff[-1].item())
        out_text = int(d_toff[-1].item())
        k = {}
        for which in ("emit", "spans"):
            r = per_round[which]
            k[which + "_ms"] = round(med(r), 4)
            k[which + "_rounds_ms"] = [round(x, 4) for x in r]
            k[which + "_spread"] = round((max(r) - min(r)) / min(r), 4)
        k["spans_over_emit"] = round(k["spans_ms"] / k["emit_ms"], 3)
        k["emit_bytes_moved"] = nbytes + nb + out_text + 24 * S
        k["spans_bytes_moved"] = nbytes + 2 * nb + 4 * n_tokens + 24 * S     # (the labels twice: the size pass and the pieces)
        k["spans_frac_of_hbm"] = round(k["spans_bytes_moved"] / k["spans_ms"] / 1e6 / bench.HBM_PEAK_GBS, 4)
        k["emit_frac_of_hbm"] = round(k["emit_bytes_moved"] / k["emit_ms"] / 1e6 / bench.HBM_PEAK_GBS, 4)
        row["kernels"] = k
        dev_off = d_soff.cpu().numpy().astype(np.uint64)
        dev_ends = d_ends[:n_tokens].cpu().numpy().view(np.uint32)
        vocab = dev_ids = None
        if args.ids:
            surf = set()
            for i in range(min(S, args.vocab_docs)):
                doc, a = bytes(utf8[int(boff[i]):int(boff[i + 1])]), 0
                for t in range(int(dev_off[i]), int(dev_off[i + 1])):
                    surf.add(doc[a:int(dev_ends[t])])
                    a = int(dev_ends[t])
            keys = sorted(surf)[::2]
            vocab = api.Vocabulary(pred, keys)
            d_ids = torch.empty(cap_ends + 1, dtype=torch.int32, device=dev)

            def ids():
                batch.token_ids(vocab, d_text.data_ptr(), d_boff.data_ptr(), S, d_soff.data_ptr(), 0, d_ends.data_ptr(), cap_ends, d_ids.data_ptr(), 0, stream)
            for _ in range(3):
                ids()
            batch.sync()
            r = []
            for _ in range(args.rounds):
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                for a, b in ev:
                    a.record(); ids(); b.record()
                torch.cuda.synchronize()
                r.append(med([a.elapsed_time(b) for a, b in ev]))
            batch.sync()
            dev_ids = d_ids[:n_tokens].cpu().numpy()
            row["ids"] = {"vocab_keys": len(keys), "vocab": vocab.info(), "ids_ms": round(med(r), 4), "ids_rounds_ms": [round(x, 4) for x in r],
                          "ids_spread": round((max(r) - min(r)) / min(r), 4), "ids_ms_per_100k_docs": round(med(r) * 1e5 / S, 4),
                          "known_share": round(float(np.mean(dev_ids != vocab.unk_id)), 4), "ids_over_spans": round(med(r) / k["spans_ms"], 3)}
            if not args.postings:
                del d_ids
        if args.postings:   # the postings pass over the ids the id pass left, beside that id pass (the same run)
            if not args.ids:
                raise SystemExit("--postings needs --ids (the ids it groups, and the yardstick)")
            n_terms = len(keys)
            d_term = torch.empty(n_terms + 1, dtype=torch.int64, device=dev)
            d_pdocs, d_ptfs = torch.empty(cap_ends + 1, dtype=torch.int32, device=dev), torch.empty(cap_ends + 1, dtype=torch.int32, device=dev)
            d_cnt = torch.zeros(2, dtype=torch.int64, device=dev)

            def postings():
                batch.postings(d_soff.data_ptr(), S, d_ids.data_ptr(), cap_ends, n_terms, 0, d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), cap_ends,
                               0, 0, d_cnt.data_ptr(), stream)
            for _ in range(2):
                postings()
            batch.sync()
            r = []
            for _ in range(args.rounds):
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                for a, b in ev:
                    a.record(); postings(); b.record()
                torch.cuda.synchronize()
                r.append(med([a.elapsed_time(b) for a, b in ev]))
            batch.sync()
            cnt = d_cnt.cpu().numpy()
            term = d_term.cpu().numpy()
            tf_sum = int(d_ptfs[:int(cnt[0])].to(torch.int64).sum().item())
            row["postings"] = {"n_terms": n_terms, "postings": int(cnt[0]), "dropped": int(cnt[1]), "sort_passes": (n_terms.bit_length() + 7) // 8,
                               "postings_ms": round(med(r), 4), "postings_rounds_ms": [round(x, 4) for x in r],
                               "postings_spread": round((max(r) - min(r)) / min(r), 4), "postings_ms_per_100k_docs": round(med(r) * 1e5 / S, 4),
                               "postings_over_ids": round(med(r) / row["ids"]["ids_ms"], 3),
                               "tfs_plus_dropped_equal_tokens": bool(tf_sum + int(cnt[1]) == n_tokens),
                               "term_offsets_end_equal_postings": bool(int(term[n_terms]) == int(cnt[0]) and int(term[0]) == 0)}
            if args.merge:   # K equal document ranges as segments, then the two merges, beside the one-pass call above
                row["merge"] = [merge_rows(torch, batch, stream, dev, args, int(K), S, n_terms, dev_off, d_soff, d_ids, d_term, d_pdocs, d_ptfs,
                                           int(cnt[0]), row["postings"]["postings_ms"]) for K in args.merge.split(",")]
            if args.search:   # BM25 top-k over the segment the one-pass call left, beside the general merge and a copy
                row["search"] = [search_rows(torch, batch, stream, dev, args, spec, S, n_terms, dev_off, d_term, d_pdocs, d_ptfs, int(cnt[0]))
                                 for spec in args.search]
            if args.boolean:   # MUST / SHOULD / MUST_NOT slots over the same segment, beside the OR search over the same slots and a copy
                row["boolean"] = [boolean_rows(torch, batch, stream, dev, args, spec, S, n_terms, dev_off, dev_ids, d_term, d_pdocs, d_ptfs, int(cnt[0]))
                                  for spec in args.boolean]
            if args.phrase or args.clause or args.sloppy:   # exact phrases over the same segment with its position lists, beside the OR search and a copy
                n_post = int(cnt[0])
                d_first, d_order = torch.empty(cap_ends + 2, dtype=torch.int64, device=dev), torch.empty(cap_ends + 1, dtype=torch.int32, device=dev)
                d_ppos = torch.empty(cap_ends + 1, dtype=torch.int32, device=dev)
                batch.postings(d_soff.data_ptr(), S, d_ids.data_ptr(), cap_ends, n_terms, 0, d_term.data_ptr(), d_pdocs.data_ptr(), d_ptfs.data_ptr(), cap_ends,
                               d_first.data_ptr(), d_order.data_ptr(), d_cnt.data_ptr(), stream)

                def positions():
                    batch.postings_positions(d_soff.data_ptr(), S, cap_ends, 0, d_term.data_ptr(), n_terms, d_first.data_ptr(), cap_ends, d_order.data_ptr(),
                                             d_ppos.data_ptr(), stream)
                positions()
                batch.sync()
                r = []
                for _ in range(args.rounds):
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                    for a, b in ev:
                        a.record(); positions(); b.record()
                    torch.cuda.synchronize()
                    r.append(med([a.elapsed_time(b) for a, b in ev]))
                batch.sync()
                n_idx = int(d_first[n_post].item())
                row["positions"] = {"indexed_tokens": n_idx, "positions_ms": round(med(r), 4), "positions_rounds_ms": [round(x, 4) for x in r],
                                    "positions_over_postings": round(med(r) / row["postings"]["postings_ms"], 3),
                                    "indexed_plus_dropped_equal_tokens": bool(n_idx + int(cnt[1]) == n_tokens)}
                row["phrase"] = [phrase_rows(torch, batch, stream, dev, args, spec, S, n_terms, dev_off, dev_ids, d_soff, d_ids, cap_ends, d_term, d_pdocs,
                                             d_ptfs, n_post, (d_first, d_ppos, n_idx)) for spec in args.phrase]
                if args.sloppy:   # a slop budget per phrase over the same phrases, beside the exact search
                    row["sloppy"] = [phrase_rows(torch, batch, stream, dev, args, spec, S, n_terms, dev_off, dev_ids, d_soff, d_ids, cap_ends, d_term,
                                                 d_pdocs, d_ptfs, n_post, (d_first, d_ppos, n_idx), sloppy=True) for spec in args.sloppy]
                if args.clause:   # phrase clauses in boolean queries, beside the boolean search over the tokens as slots and the phrase search
                    row["clause"] = [clause_rows(torch, batch, stream, dev, args, spec, S, n_terms, dev_off, dev_ids, d_term, d_pdocs, d_ptfs, n_post,
                                                 (d_first, d_ppos, n_idx)) for spec in args.clause]
                del d_first, d_order, d_ppos
            del d_ids, d_term, d_pdocs, d_ptfs, d_cnt
        if args.count:   # the counter's three launches on the same CSR, beside the id pass of the same run
            counter = api.VocabularyCounter(pred, args.count_keys)

            def count():
                batch.count_tokens(counter, d_text.data_ptr(), d_boff.data_ptr(), S, d_soff.data_ptr(), 0, d_ends.data_ptr(), cap_ends, 0, stream)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); count(); b.record()   # the first call: every surface is inserted and committed
            torch.cuda.synchronize()
            try:
                batch.sync()
            except api.VaporettoError as e:   # more distinct surfaces than --count-keys: nothing below would measure counting
                raise SystemExit("--count: %s (distinct surfaces exceed --count-keys %d)" % (e, args.count_keys))
            first_ms = a.elapsed_time(b)
            r = []
            for _ in range(args.rounds):   # the calls behind it: every surface is a committed key
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                for a, b in ev:
                    a.record(); count(); b.record()
                torch.cuda.synchronize()
                r.append(med([a.elapsed_time(b) for a, b in ev]))
            batch.sync()
            t0 = time.perf_counter()
            surfaces, counts = counter.finish()
            finish_ms = (time.perf_counter() - t0) * 1e3
            info = counter.info()
            calls = 1 + args.rounds * args.steps
            row["count"] = {"counter": info, "first_call_ms": round(first_ms, 4), "count_ms": round(med(r), 4), "count_rounds_ms": [round(x, 4) for x in r],
                            "count_spread": round((max(r) - min(r)) / min(r), 4), "count_ms_per_100k_docs": round(med(r) * 1e5 / S, 4),
                            "finish_wall_ms": round(finish_ms, 3), "distinct": len(surfaces), "top": [[s, int(c) // calls] for s, c in zip(surfaces[:5], counts[:5])],
                            "top_share": round(float(counts[0]) / max(float(counts.sum()), 1.0), 4) if len(counts) else 0.0,
                            "tokens_equal_counted_plus_skipped": bool((info["n_counted"] + info["n_skipped"]) == calls * n_tokens)}
            if args.ids:
                row["count"]["count_over_ids"] = round(med(r) / row["ids"]["ids_ms"], 3)
            del counter
        del d_out, d_toff, d_ends, d_soff, d_labels, d_text, batch
        # ---- (b) end to end, pinned buffers
        p_text = api.PinnedArray(nbytes, np.uint8); p_text.array[:] = utf8
        p_boff = api.PinnedArray(S + 1, np.uint64); p_boff.array[:] = boff
        p_ends = api.PinnedArray(max(nbytes, 1), np.uint32)
        p_toff = api.PinnedArray(S + 1, np.uint64)
        p_lab = api.PinnedArray(nb + 1, np.uint8)
        p_tok = api.PinnedArray(3 * nbytes + 64, np.uint8)
        p_tokoff = api.PinnedArray(S + 1, np.uint64)
        u, bo = p_text.array, p_boff.array

        def route_stream():
            return pred.token_stream_packed(u, bo, args.wsconst, ends_out=p_ends.array, offsets_out=p_toff.array)

        def route_labels_device():
            st = L.vpt_predict_batch_flags(pred.handle, u.ctypes.data, bo.ctypes.data, S, None, p_lab.array.ctypes.data, ooff.ctypes.data, flags)
            assert st == 0, _lib.last_error()

        def route_text_device():
            return pred.tokenize_packed(u, bo, flags=_lib.VPT_FLAG_KYTEA_FULLWIDTH | ws_flags, text_out=p_tok.array, offsets_out=p_tokoff.array)

        def timed(fn, n):
            fn()
            ts = []
            for _ in range(n):
                t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
            return ts
        e = {}
        t_stream = timed(route_stream, args.steps)
        s_off, s_ends = route_stream()
        s_off, s_ends = s_off.copy(), s_ends.copy()
        t_lab_dev = timed(route_labels_device, args.steps)
        host_n = max(3, min(args.steps, 5))
        t_lab_host = timed(lambda: csr_from_labels(u, bo, ooff, p_lab.array), host_n)
        l_off, l_ends = csr_from_labels(u, bo, ooff, p_lab.array)
        t_txt_dev = timed(route_text_device, args.steps)
        text, toff_text = route_text_device()
        t_txt_host = timed(lambda: csr_from_tokenized(text, toff_text, S), host_n)
        x_off, x_ends = csr_from_tokenized(text, toff_text, S)
        e["stream_ms"] = round(med(t_stream), 3)
        e["labels_route_ms"] = round(med(t_lab_dev) + med(t_lab_host), 3)
        e["labels_route_device_ms"], e["labels_route_host_ms"] = round(med(t_lab_dev), 3), round(med(t_lab_host), 3)
        e["text_route_ms"] = round(med(t_txt_dev) + med(t_txt_host), 3)
        e["text_route_device_ms"], e["text_route_host_ms"] = round(med(t_txt_dev), 3), round(med(t_txt_host), 3)
        e["host_scan"] = "numpy, one thread: the conversion a caller of the older routes runs after the call returns"
        if args.ids:
            t_ids = timed(lambda: pred.token_ids_packed(u, bo, vocab, args.wsconst, False), args.steps)
            i_out = pred.token_ids_packed(u, bo, vocab, args.wsconst, False)
            e["ids_stream_ms"] = round(med(t_ids), 3)
            e["ids_stream_over_stream"] = round(med(t_ids) / med(t_stream), 3)
            row["ids"]["stream_ids_equal_device_call"] = bool(np.array_equal(i_out[0], s_off) and np.array_equal(i_out[2], s_ends) and np.array_equal(i_out[5], dev_ids))
        row["end_to_end"] = e
        # ---- (c) PCIe bytes
        row["pcie"] = {"stream": {"h2d": nbytes + 8 * (S + 1), "d2h": 8 * (S + 1) + 4 * len(s_ends)},
                       "labels_route": {"h2d": nbytes + 16 * (S + 1), "d2h": nb},
                       "text_route": {"h2d": nbytes + 8 * (S + 1), "d2h": int(toff_text[-1]) + 8 * (S + 1)},
                       "note": "4 bytes a token is MORE device-to-host than 1 byte a label when tokens are shorter than four chars (mean chars per token here: %.2f)" % ((nb + S) / max(len(s_ends), 1))}
        # ---- parity
        par = {"stream_equals_device_call": bool(np.array_equal(s_off, dev_off) and np.array_equal(s_ends, dev_ends)),
               "stream_equals_labels_route": bool(np.array_equal(s_off, l_off) and np.array_equal(s_ends, l_ends)),
               "stream_equals_text_route": bool(np.array_equal(s_off, x_off) and np.array_equal(s_ends, x_ends))}
        n_par = min(args.parity_docs, S)
        texts = [bytes(utf8[int(boff[i]):int(boff[i + 1])]).decode("utf-8") for i in range(n_par)]
        w_off, w_ends = tokenref.csr(tokenref.ends_batch(raw, texts, args.wsconst))
        par["tokenref_docs"] = n_par
        par["stream_equals_tokenref"] = bool(np.array_equal(s_off[:n_par + 1], w_off) and np.array_equal(s_ends[:int(w_off[-1])], w_ends))
        row["parity"] = par
        row["tokens"] = int(len(s_ends))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del p_text, p_boff, p_ends, p_toff, p_lab, p_tok, p_tokoff, pred
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"tool": "tools/token_stream_bench.py", "args": vars(args), "rows": rows}, fh, indent=1)
    if not all(all(v for kk, v in r["parity"].items() if kk != "tokenref_docs") for r in rows):
        raise SystemExit("parity FAILED")
    if args.ids and not all(r["ids"]["stream_ids_equal_device_call"] for r in rows):
        raise SystemExit("ids parity FAILED")


if __name__ == "__main__":
    main()
