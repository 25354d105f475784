"""Query expansion against the plain search beside it: what the second search and the step in between cost.

    python tools/ab_expand.py [--docs 1000000] [--text-docs 100000] [--queries 1024] [--k 10] [--reps 5] [--out FILE]

Three things, each plain and expanded (``ExpandedIndex`` with the default ``QueryExpansion``), device events around the
call, median of ``--reps`` after a warm-up of the same shapes:

* dense: ``FAISSIndexBuilder.search_device`` over ``--docs`` random unit rows, at nq = 1 and nq = ``--queries``;
* BM25: ``BM25Index.search_device`` over ``--text-docs`` synthetic Zipf texts (``--vocab`` words, 1 - 30 tokens per
  document, 6-token queries), nq = ``--queries`` (tokenising and uploading the query CSR included: host work inside
  the device-event window, as in ``ab_hybrid.py``);
* hybrid: ``HybridIndex.search_device`` (rrf) over ``--text-docs`` rows of both kinds.

The yardstick is the plain call on the same box: an expanded search is two searches plus one small kernel, so every
stage reports ``expanded / (2 x plain)``.  The two new C-ABI calls are also timed alone on the stage's own rankings
(``rocchio_ms``, ``rm3_ms``), and the first search alone at ``fb_docs`` (it is not the plain search: k is smaller).

``--profile`` runs only the expanded legs three times: the target of

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/ab_expand.py --profile

whose ``*_kernel_stats.csv`` holds the two kernels' own time (``prf_rocchio_kernel``, ``prf_rm3_kernel``).

Prints one JSON object per stage (so a run that is cut short leaves what it measured) and the summary last.
"""
import argparse
import dataclasses
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from ab_bm25 import zipf_texts  # noqa: E402
from semantic_search_kd_amd import BM25Index, ExpandedIndex, FAISSIndexBuilder, HybridIndex, QueryExpansion  # noqa: E402
from semantic_search_kd_amd.expand import rm3_device, rocchio_device  # noqa: E402


def device_ms(fn, reps):
    fn()   # warm-up at the timed shape
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(times), 3), "range_ms": [round(min(times), 3), round(max(times), 3)]}


def unit_rows(n, gen, dev):
    x = torch.randn((n, 384), generator=gen, device=dev)
    x /= x.norm(dim=1, keepdim=True)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--text-docs", type=int, default=100_000)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    dev = torch.device("cuda:0")
    x = QueryExpansion()
    k, nq = args.k, args.queries
    gen = torch.Generator(device=dev).manual_seed(7)
    rng = np.random.default_rng(2025)
    t0 = time.perf_counter()
    dense = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    dense.build_from_embeddings(unit_rows(args.docs, gen, dev))
    emb = unit_rows(nq, gen, dev)
    texts = zipf_texts(args.text_docs, args.vocab, rng, 1, 30)
    queries = zipf_texts(nq, args.vocab, rng, 6, 6)
    bm25 = BM25Index(device="cuda:0")
    bm25.build_from_texts(list(range(args.text_docs)), texts)
    del texts
    small = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    small.build_from_embeddings(unit_rows(args.text_docs, gen, dev))
    small.doc_ids = []
    hybrid = HybridIndex(small, bm25, depth=args.depth)
    t1 = time.perf_counter()
    fwd_entries = bm25.forward_tables()[3]
    emit({"stage": "setup", "device": torch.cuda.get_device_name(0), "docs": args.docs, "text_docs": args.text_docs,
          "queries": nq, "k": k, "expansion": dataclasses.asdict(x),
          "postings": int(len(bm25.bm25.post_rows)), "forward_entries": int(fwd_entries),
          "forward_index_build_upload_s": round(time.perf_counter() - t1, 2), "setup_s": round(t1 - t0, 1)})

    e_dense, e_bm25, e_hybrid = ExpandedIndex(dense, x), ExpandedIndex(bm25, x), ExpandedIndex(hybrid, x)
    if args.profile:
        for _ in range(3):
            e_dense.search_device(emb[:1], k)
            e_dense.search_device(emb, k)
            e_bm25.search_device(queries, k)
            e_hybrid.search_device(queries, emb, k)
        torch.cuda.synchronize()
        return

    summary = {"stage": "summary", "device": torch.cuda.get_device_name(0)}

    def stage(name, plain, expanded, extra):
        p, e = device_ms(plain, args.reps), device_ms(expanded, args.reps)
        row = {"stage": name, "plain": p, "expanded": e,
               "expanded_over_twice_plain": round(e["median_ms"] / (2 * p["median_ms"]), 3)}
        row.update({key: device_ms(fn, args.reps) for key, fn in extra.items()})
        emit(row)
        summary[name] = {"plain_ms": p["median_ms"], "expanded_ms": e["median_ms"],
                         "expanded_over_twice_plain": row["expanded_over_twice_plain"],
                         **{key: row[key]["median_ms"] for key in extra}}

    for n in sorted({1, nq}):
        q = emb[:n].contiguous()
        s, i = dense.search_device(q, x.fb_docs)
        stage(f"dense_nq{n}", lambda: dense.search_device(q, k), lambda: e_dense.search_device(q, k),
              {"first_search_ms": lambda: dense.search_device(q, x.fb_docs),
               "rocchio_ms": lambda: rocchio_device(dense, q, s, i, x)})

    lims, terms, lims_host = bm25.query_csr_host(queries)
    b, j = bm25._search_csr((lims, terms), nq, x.fb_docs)
    stage(f"bm25_nq{nq}", lambda: bm25.search_device(queries, k), lambda: e_bm25.search_device(queries, k),
          {"first_search_ms": lambda: bm25._search_csr((lims, terms), nq, x.fb_docs),
           "rm3_ms": lambda: rm3_device(bm25, (lims, terms), lims_host, b, j, x)})

    d = hybrid.clip_depth()
    b, j = bm25._search_csr((lims, terms), nq, d)
    s, i = small.search_device(emb, x.fb_docs)
    stage(f"hybrid_nq{nq}", lambda: hybrid.search_device(queries, emb, k), lambda: e_hybrid.search_device(queries, emb, k),
          {"rocchio_ms": lambda: rocchio_device(small, emb, s, i, x),
           "rm3_ms": lambda: rm3_device(bm25, (lims, terms), lims_host, b, j, x),
           "bm25_search_ms": lambda: bm25._search_csr((lims, terms), nq, d)})
    emit(summary)


if __name__ == "__main__":
    main()
