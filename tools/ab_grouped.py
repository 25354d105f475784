"""A/B of the grouped search against the row search it is built on, same process, alternating.

    python tools/ab_grouped.py [--rows 1000000] [--queries 10000] [--reps 7] [--out FILE]

Per case and round, each leg is timed with device events over `--iters` back-to-back calls after a warm-up; the median
of the rounds is reported with min / max.  The baseline of both cases is `search_device(q, 32)`: the exact row search
for 32 rows per query, the first step of the grouped call.  Cases:
  * singletons: no groups set (every row its own group), k = 10, k_rows = 32 - the grouped call should cost the
    baseline plus its collapse kernel;
  * runs3: documents of 3 consecutive rows, k = 10, the default k_rows ((k - 1) * 3 + 1 = 28: proved by counting), and
    k_rows = 10 to report the share of queries that are already proved when the best 10 rows are all there is.
The corpus rows of a document resemble each other (a document vector plus noise), so a query's best rows do cluster by
document.  Prints one JSON object.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import FAISSIndexBuilder  # noqa: E402


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(17)
    n_docs = -(-args.rows // 3)
    doc_of_row = torch.arange(args.rows, device=dev) // 3
    docs = torch.nn.functional.normalize(torch.randn(n_docs, 384, device=dev, generator=g), dim=1)
    corpus = docs[doc_of_row] + 0.5 * torch.nn.functional.normalize(torch.randn(args.rows, 384, device=dev, generator=g), dim=1)
    del docs
    corpus = torch.nn.functional.normalize(corpus, dim=1)
    queries = torch.nn.functional.normalize(torch.randn(args.queries, 384, device=dev, generator=g), dim=1)
    index = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    index.build_from_embeddings(corpus)
    del corpus

    def rows32():
        index.search_device(queries, 32, normalize_queries=False)

    def grouped(k, k_rows):
        return lambda: index.search_grouped_device(queries, k, k_rows=k_rows, normalize_queries=False)

    result = {"rows": args.rows, "queries": args.queries, "reps": args.reps, "iters": args.iters}

    def run(name, legs):
        times = {leg: [] for leg, _ in legs}
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for leg, fn in legs:
                times[leg].append(_time(fn, args.iters))
        out = {}
        for leg, ts in times.items():
            out[f"{leg}_ms"] = round(statistics.median(ts), 4)
            out[f"{leg}_range"] = [round(min(ts), 4), round(max(ts), 4)]
        for leg, _ in legs[1:]:
            out[f"{leg}_over_{legs[0][0]}"] = round(out[f"{leg}_ms"] / out[f"{legs[0][0]}_ms"], 4)
        return out

    # (a) every row its own group
    out = run("singletons", [("rows32", rows32), ("grouped_k10_rows32", grouped(10, 32))])
    _, ids, groups, unproved = index.search_grouped_device(queries, 10, k_rows=32, normalize_queries=False)
    rs, ri = index.search_device(queries, 10, normalize_queries=False)
    out["equals_search_k10"] = bool(torch.equal(ids, ri)) and bool(torch.equal(groups.long(), ri))
    out["unproved"] = int(unproved.sum().item())
    result["singletons"] = out
    print("singletons", out, flush=True)

    # (b) documents of 3 rows
    index.set_groups((torch.arange(args.rows) // 3).tolist())
    default_rows = index._default_k_rows(10)
    out = run("runs3", [("rows32", rows32), (f"grouped_k10_rows{default_rows}", grouped(10, default_rows)),
                        ("grouped_k10_rows10", grouped(10, 10))])
    for k_rows in (default_rows, 10):
        _, _, groups, unproved = index.search_grouped_device(queries, 10, k_rows=k_rows, normalize_queries=False)
        out[f"proved_share_rows{k_rows}"] = round(1.0 - float(unproved.sum().item()) / args.queries, 4)
    result["runs3"] = out
    print("runs3", out, flush=True)

    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
