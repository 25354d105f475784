"""A/B of the graph search against the exact search and the IVF search: same process, same corpus, same queries
(DESIGN section 20).

    python tools/ab_graph.py [--rows 1000000] [--degree 32] [--knn-k 64] [--ef 32 64 128] [--width 1 2 4 8]
                             [--batches 1 64 10000] [--nlist 1024] [--nprobe 8 32] [--reps 5] [--out FILE] [--csv FILE]

The corpus is `tools/ab_ivf.py`'s: clustered (`--topics` unit centres, rows = unit(centre + N(0, I) / sqrt(384))), every
query a noisy copy of a row (unit(row + 0.5 N(0, I) / sqrt(384))).  The build is timed in its two halves (the k-NN search
of the index against itself; pruning + reverse edges + merge).  For every batch size the exact side is
`flat.search_device`, the IVF side `IVFIndex.search_device` at every `--nprobe`, the graph side
`GraphIndex.search_device` for every (ef, width) with recall@10 against the exact ids, the mean number of iterations
and the share of queries that ran into `max_iterations` (= ef).  Every call is timed as a replayed graph of one call
(the device time alone; median of `--reps` rounds of `--iters` replays after a warm-up) and eagerly.  `--only-cell NQ EF
WIDTH` replays that one cell a few times and nothing else (for a kernel trace).  Prints one JSON object.
"""
import argparse
import csv
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import FAISSIndexBuilder, GraphIndex, IVFIndex  # noqa: E402
from semantic_search_kd_amd.ivf import recall_at_k  # noqa: E402


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _measure(fn, iters, reps):
    """(eager ms, graph-replay ms) of one call of fn: medians of `reps` rounds."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()   # sizes the workspaces
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = statistics.median(_events(fn, iters) for _ in range(reps))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    graph = statistics.median(_events(g.replay, iters) for _ in range(reps))
    return round(eager, 4), round(graph, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=4096)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--knn-k", type=int, default=None)
    ap.add_argument("--ef", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--width", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 10_000])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="*", default=[8, 32], help="none: no IVF side")
    ap.add_argument("--iterations", type=int, default=10, help="k-means iterations of the IVF side")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only-cell", type=int, nargs=3, default=None, metavar=("NQ", "EF", "WIDTH"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--csv", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(41)
    unit = torch.nn.functional.normalize
    centres = unit(torch.randn(args.topics, 384, device=dev, generator=g), dim=1)
    topic = torch.randint(0, args.topics, (args.rows,), device=dev, generator=g)
    corpus = unit(centres[topic] + torch.randn(args.rows, 384, device=dev, generator=g) / 384 ** 0.5, dim=1)
    nq_max = max(args.batches if args.only_cell is None else [args.only_cell[0]])
    picked = torch.randperm(args.rows, device=dev, generator=g)[:nq_max]
    queries = unit(corpus[picked] + 0.5 * torch.randn(nq_max, 384, device=dev, generator=g) / 384 ** 0.5, dim=1).contiguous()
    del centres, topic

    flat = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    flat.build_from_embeddings(corpus)
    del corpus
    # the build, step by step as GraphIndex.build_graph runs it, so that its two halves can be timed apart
    builder = GraphIndex(flat=flat, M=args.degree)
    knn_k = args.knn_k if args.knn_k is not None else 2 * args.degree
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    knn = builder.knn_device(knn_k)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    fwd = builder.prune_device(knn, args.degree)
    adjacency = builder.merge_device(fwd, builder.reverse_device(fwd))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    build = {"knn": t1 - t0, "prune_reverse_merge": t2 - t1}
    build_s = t2 - t0
    index = GraphIndex.from_graph(flat, adjacency.cpu().numpy())   # (+ the entry rows: the defaults)
    del knn, fwd, adjacency, builder
    degree = (index.graph >= 0).sum(dim=1).float()
    print(f"graph built in {build_s:.1f} s: {build}", file=sys.stderr, flush=True)

    if args.only_cell is not None:
        nq, ef, width = args.only_cell
        q = queries[:nq].contiguous()
        for _ in range(5):
            index.search_device(q, args.k, ef=ef, width=width, normalize_queries=False)
        torch.cuda.synchronize()
        print(json.dumps({"only_cell": args.only_cell, "rows": args.rows}))
        return

    ivf, train_s = None, None
    if args.nprobe:
        ivf = IVFIndex(flat=flat)
        t0 = time.perf_counter()
        ivf.train(nlist=args.nlist, iterations=args.iterations)
        torch.cuda.synchronize()
        train_s = round(time.perf_counter() - t0, 2)

    result = {
        "rows": args.rows, "k": args.k, "degree": index.M, "knn_k": knn_k, "n_entry": index.n_entry,
        "build_s": round(build_s, 2), "build_knn_s": round(build["knn"], 2),
        "build_prune_reverse_merge_s": round(build["prune_reverse_merge"], 3),
        "edges_per_row_min_mean": [int(degree.min().item()), round(float(degree.mean().item()), 2)],
        "ivf_nlist": None if ivf is None else ivf.nlist, "ivf_train_s": train_s,
        "device": torch.cuda.get_device_name(0), "runs": [],
    }
    rows_csv = []
    for nq in args.batches:
        q = queries[:nq].contiguous()
        exact = flat.search_device(q, args.k, normalize_queries=False)[1].cpu().numpy()
        iters = args.iters if nq <= 64 else 2
        row = {"nq": nq}
        row["flat_eager_ms"], row["flat_graph_ms"] = _measure(
            lambda: flat.search_device(q, args.k, normalize_queries=False), iters, args.reps)
        rows_csv.append({"nq": nq, "index": "flat", "graph_ms": row["flat_graph_ms"], "eager_ms": row["flat_eager_ms"],
                         "recall_at_k": 1.0})
        row["ivf"] = []
        for nprobe in (args.nprobe if ivf is not None else []):
            found = ivf.search_device(q, args.k, nprobe=nprobe, normalize_queries=False)[1].cpu().numpy()
            eager, graph = _measure(lambda: ivf.search_device(q, args.k, nprobe=nprobe, normalize_queries=False),
                                    iters, args.reps)
            cell = {"nprobe": nprobe, "eager_ms": eager, "graph_ms": graph, "recall_at_k": round(recall_at_k(found, exact), 4)}
            row["ivf"].append(cell)
            rows_csv.append({"nq": nq, "index": "ivf", **cell})
        row["graph"] = []
        for ef in args.ef:
            for width in args.width:
                def call(ef=ef, width=width):
                    return index.search_device(q, args.k, ef=ef, width=width, normalize_queries=False)
                _, found, its = index.search_device(q, args.k, ef=ef, width=width, normalize_queries=False,
                                                    return_iterations=True)
                its = its.cpu().numpy()
                eager, graph = _measure(call, iters, args.reps)
                cell = {"ef": ef, "width": width, "eager_ms": eager, "graph_ms": graph,
                        "recall_at_k": round(recall_at_k(found.cpu().numpy(), exact), 4),
                        "mean_iterations": round(float(its.mean()), 2),
                        "hit_max_iterations": round(float((its >= ef).mean()), 4),
                        "flat_graph_over_graph": round(row["flat_graph_ms"] / graph, 2)}
                row["graph"].append(cell)
                rows_csv.append({"nq": nq, "index": "graph", **cell})
        result["runs"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    if args.csv:
        Path(args.csv).parent.mkdir(parents=True, exist_ok=True)
        fields = ["nq", "index", "nprobe", "ef", "width", "graph_ms", "eager_ms", "recall_at_k", "mean_iterations",
                  "hit_max_iterations", "flat_graph_over_graph"]
        with open(args.csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=fields)
            w.writeheader()
            w.writerows(rows_csv)


if __name__ == "__main__":
    main()
