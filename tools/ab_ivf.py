"""A/B of the IVF and IVF-PQ searches against the exact search: same process, same corpus, same queries (DESIGN
sections 18 and 19).

    python tools/ab_ivf.py [--rows 1000000] [--nlist 1024] [--nprobe 1 8 32 128] [--batches 1 64 10000]
                           [--iterations 10] [--reps 5] [--pq-m 64] [--pq-refine 100] [--pq-iterations 10] [--out FILE]

The corpus is clustered (`--topics` unit centres, rows = unit(centre + N(0, I) / sqrt(384))) and every query is a noisy
copy of a row (unit(row + 0.5 N(0, I) / sqrt(384))), so a probe of a few lists can find a query's neighbours at all; on
rows without structure no inverted file has recall to trade.  For every batch size the exact side is
`flat.search_device` (and, up to 64 queries, the one-pass path `flat.search` takes for the online shape); the IVF side is
`IVFIndex.search_device` (coarse top-nprobe search + list scan + merge) for every `--nprobe`, with recall@10 of its ids
against the exact ids beside each timing.  With `--pq-m` other than 0 the index is an `IVFPQIndex` over the same lists and
`IVFPQIndex.search_device` (probe with scores + LUT + ADC scan of the codes + exact re-scoring of `--pq-refine` candidates)
is timed for the same cells, with `refine = 0` (raw ADC) beside it.  Every call is timed twice: eagerly (device events over `--iters` back-to-back
calls: what a Python caller sees, launch overhead included) and as a replayed graph of one call (the device time
alone); median of `--reps` rounds after a warm-up.  Prints one JSON object.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import FAISSIndexBuilder, IVFIndex, IVFPQIndex, _native  # noqa: E402
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
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 10_000])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pq-m", type=int, default=64, help="0: no PQ side")
    ap.add_argument("--pq-refine", type=int, default=100)
    ap.add_argument("--pq-iterations", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(41)
    unit = torch.nn.functional.normalize
    centres = unit(torch.randn(args.topics, 384, device=dev, generator=g), dim=1)
    topic = torch.randint(0, args.topics, (args.rows,), device=dev, generator=g)
    corpus = unit(centres[topic] + torch.randn(args.rows, 384, device=dev, generator=g) / 384 ** 0.5, dim=1)
    nq_max = max(args.batches)
    picked = torch.randperm(args.rows, device=dev, generator=g)[:nq_max]
    queries = unit(corpus[picked] + 0.5 * torch.randn(nq_max, 384, device=dev, generator=g) / 384 ** 0.5, dim=1).contiguous()
    del centres, topic

    flat = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    flat.build_from_embeddings(corpus)
    del corpus
    index = IVFPQIndex(flat=flat, m=args.pq_m) if args.pq_m else IVFIndex(flat=flat)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    IVFIndex.train(index, nlist=args.nlist, iterations=args.iterations)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    pq_train_s = None
    if args.pq_m:
        t0 = time.perf_counter()
        index.train_pq(pq_iterations=args.pq_iterations)
        torch.cuda.synchronize()
        pq_train_s = round(time.perf_counter() - t0, 2)
    sizes = np.diff(index.lists_numpy()[0])

    lib = _native.load()
    result = {
        "rows": args.rows, "nlist": index.nlist, "k": args.k, "kmeans_iterations": args.iterations,
        "train_s": round(train_s, 2), "list_rows_min_mean_max": [int(sizes.min()), round(float(sizes.mean()), 1), int(sizes.max())],
        "empty_lists": int((sizes == 0).sum()), "pq_m": args.pq_m, "pq_refine": args.pq_refine,
        "pq_iterations": args.pq_iterations, "pq_train_s": pq_train_s, "device": torch.cuda.get_device_name(0), "runs": [],
    }
    for nq in args.batches:
        q = queries[:nq].contiguous()
        exact = flat.search_device(q, args.k, normalize_queries=False)[1].cpu().numpy()
        iters = args.iters if nq <= 64 else 2
        row = {"nq": nq}
        row["flat_eager_ms"], row["flat_graph_ms"] = _measure(
            lambda: flat.search_device(q, args.k, normalize_queries=False), iters, args.reps)
        if nq <= flat.ONEPASS_MAX_NQ:
            row["flat_onepass_eager_ms"], row["flat_onepass_graph_ms"] = _measure(
                lambda: flat._search_onepass_device(q, args.k, False), iters, args.reps)
        row["ivf"] = []
        for nprobe in args.nprobe:
            found = IVFIndex.search_device(index, q, args.k, nprobe=nprobe, normalize_queries=False)[1].cpu().numpy()
            p = C.c_int(0)
            lib.sskd_ivf_search_plan(nq, min(nprobe, index.nlist), args.k, flat.ntotal, index.max_list_rows, C.byref(p), None, None)
            parts = p.value
            eager, graph = _measure(lambda: IVFIndex.search_device(index, q, args.k, nprobe=nprobe, normalize_queries=False),
                                    iters, args.reps)
            probe = index.probe_device(q, nprobe, normalize_queries=False).cpu().numpy()
            row["ivf"].append({
                "nprobe": nprobe, "parts": parts, "eager_ms": eager, "graph_ms": graph,
                "recall_at_k": round(recall_at_k(found, exact), 4),
                "rows_read_fraction": round(float(sizes[probe].sum(axis=1).mean()) / args.rows, 5),
                "flat_graph_over_ivf_graph": round(row["flat_graph_ms"] / graph, 2),
            })
        row["pq"] = []
        for nprobe in (args.nprobe if args.pq_m else []):
            cell = {"nprobe": nprobe}
            for name, refine in (("refined", args.pq_refine), ("adc", 0)):
                def call(refine=refine):
                    return index.search_device(q, args.k, nprobe=nprobe, refine=refine, normalize_queries=False)
                found = call()[1].cpu().numpy()
                p = C.c_int(0)
                lib.sskd_pq_search_plan(min(nq, 4096), min(nprobe, index.nlist), args.k, refine, args.pq_m, flat.ntotal,
                                        index.max_list_rows, C.byref(p), None, None, None)
                eager, graph = _measure(call, iters, args.reps)
                cell[name] = {"refine": refine, "parts": p.value, "eager_ms": eager, "graph_ms": graph,
                              "recall_at_k": round(recall_at_k(found, exact), 4)}
            ivf_graph = next(c["graph_ms"] for c in row["ivf"] if c["nprobe"] == nprobe)
            cell["ivf_graph_over_pq_graph"] = round(ivf_graph / cell["refined"]["graph_ms"], 2)
            cell["flat_graph_over_pq_graph"] = round(row["flat_graph_ms"] / cell["refined"]["graph_ms"], 2)
            row["pq"].append(cell)
        result["runs"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
