"""A/B of `GraphIndex.insert` against `GraphIndex.add` (the rebuild): same process, same corpus, same new rows
("Incremental insertion").

    python tools/ab_graph_insert.py [--rows 1000000] [--new 10000] [--degree 32] [--knn-k 64] [--ef 32 64 128]
                                    [--queries 10000] [--only-insert] [--out FILE]

The corpus is `tools/ab_graph.py`'s: clustered (`--topics` unit centres, rows = unit(centre + N(0, I) / sqrt(384))), every
query a noisy copy of a row (unit(row + 0.5 N(0, I) / sqrt(384))).  The graph is built over the first `rows - new` rows.
Then, on copies of that state: the steps of an insertion one by one with a device synchronise after each (k-NN search of
the new rows, insert-prune, reverse plumbing, merge, link, entry add), the whole `insert` as a user calls it, and `add`
(the flat add and a rebuild over all rows: what an append cost before).  Every time is a host clock around work that ends
in a synchronise; each is ONE call - an insertion changes the index, so there is nothing to repeat - after one small
warm-up insertion on a scratch index that loads the kernels.  recall@10 against the exact ids for every `--ef`, the
inserted graph beside the rebuilt one, over all queries and over the queries drawn from the new rows.  `--only-insert`
builds, inserts once and stops (for a kernel trace).  Prints one JSON object.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import FAISSIndexBuilder, GraphIndex  # noqa: E402
from semantic_search_kd_amd.graph import entry_rows_of, n_entry_of_insert  # noqa: E402
from semantic_search_kd_amd.ivf import recall_at_k  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _graph_over(rows, adjacency, entry_rows, args):
    """A GraphIndex over its own copy of `rows` with the given adjacency (no build)."""
    flat = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    flat.build_from_embeddings(rows)
    index = GraphIndex.from_graph(flat, adjacency, entry_rows)
    index.knn_k = args.knn_k
    return index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--new", type=int, default=10_000)
    ap.add_argument("--topics", type=int, default=4096)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--knn-k", type=int, default=None)
    ap.add_argument("--ef", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only-insert", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.knn_k = args.knn_k if args.knn_k is not None else 2 * args.degree
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(41)
    unit = torch.nn.functional.normalize
    centres = unit(torch.randn(args.topics, 384, device=dev, generator=g), dim=1)
    topic = torch.randint(0, args.topics, (args.rows,), device=dev, generator=g)
    corpus = unit(centres[topic] + torch.randn(args.rows, 384, device=dev, generator=g) / 384 ** 0.5, dim=1)
    picked = torch.randperm(args.rows, device=dev, generator=g)[:args.queries]
    queries = unit(corpus[picked] + 0.5 * torch.randn(args.queries, 384, device=dev, generator=g) / 384 ** 0.5, dim=1).contiguous()
    del centres, topic
    n0, b, M, K0 = args.rows - args.new, args.new, args.degree, args.knn_k
    old_rows, new_rows = corpus[:n0].contiguous(), corpus[n0:].contiguous()
    del corpus

    # a small scratch index: one build and one insertion load every kernel the timed calls use
    scratch = GraphIndex(embedding_dim=384, metric="ip", device="cuda:0", M=M, knn_k=K0)
    scratch.build_from_embeddings(old_rows[:20_000])
    scratch.insert(new_rows[:1000])
    scratch.cleanup()
    del scratch

    base = GraphIndex(embedding_dim=384, metric="ip", device="cuda:0", M=M, knn_k=K0)
    _, build_s = _timed(lambda: base.build_from_embeddings(old_rows))
    print(f"graph over {n0} rows built in {build_s:.1f} s", file=sys.stderr, flush=True)
    adjacency, entry_rows = base.graph_numpy(), base.entry_rows_numpy()

    if args.only_insert:
        _, whole = _timed(lambda: base.insert(new_rows))
        print(json.dumps({"only_insert": True, "rows": args.rows, "new": b, "insert_s": round(whole, 4)}))
        return

    # ---- the steps, one by one (what GraphIndex.insert runs), on a copy of the built state
    stepped = _graph_over(old_rows, adjacency, entry_rows, args)
    steps = {}
    _, steps["flat_add"] = _timed(lambda: stepped.flat.add(new_rows))
    knn, steps["knn_search"] = _timed(lambda: stepped.knn_device(K0, first=n0))
    fwd, steps["insert_prune"] = _timed(lambda: stepped.insert_prune_device(stepped.graph, knn))
    (incoming_new, touched, incoming_old), steps["reverse_plumbing"] = _timed(lambda: stepped.incoming_device(fwd, n0))

    def grow_and_merge():
        grown = torch.empty((n0 + b, M), dtype=torch.int32, device=dev)
        grown[:n0].copy_(stepped.graph)
        stepped.merge_rows_device(fwd, incoming_new, n0, grown[n0:])
        return grown

    grown, steps["grow_and_merge"] = _timed(grow_and_merge)
    _, steps["link"] = _timed(lambda: stepped.link_device(grown, n0, touched, incoming_old))

    def entry_add():
        e = n_entry_of_insert(b, n0, M, None)
        rows = torch.from_numpy(n0 + entry_rows_of(b, e).astype("int64")).to(dev)
        stepped.entry.add(stepped._rows_view()[rows].contiguous())

    _, steps["entry_add"] = _timed(entry_add)
    n_touched = int(touched.numel())
    stepped_graph = grown.cpu().numpy()
    stepped.cleanup()
    del stepped, knn, fwd, incoming_new, touched, incoming_old, grown

    # ---- the whole call, and the rebuild, each on the built state
    _, insert_s = _timed(lambda: base.insert(new_rows))
    same_bits = bool((base.graph_numpy() == stepped_graph).all())
    del stepped_graph
    exact = base.flat.search_device(queries, args.k, normalize_queries=False)[1].cpu().numpy()
    from_new = (picked >= n0).cpu().numpy()

    def recalls(index):
        out = {}
        for ef in args.ef:
            found = index.search_device(queries, args.k, ef=ef, normalize_queries=False)[1].cpu().numpy()
            out[str(ef)] = {"all": round(recall_at_k(found, exact), 4),
                            "from_new_rows": round(recall_at_k(found[from_new], exact[from_new]), 4)}
        return out

    degree = (base.graph >= 0).sum(dim=1).float()
    inserted = {"recall_at_k": recalls(base), "n_entry": base.n_entry,
                "edges_per_row_min_mean": [int(degree.min().item()), round(float(degree.mean().item()), 2)]}
    base.cleanup()
    del base

    rebuilt = _graph_over(old_rows, adjacency, entry_rows, args)
    _, add_s = _timed(lambda: rebuilt.add(new_rows))
    degree = (rebuilt.graph >= 0).sum(dim=1).float()
    rebuilt_out = {"recall_at_k": recalls(rebuilt), "n_entry": rebuilt.n_entry,
                   "edges_per_row_min_mean": [int(degree.min().item()), round(float(degree.mean().item()), 2)]}

    result = {
        "rows": args.rows, "new": b, "k": args.k, "degree": M, "knn_k": K0, "queries": args.queries,
        "queries_from_new_rows": int(from_new.sum()), "build_s": round(build_s, 2),
        "insert_s": round(insert_s, 4), "insert_steps_s": {k: round(v, 4) for k, v in steps.items()},
        "insert_steps_sum_s": round(sum(steps.values()), 4), "touched_rows": n_touched,
        "stepped_equals_whole": same_bits, "add_rebuild_s": round(add_s, 2),
        "add_over_insert": round(add_s / insert_s, 1), "inserted": inserted, "rebuilt": rebuilt_out,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
