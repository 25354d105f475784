"""A/B of range search against the k-NN paths, same process, alternating.

    python tools/ab_range.py [--rows 1000000] [--queries 10000] [--reps 7] [--out FILE]

Per case and round, each leg is timed with device events over `--iters` back-to-back calls after a warm-up; the
median of the rounds is reported with min / max.  Legs:
  * batch (`--queries` queries): range search at about 10 and about 1 000 matches per query, the exact scan at
    k = 10 (`screening = False`) and the `search(k=1024)` workaround;
  * single query: range search at about 100 matches, and the one-pass k = 10 search.
The range legs pass `max_results` (no host sync; the capacity is the measured total).  Thresholds are one scalar per
case, the score quantile of a sample of rows.  Prints one JSON object.
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(13)
    corpus = torch.nn.functional.normalize(torch.randn(args.rows, 384, device=dev, generator=g), dim=1)
    queries = torch.nn.functional.normalize(torch.randn(args.queries, 384, device=dev, generator=g), dim=1)
    sample = (queries[:64] @ corpus[:: max(1, args.rows // 200_000)].T).flatten().float()
    index = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    index.build_from_embeddings(corpus)
    del corpus

    def thr_for(matches):
        return float(torch.quantile(sample[: 1 << 24], 1.0 - matches / args.rows))

    one = queries[:1].contiguous()
    t10, t1000, t100 = thr_for(10), thr_for(1000), thr_for(100)
    caps = {}
    for name, q, t in (("r10", queries, t10), ("r1000", queries, t1000), ("r100", one, t100)):
        lims, _, _ = index.range_search_device(q, t, normalize_queries=False, max_results=0)
        caps[name] = max(int(lims[-1].item()), 1)

    def rng(name, q, t):
        return lambda: index.range_search_device(q, t, normalize_queries=False, max_results=caps[name])

    def exact(k):
        def run():
            index.screening = False
            index.search_device(queries, k, normalize_queries=False)
            index.screening = True
        return run

    cases = {
        "batch_10": [("range", rng("r10", queries, t10), 3), ("exact_k10", exact(10), 3)],
        "batch_1000": [("range", rng("r1000", queries, t1000), 3), ("exact_k10", exact(10), 3), ("search_k1024", exact(1024), 1)],
        "single_100": [("range", rng("r100", one, t100), 50),
                       ("onepass_k10", lambda: index._search_onepass_device(one, 10, False, None), 50)],
    }
    result = {"rows": args.rows, "queries": args.queries, "reps": args.reps,
              "matches_per_query": {"batch_10": caps["r10"] / args.queries, "batch_1000": caps["r1000"] / args.queries,
                                    "single_100": caps["r100"]}}
    for name, legs in cases.items():
        times = {leg: [] for leg, _, _ in legs}
        for _, fn, _ in legs:
            fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for leg, fn, iters in legs:
                times[leg].append(_time(fn, iters))
        out = {}
        for leg, ts in times.items():
            out[f"{leg}_ms"] = round(statistics.median(ts), 4)
            out[f"{leg}_range"] = [round(min(ts), 4), round(max(ts), 4)]
        base = legs[1][0]
        out["range_over_" + base] = round(out["range_ms"] / out[f"{base}_ms"], 4)
        if "search_k1024_ms" in out:
            out["speedup_over_k1024"] = round(out["search_k1024_ms"] / out["range_ms"], 2)
        result[name] = out
        print(name, out, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
