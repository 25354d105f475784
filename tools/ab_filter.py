"""A/B of filtered against unfiltered search, same process, alternating.

    python tools/ab_filter.py [--rows 1000000] [--queries 10000] [--reps 7] [--out FILE]

Per case and round: the unfiltered call, then the same call with a row allow-mask, each timed with device events over
`--iters` back-to-back calls after a warm-up; the median of the rounds is reported with min / max.  Cases: screened
batch (k = 10) with an all-allowed, a random 50 % and a random 1 % mask; one-pass (nq = 1, k = 10) with an all-allowed
and a random 50 % mask.  Prints one JSON object.
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
    g = torch.Generator(device=dev).manual_seed(11)
    corpus = torch.nn.functional.normalize(torch.randn(args.rows, 384, device=dev, generator=g), dim=1)
    queries = torch.nn.functional.normalize(torch.randn(args.queries, 384, device=dev, generator=g), dim=1)
    index = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    index.build_from_embeddings(corpus)
    del corpus
    masks = {
        "all": index.row_filter(torch.ones(args.rows, dtype=torch.bool, device=dev)),
        "half": index.row_filter(torch.rand(args.rows, device=dev, generator=g) < 0.5),
        "one_percent": index.row_filter(torch.rand(args.rows, device=dev, generator=g) < 0.01),
    }
    one = queries[:1].contiguous()
    cases = {
        "screened_all": (lambda m: index.search_device(queries, 10, allow=m), "all", 5),
        "screened_half": (lambda m: index.search_device(queries, 10, allow=m), "half", 5),
        "screened_one_percent": (lambda m: index.search_device(queries, 10, allow=m), "one_percent", 5),
        "onepass_all": (lambda m: index._search_onepass_device(one, 10, False, None if m is None else m.words), "all", 50),
        "onepass_half": (lambda m: index._search_onepass_device(one, 10, False, None if m is None else m.words), "half", 50),
    }
    result = {"rows": args.rows, "queries": args.queries, "reps": args.reps}
    for name, (fn, mask, iters) in cases.items():
        base, filt = [], []
        fn(None), fn(masks[mask])   # warm-up of both instantiations
        torch.cuda.synchronize()
        for _ in range(args.reps):
            base.append(_time(lambda: fn(None), iters))
            filt.append(_time(lambda: fn(masks[mask]), iters))
        mb, mf = statistics.median(base), statistics.median(filt)
        result[name] = {"unfiltered_ms": round(mb, 4), "filtered_ms": round(mf, 4), "ratio": round(mf / mb, 4),
                        "unfiltered_range": [round(min(base), 4), round(max(base), 4)],
                        "filtered_range": [round(min(filt), 4), round(max(filt), 4)]}
        print(name, result[name], flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
