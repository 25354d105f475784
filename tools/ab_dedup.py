"""What clustering near-duplicates on the device costs against what a caller had to do before, same process, alternating
legs.

    python tools/ab_dedup.py [--rows 200000 1000000] [--reps 3] [--threshold 0.9] [--out FILE]
    python tools/ab_dedup.py --rows 200000 --profile-leg          # the new call alone, once: the leg to put under
                                                                    # rocprofv3 --kernel-trace --stats

Two families of unit rows per size, from a seed: ``random`` (almost no pair above the threshold) and ``duplicates`` (about
20 % of the rows lie in clusters of 2 .. 50 noisy copies of one vector, shuffled among the rest).  Three legs per round:

* ``baseline``: ``near_duplicates(threshold)`` and a union-find over its pair list on the host - ``scipy``'s connected
  components when it is installed (the fastest thing a caller has), else ``cluster_pairs``;
* ``new``: ``duplicate_clusters(threshold)`` - batches on tile boundaries, so every batch scans the rows from its start on;
* ``new_full_scan``: the same call with ``batch_size`` one above the default, so only every 32nd batch starts on a tile
  boundary and the rest scan all rows - the triangle path's saving is the ratio of the two.

Whole-call wall times behind a device synchronise; the median of the rounds with min / max.  Also reported: the pairs, the
host bytes of the pair list the baseline holds (pairs int64 [m, 2] + scores float32 [m]; the per-batch copies it makes on the way
come on top), and that both legs give the same labels.  Prints one JSON object.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import FAISSIndexBuilder, cluster_pairs  # noqa: E402

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:   # the host form of the package is then the baseline's union-find
    connected_components = None


def make_rows(n, family, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rows = torch.nn.functional.normalize(torch.randn(n, 384, device=dev, generator=g), dim=1)
    if family == "duplicates":
        # clusters of 2 .. 50 (26 on average) until 20 % of the rows are taken: row k of a cluster copies its first row
        rng = np.random.default_rng(seed)
        sizes = []
        while sum(sizes) < n // 5:
            sizes.append(int(rng.integers(2, 51)))
        source = np.arange(n)
        at = 0
        for c in sizes:
            if at + c > n:
                break
            source[at:at + c] = at
            at += c
        src = torch.from_numpy(source).to(dev)
        noise = torch.nn.functional.normalize(torch.randn(n, 384, device=dev, generator=g), dim=1)
        rows = torch.nn.functional.normalize(rows[src] + 0.02 * noise * (src != torch.arange(n, device=dev))[:, None], dim=1)
        rows = rows[torch.from_numpy(rng.permutation(n)).to(dev)]
    return rows.contiguous()


def host_labels(pairs, n):
    """Smallest row of every row's component, from the pair list."""
    if connected_components is None:
        return cluster_pairs(pairs, n).labels
    graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    first = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp]


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def _stats(xs):
    return {"ms": round(statistics.median(xs), 2), "range": [round(min(xs), 2), round(max(xs), 2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[200_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["random", "duplicates"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--profile-leg", action="store_true", help="run only the new call, once per shape, after one warm-up of a small index")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"threshold": args.threshold, "reps": args.reps,
              "host_union_find": "scipy.sparse.csgraph.connected_components" if connected_components else "cluster_pairs"}
    for n in args.rows:
        for family in args.families:
            index = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
            index.build_from_embeddings(make_rows(n, family, dev, seed=29))
            index.doc_ids = []

            def baseline():
                pairs, scores = index.near_duplicates(args.threshold)
                return host_labels(pairs, n), pairs.shape[0], pairs.nbytes + scores.nbytes

            new = lambda: index.duplicate_clusters(args.threshold)
            new_full = lambda: index.duplicate_clusters(args.threshold, batch_size=4097)
            key = f"{family}_{n}"
            if args.profile_leg:
                ms, out = _wall(new)
                result[key] = {"new_ms": round(ms, 2), "clusters": out.n_clusters}
                print(key, result[key], flush=True)
                continue
            (_, (want, n_pairs, pair_bytes)), (_, got), (_, got_full) = _wall(baseline), _wall(new), _wall(new_full)   # warm-up
            same = bool(np.array_equal(want, got.labels) and np.array_equal(got.labels, got_full.labels))
            times = {"baseline": [], "new": [], "new_full_scan": []}
            for _ in range(args.reps):
                for name, fn in (("baseline", baseline), ("new", new), ("new_full_scan", new_full)):
                    times[name].append(_wall(fn)[0])
            med = {name: statistics.median(ts) for name, ts in times.items()}
            result[key] = {"rows": n, "pairs": int(n_pairs), "clusters": got.n_clusters, "labels_equal": same,
                           "pair_list_host_bytes": int(pair_bytes), **{name: _stats(ts) for name, ts in times.items()},
                           "new_over_baseline": round(med["new"] / med["baseline"], 4),
                           "triangle_over_full_scan": round(med["new"] / med["new_full_scan"], 4)}
            print(key, result[key], flush=True)
            del index
            torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
