"""What index compaction costs and what it buys, same process, alternating legs.

    python tools/ab_compact.py [--rows 1000000] [--queries 10000] [--reps 7] [--out FILE]

1. Compaction time.  Per removed share (10 %, 50 %, 90 % of the rows, at random) and round: a plain device-to-device
   ``Tensor.copy_`` of ``n_live x 1 536`` bytes, then ``sskd_row_mask_rank`` + ``sskd_index_compact_rows`` into a
   buffer of the same size, each timed with device events over ``--iters`` back-to-back calls after a warm-up.  The
   kernels move exactly the copy's bytes plus 4 B of mask and 8 B of prefix per tile.  The rank call is also timed alone.
2. What it buys.  Screened ``search_device`` (k = 10) over the index with 50 % of its rows removed: tombstoned, then
   the same index after ``compact()``, then a fresh build of half as many rows as the yardstick - the three legs
   alternate per round.

The median of the rounds is reported with min / max.  Prints one JSON object.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import FAISSIndexBuilder, _native  # noqa: E402


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _stats(xs):
    return {"ms": round(statistics.median(xs), 4), "range": [round(min(xs), 4), round(max(xs), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.load()
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(13)
    n = args.rows
    corpus = torch.nn.functional.normalize(torch.randn(n, 384, device=dev, generator=g), dim=1)
    queries = torch.nn.functional.normalize(torch.randn(args.queries, 384, device=dev, generator=g), dim=1)
    index = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    index.build_from_embeddings(corpus)
    result = {"rows": n, "queries": args.queries, "reps": args.reps, "iters": args.iters}

    # 1. compaction against a plain copy of the surviving bytes
    words = int(lib.sskd_row_mask_words(n))
    prefix = torch.empty(words + 1, dtype=torch.int64, device=dev)
    for name, share in (("removed_10", 0.10), ("removed_50", 0.50), ("removed_90", 0.90)):
        live = torch.rand(n, device=dev, generator=g) >= share
        mask = index.row_filter(live).words
        n_live = int(live.sum().item())
        elems = int(lib.sskd_index_padded_rows(n_live)) * 384
        dst = torch.empty(elems, dtype=torch.float32, device=dev)
        src_part = index._tiled[: n_live * 384]

        def copy():
            dst[: n_live * 384].copy_(src_part)

        def rank():
            _native.check(lib.sskd_row_mask_rank(mask.data_ptr(), n, prefix.data_ptr(), stream))

        def compact():
            rank()
            _native.check(lib.sskd_index_compact_rows(index._tiled.data_ptr(), n, mask.data_ptr(), prefix.data_ptr(),
                                                      dst.data_ptr(), stream))

        copy(), compact()
        torch.cuda.synchronize()
        assert int(prefix[-1].item()) == n_live
        t_copy, t_compact, t_rank = [], [], []
        for _ in range(args.reps):
            t_copy.append(_time(copy, args.iters))
            t_compact.append(_time(compact, args.iters))
            t_rank.append(_time(rank, args.iters))
        mc, mk = statistics.median(t_copy), statistics.median(t_compact)
        result[name] = {"n_live": n_live, "bytes": n_live * 1536, "copy": _stats(t_copy), "rank_plus_compact": _stats(t_compact),
                        "rank_alone": _stats(t_rank), "ratio": round(mk / mc, 4),
                        "copy_gbps": round(2 * n_live * 1536 / mc / 1e6, 1),
                        "compact_gbps": round(2 * n_live * 1536 / mk / 1e6, 1)}
        print(name, result[name], flush=True)
        del dst, mask, live

    # 2. screened search: tombstoned, compacted, and a fresh index of half the rows
    gone = torch.nonzero(torch.rand(n, device=dev, generator=g) < 0.5).reshape(-1)
    tomb = index
    tomb.remove_ids(gone)
    compacted = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    compacted.build_from_embeddings(corpus)
    compacted.remove_ids(gone)
    kept = compacted.compact()
    fresh = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    fresh.build_from_embeddings(corpus[: n // 2])
    del corpus
    legs = {"tombstoned": tomb, "compacted": compacted, "fresh_half": fresh}
    out = {}
    for name, ix in legs.items():
        out[name] = ix.search_device(queries, 10)   # warm-up: builds every sidecar
        assert ix.last_status is not None, "the screened path must serve this shape"
    torch.cuda.synchronize()
    kept_dev = torch.from_numpy(kept).to(dev)
    assert torch.equal(out["tombstoned"][0], out["compacted"][0])
    assert torch.equal(out["tombstoned"][1], kept_dev[out["compacted"][1]])
    times = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, ix in legs.items():
            times[name].append(_time(lambda: ix.search_device(queries, 10), args.iters))
    result["search_half_removed"] = {name: {"rows": legs[name].ntotal, **_stats(ts)} for name, ts in times.items()}
    result["search_half_removed"]["compacted_over_tombstoned"] = round(
        statistics.median(times["compacted"]) / statistics.median(times["tombstoned"]), 4)
    result["search_half_removed"]["compacted_over_fresh_half"] = round(
        statistics.median(times["compacted"]) / statistics.median(times["fresh_half"]), 4)
    print("search_half_removed", result["search_half_removed"], flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
