"""Timing of the compressed late-interaction re-rank (`sskd_latec_rerank`) against the bf16 one (`sskd_late_rerank`,
unchanged) in the same process: same documents, same queries, same candidates.

    python tools/ab_late_compressed.py [--rows 100000] [--mean-td 80] [--tq 32] [--candidates 100] [--batches 1 1024]
                                       [--bits 2 4] [--centroids 4096 65536] [--reps 5] [--iters 20] [--out FILE]
                                       [--dump-outputs DIR]

The store is the one of `tools/ab_late.py`: `--rows` documents of about `--mean-td` random unit tokens.  For every
(`--bits`, `--centroids`) a codec is made by `train_codec` (k-means seeding only: `iterations=0`, the timing does not
depend on how good the centroids are, it depends on how the centroid ids spread) and the same tokens are compressed
under it.  Per batch size every store's `rerank_device` (k = 10, raw scores too) is captured as a graph of one call and
the graphs are replayed in turn, `--reps` rounds of `--iters` replays each, alternating the stores inside a round (a
replay is first checked to reproduce the eager call's scores bit for bit; eager calls are timed the same way); the
median per store is reported with its ratio to the bf16 store's.  From the time: the bytes a pair needs - compressed
`sum Td * (8 + 48 nbits)` from the store plus `sum Td * 768` of centroid rows (cache-resident when C is small) - over
the time, and the bf16 FLOP/s the MFMAs execute against the peak.  The top-10 overlap with the bf16 ranking is reported
for what it is: on random tokens it says nothing about real text.  `--dump-outputs DIR` saves every store's raw scores
as `DIR/latec_raw_<store>_nq<NQ>.npy`.  Prints one JSON object.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import FAISSIndexBuilder, LateInteractionIndex  # noqa: E402

HBM_PEAK = 8.0e12
MFMA_BF16_PEAK = 2.5e15
DIM = 384


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _unit_rows(n, gen, chunk=1 << 20):
    out = torch.empty((n, DIM), dtype=torch.bfloat16, device="cuda")
    for lo in range(0, n, chunk):
        x = torch.randn((min(chunk, n - lo), DIM), device="cuda", generator=gen)
        out[lo: lo + x.shape[0]] = torch.nn.functional.normalize(x, dim=1).to(torch.bfloat16)
    return out


def _dump(out_dir, name, tensor):
    """`--dump-outputs`: one output as `.npy` (the inputs are seeded: the files of two builds are compared with `cmp`)."""
    Path(out_dir).mkdir(parents=True, exist_ok=True)
    np.save(Path(out_dir) / f"{name}.npy", tensor.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--mean-td", type=int, default=80)
    ap.add_argument("--tq", type=int, default=32)
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--bits", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--centroids", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--dump-outputs", type=str, default=None)
    args = ap.parse_args()

    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    td = np.clip(np.rint(rng.normal(args.mean_td, args.mean_td / 4, args.rows)), 8, 180).astype(np.int64)
    lims = np.concatenate([[0], np.cumsum(td)]).astype(np.int64)
    flat = FAISSIndexBuilder(embedding_dim=DIM, index_type="HNSW", metric="ip", device="cuda:0")
    flat.build_from_embeddings(torch.nn.functional.normalize(torch.randn((args.rows, DIM), device="cuda", generator=gen), dim=1))
    base = LateInteractionIndex(flat)
    base.set_tokens(_unit_rows(int(lims[-1]), gen), lims)
    stores = {"bf16": base}
    result = {"rows": args.rows, "tokens": int(lims[-1]), "mean_td": float(td.mean()), "tq": args.tq,
              "candidates": args.candidates, "stores": {"bf16": {"bytes": base.nbytes, "bytes_per_token": 768}}, "cells": []}
    for C in args.centroids:
        for nbits in args.bits:
            late = LateInteractionIndex(flat)
            late.set_tokens(base.tokens, lims)                       # the same device tensor, not a copy
            t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0[0].record()
            late.train_codec(nbits=nbits, n_centroids=C, sample_tokens=min(int(lims[-1]), 4 * C), iterations=0)
            late.compress()
            t0[1].record()
            t0[1].synchronize()
            name = f"b{nbits}-C{C}"
            stores[name] = late
            used = int(torch.unique(late.cid).numel())
            result["stores"][name] = {"bytes": late.nbytes, "bytes_per_token": 8 + 48 * nbits, "nbits": nbits, "n_centroids": C,
                                      "centroids_in_use": used, "codec_bytes": C * 768 + 4 * (2 * (1 << nbits) - 1),
                                      "train_and_compress_s": round(t0[0].elapsed_time(t0[1]) / 1e3, 2)}

    for nq in args.batches:
        q_tok = _unit_rows(nq * args.tq, gen)
        cand = torch.randint(0, args.rows, (nq, args.candidates), device="cuda", generator=gen)
        graphs, tops = {}, {}
        for name, late in stores.items():
            queries = late.prepare_queries(q_tok, np.arange(nq + 1, dtype=np.int64) * args.tq)
            call = lambda late=late, queries=queries: late.rerank_device(queries, None, cand, 10, return_raw=True)   # noqa: E731
            eager_out = call()
            tops[name] = eager_out[1].cpu().numpy()
            if args.dump_outputs:
                _dump(args.dump_outputs, f"latec_raw_{name}_nq{nq}", eager_out[2])
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                graph_out = call()
            graph_out[2].fill_(0)
            g.replay()
            torch.cuda.synchronize()
            if not torch.equal(graph_out[2].view(torch.int32), eager_out[2].view(torch.int32)):
                raise RuntimeError(f"{name}, nq={nq}: the replayed graph does not reproduce the eager scores")
            graphs[name] = (g, call, graph_out)
        times = {name: [] for name in graphs}
        eager = {name: [] for name in graphs}
        for _ in range(args.reps):                                   # the stores alternate inside a round
            for name, (g, call, _) in graphs.items():
                times[name].append(_events(g.replay, args.iters))
            for name, (g, call, _) in graphs.items():
                eager[name].append(_events(call, args.iters))
        pair_td = td[cand.cpu().numpy()]
        tokens = float(pair_td.sum())
        flops = float((np.ceil(pair_td / 32) * 32).sum()) * 2 * DIM * (-(-args.tq // 32) * 32)
        cell = {"nq": nq, "pair_tokens": tokens, "stores": {}}
        t_bf16 = statistics.median(times["bf16"])
        for name in graphs:
            t_ms = statistics.median(times[name])
            t = t_ms * 1e-3
            per_token = result["stores"][name]["bytes_per_token"]
            row = {"graph_ms": round(t_ms, 4), "eager_ms": round(statistics.median(eager[name]), 4), "min_ms": round(min(times[name]), 4), "max_ms": round(max(times[name]), 4),
                   "ratio_to_bf16": round(t_ms / t_bf16, 3), "store_TBps": round(tokens * per_token / t / 1e12, 3),
                   "store_hbm_fraction": round(tokens * per_token / t / HBM_PEAK, 4),
                   "PFLOPs": round(flops / t / 1e15, 4), "mfma_fraction": round(flops / t / MFMA_BF16_PEAK, 4)}
            if name != "bf16":
                row["centroid_TBps"] = round(tokens * 768 / t / 1e12, 3)
                row["top10_shared_with_bf16"] = round(float(np.mean([len(set(a) & set(b)) for a, b in zip(tops[name], tops["bf16"])])), 2)
            cell["stores"][name] = row
        result["cells"].append(cell)
        del graphs

    text = json.dumps(result)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
