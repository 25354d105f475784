"""Timing of retrieval from the compressed token store's own centroid lists (`search_tokens_device`: centroid scores,
probes, union, centroid interaction, selection, compressed MaxSim) against the existing path (`search_device`: the flat
exact first stage over pooled vectors, then the same compressed MaxSim; unchanged) in the same process.

    python tools/ab_plaid.py [--rows 100000] [--mean-td 80] [--tq 32] [--batches 1 1024] [--centroids 4096 65536]
                             [--nprobe 2] [--ndocs 256] [--reps 5] [--iters 20] [--out FILE] [--trace-only]
                             [--dump-outputs DIR]

The store is the one of `tools/ab_late.py` and `tools/ab_late_compressed.py`: `--rows` documents of about `--mean-td`
random unit tokens, compressed to 2 bits under a codec of `train_codec(iterations=0)` per `--centroids`.  Per batch size
both paths (k = 10) are captured as a graph of one call each and the graphs are replayed in turn, `--reps` rounds of
`--iters` replays, alternating inside a round (a replay is first checked to reproduce the eager call bit for bit); the
median per path is reported.  Also reported: the mean `n_cand`, and what the interaction gathers - `n_cand * mean Td`
rows of `Tq` floats per query, an estimate that takes every candidate for a document of mean length.  Random tokens have
nothing to cluster: the figures say what the kernels cost at these list lengths, nothing about ranking quality.

`--trace-only` runs three eager calls of `search_tokens_device` per cell and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the per-stage kernel times.  `--dump-outputs DIR` saves every cell's candidate
ids and approximate scores as `DIR/plaid_{ids,approx}_C<C>_nq<NQ>.npy`.  Prints one JSON object.
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


def _captured(call, what):
    """`call` run once eagerly, captured, and the replay checked against the eager outputs bit for bit."""
    eager = call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for t in out:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        if not torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)):
            raise RuntimeError(f"{what}: the replayed graph does not reproduce the eager call")
    return g, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--mean-td", type=int, default=80)
    ap.add_argument("--tq", type=int, default=32)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--centroids", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--nprobe", type=int, default=2)
    ap.add_argument("--ndocs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--dump-outputs", type=str, default=None)
    args = ap.parse_args()

    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    td = np.clip(np.rint(rng.normal(args.mean_td, args.mean_td / 4, args.rows)), 8, 180).astype(np.int64)
    lims = np.concatenate([[0], np.cumsum(td)]).astype(np.int64)
    flat = FAISSIndexBuilder(embedding_dim=DIM, index_type="HNSW", metric="ip", device="cuda:0")
    flat.build_from_embeddings(torch.nn.functional.normalize(torch.randn((args.rows, DIM), device="cuda", generator=gen), dim=1))
    tokens = _unit_rows(int(lims[-1]), gen)
    result = {"rows": args.rows, "tokens": int(lims[-1]), "mean_td": float(td.mean()), "tq": args.tq, "nbits": 2,
              "nprobe": args.nprobe, "ndocs": args.ndocs, "k": 10, "stores": {}, "cells": []}
    stores = {}
    for C in args.centroids:
        late = LateInteractionIndex(flat)
        late.set_tokens(tokens, lims)                                # the same device tensor, not a copy
        late.train_codec(nbits=2, n_centroids=C, sample_tokens=min(int(lims[-1]), 4 * C), iterations=0)
        late.compress()
        t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0[0].record()
        late.build_centroid_lists()
        t0[1].record()
        t0[1].synchronize()
        per_list = np.diff(late.centroid_lists_numpy()[0])
        stores[C] = late
        result["stores"][f"C{C}"] = {"store_bytes": late.nbytes, "list_bytes": late.centroid_list_bytes,
                                     "list_pairs": int(per_list.sum()), "mean_list_rows": round(float(per_list.mean()), 1),
                                     "max_list_rows": int(per_list.max()), "build_lists_s": round(t0[0].elapsed_time(t0[1]) / 1e3, 3)}
    del tokens

    for nq in args.batches:
        q_tok = _unit_rows(nq * args.tq, gen)
        q_lims = np.arange(nq + 1, dtype=np.int64) * args.tq
        q_emb = torch.nn.functional.normalize(torch.randn((nq, DIM), device="cuda", generator=gen), dim=1)
        for C, late in stores.items():
            queries = late.prepare_token_queries(q_tok, q_lims)
            by_lists = lambda late=late, queries=queries: late.search_tokens_device(   # noqa: E731
                queries, None, 10, nprobe=args.nprobe, ndocs=args.ndocs, return_candidates=True)
            by_flat = lambda late=late, queries=queries: late.search_device(q_emb, queries, None, 10, candidates=args.ndocs)   # noqa: E731
            if args.trace_only:
                for _ in range(3):
                    by_lists()
                torch.cuda.synchronize()
                result["cells"].append({"nq": nq, "centroids": C, "traced_calls": 3})
                continue
            first = by_lists()
            n_cand = first[4].cpu().numpy()
            if args.dump_outputs:
                _dump(args.dump_outputs, f"plaid_ids_C{C}_nq{nq}", first[2])
                _dump(args.dump_outputs, f"plaid_approx_C{C}_nq{nq}", first[3])
            graphs = {"centroids": _captured(by_lists, f"centroids, C={C}, nq={nq}")[0],
                      "flat": _captured(by_flat, f"flat, C={C}, nq={nq}")[0]}
            times = {name: [] for name in graphs}
            for _ in range(args.reps):                               # the paths alternate inside a round
                for name, g in graphs.items():
                    times[name].append(_events(g.replay, args.iters))
            med = {name: statistics.median(t) for name, t in times.items()}
            gather_bytes = float(n_cand.sum()) * float(td.mean()) * args.tq * 4
            result["cells"].append({
                "nq": nq, "centroids": C, "chunks": len(late._token_chunks(queries)),
                "centroids_ms": round(med["centroids"], 4), "flat_ms": round(med["flat"], 4),
                "centroids_min_max_ms": [round(min(times["centroids"]), 4), round(max(times["centroids"]), 4)],
                "flat_min_max_ms": [round(min(times["flat"]), 4), round(max(times["flat"]), 4)],
                "ratio_to_flat": round(med["centroids"] / med["flat"], 2),
                "mean_n_cand": round(float(n_cand.mean()), 1), "n_cand_share_of_rows": round(float(n_cand.mean()) / args.rows, 4),
                "interaction_gather_bytes_estimate": gather_bytes})
            print(f"nq={nq} C={C}: {result['cells'][-1]}", file=sys.stderr, flush=True)
            del graphs

    text = json.dumps(result)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
