"""Timing of the late-interaction re-rank against a torch restatement on the same bf16 tokens: same process, same
store, same candidates.

    python tools/ab_late.py [--rows 100000] [--mean-td 80] [--tq 32] [--candidates 100] [--batches 1 1024]
                            [--reps 5] [--iters 20] [--out FILE] [--only-cell NQ] [--no-torch] [--no-serve]
                            [--dump-outputs DIR]

The store holds `--rows` documents whose lengths are drawn around `--mean-td` tokens (normal, sigma a quarter of the
mean, clipped to [8, 180]); every token is a random unit row.  For every batch size the candidates are `--candidates`
random rows per query.  `sskd_late_rerank` (through `LateInteractionIndex.rerank_device`, k = 10) is timed as a replayed
graph of one call (device time alone; median of `--reps` rounds of `--iters` replays) and eagerly.  From the graph time:
the gather bandwidth `sum Td * 768 B / t` against the HBM peak (8 TB/s) and the bf16 FLOP/s `2 * 384 * Tq_pad * Td_pad`
per pair (what the MFMAs execute: Tq and Td padded to 32) against the MFMA peak (2.5 PFLOP/s).  The torch side restates
the computation on the same tokens - padded gather, einsum, amax, sum - in chunks of queries that fit, timed eagerly
with events, and its scores are compared with the kernel's.  The last section times the library path of one `/search`
(encode the pooled query, first stage, and with the store: encode the query's tokens, pack, re-rank) on a synthetic
12-layer encoder, with and without the store.  `--only-cell NQ` replays that one cell a few times and nothing else (for
a kernel trace).  `--dump-outputs DIR` saves every cell's raw scores as `DIR/late_raw_nq<NQ>.npy`.  Prints one JSON object.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import BertConfig, FAISSIndexBuilder, LateInteractionIndex, Mi355xSentenceEncoder  # noqa: E402
from semantic_search_kd_amd.late import pack_tokens  # noqa: E402

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


def _measure(fn, iters, reps):
    """(eager ms, graph-replay ms) of one call of fn: medians of `reps` rounds."""
    fn()
    torch.cuda.synchronize()
    eager = statistics.median(_events(fn, iters) for _ in range(reps))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    graph = statistics.median(_events(g.replay, iters) for _ in range(reps))
    return round(eager, 4), round(graph, 4)


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


def torch_maxsim(q_tok, tq, store, lims_dev, cand, chunk):
    """The restatement: q_tok bf16 [nq * tq, 384] (every query tq tokens), cand int64 [nq, R] -> fp32 [nq, R]."""
    nq, R = cand.shape
    q = q_tok.view(nq, tq, DIM)
    beg, end = lims_dev[cand], lims_dev[cand + 1]
    td_max = int((end - beg).max())
    steps = torch.arange(td_max, device="cuda")
    out = torch.empty((nq, R), dtype=torch.float32, device="cuda")
    for lo in range(0, nq, chunk):
        b, e = beg[lo: lo + chunk], end[lo: lo + chunk]
        rows = (b[..., None] + steps).clamp(max=store.shape[0] - 1)                 # [c, R, td_max]
        docs = store[rows]                                                          # padded gather
        dots = torch.einsum("qik,qrjk->qrij", q[lo: lo + chunk], docs).float()
        dots = dots.masked_fill(~(steps < (e - b)[..., None])[:, :, None, :], float("-inf"))
        out[lo: lo + chunk] = dots.amax(dim=3).sum(dim=2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--mean-td", type=int, default=80)
    ap.add_argument("--tq", type=int, default=32)
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-chunk", type=int, default=64)
    ap.add_argument("--only-cell", type=int, default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-serve", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--dump-outputs", type=str, default=None)
    args = ap.parse_args()

    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    td = np.clip(np.rint(rng.normal(args.mean_td, args.mean_td / 4, args.rows)), 8, 180).astype(np.int64)
    lims = np.concatenate([[0], np.cumsum(td)]).astype(np.int64)
    flat = FAISSIndexBuilder(embedding_dim=DIM, index_type="HNSW", metric="ip", device="cuda:0")
    flat.build_from_embeddings(torch.nn.functional.normalize(torch.randn((args.rows, DIM), device="cuda", generator=gen), dim=1))
    late = LateInteractionIndex(flat)
    late.set_tokens(_unit_rows(int(lims[-1]), gen), lims)
    result = {"rows": args.rows, "tokens": int(lims[-1]), "store_bytes": late.nbytes, "mean_td": float(td.mean()),
              "tq": args.tq, "candidates": args.candidates, "cells": []}

    for nq in ([args.only_cell] if args.only_cell else args.batches):
        q_tok = _unit_rows(nq * args.tq, gen)
        queries = late.prepare_queries(q_tok, np.arange(nq + 1, dtype=np.int64) * args.tq)
        cand = torch.randint(0, args.rows, (nq, args.candidates), device="cuda", generator=gen)
        call = lambda: late.rerank_device(queries, None, cand, 10, return_raw=True)   # noqa: E731
        if args.only_cell:
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            continue
        eager, graph = _measure(call, args.iters, args.reps)
        if args.dump_outputs:
            _dump(args.dump_outputs, f"late_raw_nq{nq}", call()[2])
        pair_td = td[cand.cpu().numpy()]
        gathered = float(pair_td.sum()) * DIM * 2
        flops = float((np.ceil(pair_td / 32) * 32).sum()) * 2 * DIM * (-(-args.tq // 32) * 32)
        t = graph * 1e-3
        cell = {"nq": nq, "eager_ms": eager, "graph_ms": graph, "gathered_bytes": gathered,
                "gather_TBps": round(gathered / t / 1e12, 3), "hbm_fraction": round(gathered / t / HBM_PEAK, 3),
                "PFLOPs": round(flops / t / 1e15, 4), "mfma_fraction": round(flops / t / MFMA_BF16_PEAK, 4)}
        if not args.no_torch:
            ref = lambda: torch_maxsim(q_tok, args.tq, late.tokens, late._lims_dev, cand, args.torch_chunk)   # noqa: E731
            want = ref()
            got = call()[2]
            torch.cuda.synchronize()
            cell["torch_eager_ms"] = round(statistics.median(_events(ref, max(1, args.iters // 4)) for _ in range(args.reps)), 4)
            cell["max_abs_diff_vs_torch"] = float((got - want).abs().max())
            cell["speedup_vs_torch"] = round(cell["torch_eager_ms"] / eager, 2)
        result["cells"].append(cell)

    if not args.no_serve and not args.only_cell:
        # the library path of one /search: a 16-token query on a synthetic 12-layer encoder
        enc = Mi355xSentenceEncoder.from_synthetic(BertConfig(num_hidden_layers=12), device="cuda:0")
        ids = torch.randint(1000, 20000, (1, 16), dtype=torch.int32, device="cuda", generator=gen)
        mask = torch.ones_like(ids)
        length, offset = torch.tensor([16], dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        q_lims = np.array([0, 16], dtype=np.int64)

        def without():
            return flat.search_device(enc.encode_token_ids(ids, mask), 10)

        def with_store():
            _, first = flat.search_device(enc.encode_token_ids(ids, mask), args.candidates)
            tokens = torch.empty((16, DIM), dtype=torch.bfloat16, device="cuda")
            pack_tokens(enc.hidden_states(ids, mask), length, offset, tokens)
            return late.rerank_device(tokens, q_lims, first, 10)

        for fn in (without, with_store):
            fn()
        torch.cuda.synchronize()
        result["search_path_nq1"] = {
            "without_store_ms": round(statistics.median(_events(without, args.iters) for _ in range(args.reps)), 4),
            "with_store_ms": round(statistics.median(_events(with_store, args.iters) for _ in range(args.reps)), 4)}

    text = json.dumps(result)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
