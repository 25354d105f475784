"""Hybrid retrieval on the device against the host fusion a user had before ``sskd_hybrid_fuse``.

    python tools/ab_hybrid.py [--docs 1000000] [--queries 10000] [--depth 100] [--k 10] [--reps 5] [--out FILE]

Corpus: ``--docs`` random unit rows (dense side) and as many synthetic Zipf texts (BM25 side; ``--vocab`` words, 1 - 30
tokens per document), nothing downloaded; queries: random unit vectors with 6-token Zipf texts.

* device: ``HybridIndex.search_device`` in both methods, and its three device calls one by one (the dense search at
  ``depth``, the BM25 search at ``depth``, ``sskd_hybrid_fuse`` alone on those two results), device events around each,
  median of ``--reps`` after a warm-up of the same shapes.
* host: the two device results brought to the host (``.cpu()``) and fused there - what a user of the two indexes had to
  do: ``rrf`` as a per-query Python loop (the checker's rule) and as a vectorised NumPy version (sort by row, add the
  duplicates, stable sort by score); both are compared bitwise with the device.  ``linear`` on the host cannot score
  the rows one list lacks (neither index scores a given row on request), so its host leg fuses the rows BOTH lists
  hold only - less work and another result, timed for scale and not compared.

Prints one JSON object per stage (so a run that is cut short leaves what it measured) and the summary last.
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
sys.path.insert(0, str(Path(__file__).resolve().parent))
from ab_bm25 import zipf_texts  # noqa: E402
from semantic_search_kd_amd import BM25Index, FAISSIndexBuilder, HybridIndex, _native  # noqa: E402


def device_ms(fn, reps):
    fn()   # warm-up at the timed shape
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(times), 3), "range_ms": [round(min(times), 3), round(max(times), 3)]}


def host_rrf_loop(S, I, B, J, k, ws, wb, rrf_k):
    nq = I.shape[0]
    out_s, out_i = np.full((nq, k), -np.inf), np.full((nq, k), -1, np.int64)
    for q in range(nq):
        fused = {}
        rank = 0
        for r in I[q].tolist():
            if r < 0:
                break
            rank += 1
            fused[r] = ws * (1.0 / (rrf_k + rank))
        rank = 0
        for r, b in zip(J[q].tolist(), B[q].tolist()):
            if r < 0:
                break
            if b == 0.0:
                continue
            rank += 1
            fused[r] = fused.get(r, 0.0) + wb * (1.0 / (rrf_k + rank))
        top = sorted(fused, key=lambda r: (-fused[r], r))[:k]
        out_s[q, : len(top)] = [fused[r] for r in top]
        out_i[q, : len(top)] = top
    return out_s, out_i


def host_rrf_numpy(S, I, B, J, k, ws, wb, rrf_k):
    """The same rule for whole batches (rankings without -1 holes: every id >= 0 comes before the padding)."""
    big = np.iinfo(np.int64).max
    ok_s, ok_b = I >= 0, (J >= 0) & (B != 0.0)
    term_s = np.where(ok_s, ws * (1.0 / (rrf_k + np.cumsum(ok_s, axis=1))), -np.inf)
    term_b = np.where(ok_b, wb * (1.0 / (rrf_k + np.cumsum(ok_b, axis=1))), -np.inf)
    rows = np.concatenate([np.where(ok_s, I, big), np.where(ok_b, J, big)], axis=1)
    fused = np.concatenate([term_s, term_b], axis=1)
    order = np.argsort(rows, axis=1, kind="stable")     # a row's dense entry comes before its BM25 entry
    rows, fused = np.take_along_axis(rows, order, 1), np.take_along_axis(fused, order, 1)
    dup = (rows[:, 1:] == rows[:, :-1]) & (rows[:, 1:] != big)
    fused[:, :-1][dup] += fused[:, 1:][dup]
    fused[:, 1:][dup] = -np.inf
    rows[:, 1:][dup] = big
    order = np.argsort(-fused, axis=1, kind="stable")[:, :k]   # stable: rows ascend inside a tie
    out_s, out_i = np.take_along_axis(fused, order, 1), np.take_along_axis(rows, order, 1)
    out_i[out_i == big] = -1
    return out_s, out_i


def host_linear_intersection_loop(S, I, B, J, k, ws, wb):
    nq = I.shape[0]
    out_s, out_i = np.full((nq, k), -np.inf), np.full((nq, k), -1, np.int64)
    for q in range(nq):
        s_of = {r: float(s) for r, s in zip(I[q].tolist(), S[q].tolist()) if r >= 0}
        both = {r: (s_of[r], b) for r, b in zip(J[q].tolist(), B[q].tolist()) if r in s_of and b != 0.0}
        if not both:
            continue
        s_lo, s_hi = min(v[0] for v in both.values()), max(v[0] for v in both.values())
        b_lo, b_hi = min(v[1] for v in both.values()), max(v[1] for v in both.values())
        fused = {r: ws * ((s - s_lo) / (s_hi - s_lo) if s_hi != s_lo else 0.0) +
                 wb * ((b - b_lo) / (b_hi - b_lo) if b_hi != b_lo else 0.0) for r, (s, b) in both.items()}
        top = sorted(fused, key=lambda r: (-fused[r], r))[:k]
        out_s[q, : len(top)] = [fused[r] for r in top]
        out_i[q, : len(top)] = top
    return out_s, out_i


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2025)
    t0 = time.perf_counter()
    texts = zipf_texts(args.docs, args.vocab, rng, 1, 30)
    queries = zipf_texts(args.queries, args.vocab, rng, 6, 6)
    bm25 = BM25Index(device="cuda:0")
    bm25.build_from_texts(list(range(args.docs)), texts)
    del texts
    gen = torch.Generator(device=dev).manual_seed(7)
    dense = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    rows = torch.randn((args.docs, 384), generator=gen, device=dev)
    rows /= rows.norm(dim=1, keepdim=True)
    dense.build_from_embeddings(rows)
    dense.doc_ids = []
    del rows
    emb = torch.randn((args.queries, 384), generator=gen, device=dev)
    emb /= emb.norm(dim=1, keepdim=True)
    hybrid = HybridIndex(dense, bm25, depth=args.depth)
    d, k, nq = hybrid.clip_depth(), args.k, args.queries
    emit({"stage": "setup", "device": torch.cuda.get_device_name(0), "docs": args.docs, "queries": nq, "depth": d, "k": k,
          "postings": int(len(bm25.bm25.post_rows)), "setup_s": round(time.perf_counter() - t0, 1)})

    # the three calls one by one
    csr = bm25.query_csr(queries)
    t_dense = device_ms(lambda: dense.search_device(emb, d), args.reps)
    emit({"stage": "dense_search", **t_dense})
    t_bm25 = device_ms(lambda: bm25._search_csr(csr, nq, d), args.reps)
    emit({"stage": "bm25_search", **t_bm25})
    S, I = dense.search_device(emb, d)
    B, J = bm25._search_csr(csr, nq, d)
    _, offsets, post_rows, post_w, idf = bm25._tables()
    lib = _native.load()
    out_s = torch.empty((nq, k), dtype=torch.float64, device=dev)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_c = torch.empty(nq, dtype=torch.int32, device=dev)
    stream = _native.current_stream_ptr(dev)

    def fuse(method):
        _native.check(lib.sskd_hybrid_fuse(
            dense._tiled.data_ptr(), args.docs, emb.data_ptr(), S.data_ptr(), I.data_ptr(), d, offsets.data_ptr(),
            post_rows.data_ptr(), post_w.data_ptr(), idf.data_ptr(), bm25.bm25.n_terms, csr[0].data_ptr(),
            csr[1].data_ptr(), B.data_ptr(), J.data_ptr(), d, None, method, 0.7, 0.3, 60.0, nq, k, 0, out_s.data_ptr(),
            out_i.data_ptr(), out_c.data_ptr(), None, None, stream))

    t_fuse = {}
    for name, code in (("rrf", 0), ("linear", 1)):
        t_fuse[name] = device_ms(lambda: fuse(code), args.reps)
        emit({"stage": f"fuse_{name}", **t_fuse[name], "union_mean": round(float(out_c.float().mean().item()), 1)})
    # the whole call (tokenising and uploading the query CSR included: host work inside the device-event window)
    t_whole = {}
    for name in ("rrf", "linear"):
        t_whole[name] = device_ms(lambda: hybrid.search_device(queries, emb, k, fusion_method=name), args.reps)
        emit({"stage": f"search_device_{name}", **t_whole[name]})

    # host legs on the same two device results
    torch.cuda.synchronize()
    (hS, hI, hB, hJ), t_copy = clock(lambda: (S.cpu().numpy(), I.cpu().numpy(), B.cpu().numpy(), J.cpu().numpy()))
    fuse(0)
    dev_s, dev_i = out_s.cpu().numpy(), out_i.cpu().numpy()
    (np_s, np_i), t_np = clock(lambda: host_rrf_numpy(hS, hI, hB, hJ, k, 0.7, 0.3, 60.0))
    (lp_s, lp_i), t_loop = clock(lambda: host_rrf_loop(hS, hI, hB, hJ, k, 0.7, 0.3, 60.0))
    _, t_lin = clock(lambda: host_linear_intersection_loop(hS, hI, hB, hJ, k, 0.7, 0.3))
    same = lambda s, i: bool(np.array_equal(i, dev_i) and np.array_equal(s.view(np.int64), dev_s.view(np.int64)))  # noqa: E731
    fuse_rrf_ms = t_fuse["rrf"]["median_ms"]
    emit({
        "stage": "summary", "device": torch.cuda.get_device_name(0), "docs": args.docs, "queries": nq, "depth": d, "k": k,
        "dense_search_ms": t_dense["median_ms"], "bm25_search_ms": t_bm25["median_ms"],
        "fuse_rrf_ms": fuse_rrf_ms, "fuse_linear_ms": t_fuse["linear"]["median_ms"],
        "search_device_rrf_ms": t_whole["rrf"]["median_ms"], "search_device_linear_ms": t_whole["linear"]["median_ms"],
        "host_copy_ms": round(t_copy * 1e3, 3), "host_rrf_numpy_ms": round(t_np * 1e3, 3),
        "host_rrf_loop_ms": round(t_loop * 1e3, 3), "host_linear_intersection_loop_ms": round(t_lin * 1e3, 3),
        "host_rrf_numpy_over_device_fuse": round((t_copy + t_np) * 1e3 / fuse_rrf_ms, 1),
        "host_rrf_loop_over_device_fuse": round((t_copy + t_loop) * 1e3 / fuse_rrf_ms, 1),
        "host_numpy_agrees_bitwise": same(np_s, np_i), "host_loop_agrees_bitwise": same(lp_s, lp_i),
    })


if __name__ == "__main__":
    main()
