"""A/B of mining with and without denoising: search + select (the path without the feature) against search +
`sskd_rank_denoise` + select, same process, same index, queries and positives.

    python tools/ab_denoise.py [--rows 100000] [--queries 10000] [--search-k 100] [--rounds 7] [--out FILE]

The corpus is documents of 3 consecutive rows: row j of a document is words 10 j .. 10 j + 50 of its 70 random words
(about 350 characters, neighbouring chunks share 40 of 50 words), and the embeddings are a document vector plus noise,
so the window of a query holds the siblings of its positives.  Every query is close to one document and has 1 to 3
positives (rows of that document).
  * device: `search_device` alone, `mine_negatives_device` without and with `denoising` alternate; each is timed with
    device events over `--iters` back-to-back calls after a warm-up; median (and range) of `--rounds` rounds.
    denoise = (with) - (without).  The yardstick is the search the call follows.
  * host: the Python `text_overlap` loop (candidate x positive) over the first `--host-queries` queries' windows, wall
    clock, for scale; its drop decisions are compared with the kernel's.
Prints one JSON object.
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
from semantic_search_kd_amd import Denoising, FAISSIndexBuilder, TrigramStore, text_overlap  # noqa: E402


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _texts(n_rows, rng):
    syll = ["ka", "to", "mi", "re", "su", "no", "la", "ve", "di", "po", "an", "er", "is", "ou", "th", "qu"]
    vocab = ["".join(syll[int(s)] for s in rng.integers(0, 16, int(rng.integers(2, 5)))) for _ in range(5000)]
    out = []
    for _ in range(-(-n_rows // 3)):
        words = [vocab[int(i)] for i in rng.integers(0, 5000, 70)]
        out += [" ".join(words[10 * j : 10 * j + 50]) for j in range(3)]
    return out[:n_rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--host-queries", type=int, default=100)
    ap.add_argument("--search-k", type=int, default=100)
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    texts = _texts(args.rows, rng)
    t0 = time.perf_counter()
    store = TrigramStore.build_from_texts(texts)
    build_s = time.perf_counter() - t0

    g = torch.Generator(device=dev).manual_seed(37)
    n_docs = -(-args.rows // 3)
    doc_of_row = torch.arange(args.rows, device=dev) // 3
    docs = torch.nn.functional.normalize(torch.randn(n_docs, 384, device=dev, generator=g), dim=1)
    corpus = docs[doc_of_row] + 0.5 * torch.nn.functional.normalize(torch.randn(args.rows, 384, device=dev, generator=g), dim=1)
    corpus = torch.nn.functional.normalize(corpus, dim=1)
    target = torch.randint(0, n_docs, (args.queries,), device=dev, generator=g)
    queries = docs[target] + 0.7 * torch.nn.functional.normalize(torch.randn(args.queries, 384, device=dev, generator=g), dim=1)
    queries = torch.nn.functional.normalize(queries, dim=1).contiguous()
    index = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    index.build_from_embeddings(corpus)
    del corpus, docs
    n_pos = rng.integers(1, 4, args.queries)
    first = target.cpu().numpy() * 3
    pos_lists = [[int(r) for r in range(f, min(f + m, args.rows))] for f, m in zip(first, n_pos)]
    lims = np.zeros(args.queries + 1, np.int64)
    np.cumsum([len(x) for x in pos_lists], out=lims[1:])
    d_lims = torch.from_numpy(lims).to(dev)
    d_rows = torch.from_numpy(np.concatenate(pos_lists).astype(np.int32)).to(dev)
    rule = Denoising(0.8, None)
    kw = dict(top_k=args.top_k, search_k=args.search_k, margin=0.1, normalize_queries=False)

    def search_only():
        index.search_device(queries, args.search_k, normalize_queries=False)

    def plain():
        return index.mine_negatives_device(queries, d_lims, d_rows, **kw)

    def denoised():
        return index.mine_negatives_device(queries, d_lims, d_rows, denoising=rule, trigrams=store, **kw)

    search_only()
    counts_plain = plain()[2].cpu().numpy()
    counts_denoised = denoised()[2].cpu().numpy()
    torch.cuda.synchronize()
    t_search, t_plain, t_den = [], [], []
    for _ in range(args.rounds):
        t_search.append(_time(search_only, args.iters))
        t_plain.append(_time(plain, args.iters))
        t_den.append(_time(denoised, args.iters))
    search_ms, plain_ms, den_ms = (statistics.median(t) for t in (t_search, t_plain, t_den))

    # the host loop, for scale, and the kernel's decisions against it
    hq = min(args.host_queries, args.queries)
    rank_scores, rank_rows = index.search_device(queries[:hq], args.search_k, normalize_queries=False)
    out = index.denoise_ranking_device(rank_scores, rank_rows, d_lims[: hq + 1], d_rows, rule, trigrams=store, diagnostics=True)
    window, reason = rank_rows.cpu().numpy(), out[5].cpu().numpy()
    t0 = time.perf_counter()
    host_drop = np.zeros(window.shape, bool)
    for q in range(hq):
        for r, row in enumerate(window[q]):
            if row >= 0:
                host_drop[q, r] = max(text_overlap(texts[row], texts[p]) for p in pos_lists[q]) > 0.8
    host_s = time.perf_counter() - t0

    r4 = lambda x: round(float(x), 4)
    result = {
        "rows": args.rows, "queries": args.queries, "search_k": args.search_k, "top_k": args.top_k,
        "mean_chars": r4(np.mean([len(t) for t in texts[:10000]])), "mean_keys_per_row": r4(store.keys.size / store.n_sets),
        "store_bytes": store.nbytes, "store_bytes_per_row": r4(store.nbytes / store.n_sets), "store_build_s": r4(build_s),
        "search_ms": r4(search_ms), "search_range": [r4(min(t_search)), r4(max(t_search))],
        "search_select_ms": r4(plain_ms), "search_select_range": [r4(min(t_plain)), r4(max(t_plain))],
        "search_denoise_select_ms": r4(den_ms), "search_denoise_select_range": [r4(min(t_den)), r4(max(t_den))],
        "denoise_ms": r4(den_ms - plain_ms), "denoise_over_search": r4((den_ms - plain_ms) / search_ms),
        "host_loop_queries": hq, "host_loop_ms_per_query": r4(host_s * 1e3 / hq),
        "host_loop_ms_extrapolated": round(host_s * 1e3 / hq * args.queries, 1),
        "same_decisions_as_host_loop": bool(np.array_equal(host_drop, (reason & 1).astype(bool))),
        "dropped_per_query": r4(host_drop.sum() / hq),
        "mean_survivors_plain": r4(counts_plain.mean()), "mean_survivors_denoised": r4(counts_denoised.mean()),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
